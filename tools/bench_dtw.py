"""Time of the aligned score (`AlignedDistance`: `vqvs_mel_cepstra` on both sides, then `vqvs_dtw_distance`, one workgroup per pair
walking the anti-diagonals in LDS) for

  64 pairs of 4 s  (401 x 401 frames at the default constants)   and   16 pairs of 10 s  (1001 x 1001 frames)

against (a) the float64 numpy restatement of tests/dtw_ref.py on the CPU, ONE pair; (b) the same recurrence as an anti-diagonal
loop of tensor expressions on the device, the whole batch at once (local costs of all cells first, skewed so that a diagonal is a
row; per diagonal a handful of elementwise kernels over [B, Fa]); and (c), for proportion, the --decode-steps (50) step packed
decode (`VQVAE.encode_long_batch` / `decode_long_batch`, a deterministically initialised model of --base-channels in the
--precision mode) that an evaluation runs in front of the score.

Every device side is warmed, then the sides alternate --reps times (at least 5), `--inner` back-to-back fused calls and one call
of the others between two device events; the CPU side is timed by the wall clock, --cpu-reps times.  The result holds every time,
the medians and each side's spread (max - min) / median.  Before anything is timed the three sides' costs and path lengths are
compared.  One JSON object on stdout, also written to --out."""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import argparse
import json
import math
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from vq_voice_swap_amd import VQVAE, AlignedDistance, SpectralDistance  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402

import dtw_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--cpu-reps", type=int, default=3)
ap.add_argument("--inner", type=int, default=5, help="fused calls per timed repetition")
ap.add_argument("--decode-steps", type=int, default=50)
ap.add_argument("--base-channels", type=int, default=64)
ap.add_argument("--precision", default="fp16", choices=["fp32", "fp16", "bf16"])
ap.add_argument("--out", default=None, help="also write the JSON object to this file (profiles/dtw_bench.json is such a run)")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
dev = torch.device("cuda:0")
spectral = SpectralDistance()
aligned = AlignedDistance(spectral)
DB = 10.0 / math.log(10.0)
WINDOW, HOP = 64000, 57600  # convert_dataset.py's defaults: 4 s windows, 0.4 s overlap


def voices(B, T, semitones, warp, seed):
    """Five-harmonic voices gliding over an octave, one register per clip, with 1 % noise; `warp` bends the time axis."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = (torch.arange(T, dtype=torch.float64)[None] / T) ** warp
    f = (90.0 + 120.0 * torch.rand(B, 1, generator=torch.Generator().manual_seed(1), dtype=torch.float64)) * 2.0 ** (n + semitones / 12.0)
    phase = 2 * math.pi * torch.cumsum(f, 1) / spectral.sample_rate
    w = sum(torch.sin(k * phase) / k for k in range(1, 6)) / sum(1.0 / k for k in range(1, 6))
    return (0.5 * w + 0.005 * torch.randn(B, T, generator=g, dtype=torch.float64)).float().to(dev).contiguous()


def expressions(ca, cb):
    """[B, Fa, n], [B, Fb, n] float32 cepstra -> (cost [B] float64, steps [B]): the recurrence, one anti-diagonal per iteration."""
    B, Fa, Fb = ca.shape[0], ca.shape[1], cb.shape[1]
    diff = ca.double()[:, :, None, 1:] - cb.double()[:, None, :, 1:]
    d = DB * torch.sqrt(2.0 * (diff * diff).sum(-1))                                  # [B, Fa, Fb]
    i = torch.arange(Fa, device=ca.device)
    k = torch.arange(Fa + Fb - 1, device=ca.device)
    j = k[:, None] - i[None, :]                                                       # [K, Fa]
    valid = (j >= 0) & (j < Fb)
    inf = torch.full((), math.inf, device=ca.device, dtype=torch.float64)
    skew = torch.where(valid[None], d.gather(2, j.clamp(0, Fb - 1).t()[None].expand(B, Fa, -1)).transpose(1, 2), inf)   # [B, K, Fa]
    shift = lambda t, fill: torch.cat([torch.full_like(t[:, :1], fill), t[:, :-1]], 1)  # noqa: E731  row i takes row i - 1
    prev1, prev2 = torch.full((B, Fa), math.inf, device=ca.device, dtype=torch.float64), torch.full((B, Fa), math.inf, device=ca.device, dtype=torch.float64)
    n1, n2 = torch.zeros(B, Fa, device=ca.device, dtype=torch.int32), torch.zeros(B, Fa, device=ca.device, dtype=torch.int32)
    for kk in range(Fa + Fb - 1):
        diag, up, left = shift(prev2, math.inf), shift(prev1, math.inf), prev1
        best, steps = diag, shift(n2, 0)
        take = up < best
        best, steps = torch.where(take, up, best), torch.where(take, shift(n1, 0), steps)
        take = left < best
        best, steps = torch.where(take, left, best), torch.where(take, n1, steps)
        if kk == 0:
            best = torch.zeros_like(best)
        prev2, n2, prev1, n1 = prev1, n1, skew[:, kk] + best, steps + 1
    return prev1[:, Fa - 1], n1[:, Fa - 1]


def measure(sides, reps):
    """sides: {name: (fn, calls per repetition)}; every fn is warmed once, then the sides alternate.  Device-event times in ms per call."""
    times = {name: [] for name in sides}
    for fn, _ in sides.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, (fn, calls) in sides.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / calls)
    return {name: summary(times[name]) for name in sides}


def summary(ms):
    med = statistics.median(ms)
    return {"ms": [round(t, 4) for t in ms], "median_ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4)}


model = VQVAE(base_channels=a.base_channels, pred_name="unet", num_labels=3)
det_init_(model.state_dict().items())
model.eval().to(dev).set_precision(a.precision)

out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "cpu_reps": a.cpu_reps,
       "constants": {"n_fft": spectral.n_fft, "hop": spectral.hop, "n_mels": spectral.n_mels, "n_ceps": spectral.n_ceps},
       "decode_config": {"steps": a.decode_steps, "base_channels": a.base_channels, "precision": a.precision, "sampler": "ddpm", "window": WINDOW, "hop": HOP},
       "timing": "device events around `inner` fused calls (expressions and decode: one call); numpy: wall clock, one pair", "shapes": {}}
for name, B, T in (("64x4s", 64, 64000), ("16x10s", 16, 160000)):
    x, y = voices(B, T, 0.0, 1.0, 2), voices(B, T, 3.0, 1.3, 3)
    lengths = [T] * B
    F = spectral.frames(T)
    ca, cb = spectral.cepstra(x, lengths)["ceps"], spectral.cepstra(y, lengths)["ceps"]
    got = aligned(x, lengths, y, lengths)
    cost_e, steps_e = expressions(ca, cb)
    ref = dtw_ref.dtw_ref(ca[0].cpu().numpy(), cb[0].cpu().numpy())
    agree = {"fused_vs_numpy_pair0_bit_equal": float(got["cost"][0]) == ref["cost"], "steps_pair0": [int(got["steps"][0]), ref["steps"]],
             "fused_vs_expressions_max_rel_diff": float(((got["cost"] - cost_e).abs() / got["cost"]).max()),
             "steps_equal": bool(torch.equal(got["steps"], steps_e)), "mean_stretch": float(got["steps"].sum()) / (B * F),
             "mcd_dtw": float(got["cost"].sum() / got["steps"].sum()), "smallest_margin_pair0": ref["margin"]}
    assert agree["fused_vs_expressions_max_rel_diff"] <= 1e-12 and abs(float(got["cost"][0]) - ref["cost"]) <= 1e-12 * ref["cost"], f"the sides disagree: {agree}"
    waves = [x[r][None, None] for r in range(B)]
    labels = (torch.arange(B, device=dev) % 3).to(torch.int64)
    codes, counts = model.encode_long_batch(waves, WINDOW, HOP, 64)

    def decode():
        return model.decode_long_batch(codes, labels, counts=counts, num_samples=lengths, window=WINDOW, hop=HOP, steps=a.decode_steps, constrain=True,
                                       seed=3, clip_offset=0, window_batch=64, sampler="ddpm")

    res = {"B": B, "T": T, "frames": F, "windows": sum(counts), "agreement_before_timing": agree}
    res.update(measure({"expressions": (lambda: expressions(ca, cb), 1), "fused": (lambda: aligned(x, lengths, y, lengths), a.inner),
                        "cepstra_only": (lambda: (spectral.cepstra(x, lengths), spectral.cepstra(y, lengths)), a.inner), "decode": (decode, 1)}, a.reps))
    cpu, pair = [], (ca[0].cpu().numpy(), cb[0].cpu().numpy())
    for _ in range(a.cpu_reps):
        t0 = time.perf_counter()
        dtw_ref.dtw_ref(*pair)
        cpu.append((time.perf_counter() - t0) * 1e3)
    res["numpy_one_pair"] = summary(cpu)
    res["fused_over_expressions"] = round(res["fused"]["median_ms"] / res["expressions"]["median_ms"], 6)
    res["fused_over_decode"] = round(res["fused"]["median_ms"] / res["decode"]["median_ms"], 6)
    res["fused_batch_over_numpy_one_pair"] = round(res["fused"]["median_ms"] / res["numpy_one_pair"]["median_ms"], 6)
    out["shapes"][name] = res

text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
