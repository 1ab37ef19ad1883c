"""Time of the fused conversion-quality score (`vqvs_spectral_distance` through `SpectralDistance`: per-clip MCD and LSD sums of two
waveform batches from one kernel, float64 accumulation, nothing intermediate in memory) against a tensor-expression path to the
same two results on the device: `torch.stft` (float32 FFT, reflect padding, the same window) of both batches, two matmuls (mel
filter bank, DCT), `log`, two norms and a float64 sum over frames.  Same buffers, same process, the two sides alternating:

  (B, T) = (64, 64000) with the default constants (n_fft 400, hop 160, 40 mel bands, 13 coefficients)

and, for proportion, one --decode-steps (50) step `VQVAE.decode` of the same batch (a deterministically initialised model of
--base-channels in the --precision mode): the work an evaluation pass does per batch in front of the score.

Each side is warmed, then runs --reps times (at least 5) of --inner back-to-back calls between two device events (the decode: one
call per repetition); the result holds every time per call, the medians and each side's spread (max - min) / median.  Before
anything is timed the two sides' sums are compared to the float32 path's own rounding.  The fused kernel is written to be exact
and order-fixed, not fast; no ratio is expected.  One JSON object on stdout, also written to --out."""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import argparse
import json
import math
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vq_voice_swap_amd import VQVAE, SpectralDistance, randn_clips  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=10, help="calls per timed repetition")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--samples", type=int, default=64000)
ap.add_argument("--decode-steps", type=int, default=50)
ap.add_argument("--base-channels", type=int, default=64)
ap.add_argument("--precision", default="fp16", choices=["fp32", "fp16", "bf16"])
ap.add_argument("--out", default=None, help="also write the JSON object to this file (profiles/spectral_bench.json is such a run)")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
dev = torch.device("cuda:0")
B, T = a.batch, a.samples
distance = SpectralDistance()
k = distance.constants(dev)
DB = 10.0 / math.log(10.0)


def expressions(x, y):
    """[B, T] waveforms: the tensor-expression path (float32 throughout, float64 only for the sum over frames)."""
    def log_mel_and_cepstrum(w):
        spec = torch.stft(w, distance.n_fft, hop_length=distance.hop, window=k["window"], center=True, pad_mode="reflect", return_complex=True)
        mel = (spec.real ** 2 + spec.imag ** 2).transpose(1, 2) @ k["fb"]  # [B, frames, n_mels]
        L = torch.log(mel + distance.eps)
        return L, L @ k["dct"]

    (La, ca), (Lb, cb) = log_mel_and_cepstrum(x), log_mel_and_cepstrum(y)
    mcd = DB * torch.sqrt(2.0 * (ca[..., 1:] - cb[..., 1:]).pow(2).sum(-1))
    lsd = DB * torch.sqrt((La - Lb).pow(2).mean(-1))
    return mcd.sum(-1, dtype=torch.float64), lsd.sum(-1, dtype=torch.float64)


def fused(x, y):
    out = distance(x, y)
    return out["mcd"], out["lsd"]


def measure(sides, reps, inner):
    """sides: {name: (fn, calls per repetition)}; every fn is warmed, then the sides alternate.  Device-event times in ms per call."""
    times = {name: [] for name in sides}
    for fn, _ in sides.values():
        for _ in range(2):
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
    res = {}
    for name in sides:
        med = statistics.median(times[name])
        res[name] = {"ms": [round(t, 4) for t in times[name]], "median_ms": round(med, 4), "spread": round((max(times[name]) - min(times[name])) / med, 4)}
    return res


# a source and a "conversion" of it: the same clips with a tenth of another draw added, inside [-1, 1]
x = (0.3 * randn_clips(B, T, dev, 1)).clamp(-1, 1)[:, 0].contiguous()
y = (x + 0.03 * randn_clips(B, T, dev, 2)[:, 0]).clamp(-1, 1).contiguous()
m1, l1 = expressions(x, y)
m2, l2 = fused(x, y)
agree = {"mcd_rel_diff": float(((m1 - m2).abs() / m2).max()), "lsd_rel_diff": float(((l1 - l2).abs() / l2).max())}
assert max(agree.values()) <= 1e-3, f"the two sides' sums disagree: {agree}"

model = VQVAE(base_channels=a.base_channels, pred_name="unet", num_labels=3)
det_init_(model.state_dict().items())
model.eval().to(dev).set_precision(a.precision)
labels = (torch.arange(B, device=dev) % 3).to(torch.int64)
codes = model.encode(x[:, None])


def decode():
    return model.decode(codes, labels, steps=a.decode_steps, constrain=True, sampler="ddpm", seed=3, clip_offset=0)


out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "B": B, "T": T, "frames": distance.frames(T),
       "constants": {"n_fft": distance.n_fft, "hop": distance.hop, "n_mels": distance.n_mels, "n_ceps": distance.n_ceps},
       "decode_config": {"steps": a.decode_steps, "base_channels": a.base_channels, "precision": a.precision, "sampler": "ddpm"},
       "timing": "device events around `inner` calls (the decode: one call)", "agreement_before_timing": agree}
out.update(measure({"expressions": (lambda: expressions(x, y), a.inner), "fused": (lambda: fused(x, y), a.inner), "decode": (decode, 1)},
                   a.reps, a.inner))
out["fused_over_expressions"] = round(out["fused"]["median_ms"] / out["expressions"]["median_ms"], 4)
out["fused_over_decode"] = round(out["fused"]["median_ms"] / out["decode"]["median_ms"], 6)

text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
