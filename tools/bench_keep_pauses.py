"""Times of the pause feature, same process, the compared forms alternating, device events around every sample:

  keep      `vqvs_keep_region_windows_packed` on a pack against the loop of per-recording `vqvs_keep_region_windows` calls it
            replaces, at 32 x 2, 64 x 1 and 8 x 8 (recordings x windows) windows of 64000 every 57600, the second half of every row kept
  detector  `vqvs_pause_mask` against the same definition as tensor expressions (view / sum / cummax / cummin / repeat_interleave) at 64
            rows of 4 s and at one row of 10 minutes, 16 kHz, frames of 160, rows that alternate 0.5 s of noise and 0.5 s of silence;
            `vqvs_windows_kept` on the detector's mask beside it
  decode    `VQVAE.decode_long_batch` on a seeded synthetic pack -- 32 recordings of 7 s whose second half is silence, unet64, fp16, 50
            DDPM steps, windows of 4 s with 0.4 s overlap -- with sources= / keep_pauses= and skipping on, the same with skip_kept=False,
            and the plain packed decode (no sources: the path as it was before the feature)

Each keep / detector sample is --inner consecutive calls between two device events; each side runs --reps samples (at least 5) after a
warm-up.  A decode sample is one call.  The result holds every sample, the medians and each side's spread (max - min) / median.  No
ratio is promised or gated: the file records what was found.  One JSON object on stdout, also written to --out when given
(profiles/keep_pauses_bench.json is where a run belongs)."""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import argparse
import json
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vq_voice_swap_amd import VQVAE, _native, pauses, randn_clips  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402
from vq_voice_swap_amd.longform import pack_layout, plan_pack  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=50, help="calls per timed sample of the keep and detector kernels")
ap.add_argument("--decode-reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
assert a.reps >= 5 and a.decode_reps >= 3, "--reps must be at least 5 and --decode-reps at least 3"
assert torch.cuda.is_available(), "bench_keep_pauses.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
L = _native.lib()
RATE, ALPHA = 16000, 0.3
W, H = 4 * RATE, 4 * RATE - 6400


def timed(sides, reps, inner, warm=2):
    """name -> microseconds per call of every sample: the sides alternate inside every repetition."""
    for fn in sides.values():  # warm-up: code objects loaded, the allocator's blocks in place
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1e3 / inner)
    return times


def summary(samples, digits=2):
    med = statistics.median(samples)
    return {"samples": [round(t, digits) for t in samples], "median": round(med, digits), "spread": round((max(samples) - min(samples)) / med, 4)}


res = {"device": torch.cuda.get_device_name(0), "library": L.vqvs_version().decode(), "reps": a.reps, "inner": a.inner, "W": W, "H": H,
       "units": {"keep": "us per call", "detector": "us per call", "decode": "ms per call"}}

# ---- 1. the packed keep against the loop of single calls
alpha1 = torch.full((1,), ALPHA, device=dev)
res["keep"] = {}
for R, n in ((32, 2), (64, 1), (8, 8)):
    counts = [n] * R
    first, offsets, total = pack_layout(counts, W, H)
    row = (n - 1) * H + W
    x, x0 = (randn_clips(1, total, dev, s).view(total) for s in (1, 2))
    keep = torch.zeros(total, dtype=torch.uint8, device=dev)
    for o in offsets:
        keep[o + row // 2:o + row] = 1
    windows = torch.zeros(R * n, W, device=dev)
    first_t = torch.tensor(first, dtype=torch.int32, device=dev)
    st = _native._stream_ptr()

    def packed():
        _native.check(L.vqvs_keep_region_windows_packed(x.data_ptr(), windows.data_ptr(), x0.data_ptr(), keep.data_ptr(), None, alpha1.data_ptr(),
                                                        first_t.data_ptr(), R, W, H, 1.0, 0, 0, 0, st))

    def loop():
        for r, o in enumerate(offsets):
            _native.check(L.vqvs_keep_region_windows(x.data_ptr() + 4 * o, windows.data_ptr() + 4 * first[r] * W, x0.data_ptr() + 4 * o,
                                                     keep.data_ptr() + o, None, alpha1.data_ptr(), n, W, H, 1.0, 0, r, 0, st))

    t = timed({"packed": packed, "loop_of_single_calls": loop}, a.reps, a.inner)
    entry = {k: summary(v) for k, v in t.items()}
    entry["packed_over_loop"] = round(entry["packed"]["median"] / entry["loop_of_single_calls"]["median"], 4)
    entry["samples_in_pack"] = total
    res["keep"][f"{R}x{n}"] = entry

# ---- 2. the detector against tensor expressions
FRAME, MIN_FRAMES, GUARD, DB = 160, 30, 5, -50.0
THR = pauses.threshold_energy(DB)


def detector_tensor(rows, frame, thr, min_frames, guard):
    """The scan form of the definition on R equal rows [R, Lr], Lr a multiple of `frame`: uint8 [R, Lr]."""
    R_, Lr = rows.shape
    F = Lr // frame
    q = torch.nan_to_num(torch.round(rows * 32768.0), nan=0.0).clamp(-32768.0, 32767.0).to(torch.int64)
    loud = (q * q).view(R_, F, frame).sum(-1) > thr * frame
    f = torch.arange(F, device=rows.device).expand(R_, F)
    left = torch.cummax(torch.where(loud, f, torch.full_like(f, -1)), dim=1).values
    right = torch.flip(torch.cummin(torch.flip(torch.where(loud, f, torch.full_like(f, F)), [1]), dim=1).values, [1])
    kept = ~loud & (right - left - 1 >= min_frames) & ((left < 0) | (f - left > guard)) & ((right >= F) | (right - f > guard))
    return kept.to(torch.uint8).repeat_interleave(frame, dim=1)


res["detector"] = {"frame": FRAME, "threshold_db": DB, "thr": THR, "min_frames": MIN_FRAMES, "guard_frames": GUARD}
for name, R, n in (("64_rows_of_4s", 64, 1), ("1_row_of_10min", 1, 166)):
    counts = [n] * R
    first, offsets, total = pack_layout(counts, W, H)
    row = (n - 1) * H + W  # a multiple of FRAME at these sizes
    assert row % FRAME == 0 and row % (RATE // 2) == 0
    rows = randn_clips(R, row, dev, 3).view(R, row) * 0.1
    rows.view(R, -1, RATE // 2)[:, 1::2] = 0.0  # every other half second is silence
    flat = rows.reshape(1, 1, total).contiguous()
    got = pauses.pause_mask(flat, counts, W, H, threshold_db=DB, frame=FRAME, min_pause_frames=MIN_FRAMES, guard_frames=GUARD)
    assert torch.equal(got.view(R, row), detector_tensor(rows, FRAME, THR, MIN_FRAMES, GUARD)), "the two forms disagree"
    t = timed({"kernel": lambda: pauses.pause_mask(flat, counts, W, H, threshold_db=DB, frame=FRAME, min_pause_frames=MIN_FRAMES, guard_frames=GUARD),
               "tensor_expressions": lambda: detector_tensor(rows, FRAME, THR, MIN_FRAMES, GUARD),
               "windows_kept": lambda: pauses.windows_kept(got, counts, W, H)}, a.reps, a.inner)
    entry = {k: summary(v) for k, v in t.items()}
    entry["kernel_over_tensor"] = round(entry["kernel"]["median"] / entry["tensor_expressions"]["median"], 4)
    entry.update(samples_in_pack=total, kept_fraction=round(float(got.float().mean()), 4),
                 GBps_at_median=round(5 * total / (entry["kernel"]["median"] * 1e-6) / 1e9, 1))  # 4 bytes read and 1 written per sample
    res["detector"][name] = entry

# ---- 3. the packed decode with pauses kept, skipped and not, against the plain packed decode
R, SECONDS = 32, 7
model = VQVAE(base_channels=64, pred_name="unet", num_labels=4)
det_init_(model.state_dict().items())
model.eval().to(dev)
model.set_precision("fp16")
num_samples = [SECONDS * RATE] * R
waves = []
for r in range(R):
    w = randn_clips(1, SECONDS * RATE, dev, 100 + r) * 0.1
    w[..., SECONDS * RATE // 2:] = 0.0
    waves.append(w.clamp(-1, 1))
codes, counts = model.encode_long_batch(waves, W, H)
labels = torch.arange(R, device=dev) % 4
kw = dict(counts=counts, num_samples=num_samples, window=W, hop=H, steps=a.steps, constrain=True, seed=5, window_batch=64)
detector = dict(threshold_db=DB, frame=FRAME, min_pause_frames=MIN_FRAMES, guard_frames=GUARD)
stats = {}
outs = {}


def decode(name, **extra):
    def run():
        outs[name] = model.decode_long_batch(codes, labels, **kw, **extra)
    return run


sides = {"pauses_kept_skipping": decode("skip", sources=waves, keep_pauses=detector, stats=stats),
         "pauses_kept_no_skipping": decode("noskip", sources=waves, keep_pauses=detector, skip_kept=False),
         "plain_packed_decode": decode("plain")}
t = timed(sides, a.decode_reps, 1, warm=1)
assert all(torch.equal(x_, y_) for x_, y_ in zip(outs["skip"], outs["noskip"])), "skipping changed an output"
res["decode"] = {k: summary([s / 1e3 for s in v], 1) for k, v in t.items()}
res["decode"].update(recordings=R, seconds=SECONDS, steps=a.steps, model="unet64 fp16", windows=sum(counts), skipped_windows=stats["skipped_windows"],
                     kept_fraction=round(stats["kept_samples"] / sum(num_samples), 4), window_batch=64,
                     skipping_over_no_skipping=round(res["decode"]["pauses_kept_skipping"]["median"] / res["decode"]["pauses_kept_no_skipping"]["median"], 4),
                     skipping_over_plain=round(res["decode"]["pauses_kept_skipping"]["median"] / res["decode"]["plain_packed_decode"]["median"], 4),
                     no_skipping_over_plain=round(res["decode"]["pauses_kept_no_skipping"]["median"] / res["decode"]["plain_packed_decode"]["median"], 4))
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
