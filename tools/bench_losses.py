"""Time and peak device memory of the fused denoising-loss path (`Diffusion.denoising_losses`, `speaker_search_losses`) against the
tensor-expression path it stands beside (`Diffusion.ddpm_losses`; the reference's evaluate_losses loop on `sample_q`), same
predictor, same process, the two sides alternating:

  eval    unet64, 64 clips x 64000 samples, one loss per clip
  search  VQVAE(64) decoder, 64 labels x 16 timesteps of ONE 64000-sample clip, micro-batches of 64, one noise draw

Each side runs --reps times (at least 5); the result holds every time, the medians, each side's spread (max - min) / median, and
torch's peak allocation per side (the native handle's arena is outside that count and common to both).  One JSON object on
stdout, also written to --out when given."""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import argparse
import json
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vq_voice_swap_amd import DiffusionModel, VQVAE, randn_clips, speaker_search_losses  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--precision", default="fp16,fp32")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None, help="also write the JSON object to this file (profiles/loss_bench.json is such a run)")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
dev = torch.device("cuda:0")
T = 64000


def det(m):
    det_init_(m.state_dict().items())
    return m.eval().to(dev)


def measure(sides, reps):
    """sides: {name: fn}; every fn is warmed once, then the sides alternate.  Times in ms, peaks in MiB above the standing allocation."""
    times, peaks = {k: [] for k in sides}, {}
    for k, fn in sides.items():
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks[k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    for _ in range(reps):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for k in sides:
        med = statistics.median(times[k])
        res[k] = {"ms": [round(t, 3) for t in times[k]], "median_ms": round(med, 3),
                  "spread": round((max(times[k]) - min(times[k])) / med, 4), "peak_MiB": peaks[k]}
    fused, tensor = res["fused"], res["tensor"]
    res["fused_over_tensor"] = round(fused["median_ms"] / tensor["median_ms"], 4)
    res["not_slower_beyond_spread"] = fused["median_ms"] <= tensor["median_ms"] * (1 + max(fused["spread"], tensor["spread"]))
    return res


def tensor_search(model, target, encoded, labels, ts, batch_size, eps):
    """The reference's loop (voice_search_vqvae.py:82-103) on the tensor expressions: clip, noise and conditioning repeated per row."""
    out = []
    for i in range(0, len(labels), batch_size):
        labels_mb, ts_mb = labels[i:i + batch_size], ts[i:i + batch_size]
        n = len(ts_mb)
        eps_mb = eps.repeat(n, 1, 1)
        x_t = model.diffusion.sample_q(target.repeat(n, 1, 1), ts_mb, epsilon=eps_mb)
        pred = model.predictor(x_t, ts_mb, cond=encoded.repeat(n, 1, 1), labels=labels_mb)
        out.append(((pred - eps_mb) ** 2).flatten(1).mean(1))
    return torch.cat(out)


out = {"device": torch.cuda.get_device_name(0), "T": T, "reps": a.reps}
for prec in a.precision.split(","):
    m = det(DiffusionModel("unet", 64))
    m.set_precision(prec)
    x = 0.3 * randn_clips(64, T, dev, 1)
    ts = torch.linspace(0.01, 0.99, 64, device=dev)
    out[f"eval_unet64_B64_{prec}"] = measure({
        "tensor": lambda: m.diffusion.ddpm_losses(x, m.predictor, ts),
        "fused": lambda: m.diffusion.denoising_losses(x, m.predictor, ts, seed=3),
    }, a.reps)
    del m, x
    torch.cuda.empty_cache()

    v = det(VQVAE(base_channels=64, pred_name="unet", num_labels=64))
    v.set_precision(prec)
    target = 0.1 * randn_clips(1, T, dev, 2)
    encoded = v.vq.embed(v.encode(target))
    labels = torch.arange(64, device=dev).repeat_interleave(16)
    ts = torch.linspace(0.0, 1.0, 16, device=dev).repeat(64)
    eps = randn_clips(1, T, dev, 4, stream_id=2)
    out[f"search_vqvae64_64labels_16ts_{prec}"] = measure({
        "tensor": lambda: tensor_search(v, target, encoded, labels, ts, 64, eps),
        "fused": lambda: speaker_search_losses(v, target, encoded, labels, ts, 64, 1, 4),
    }, a.reps)
    del v
    torch.cuda.empty_cache()

text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
