"""Time of the explicit-vector forward and of the speaker mix kernel against what they stand beside, same process, the sides
alternating, every side warmed first:

  forward   unet64 with 8 labels, 64 clips x 64000 samples, fp16 and fp32: `forward(vectors=class_embed.weight[labels])`
            (vqvs_unet_forward_vec) against `forward(labels=labels)` (vqvs_unet_forward) on the same handle.  It is the same schedule
            with one pointer swapped; the outputs are compared bit for bit before anything is timed.
  mix       `vqvs_speaker_mix` against the tensor expression (w[..., None] * table[idx]).sum(1) at (B, K, J, E) = (64, 251, 2, 256) and
            (512, 251, 16, 256).  Both are a few microseconds of device work, so a timed sample is --mix-calls calls in a row and the
            figure is the time per call: launch overhead is most of it, on both sides.  The kernel exists for its defined arithmetic
            (a voice is reproducible from its spec), not for this number.

Each side runs --reps times (at least 5); the result holds every time, the medians and each side's spread (max - min) / median.
One JSON object on stdout, also written to --out when given (profiles/speaker_vectors_bench.json is such a run)."""
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

from vq_voice_swap_amd import UNetPredictor, _native, randn_clips, speaker_mix  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--base", type=int, default=64)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--T", type=int, default=64000)
ap.add_argument("--mix-calls", type=int, default=2000, help="calls in a row per timed sample of the mix")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
assert torch.cuda.is_available(), "bench_speaker_vectors.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
B, T = a.batch, a.T


def measure(sides, reps, calls=1):
    """sides: {name: fn}; every fn is warmed twice, then the sides alternate.  Wall-clock ms per call around a device synchronisation."""
    times = {k: [] for k in sides}
    for fn in sides.values():
        fn()
        fn()
    for _ in range(reps):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / calls)
    res = {}
    for k in sides:
        med = statistics.median(times[k])
        res[k] = {"ms": [round(t, 5) for t in times[k]], "median_ms": round(med, 5), "spread": round((max(times[k]) - min(times[k])) / med, 4)}
    return res


out = {"device": torch.cuda.get_device_name(0), "base": a.base, "B": B, "T": T, "reps": a.reps, "forward": {}, "mix": {}}

m = UNetPredictor(a.base, num_labels=8)
det_init_(m.state_dict().items())
m = m.eval().to(dev)
x = randn_clips(B, T, dev, 1)
ts = torch.linspace(0.05, 0.95, B, device=dev)
labels = (torch.arange(B, device=dev) % 8).to(torch.int64)
vectors = m.class_embed.weight.detach()[labels].contiguous()
for precision in ("fp16", "fp32"):
    m.set_precision(precision)
    same = bool(torch.equal(m(x, ts, labels=labels), m(x, ts, vectors=vectors)))
    res = measure({"labels": lambda: m(x, ts, labels=labels), "vectors": lambda: m(x, ts, vectors=vectors)}, a.reps)
    res["vectors_over_labels"] = round(res["vectors"]["median_ms"] / res["labels"]["median_ms"], 4)
    res["bit_equal"] = same
    out["forward"][precision] = res
m.invalidate()
torch.cuda.empty_cache()

for Bm, K, J, E in ((64, 251, 2, 256), (512, 251, 16, 256)):
    g = torch.Generator().manual_seed(Bm)
    table = torch.randn(K, E, generator=g).to(dev)
    idx = torch.randint(0, K, (Bm, J), generator=g).to(device=dev, dtype=torch.int32)
    w = torch.rand(Bm, J, generator=g).to(dev)
    idx_long = idx.long()
    dst = torch.empty(Bm, E, device=dev)
    # the binding checks the index range with one device->host sync per call; the loop below times the launch path without it
    L, st = _native.lib(), _native._stream_ptr()

    def kernel():
        _native.check(L.vqvs_speaker_mix(table.data_ptr(), K, E, idx.data_ptr(), w.data_ptr(), J, dst.data_ptr(), Bm, st))

    def tensor():
        return (w[..., None] * table[idx_long]).sum(1)

    close = float((speaker_mix(table, idx, w) - tensor()).abs().max())
    res = measure({"kernel": kernel, "tensor": tensor}, a.reps, a.mix_calls)
    res["kernel_over_tensor"] = round(res["kernel"]["median_ms"] / res["tensor"]["median_ms"], 4)
    res["calls_per_sample"] = a.mix_calls
    res["max_abs_difference"] = close  # (the tensor expression sums in torch's order: the same value up to float32 rounding)
    out["mix"][f"B{Bm}_K{K}_J{J}_E{E}"] = res

text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
