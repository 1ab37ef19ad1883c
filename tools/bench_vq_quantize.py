"""Time and peak device memory of the fused quantise-and-score call (`vqvs_vq_quantize`: codes, embedding, per-clip sum of
(z - e)^2 and code counts in one kernel) against the path the parent commit offers for the same four results:
`vqvs_vq_argmin` + `vqvs_vq_embed` + the torch expression ((z - e) ** 2).flatten(1).sum(1) in float64 + `torch.bincount`
(which reads the largest code back to the host to size its output) added into the running histogram.  Same buffers, same process, the two sides alternating:

  B = 64 clips x T1 = 250 positions, K = 512 codes, Cd = 512 and 1024 channels

Each side runs --reps times (at least 5) of --inner back-to-back calls; the result holds every time per call, the medians, each
side's spread (max - min) / median and torch's peak allocation per side.  The two sides' codes, embeddings and counts are
compared bitwise and the error sums to 4 * 2^-24 before anything is timed.  One JSON object on stdout, also written to --out
when given."""
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

from vq_voice_swap_amd import _native, randn_clips  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=20, help="calls per timed repetition")
ap.add_argument("--out", default=None, help="also write the JSON object to this file (profiles/vq_quantize_bench.json is such a run)")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
dev = torch.device("cuda:0")
B, T1, K = 64, 250, 512
L = _native.lib()


def separate(z, d, hist):
    """The parent commit's path to the same four results."""
    n, c, t1 = z.shape
    idx = torch.empty(n, t1, device=dev, dtype=torch.int64)
    emb = torch.empty_like(z)
    _native.check(L.vqvs_vq_argmin(z.data_ptr(), d.data_ptr(), idx.data_ptr(), n, c, t1, d.shape[0], _native._stream_ptr()))
    _native.check(L.vqvs_vq_embed(idx.data_ptr(), d.data_ptr(), emb.data_ptr(), n, c, t1, d.shape[0], _native._stream_ptr()))
    sq = ((z - emb) ** 2).flatten(1).sum(1, dtype=torch.float64)
    hist += torch.bincount(idx.reshape(-1), minlength=d.shape[0])
    return idx, emb, sq


def fused(z, d, hist):
    n, c, t1 = z.shape
    idx = torch.empty(n, t1, device=dev, dtype=torch.int64)
    emb = torch.empty_like(z)
    sq = torch.empty(n, device=dev, dtype=torch.float64)
    _native.check(L.vqvs_vq_quantize(z.data_ptr(), d.data_ptr(), idx.data_ptr(), emb.data_ptr(), sq.data_ptr(), hist.data_ptr(), n, c, t1,
                                     d.shape[0], _native._stream_ptr()))
    return idx, emb, sq


def measure(sides, reps, inner):
    """sides: {name: fn}; every fn is warmed once, then the sides alternate.  Times in ms per call, peaks in MiB above the standing allocation."""
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
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / inner)
    res = {}
    for k in sides:
        med = statistics.median(times[k])
        res[k] = {"ms": [round(t, 4) for t in times[k]], "median_ms": round(med, 4),
                  "spread": round((max(times[k]) - min(times[k])) / med, 4), "peak_MiB": peaks[k]}
    res["fused_over_separate"] = round(res["fused"]["median_ms"] / res["separate"]["median_ms"], 4)
    return res


out = {"device": torch.cuda.get_device_name(0), "B": B, "T1": T1, "K": K, "reps": a.reps, "inner": a.inner}
for Cd in (512, 1024):
    z = randn_clips(B, Cd * T1, dev, 1).reshape(B, Cd, T1).contiguous()
    d = randn_clips(K, Cd, dev, 2).reshape(K, Cd).contiguous()
    h1, h2 = (torch.zeros(K, device=dev, dtype=torch.int64) for _ in range(2))
    i1, e1, s1 = separate(z, d, h1)
    i2, e2, s2 = fused(z, d, h2)
    assert torch.equal(i1, i2) and torch.equal(e1, e2) and torch.equal(h1, h2), "the two sides disagree"
    want = ((z.double() - e1.double()) ** 2).flatten(1).sum(1)
    assert ((s2 - want).abs() / want).max().item() <= 4 * 2.0 ** -24
    del i1, e1, s1, i2, e2, s2, want
    out[f"Cd{Cd}"] = measure({"separate": lambda: separate(z, d, h1), "fused": lambda: fused(z, d, h2)}, a.reps, a.inner)
    del z, d
    torch.cuda.empty_cache()

text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
