"""Time of the fused scoring call (`vqvs_xent_score`: per-clip NLL sums, top-1 and top-k counts and confusion counts from one
kernel) against the tensor-expression path to the same four results, all on the device: `log_softmax` (float32, as
`F.cross_entropy` on the logits computes it) + `gather` + sum in float64, `argmax`, `topk`, and `bincount` of
target * K + argmax added into the running confusion matrix.  Same buffers, same process, the two sides alternating:

  (B, K, L) = (4, 512, 250): one encoder-predictor batch;  (64, 251, 1): one classifier batch

Each side is warmed, then runs --reps times (at least 5) of --inner back-to-back calls between two device events; the result
holds every time per call, the medians and each side's spread (max - min) / median.  Before anything is timed the counts of the
two sides are compared exactly and the NLL sums to the float32 path's own rounding.  Neither side is where an evaluation pass
spends its time (the forward in front of it is); no ratio is expected.  One JSON object on stdout, also written to --out."""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import argparse
import json
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vq_voice_swap_amd import _native, randn_clips  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=50, help="calls per timed repetition")
ap.add_argument("--topk", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the JSON object to this file (profiles/guidance_eval_bench.json is such a run)")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
dev = torch.device("cuda:0")
lib = _native.lib()
SHAPES = [(4, 512, 250), (64, 251, 1)]


def expressions(logits, targets, conf, k):
    """[B, K, L] logits, [B, L] targets: the tensor-expression path."""
    K = logits.shape[1]
    logp = torch.log_softmax(logits, dim=1)
    nll = -logp.gather(1, targets[:, None]).squeeze(1).sum(1, dtype=torch.float64)
    pred = logits.argmax(1)
    top1 = (pred == targets).sum(1)
    topk = (logits.topk(k, dim=1).indices == targets[:, None]).any(1).sum(1)
    conf += torch.bincount((targets * K + pred).reshape(-1), minlength=K * K).reshape(K, K)
    return nll, top1, topk


def fused(logits, targets, conf, k):
    B, K, L = logits.shape
    nll = torch.empty(B, device=dev, dtype=torch.float64)
    top1, topk = (torch.empty(B, device=dev, dtype=torch.int64) for _ in range(2))
    _native.check(lib.vqvs_xent_score(logits.data_ptr(), targets.data_ptr(), nll.data_ptr(), top1.data_ptr(), topk.data_ptr(), k,
                                      conf.data_ptr(), B, K, L, _native._stream_ptr()))
    return nll, top1, topk


def measure(sides, reps, inner):
    """sides: {name: fn}; every fn is warmed, then the sides alternate.  Device-event times in ms per call."""
    times = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in sides.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(inner):
                fn()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop) / inner)
    res = {}
    for k in sides:
        med = statistics.median(times[k])
        res[k] = {"ms": [round(t, 5) for t in times[k]], "median_ms": round(med, 5), "spread": round((max(times[k]) - min(times[k])) / med, 4)}
    res["fused_over_expressions"] = round(res["fused"]["median_ms"] / res["expressions"]["median_ms"], 4)
    return res


out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "topk": a.topk, "timing": "device events around `inner` calls"}
for B, K, L in SHAPES:
    logits = (2.0 * randn_clips(B, K * L, dev, 1)).reshape(B, K, L).contiguous()
    targets = (randn_clips(B, L, dev, 2).reshape(B, L).abs() * 1000).to(torch.int64) % K
    k = min(a.topk, K)
    c1, c2 = (torch.zeros(K, K, device=dev, dtype=torch.int64) for _ in range(2))
    n1, t1, k1 = expressions(logits, targets, c1, k)
    n2, t2, k2 = fused(logits, targets, c2, k)
    assert torch.equal(t1, t2) and torch.equal(k1, k2) and torch.equal(c1, c2), "the two sides' counts disagree"  # (no exact ties in random logits)
    assert ((n1 - n2).abs() / n2.abs()).max().item() <= 1e-5, "the two sides' NLL sums disagree"
    out[f"B{B}_K{K}_L{L}"] = measure({"expressions": lambda: expressions(logits, targets, c1, k), "fused": lambda: fused(logits, targets, c2, k)},
                                     a.reps, a.inner)

text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
