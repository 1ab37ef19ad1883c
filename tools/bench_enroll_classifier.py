"""Time of one classifier-enrolment step (vq_voice_swap_amd/enroll.py, `ClassifierEnroller`) and of its two head kernels against what
they stand beside, same process, the sides alternating, every side warmed first:

  step   a default-topology classifier of --base channels and 251 labels, 4 new speakers, B = 8 clips x T = 64000 samples, in the fp32
         and the fp16 mode: `ClassifierEnroller.step` (noising, `vqvs_classifier_features`, `vqvs_head_xent_grad`, `vqvs_head_adamw`)
         against `Classifier.features` alone on the same noised batch
  head   `vqvs_head_xent_grad` + `vqvs_head_adamw` against the tensor-expression path on the same numbers -- F.gelu, F.linear of the
         old and of the new rows, log_softmax, autograd to the new rows, torch.optim.AdamW -- at (B, K, n, F) = (8, 251, 4, 512) and
         (64, 251, 16, 1024).  The kernels sum in float64 in a fixed order; the tensor path is float32 and makes no such promise.

Clock: device events around --inner consecutive calls of a side, divided by --inner; each side --reps times (at least 5).  The result
holds every time, the medians and each side's spread (max - min) / median.  One JSON object on stdout, also written to --out."""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import argparse
import json
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vq_voice_swap_amd import Classifier, randn_clips  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402
from vq_voice_swap_amd.enroll import ClassifierEnroller, head_adamw_step, head_xent_grad  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=10, help="calls of a side inside one pair of device events")
ap.add_argument("--base", type=int, default=64)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--T", type=int, default=64000)
ap.add_argument("--out", default=None, help="also write the JSON object to this file (profiles/enroll_classifier_bench.json is such a run)")
a = ap.parse_args()
assert a.reps >= 5 and a.inner >= 1, "--reps must be at least 5, --inner positive"
assert torch.cuda.is_available(), "no ROCm device visible: nothing here can be timed on a CPU"
dev = torch.device("cuda:0")


def measure(sides, reps, inner):
    """sides: {name: fn}; every fn is warmed twice, then the sides alternate.  ms per call from device events around `inner` calls."""
    times = {k: [] for k in sides}
    for fn in sides.values():
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    res = {}
    for k in sides:
        med = statistics.median(times[k])
        res[k] = {"ms": [round(t, 5) for t in times[k]], "median_ms": round(med, 5), "spread": round((max(times[k]) - min(times[k])) / med, 4)}
    return res


out = {"device": torch.cuda.get_device_name(0), "base": a.base, "B": a.batch, "T": a.T, "reps": a.reps, "inner": a.inner,
       "clock": "device events around `inner` calls of a side, per call"}

# ---- one enrolment step against the stem's forward alone
K, n, B, T = 251, 4, a.batch, a.T
clf = Classifier(K, base_channels=a.base)
det_init_(clf.state_dict().items())
clf = clf.eval().to(dev)
x0 = 0.3 * randn_clips(B, T, dev, 1)
noise = randn_clips(B, T, dev, 2)
ts = torch.linspace(0.05, 0.95, B)
labels = torch.tensor([K + (b % n) if b % 4 else b % K for b in range(B)], device=dev)
out["step"] = {"K": K, "n": n, "F": clf.feature_dim}
for prec in ("fp32", "fp16"):
    clf.set_precision(prec)
    en = ClassifierEnroller(clf, n, lr=1e-4)
    x_t = en.losses(x0, labels, ts=ts, noise=noise)["x_t"]
    ts_dev = ts.to(dev)
    res = measure({"step": lambda: en.step(x0, labels, ts=ts, noise=noise), "features_alone": lambda: clf.features(x_t, ts_dev)}, a.reps, a.inner)
    res["step_over_features"] = round(res["step"]["median_ms"] / res["features_alone"]["median_ms"], 4)
    clf.check_status()
    out["step"][prec] = res
del clf, en
torch.cuda.empty_cache()

# ---- the two head kernels against the tensor-expression path
out["head"] = []
for (B, K, n, Fd) in ((8, 251, 4, 512), (64, 251, 16, 1024)):
    g = torch.Generator().manual_seed(B)
    feat = torch.randn(B, Fd, generator=g).to(dev)
    w_old = (torch.randn(K, Fd, generator=g) / Fd ** 0.5).to(dev)
    b_old = (0.1 * torch.randn(K, generator=g)).to(dev)
    rows0 = torch.randn(n, Fd + 1, generator=g) / Fd ** 0.5
    y = torch.tensor([K + (b % n) if b % 4 else b % K for b in range(B)], device=dev)
    rows, mom, var = rows0.to(dev), torch.zeros(n, Fd + 1, device=dev), torch.zeros(n, Fd + 1, device=dev)
    count = [0]

    def kernels():
        r = head_xent_grad(feat, w_old, b_old, rows, y, want_logits=False)
        count[0] += 1
        head_adamw_step(rows, mom, var, r["act"], r["coef"], count[0], 1e-4, (0.9, 0.999), 1e-8, 0.0)

    new_w = torch.nn.Parameter(rows0[:, :-1].clone().to(dev))
    new_b = torch.nn.Parameter(rows0[:, -1].clone().to(dev))
    opt = torch.optim.AdamW([new_w, new_b], lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    rng = torch.arange(B, device=dev)

    def tensors():
        opt.zero_grad(set_to_none=True)
        act = F.gelu(feat)
        logits = torch.cat([F.linear(act, w_old, b_old), F.linear(act, new_w, new_b)], dim=1)
        nlls = -torch.log_softmax(logits, dim=-1)[rng, y]
        nlls.mean().backward()
        opt.step()

    res = measure({"kernels": kernels, "tensor": tensors}, a.reps, a.inner)
    res["kernels_over_tensor"] = round(res["kernels"]["median_ms"] / res["tensor"]["median_ms"], 4)
    res["shape"] = {"B": B, "K": K, "n": n, "F": Fd}
    res["launches"] = {"kernels": 2, "tensor": "F.gelu, two F.linear, cat, log_softmax, gather, mean, their backward and the optimiser's kernels"}
    out["head"].append(res)

text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
