"""Time of one speaker-enrolment step (vq_voice_swap_amd/enroll.py) and of its new kernels against what they stand beside, same
process, the sides alternating, every side warmed first:

  step        unet64 with 8 labels, B = 8 clips x T = 64000 samples, fp32: `embedding_grad` + `vqvs_embed_adamw` against the forward
              schedule alone ON THE SAME predictor-gradient handle (vqvs_unet_embed_grad without mse / grad)
  film_grad   the film_grad launches of one such step (per-op HIP events of the handle's profiling hook, summed over the blocks)
              against the tensor expressions (du2 * h_hat).sum(-1) and du2.sum(-1) on tensors of every block's shape, bracketed by
              events per block in the same way
  adamw       `vqvs_embed_adamw` (2 rows, E = 256, 8 clips) against index_add_ + torch.optim.AdamW on the same table

Each side runs --reps times (at least 5); the result holds every time, the medians and each side's spread (max - min) / median.
One JSON object on stdout, also written to --out when given."""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import argparse
import json
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vq_voice_swap_amd import UNetPredictor, _native, randn_clips  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402
from vq_voice_swap_amd.enroll import adamw_step  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--base", type=int, default=64)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--T", type=int, default=64000)
ap.add_argument("--out", default=None, help="also write the JSON object to this file (profiles/enroll_bench.json is such a run)")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
dev = torch.device("cuda:0")
B, T, E = a.batch, a.T, 4 * a.base


def measure(sides, reps):
    """sides: {name: fn}; every fn is warmed twice, then the sides alternate.  Wall-clock ms around a device synchronisation."""
    times = {k: [] for k in sides}
    for fn in sides.values():
        fn()
        fn()
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
        res[k] = {"ms": [round(t, 4) for t in times[k]], "median_ms": round(med, 4), "spread": round((max(times[k]) - min(times[k])) / med, 4)}
    return res


m = UNetPredictor(a.base, num_labels=8)
det_init_(m.state_dict().items())
m = m.eval().to(dev)
x_t, eps = randn_clips(B, T, dev, 1), randn_clips(B, T, dev, 2)
ts = torch.linspace(0.05, 0.95, B, device=dev)
row_of_clip = (torch.arange(B, device=dev) % 2).to(torch.int64)
rows = torch.randn(2, E, device=dev)
mom, var = torch.zeros_like(rows), torch.zeros_like(rows)
pred = torch.empty(B, 1, T, device=dev)
count = [0]


def step():
    _, grads = m.embedding_grad(x_t, ts, eps, rows[row_of_clip])
    count[0] += 1
    adamw_step(rows, mom, var, grads, row_of_clip, count[0], 1e-4, (0.9, 0.999), 1e-8, 0.0)


def forward_alone():
    vec = rows[row_of_clip]
    h = m._grad_handle(dev, B, T)
    _native.check(_native.lib().vqvs_unet_embed_grad(h.ptr, x_t.data_ptr(), ts.data_ptr(), None, vec.data_ptr(), None, None, None,
                                                     pred.data_ptr(), B, T, _native._stream_ptr()))


out = {"device": torch.cuda.get_device_name(0), "base": a.base, "B": B, "T": T, "precision": "fp32", "reps": a.reps}
res = measure({"step": step, "forward_alone": forward_alone}, a.reps)
res["step_over_forward"] = round(res["step"]["median_ms"] / res["forward_alone"]["median_ms"], 4)
h = m._grad_handle(dev, B, T)
res["handle_GiB"] = round(h.device_bytes() / 2 ** 30, 3)
kinds = [k for k, _, _ in h.op_info(B, T)]
res["ops_per_step"] = len(kinds)  # schedule entries of the handle
# kernels: film_grad and mse_head entries enqueue two each (tile pass + fixed-order finish), and the AdamW kernel is no entry of the handle
res["launches_per_step"] = len(kinds) + kinds.count("film_grad") + kinds.count("mse_head") + 1
out["step"] = res

# film_grad: the handle's own per-op events, summed over the blocks, per profiled step
descs = h.op_desc()
h.set_profiling(True)
film = []
for _ in range(a.reps + 1):
    step()
    ms = h.profile_read()
    film.append(sum(t for t, k in zip(ms, kinds) if k == "film_grad"))
h.set_profiling(False)
film = film[1:]
shapes = []
for k, d in zip(kinds, descs):
    if k == "film_grad":
        C, ls = (int(v) for v in re.match(r"C=(\d+) L>>(-?\d+)", d).groups())
        shapes.append((C, T >> ls))
tensors = [(torch.randn(B, C, L, device=dev), torch.randn(B, C, L, device=dev), torch.randn(B, C, 1, device=dev), torch.rand(B, C, 1, device=dev) + 0.5,
            torch.randn(1, C, 1, device=dev), torch.randn(1, C, 1, device=dev)) for C, L in shapes]


def film_tensor():
    """The tensor expressions of every block, each block bracketed by its own pair of events (the clock of the kernel side): ms summed."""
    marks = []
    for du2, h1, mean, rstd, gamma, beta in tensors:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h_hat = gamma * rstd * (h1 - mean) + beta
        (du2 * h_hat).sum(-1)
        du2.sum(-1)
        e1.record()
        marks.append((e0, e1))
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in marks)


film_tensor()
film_tensor()
tens = [film_tensor() for _ in range(a.reps)]
med, tmed = statistics.median(film), statistics.median(tens)
out["film_grad"] = {"blocks": len(shapes), "clock": "HIP events around every block's work on both sides, summed over the blocks",
                    "kernel": {"ms": [round(t, 4) for t in film], "median_ms": round(med, 4), "spread": round((max(film) - min(film)) / med, 4)},
                    "tensor": {"ms": [round(t, 4) for t in tens], "median_ms": round(tmed, 4), "spread": round((max(tens) - min(tens)) / tmed, 4)},
                    "kernel_over_tensor": round(med / tmed, 4)}
del tensors
torch.cuda.empty_cache()

# AdamW: the kernel against index_add_ + torch.optim.AdamW
grads = 1e-3 * torch.randn(B, E, device=dev)
p = torch.nn.Parameter(rows.clone())
opt = torch.optim.AdamW([p], lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
k2 = [0]


def adamw_kernel():
    k2[0] += 1
    adamw_step(rows, mom, var, grads, row_of_clip, k2[0], 1e-4, (0.9, 0.999), 1e-8, 0.0)


def adamw_torch():
    table = torch.zeros_like(p)
    table.index_add_(0, row_of_clip, grads)
    p.grad = table / B
    opt.step()


res = measure({"kernel": adamw_kernel, "torch": adamw_torch}, a.reps)
res["kernel_over_torch"] = round(res["kernel"]["median_ms"] / res["torch"]["median_ms"], 4)
out["adamw"] = res

text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
