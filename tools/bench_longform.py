"""Time of the fused long-form reverse step (`vqvs_ddpm_step_windows`: one x0-sum launch and one step launch) against the same step
written as tensor expressions (unfold, the element-wise arithmetic of the step per window, weighted fold, unfold again), same
process, the two sides alternating:

  step  (n, W, H) = (16, 64000, 57600): a 58 s recording in 4 s windows with 0.4 s of overlap, constrain on, explicit noise on
        both sides (the tensor side has no counter-based generator), the next window batch written by both

Each timed sample is --inner consecutive steps between two device synchronisations (one step is tens of microseconds: a single one
would time the launch and the clock); each side runs --reps samples (at least 5) after a warm-up.  The result holds every
per-step time, the medians, each side's spread (max - min) / median, the largest difference of the two sides' outputs, and the
bytes the fused step must move, from the shapes.  No ratio is promised or gated: the file records what was found.  One JSON object on
stdout, also written to --out when given (profiles/longform_bench.json is where a run belongs)."""
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
ap.add_argument("--inner", type=int, default=200, help="steps per timed sample")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
assert torch.cuda.is_available(), "bench_longform.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
n, W, H = 16, 64000, 57600
V, Np = W - H, (n - 1) * H + W
A_T, A_PREV = 0.3, 0.37

x = randn_clips(1, Np, dev, 1).view(Np)
eps = randn_clips(n, W, dev, 2).view(n, W)
noise = randn_clips(1, Np, dev, 3).view(Np)
a_t, a_prev = torch.tensor([A_T], device=dev), torch.tensor([A_PREV], device=dev)
x_prev, windows = torch.empty_like(x), torch.empty_like(eps)
L = _native.lib()
FLAGS = _native.DDPM_CONSTRAIN


def fused():
    _native.check(L.vqvs_ddpm_step_windows(x.data_ptr(), eps.data_ptr(), noise.data_ptr(), a_t.data_ptr(), a_prev.data_ptr(), x_prev.data_ptr(),
                                           windows.data_ptr(), n, W, H, FLAGS, 1.0, 0, 0, 0, _native._stream_ptr()))
    return x_prev, windows


# the tensor side: scalars and blend weights prepared once, outside the timed region
alphas = a_t / a_prev
betas = 1 - alphas
c1, c2 = alphas.rsqrt(), betas * (1 - a_t).rsqrt()
sig = (betas * (1 - a_prev) / (1 - a_t)).sqrt()
sq1mat, rsat, sqat, rs1mat = (1 - a_t).sqrt(), a_t.rsqrt(), a_t.sqrt(), (1 - a_t).rsqrt()
weight = torch.ones(n, W, device=dev)
ramp = (torch.arange(V, device=dev, dtype=torch.float32) + 0.5) / V
weight[1:, :V] = ramp
weight[:-1, H:] = 1 - ramp


def tensor():
    xw = x.unfold(0, W, H)
    x0 = (xw - sq1mat * eps) * rsat
    x0 = (x0 - x0.mean(dim=1, keepdim=True)).clamp(-1, 1)
    e = (xw - x0 * sqat) * rs1mat
    folded = torch.nn.functional.fold((e * weight).t().unsqueeze(0), (1, Np), (1, W), stride=(1, H)).view(Np)
    out = c1 * (x - c2 * folded) + sig * noise
    return out, out.unfold(0, W, H).contiguous()


sides = {"fused": fused, "tensor": tensor}
outs = {}
for k, fn in sides.items():  # warm-up: code objects loaded, the allocator's blocks in place
    for _ in range(3):
        outs[k] = [t.clone() for t in fn()]
    torch.cuda.synchronize()
times = {k: [] for k in sides}
for _ in range(a.reps):
    for k, fn in sides.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / a.inner * 1e6)

res = {"device": torch.cuda.get_device_name(0), "n": n, "W": W, "H": H, "Np": Np, "flags": "constrain", "reps": a.reps, "inner": a.inner,
       "library": L.vqvs_version().decode()}
for k in sides:
    med = statistics.median(times[k])
    res[k] = {"us_per_step": [round(t, 2) for t in times[k]], "median_us": round(med, 2),
              "spread": round((max(times[k]) - min(times[k])) / med, 4)}
# what the fused step must move: the x0 sums read x and eps through the windows; the step reads x, eps and the noise and writes the
# state and the window batch (the chunk sums are a few hundred bytes)
res["fused_bytes_per_step"] = 4 * (2 * n * W + (Np + n * W + Np) + (Np + n * W))
res["fused_GBps_at_median"] = round(res["fused_bytes_per_step"] / (res["fused"]["median_us"] * 1e-6) / 1e9, 1)
res["fused_over_tensor"] = round(res["fused"]["median_us"] / res["tensor"]["median_us"], 4)
res["max_abs_diff_x_prev"] = (outs["fused"][0] - outs["tensor"][0]).abs().max().item()
res["max_abs_diff_windows"] = (outs["fused"][1] - outs["tensor"][1]).abs().max().item()
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
