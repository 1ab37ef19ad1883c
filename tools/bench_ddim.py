"""Time of the DDIM step kernels at (B, T) = (64, 64000), constrain on, explicit noise, the gradient of a guided step given as a tensor
(the guidance model's own time is not part of any side), same process, the four sides alternating:

  ddim_guided    `vqvs_ddim_step` with a gradient: one x0-sum launch and one step launch
  ddim_unguided  `vqvs_ddim_step` without one
  ddpm_guided    what a guided DDPM step launches around its cond_fn: `vqvs_ddpm_mean`, `vqvs_ddpm_guided_eps`, `vqvs_ddpm_step`
  tensor         the guided DDIM step written as torch tensor expressions (coefficients prepared once, outside the timed region)

Each timed sample is --inner consecutive steps between two device synchronisations; each side runs --reps samples (at least 5)
after a warm-up.  The result holds every per-step time, the medians, each side's spread (max - min) / median, the bytes each fused
side must move, from the shapes, and the largest difference between the fused guided step and the tensor side.  No ratio is promised
or gated: the file records what was found.  One JSON object on stdout, also written to --out when given (profiles/ddim_bench.json is
where a run belongs)."""
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
ap.add_argument("--inner", type=int, default=100, help="steps per timed sample")
ap.add_argument("--eta", type=float, default=0.5)
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
assert torch.cuda.is_available(), "bench_ddim.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
B, T = 64, 64000
A_T, A_TO = 0.3, 0.37

x, eps, grad, noise = (randn_clips(B, T, dev, s).view(B, T) for s in (1, 2, 3, 4))
a_t, a_to = torch.full((B,), A_T, device=dev), torch.full((B,), A_TO, device=dev)
out, mean, eps2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
L = _native.lib()
CONSTRAIN = _native.DDIM_CONSTRAIN


def ddim(g):
    _native.check(L.vqvs_ddim_step(x.data_ptr(), eps.data_ptr(), _native._ptr(g), noise.data_ptr(), a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(),
                                   B, T, CONSTRAIN, a.eta, 1.0, 0, 0, 0, _native._stream_ptr()))
    return out


def ddpm_guided():
    st = _native._stream_ptr()
    _native.check(L.vqvs_ddpm_mean(x.data_ptr(), eps.data_ptr(), a_t.data_ptr(), a_to.data_ptr(), mean.data_ptr(), B, T, st))
    _native.check(L.vqvs_ddpm_guided_eps(x.data_ptr(), mean.data_ptr(), grad.data_ptr(), a_t.data_ptr(), a_to.data_ptr(), eps2.data_ptr(), B, T,
                                         CONSTRAIN, st))
    _native.check(L.vqvs_ddpm_step(x.data_ptr(), eps2.data_ptr(), noise.data_ptr(), a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), B, T, CONSTRAIN,
                                   1.0, 0, 0, 0, st))
    return out


# the tensor side: the coefficients in float64 from the float32 alphas, rounded once, as the kernel forms them
at64, ato64 = a_t.double().view(B, 1), a_to.double().view(B, 1)
sig64 = a.eta * ((1 - ato64) / (1 - at64)).sqrt() * (1 - at64 / ato64).sqrt()
sq1mat, rsat, sqat, rs1mat, sqto, sig, ce = (v.float() for v in ((1 - at64).sqrt(), at64.rsqrt(), at64.sqrt(), (1 - at64).rsqrt(), ato64.sqrt(), sig64,
                                                                  (1 - ato64 - sig64 ** 2).sqrt()))


def tensor():
    e = eps - sq1mat * grad
    x0 = (x - sq1mat * e) * rsat
    x0 = (x0 - x0.mean(dim=1, keepdim=True)).clamp(-1, 1)
    e2 = (x - x0 * sqat) * rs1mat
    return sqto * x0 + ce * e2 + sig * noise


sides = {"ddim_guided": lambda: ddim(grad), "ddim_unguided": lambda: ddim(None), "ddpm_guided": ddpm_guided, "tensor": tensor}
outs = {}
for k, fn in sides.items():  # warm-up: code objects loaded, the allocator's blocks in place
    for _ in range(3):
        outs[k] = fn().clone()
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

res = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "flags": "constrain", "eta": a.eta, "reps": a.reps, "inner": a.inner,
       "library": L.vqvs_version().decode()}
for k in sides:
    med = statistics.median(times[k])
    res[k] = {"us_per_step": [round(t, 2) for t in times[k]], "median_us": round(med, 2),
              "spread": round((max(times[k]) - min(times[k])) / med, 4)}
# what each fused side must move, in [B, T] float32 tensors: the x0 sums read x and eps (and grad); the step reads x, eps (grad), noise
# and writes the state.  The DDPM chain: mean reads 2 and writes 1, guided_eps reads 3 and writes 1, then its own sums (2) and step (3 + 1).
tensors = {"ddim_guided": 3 + 5, "ddim_unguided": 2 + 4, "ddpm_guided": 3 + 4 + 2 + 4}
for k, n in tensors.items():
    res[k]["bytes_per_step"] = 4 * B * T * n
    res[k]["GBps_at_median"] = round(res[k]["bytes_per_step"] / (res[k]["median_us"] * 1e-6) / 1e9, 1)
res["ddim_guided_over_ddpm_guided"] = round(res["ddim_guided"]["median_us"] / res["ddpm_guided"]["median_us"], 4)
res["ddim_guided_over_tensor"] = round(res["ddim_guided"]["median_us"] / res["tensor"]["median_us"], 4)
res["max_abs_diff_ddim_guided_vs_tensor"] = (outs["ddim_guided"] - outs["tensor"]).abs().max().item()
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
