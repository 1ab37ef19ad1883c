"""Time of the DPM-Solver++(2M) step kernels, constrain on, the gradient of a guided step given as a tensor (the guidance model's own
time is not part of any side), same process, the sides alternating:

  at (B, T) = (64, 64000)
  fused_{second,first}_{guided,unguided}   `vqvs_dpmpp_step` with / without the history (x0_prev, alpha_from) and with / without a
                                           gradient: one x0-sum launch and one step launch, both outputs written
  tensor_{second,first}_{guided,unguided}  the same step written as torch tensor expressions (coefficients prepared once, outside the
                                           timed region), both outputs
  ddim_unguided                            `vqvs_ddim_step` at eta = 0 without a gradient: the first-order step the sampler replaces
  at (n, W, H) = (167, 64000, 57600): a 10-minute recording at 16 kHz in 4 s windows with 0.4 s of overlap
  windows_second_guided, windows_first_unguided   `vqvs_dpmpp_step_windows`, the history in the long layout, the next window batch written

Each timed sample is --inner consecutive steps between two device synchronisations; each side runs --reps samples (at least 5)
after a warm-up.  The result holds every per-step time, the medians, each side's spread (max - min) / median, the bytes each fused
side must move, from the shapes, and the largest difference between each fused clip side and its tensor side.  No ratio is promised
or gated: the file records what was found.  One JSON object on stdout, also written to --out when given (profiles/dpmpp_bench.json
is where a run belongs)."""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import argparse
import json
import math
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
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
assert torch.cuda.is_available(), "bench_dpmpp.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
B, T = 64, 64000
n, W, H = 167, 64000, 57600
Np = (n - 1) * H + W
A_FROM, A_T, A_TO = 0.24, 0.3, 0.37
L = _native.lib()
CONSTRAIN = _native.DDIM_CONSTRAIN
ptr = _native._ptr

x, eps, grad = (randn_clips(B, T, dev, s).view(B, T) for s in (1, 2, 3))
prev = (0.3 * randn_clips(B, T, dev, 4).view(B, T)).clamp(-1, 1)
a_from, a_t, a_to = (torch.full((B,), v, device=dev) for v in (A_FROM, A_T, A_TO))
out, x0 = torch.empty_like(x), torch.empty_like(x)


def fused(second, guided):
    _native.check(L.vqvs_dpmpp_step(x.data_ptr(), eps.data_ptr(), ptr(grad if guided else None), ptr(prev if second else None),
                                    ptr(a_from if second else None), a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), x0.data_ptr(), B, T,
                                    CONSTRAIN, _native._stream_ptr()))
    return out, x0


def ddim_unguided():
    _native.check(L.vqvs_ddim_step(x.data_ptr(), eps.data_ptr(), None, None, a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), B, T, CONSTRAIN,
                                   0.0, 1.0, 0, 0, 0, _native._stream_ptr()))
    return out, None


# the tensor side: the coefficients in float64 from the float32 alphas, rounded once, as the kernel forms them
def lam(v):
    return 0.5 * (math.log(v) - math.log1p(-v))


af, at, ato = (float(torch.tensor(v, dtype=torch.float32)) for v in (A_FROM, A_T, A_TO))
sq1mat, rsat = math.sqrt(1 - at), 1 / math.sqrt(at)
cx = math.sqrt(1 - ato) / math.sqrt(1 - at)
phi = math.sqrt(ato) - math.sqrt(1 - ato) * math.sqrt(at) / math.sqrt(1 - at)
q = (lam(ato) - lam(at)) / (2 * (lam(at) - lam(af)))


def tensor(second, guided):
    e = eps - sq1mat * grad if guided else eps
    p0 = (x - sq1mat * e) * rsat
    p0 = (p0 - p0.mean(dim=1, keepdim=True)).clamp(-1, 1)
    if second:
        return cx * x + (phi * (1 + q)) * p0 + (-phi * q) * prev, p0
    return cx * x + phi * p0, p0


# the windows form
xl = randn_clips(1, Np, dev, 5).view(Np)
epsw, gradw = (randn_clips(n, W, dev, s).view(n, W) for s in (6, 7))
prevl = (0.3 * randn_clips(1, Np, dev, 8).view(Np)).clamp(-1, 1)
outl, x0l, windows = torch.empty_like(xl), torch.empty_like(xl), torch.empty_like(epsw)


def fused_windows(second, guided):
    _native.check(L.vqvs_dpmpp_step_windows(xl.data_ptr(), epsw.data_ptr(), ptr(gradw if guided else None), ptr(prevl if second else None),
                                            ptr(a_from if second else None), a_t.data_ptr(), a_to.data_ptr(), outl.data_ptr(), x0l.data_ptr(),
                                            windows.data_ptr(), n, W, H, CONSTRAIN, _native._stream_ptr()))
    return outl, x0l


sides = {}
for second in (True, False):
    for guided in (True, False):
        tag = f"{'second' if second else 'first'}_{'guided' if guided else 'unguided'}"
        sides["fused_" + tag] = lambda s=second, g=guided: fused(s, g)
        sides["tensor_" + tag] = lambda s=second, g=guided: tensor(s, g)
sides["ddim_unguided"] = ddim_unguided
sides["windows_second_guided"] = lambda: fused_windows(True, True)
sides["windows_first_unguided"] = lambda: fused_windows(False, False)
outs = {}
for k, fn in sides.items():  # warm-up: code objects loaded, the allocator's blocks in place
    for _ in range(3):
        outs[k] = [None if t is None else t.clone() for t in fn()]
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

res = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "n": n, "W": W, "H": H, "Np": Np, "flags": "constrain", "reps": a.reps,
       "inner": a.inner, "library": L.vqvs_version().decode()}
for k in sides:
    med = statistics.median(times[k])
    res[k] = {"us_per_step": [round(t, 2) for t in times[k]], "median_us": round(med, 2),
              "spread": round((max(times[k]) - min(times[k])) / med, 4)}
# what each fused side must move, in float32 values: the x0 sums read x and eps (and grad); the step reads x, eps (grad, x0_prev) and
# writes x_to and x0 (the windows form: the long rows and the window batches, the next window batch as well)
for second in (True, False):
    for guided in (True, False):
        tag = f"{'second' if second else 'first'}_{'guided' if guided else 'unguided'}"
        r = res["fused_" + tag]
        r["bytes_per_step"] = 4 * B * T * ((2 + guided) + (2 + guided + second) + 2)
        r["GBps_at_median"] = round(r["bytes_per_step"] / (r["median_us"] * 1e-6) / 1e9, 1)
        r["over_tensor"] = round(r["median_us"] / res["tensor_" + tag]["median_us"], 4)
        for i, name in enumerate(("x_to", "x0")):
            r["max_abs_diff_vs_tensor_" + name] = (outs["fused_" + tag][i] - outs["tensor_" + tag][i]).abs().max().item()
res["ddim_unguided"]["bytes_per_step"] = 4 * B * T * (2 + 2 + 1)
res["ddim_unguided"]["GBps_at_median"] = round(res["ddim_unguided"]["bytes_per_step"] / (res["ddim_unguided"]["median_us"] * 1e-6) / 1e9, 1)
res["fused_first_unguided_over_ddim_unguided"] = round(res["fused_first_unguided"]["median_us"] / res["ddim_unguided"]["median_us"], 4)
for k, second, guided in (("windows_second_guided", 1, 1), ("windows_first_unguided", 0, 0)):
    r = res[k]
    r["bytes_per_step"] = 4 * ((1 + guided) * n * W + n * W + ((1 + second) * Np + (1 + guided) * n * W) + (2 * Np + n * W))
    r["GBps_at_median"] = round(r["bytes_per_step"] / (r["median_us"] * 1e-6) / 1e9, 1)
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
