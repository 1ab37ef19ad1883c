"""Time of the keep-region kernels against the same operation written as torch tensor expressions, same process, the sides alternating:

  single    (B, T) = (64, 64000), seconds 1 .. 3 of every 4 s clip kept
    fused   `vqvs_keep_region` in place, the noise drawn in the kernel
    tensor  torch.where(keep, ca * x0 + cn * torch.randn_like(x0), x)
  windows   one 10-minute state at 16 kHz in windows of 4 s with 0.4 s overlap, 10 s of every 30 s kept
    fused   `vqvs_keep_region_windows` in place on the long state and on the window batch
    tensor  the same torch.where on the long state, then the window batch gathered again (`gather_windows`)

Each timed sample is --inner consecutive calls between two device synchronisations; each side runs --reps samples (at least 5) after
a warm-up.  The result holds every per-call time, the medians, each side's spread (max - min) / median and the bytes the fused side must
move, from the shapes and the mask.  No ratio is promised or gated: the file records what was found.  One JSON object on stdout, also
written to --out when given (profiles/keep_bench.json is where a run belongs)."""
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

from vq_voice_swap_amd import _native, plan_windows, randn_clips  # noqa: E402
from vq_voice_swap_amd.longform import gather_windows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=100, help="calls per timed sample")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
assert torch.cuda.is_available(), "bench_keep.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
L = _native.lib()
RATE, ALPHA = 16000, 0.3
CA, CN = float(torch.tensor(ALPHA, dtype=torch.float64).sqrt().float()), float((1 - torch.tensor(ALPHA, dtype=torch.float64)).sqrt().float())

# ---- single clips
B, T = 64, 64000
x, x0 = (randn_clips(B, T, dev, s).view(B, T) for s in (1, 2))
keep = torch.zeros(B, T, dtype=torch.bool, device=dev)
keep[:, 1 * RATE:3 * RATE] = True
keep_u8 = keep.to(torch.uint8)
alpha = torch.full((B,), ALPHA, device=dev)


def single_fused():
    _native.check(L.vqvs_keep_region(x.data_ptr(), x0.data_ptr(), keep_u8.data_ptr(), None, alpha.data_ptr(), B, T, 1.0, 0, 0, 0,
                                     _native._stream_ptr()))
    return x


def single_tensor():
    return torch.where(keep, CA * x0 + CN * torch.randn_like(x0), x)


# ---- one long state
W, H = 4 * RATE, 4 * RATE - 6400
n, Np = plan_windows(600 * RATE, W, H)
xl, x0l = (randn_clips(1, Np, dev, s).view(Np) for s in (3, 4))
keepl = torch.zeros(Np, dtype=torch.bool, device=dev)
for t0 in range(0, Np, 30 * RATE):
    keepl[t0 + 10 * RATE:t0 + 20 * RATE] = True
keepl_u8 = keepl.to(torch.uint8)
windows = gather_windows(xl, W, H)
alpha1 = torch.full((1,), ALPHA, device=dev)


def windows_fused():
    _native.check(L.vqvs_keep_region_windows(xl.data_ptr(), windows.data_ptr(), x0l.data_ptr(), keepl_u8.data_ptr(), None, alpha1.data_ptr(),
                                             n, W, H, 1.0, 0, 0, 0, _native._stream_ptr()))
    return xl


def windows_tensor():
    new = torch.where(keepl, CA * x0l + CN * torch.randn_like(x0l), xl)
    return new, gather_windows(new, W, H)


sides = {"single_fused": single_fused, "single_tensor": single_tensor, "windows_fused": windows_fused, "windows_tensor": windows_tensor}
for fn in sides.values():  # warm-up: code objects loaded, the allocator's blocks in place
    for _ in range(3):
        fn()
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

res = {"device": torch.cuda.get_device_name(0), "alpha": ALPHA, "reps": a.reps, "inner": a.inner, "library": L.vqvs_version().decode(),
       "single": {"B": B, "T": T, "kept_fraction": round(float(keep.float().mean()), 4)},
       "windows": {"n": n, "W": W, "H": H, "Np": Np, "kept_fraction": round(float(keepl.float().mean()), 4)}}
for k in sides:
    med = statistics.median(times[k])
    res[k] = {"us_per_call": [round(t, 2) for t in times[k]], "median_us": round(med, 2),
              "spread": round((max(times[k]) - min(times[k])) / med, 4)}
# what the fused sides must move: every mask byte; per kept sample the source (4 bytes) and the state written (4), and in the windows
# form each window copy as well (every kept sample of an overlap has two)
kept1 = int(keep.sum())
res["single_fused"]["bytes_per_call"] = B * T + 8 * kept1
keptl = int(keepl.sum())
copies = int(gather_windows(keepl_u8.float(), W, H).sum())
res["windows_fused"]["bytes_per_call"] = Np + 8 * keptl + 4 * copies
for k in ("single_fused", "windows_fused"):
    res[k]["GBps_at_median"] = round(res[k]["bytes_per_call"] / (res[k]["median_us"] * 1e-6) / 1e9, 1)
res["single_fused_over_tensor"] = round(res["single_fused"]["median_us"] / res["single_tensor"]["median_us"], 4)
res["windows_fused_over_tensor"] = round(res["windows_fused"]["median_us"] / res["windows_tensor"]["median_us"], 4)
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
