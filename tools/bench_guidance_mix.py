"""Time of the guidance mix `vqvs_guidance_mix` against the chain of tensor expressions it replaced in `VQVAE.decode_uncond_guidance`
(pred = base; pred = pred + scale * (base - outs[k * n:(k + 1) * n]) per guidance term), same process, the sides alternating:

  mix       (rows, row_len) = (64, 64000), reps 2 and 3
    kernel  `vqvs_guidance_mix` into a buffer of its own (the decoder calls it in place over block 0: the same reads and writes, but
            repeated in place the values would run away)
    chain   the expressions: per term a subtraction, a product and a sum, each a pass over the state with its own temporary
  both WARM -- the same buffers call after call: 16 MB per block, the whole batch stays in the 256 MiB Infinity Cache -- and COLD --
  the calls walk enough buffer sets that --cold-mib (600) MiB lie between two uses of a line, so every read comes from HBM;

  step      one guided step of a decode: the predictor's forward on the reps-fold batch (--batch clips of 64000 samples, base 32, fp32,
            the mode guidance runs in) and the mix behind it, each timed on its own; the mix's share of the two is reported.

Each timed sample is --inner consecutive calls between two device synchronisations; each side runs --reps samples (at least 5) after a
warm-up.  The result holds every per-call time, the medians, each side's spread (max - min) / median, the bytes each side must move
(kernel: reps reads and a write per element; chain: per term a subtraction -- two reads, a write --, a product -- a read, a write -- and
a sum -- two reads, a write --: 8 passes) and the rates at the medians.  On the cold sides the inputs are cold; the kernel's output
buffer and the chain's temporaries, which the allocator hands back call after call, are not.  No ratio is promised or gated: the file
records what was found.  One JSON object on stdout, also written to --out when given (profiles/guidance_mix_bench.json is where a run
belongs)."""
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

from vq_voice_swap_amd import VQVAE, _native, randn_clips  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402
from vq_voice_swap_amd.diffusion import guidance_mix  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=100, help="calls per timed sample")
ap.add_argument("--cold-mib", type=int, default=600, help="bytes between two uses of a buffer on the cold sides (the Infinity Cache holds 256 MiB)")
ap.add_argument("--batch", type=int, default=16, help="clips of the guided step")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
assert torch.cuda.is_available(), "bench_guidance_mix.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
L = _native.lib()
ROWS, LEN = 64, 64000
S1, S2 = 1.5, 0.7


def chain(outs, n, reps):
    base = outs[:n]
    pred = base
    for k, scale in zip(range(1, reps), (S1, S2)):
        pred = pred + scale * (base - outs[k * n:(k + 1) * n])
    return pred


eps = torch.empty(ROWS, LEN, device=dev)


def kernel(outs, n, reps):
    return guidance_mix(outs, reps, S1, S2, out=eps)


sides, counters = {}, {}
for reps in (2, 3):
    sets = -(-(a.cold_mib << 20) // (reps * ROWS * LEN * 4)) + 1
    bufs = [randn_clips(reps * ROWS, LEN, dev, 10 * reps + s).view(reps * ROWS, LEN) for s in range(sets)]
    for name, fn in (("kernel", kernel), ("chain", chain)):
        sides[f"{name}_reps{reps}_warm"] = lambda fn=fn, reps=reps, b=bufs[0]: fn(b, ROWS, reps)

        def cold(fn=fn, reps=reps, bufs=bufs, key=f"{name}_reps{reps}_cold"):
            counters[key] = (counters.get(key, -1) + 1) % len(bufs)
            return fn(bufs[counters[key]], ROWS, reps)

        sides[f"{name}_reps{reps}_cold"] = cold

# ---- one guided step: the forward on the reps-fold batch, and the mix behind it
model = VQVAE(base_channels=32, pred_name="unet", num_labels=4)
det_init_(model.state_dict().items())
model.to(dev).eval().set_precision("fp32")
B = a.batch
xs = randn_clips(B, LEN, dev, 99)
ts = torch.full((B,), 0.5, device=dev)
cond = randn_clips(B, model.cond_channels * (LEN // 256), dev, 98).view(B, model.cond_channels, LEN // 256)
labels = torch.arange(B, device=dev) % 3 + 1
step_outs = {}
for reps in (2, 3):
    x_b, t_b = torch.cat([xs] * reps), torch.cat([ts] * reps)
    c_b = torch.cat([cond] + [torch.zeros_like(cond)] * (reps - 2) + [cond])
    l_b = torch.cat([labels] * (reps - 1) + [torch.zeros_like(labels)])
    sides[f"step_forward_reps{reps}"] = lambda x_b=x_b, t_b=t_b, c_b=c_b, l_b=l_b: model.predictor(x_b, t_b, cond=c_b, labels=l_b)
    step_outs[reps] = model.predictor(x_b, t_b, cond=c_b, labels=l_b)
    step_eps = torch.empty(B, 1, LEN, device=dev)
    sides[f"step_mix_reps{reps}"] = lambda reps=reps, step_eps=step_eps: guidance_mix(step_outs[reps], reps, S1, S2, out=step_eps)

for fn in sides.values():  # warm-up: code objects loaded, the allocator's blocks in place
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
model.predictor.check_status()
times = {k: [] for k in sides}
for _ in range(a.reps):
    for k, fn in sides.items():
        inner = max(1, a.inner // 10) if k.startswith("step_forward") else a.inner
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / inner * 1e6)

res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "cold_mib": a.cold_mib, "library": L.vqvs_version().decode(),
       "mix": {"rows": ROWS, "row_len": LEN, "scales": [S1, S2]},
       "step": {"batch": B, "T": LEN, "base_channels": 32, "precision": "fp32"}}
for k in sides:
    med = statistics.median(times[k])
    res[k] = {"us_per_call": [round(t, 2) for t in times[k]], "median_us": round(med, 2), "spread": round((max(times[k]) - min(times[k])) / med, 4)}
block = ROWS * LEN * 4
for reps in (2, 3):
    for temp in ("warm", "cold"):
        kern, ch = res[f"kernel_reps{reps}_{temp}"], res[f"chain_reps{reps}_{temp}"]
        kern["bytes_per_call"] = (reps + 1) * block        # reps reads and one write per element
        ch["bytes_per_call"] = 8 * (reps - 1) * block      # per term: sub (2 reads, 1 write), mul (1, 1), add (2, 1)
        for side in (kern, ch):
            side["GBps_at_median"] = round(side["bytes_per_call"] / (side["median_us"] * 1e-6) / 1e9, 1)
        res[f"kernel_over_chain_reps{reps}_{temp}"] = round(kern["median_us"] / ch["median_us"], 4)
    fwd, mix = res[f"step_forward_reps{reps}"]["median_us"], res[f"step_mix_reps{reps}"]["median_us"]
    res[f"step_mix_share_reps{reps}"] = round(mix / (fwd + mix), 5)
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
