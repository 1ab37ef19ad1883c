"""What packing a corpus buys, same process, the two sides of every comparison alternating:

  (a) the step: one `vqvs_*_step_windows_packed` call against the loop of R calls of the single-recording entry point it replaces, at
      (W, H) = (64000, 57600) and (R, n_r) = 32 x 2, 64 x 1 and 8 x 8, for DDPM (plain and with constrain), DDIM (eta 0.5) and
      DPM-Solver++ (with a history); drawn noise, the next window batch written.  Both sides include what the host spends enqueueing:
      that is the cost the packed call removes.
  (b) end to end: a det_init unet64 VQ-VAE in fp16, DDPM at 50 steps with constrain; 32 recordings of 7 s through one
      `decode_long_batch` against one `decode_long` each.

The outputs of the two sides of every comparison are asserted bitwise equal before anything is timed.  Timing is between device
synchronisations after a warm-up; (a) times --inner consecutive steps per sample and --reps samples per side, (b) --e2e-reps
conversions per side.  The result holds every time, the medians, each side's spread (max - min) / median and the ratios.  One
condition is checked and reported, not tuned for: at 32 x 2 and 64 x 1 the packed call is not slower than its loop
(`packed_not_slower`).  One JSON object on stdout, also written to --out (profiles/convert_dataset_bench.json is where a run belongs)."""
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
from vq_voice_swap_amd.longform import pack_layout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=50, help="steps per timed sample of (a)")
ap.add_argument("--e2e-reps", type=int, default=3, help="conversions per side of (b); 0 skips (b)")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
assert a.reps >= 5, "--reps must be at least 5"
assert torch.cuda.is_available(), "bench_convert_dataset.py measures on the GPU: there is nothing to time without one"
dev = torch.device("cuda:0")
W, H = 64000, 57600
L, ptr = _native.lib(), _native._ptr
a_from, a_t, a_to = (torch.tensor([v], device=dev) for v in (0.24, 0.3, 0.37))
SAMPLERS = {"ddpm": ("ddpm", 0), "ddpm_constrain": ("ddpm", _native.DDPM_CONSTRAIN), "ddim": ("ddim", 0), "dpmpp": ("dpmpp", 0)}


def summary(ts):
    med = statistics.median(ts)
    return {"times": [round(t, 3) for t in ts], "median": round(med, 3), "spread": round((max(ts) - min(ts)) / med, 4)}


def alternate(sides, reps, inner):
    times = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / inner)
    return times


def step_fn(name, packed):
    return getattr(L, f"vqvs_{name}_step_windows" + ("_packed" if packed else ""))


def step(name, flags, packed, geom, x, eps, prev, out, x0, win, clip):
    """One call of either form (`geom`: (d_first, R) or (n,)); drawn noise, step 3 of seed 1."""
    st, fn = _native._stream_ptr(), step_fn(name, packed)
    if name == "ddpm":
        rc = fn(x.data_ptr(), eps.data_ptr(), None, a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), win.data_ptr(), *geom, W, H, flags, 1.0, 1,
                clip, 3, st)
    elif name == "ddim":
        rc = fn(x.data_ptr(), eps.data_ptr(), None, None, a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), win.data_ptr(), *geom, W, H, flags,
                0.5, 1.0, 1, clip, 3, st)
    else:
        rc = fn(x.data_ptr(), eps.data_ptr(), None, prev.data_ptr(), a_from.data_ptr(), a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(),
                x0.data_ptr(), win.data_ptr(), *geom, W, H, flags, st)
    _native.check(rc)


res = {"device": torch.cuda.get_device_name(0), "W": W, "H": H, "reps": a.reps, "inner": a.inner, "library": L.vqvs_version().decode(),
       "step": {}}
for R, n in ((32, 2), (64, 1), (8, 8)):
    counts = [n] * R
    first, offsets, total = pack_layout(counts, W, H)
    N, row = first[-1], (n - 1) * H + W
    d_first = torch.tensor(first, dtype=torch.int32, device=dev)
    x = randn_clips(1, total, dev, 1).view(total)
    prev = (0.3 * randn_clips(1, total, dev, 2).view(total)).clamp(-1, 1)
    eps = randn_clips(N, W, dev, 3).view(N, W)
    outs = {side: (torch.empty_like(x), torch.empty_like(x), torch.empty_like(eps)) for side in ("packed", "loop")}
    case = res["step"][f"{R}x{n}"] = {"R": R, "n": n, "windows": N, "samples": total}
    for tag, (name, flags) in SAMPLERS.items():
        def packed(name=name, flags=flags):
            o, x0, w = outs["packed"]
            step(name, flags, True, (d_first.data_ptr(), R), x, eps, prev, o, x0, w, 7)

        def loop(name=name, flags=flags):
            o, x0, w = outs["loop"]
            for r in range(R):
                sl = slice(offsets[r], offsets[r] + row)
                step(name, flags, False, (n,), x[sl], eps[first[r]:first[r + 1]], prev[sl], o[sl], x0[sl], w[first[r]:first[r + 1]], 7 + r)

        sides = {"packed": packed, "loop": loop}
        for fn in sides.values():  # warm-up: code objects loaded, the scratch buffer in place
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for i, what in enumerate(("x_to", "x0", "windows")):
            if what != "x0" or name == "dpmpp":
                assert torch.equal(outs["packed"][i], outs["loop"][i]), f"{tag} at {R} x {n}: {what} of the packed call is not the loop's"
        times = alternate(sides, a.reps, a.inner)
        r = case[tag] = {k + "_us": summary([t * 1e6 for t in v]) for k, v in times.items()}
        r["launches_packed"], r["launches_loop"] = (1 + bool(flags), R * (1 + bool(flags)))
        r["packed_over_loop"] = round(r["packed_us"]["median"] / r["loop_us"]["median"], 4)
res["packed_not_slower"] = {f"{shape} {tag}": res["step"][shape][tag]["packed_over_loop"] <= 1.0 for shape in ("32x2", "64x1") for tag in SAMPLERS}

if a.e2e_reps:
    R, seconds, steps = 32, 7, 50
    model = VQVAE(base_channels=64, pred_name="unet", num_labels=8)
    det_init_(model.state_dict().items())
    model.eval().to(dev)
    model.set_precision("fp16")
    waves = [(0.3 * randn_clips(1, seconds * 16000, dev, 20 + r)).clamp(-1, 1) for r in range(R)]
    label = torch.tensor([3], device=dev)
    codes, counts = model.encode_long_batch(waves, W, H)
    each = [codes[sum(counts[:r]):sum(counts[:r + 1])] for r in range(R)]
    kw = dict(window=W, hop=H, steps=steps, constrain=True, seed=5)

    def batch():
        return model.decode_long_batch(codes, label, counts=counts, num_samples=[w.shape[-1] for w in waves], clip_offset=100, **kw)

    def one_by_one():
        return [model.decode_long(each[r], label, num_samples=waves[r].shape[-1], clip_offset=100 + r, **kw) for r in range(R)]

    got, want = batch(), one_by_one()  # (the warm-up as well)
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want)), "decode_long_batch is not decode_long of each recording"
    times = alternate({"decode_long_batch": batch, "decode_long_each": one_by_one}, a.e2e_reps, 1)
    e2e = res["end_to_end"] = {"model": "unet64 VQ-VAE, det_init, fp16", "sampler": "ddpm", "steps": steps, "constrain": True, "recordings": R,
                               "seconds_each": seconds, "windows": sum(counts)}
    e2e.update({k + "_s": summary(v) for k, v in times.items()})
    e2e["batch_over_each"] = round(e2e["decode_long_batch_s"]["median"] / e2e["decode_long_each_s"]["median"], 4)
    e2e["audio_seconds_per_second_batch"] = round(R * seconds / e2e["decode_long_batch_s"]["median"], 1)
    e2e["audio_seconds_per_second_each"] = round(R * seconds / e2e["decode_long_each_s"]["median"], 1)
text = json.dumps(res, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
