"""The compiled counter-based normal generator (csrc/philox.hpp) and the seeded sampling paths that draw from it, against the
numpy reference tests/philox_ref.py (itself pinned to the published Philox vectors by tests/test_rng.py):

  a. `vqvs_randn`, every value, over shapes that cross a quad, a 256-thread block and unaligned row starts, seeds and clip offsets
     past 32 bits, and the three stream ids;
  b. the step word (`vqvs_ddpm_step` with generated noise, steps 0 ... 49) and the loss stream (`vqvs_ddpm_noise`);
  c. the generated-noise branch of the step kernel under all four flag combinations, against the CPU oracle's step;
  d. `ddpm_sample` and `sample_clips` with a seed, end to end against the CPU oracle fed the reference's x_T and noises.

No run on an MI355X has been recorded yet: no figure is quoted here and profiles/rng_margins.jsonl does not exist.  A run with
VQVS_RNG_MARGINS=profiles/rng_margins.jsonl writes the measured maxima of a, b, c and d next to their bounds.  On the host, the
generator's header compiled as plain C++ (glibc's float32 sinf / cosf / logf) is within 1.8e-6 of the reference over 192
(seed, clip, step, stream) combinations of 4100 values each."""
import json
import os

import numpy as np
import pytest
import torch

import philox_ref
from oracle import ref_cpu
from vq_voice_swap_amd import DiffusionModel, _native, randn_clips
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule
from vq_voice_swap_amd.sampler import sample_clips

from util import gate, seeded

pytestmark = pytest.mark.gpu

WAVE_RMS = 1e-3  # the project's gate on sampled waveforms (tests/test_parity_gpu.py)
NORMAL_ABS = 1.2e-5  # |device normal - reference normal|: derived in test_randn_every_value_vs_reference
STEP_REL = 2e-6  # the project's bound on one reverse step against the oracle (test_ddpm_previous_vs_golden)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(name, value, bound):
    rec = {"test": name, "max_abs_err": float(value), "bound": float(bound), "fraction_of_bound": float(value / bound)}
    print(f"[margin] {name}: max abs err {value:.3e} (bound {bound:.3e})")
    path = os.environ.get("VQVS_RNG_MARGINS")  # a .jsonl file to append to (profiles/rng_margins.jsonl is such a run)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def guarded(B, T, dev):
    """[B + 1, T] of NaN: B rows for a kernel to fill and one guard row behind them."""
    return torch.full((B + 1, T), float("nan"), device=dev)


def filled_rows(buf, B):
    """The B rows as float64 numpy, after checking that every one of their elements was written and the guard row was not."""
    host = buf.cpu()
    assert torch.isnan(host[B]).all(), "the kernel wrote past its last row"
    assert torch.isfinite(host[:B]).all(), "the kernel left elements of its rows unwritten (or wrote non-finite values)"
    return host[:B].double().numpy()


def randn_call(B, T, seed, clip_offset, stream_id, dev):
    buf = guarded(B, T, dev)
    _native.check(_native.lib().vqvs_randn(buf.data_ptr(), B, T, seed, clip_offset, stream_id, _native._stream_ptr()))
    return filled_rows(buf, B)


def ref_rows(T, seed, clips, stream, step=0):
    return np.concatenate([philox_ref.randn(1, T, seed, int(c), stream, step) for c in clips])


def differ(a, b):
    """Two draws: unrelated values, not a shifted or partly shared copy (equal float32 normals at one index: ~1e-6 of them)."""
    return (a != b).mean() > 0.999 and np.abs(a - b).mean() > 0.5


# ---------------------------------------------------------------- a. vqvs_randn
SHAPES = [(1, 1), (1, 3), (3, 1001), (2, 1028), (2, 4096)]
SEEDS = [0, 5, (1 << 32) + 7, (1 << 63) - 1]
OFFSETS = [0, 3, (1 << 32) + 1]
STREAMS = [0, 1, 2]
# 20 of the 180 combinations: every (shape, seed) pair once (5 and 4 are coprime), every (offset, stream) pair at least twice
RANDN_CASES = [(SHAPES[i % 5], SEEDS[i % 4], OFFSETS[i % 3], STREAMS[(i // 3) % 3]) for i in range(20)]


def test_randn_cases_cover_every_axis_value():
    for axis, values in enumerate((SHAPES, SEEDS, OFFSETS, STREAMS)):
        assert {c[axis] for c in RANDN_CASES} == set(values)


def test_randn_every_value_vs_reference(dev):
    """|got - want| <= 1.2e-5 for every element.  The uniforms are exact (24-bit integers scaled by 2^-24; the float32 rounding of
    "+ 0.5" is part of the definition and the reference makes it too).  The angle 2 pi u carries at most half an ulp of [4, 8)
    (2.4e-7) from the product, the float32 2 pi constant (1.8e-7 at u ~ 1) and about 2 ulp of sincosf: together about 7e-7,
    multiplied by a radius r <= sqrt(-2 ln 2^-25) = 5.89: 4.1e-6.  r itself carries a few 2^-24 relative: 1.4e-6.  Worst case
    about 6e-6, doubled because the device libm's ulp figures are taken from its documentation, not verified: 1.2e-5.  (A float32
    numpy emulation measures 1.7e-6; a wrong draw differs by O(1).)

    (3, 1001) is the shape whose rows 1 and 2 start 4 bytes off a 16-byte boundary while randn_kernel stores whole quads with
    one 16-byte store: gfx950 carries out unaligned global stores, the values here are right, so that kernel keeps its store."""
    worst = 0.0
    for (B, T), seed, off, stream in RANDN_CASES:
        got = randn_call(B, T, seed, off, stream, dev)
        want = philox_ref.randn(B, T, seed, off, stream)
        err = np.abs(got - want).max()
        print(f"randn B={B} T={T} seed={seed:#x} clip_offset={off:#x} stream={stream}: max abs err {err:.3e}")
        assert err <= NORMAL_ABS, ((B, T), seed, off, stream, err)
        worst = max(worst, err)
    record("a vqvs_randn vs reference, 20 cases", worst, NORMAL_ABS)
    # the Python entry point passes its arguments through in this order
    got = randn_clips(3, 1001, dev, SEEDS[2], clip_offset=OFFSETS[2], stream_id=2).cpu().double().numpy().reshape(3, 1001)
    assert np.abs(got - philox_ref.randn(3, 1001, SEEDS[2], OFFSETS[2], 2)).max() <= NORMAL_ABS
    got = randn_clips(2, 1028, dev, 5).cpu().double().numpy().reshape(2, 1028)  # the defaults: clip 0, stream 1 (x_T)
    assert np.abs(got - philox_ref.randn(2, 1028, 5, 0, philox_ref.STREAM_XT)).max() <= NORMAL_ABS


# ---------------------------------------------------------------- b. the step word and the loss stream
def step_call(x, eps, noise, a_t, a_prev, flags, noise_scale, seed, clip_offset, step_index):
    B, T = x.shape
    buf = guarded(B, T, x.device)
    _native.check(_native.lib().vqvs_ddpm_step(x.data_ptr(), eps.data_ptr(), _native._ptr(noise), a_t.data_ptr(), a_prev.data_ptr(),
                                               buf.data_ptr(), B, T, flags, noise_scale, seed, clip_offset, step_index,
                                               _native._stream_ptr()))
    return filled_rows(buf, B)


def noise_call(x0, alpha, idx, B, T, seed, clip_offset):
    buf = guarded(B, T, x0.device)
    _native.check(_native.lib().vqvs_ddpm_noise(x0.data_ptr(), x0.shape[0], alpha.data_ptr(), None, 0, _native._ptr(idx), buf.data_ptr(),
                                                B, T, seed, clip_offset, _native._stream_ptr()))
    return filled_rows(buf, B)


# Per-clip alpha_bar(t), alpha_bar(t - step) whose float32 coefficient arithmetic (sampler_kernels.hip: step_coef) is exact up to
# the last division and the square root: alphas = 1/2, 1/2, 1/4; sigma^2 = (1 - alphas)(1 - a_prev) / (1 - a_t) = 1/3, 1/5, 3/7.
A_T = [0.25, 0.375, 0.125]
A_PREV = [0.5, 0.75, 0.5]
STEP_SEED = (1 << 32) + 7


@pytest.mark.parametrize("B,T", [(3, 1001), (2, 4100)])
@pytest.mark.parametrize("clip_offset", [0, (1 << 32) + 1])
def test_step_word_vs_reference(dev, B, T, clip_offset):
    """x_t = 0, eps = 0, no flags, noise_scale = 1: the step kernel returns sigma z.  Divided by sigma (float64, from the same
    alpha values) it is z of (seed, clip, step s, stream 0) within the bound of a plus 3 * 2^-24 |z|: sigma^2 and sigma are each
    rounded once on the device (the rest of the coefficient arithmetic is exact for these alphas): 1.5 * 2^-24 relative in sigma;
    the product sigma z is rounded once more."""
    zero = torch.zeros(B, T, device=dev)
    a_t, a_prev = torch.tensor(A_T[:B], device=dev), torch.tensor(A_PREV[:B], device=dev)
    at64, ap64 = np.array(A_T[:B]), np.array(A_PREV[:B])
    sig = np.sqrt((1 - at64 / ap64) * (1 - ap64) / (1 - at64))[:, None]
    clips = [clip_offset + b for b in range(B)]
    worst, draws = 0.0, {}
    for s in (0, 1, 7, 49, 2, 8, 50):
        got = step_call(zero, zero, None, a_t, a_prev, 0, 1.0, STEP_SEED, clip_offset, s) / sig
        draws[s] = got
        if s in (2, 8, 50):  # only drawn as the successors of 1, 7 and 49
            continue
        want = ref_rows(T, STEP_SEED, clips, philox_ref.STREAM_STEP, step=s)
        excess = np.abs(got - want) - 3 * 2.0 ** -24 * np.abs(want)
        print(f"step word B={B} T={T} clip_offset={clip_offset:#x} step={s}: max abs err {np.abs(got - want).max():.3e}")
        assert excess.max() <= NORMAL_ABS, (s, excess.max())
        worst = max(worst, excess.max())
    record(f"b step word vs reference B={B} T={T} clip_offset={clip_offset:#x} (less 3 * 2^-24 |z|)", worst, NORMAL_ABS)
    # steps s and s + 1 are different draws (it follows from the comparison above; asserted anyway) ...
    for s in (0, 1, 7, 49):
        assert differ(draws[s], draws[s + 1]), s
    # ... and so are streams 0 (this kernel), 1 and 2 (vqvs_randn) of the same seed, clips and step 0
    by_stream = [draws[0]] + [randn_call(B, T, STEP_SEED, clip_offset, k, dev) for k in (1, 2)]
    z0 = randn_call(B, T, STEP_SEED, clip_offset, 0, dev)  # stream 0 at step 0 is vqvs_randn's stream 0: the same device normals
    assert (np.abs(draws[0] - z0) <= 3 * 2.0 ** -24 * np.abs(z0)).all()
    for i in range(3):
        for j in range(i + 1, 3):
            assert differ(by_stream[i], by_stream[j]), (i, j)


@pytest.mark.parametrize("B,T", [(3, 1001), (2, 4100)])
def test_loss_stream_vs_reference(dev, B, T):
    """x_0 = 0 and alpha_bar = 0: `vqvs_ddpm_noise` returns 0 * 0 + 1 * eps, the generated epsilon itself (stream 2, step 0), at the
    clips its noise_index tensor names -- or clip_offset + row without one."""
    x0, alpha = torch.zeros(1, T, device=dev), torch.zeros(B, device=dev)
    seed = (1 << 63) - 1
    clips = [(1 << 32) + 1, 0, 7][:B]
    idx = torch.tensor(clips, dtype=torch.int64, device=dev)
    got = noise_call(x0, alpha, idx, B, T, seed, 1234)  # (the offset is not used when indices are given)
    err = np.abs(got - ref_rows(T, seed, clips, philox_ref.STREAM_LOSS)).max()
    off = (1 << 32) + 1
    got_off = noise_call(x0, alpha, None, B, T, seed, off)
    err_off = np.abs(got_off - philox_ref.randn(B, T, seed, off, philox_ref.STREAM_LOSS)).max()
    record(f"b loss stream vs reference B={B} T={T}", max(err, err_off), NORMAL_ABS)
    assert err <= NORMAL_ABS and err_off <= NORMAL_ABS, (err, err_off)
    assert np.array_equal(got[0], got_off[0])  # the same clip, named either way
    # streams 0, 1 and 2 of the same seed and clips are different draws
    by_stream = [randn_call(B, T, seed, off, k, dev) for k in (0, 1)] + [got_off]
    for i in range(3):
        for j in range(i + 1, 3):
            assert differ(by_stream[i], by_stream[j]), (i, j)


# ---------------------------------------------------------------- c. generated noise in the step kernel, all flags
@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("T", [1001, 4101])
def test_generated_noise_step_vs_oracle(dev, schedule, T):
    """`ddpm_previous` with noise=None against the CPU oracle's step fed the reference normals (as float32).  Bound: the project's
    own 2e-6 * max(1, max |want|) for this kernel with explicit noise (test_ddpm_previous_vs_golden), plus the 1.2e-5 of a for the
    device's normals, which enter multiplied by sigma <= 1.  T = 4101: two partial sums of the constrain mean, the second ragged."""
    B, seed, off = 3, (1 << 32) + 7, 5
    d = Diffusion(make_schedule(schedule))
    x, eps = seeded((B, 1, T), 31), seeded((B, 1, T), 32)
    ts = torch.tensor([0.9, 0.5, 0.2])
    xd, ed, tsd = x.to(dev), eps.to(dev), ts.to(dev)
    worst = 0.0
    for step_index in (0, 7):
        noise = torch.from_numpy(philox_ref.randn(B, T, seed, off, philox_ref.STREAM_STEP, step=step_index).astype(np.float32)).view(B, 1, T)
        for sigma_large in (False, True):
            for constrain in (False, True):
                kw = dict(sigma_large=sigma_large, constrain=constrain)
                want = ref_cpu.ddpm_previous(schedule, x, ts, 0.05, eps, noise, **kw)
                bound = STEP_REL * max(1.0, want.abs().max().item()) + NORMAL_ABS
                got = d.ddpm_previous(xd, tsd, 0.05, ed, seed=seed, clip_offset=off, step_index=step_index, **kw).cpu()
                given = d.ddpm_previous(xd, tsd, 0.05, ed, noise=noise.to(dev), **kw).cpu()
                errs = [(got - want).abs().max().item(), (given - want).abs().max().item(), (got - given).abs().max().item()]
                print(f"step {schedule} T={T} step_index={step_index} {kw}: generated vs oracle {errs[0]:.3e}, given vs oracle {errs[1]:.3e}, "
                      f"generated vs given {errs[2]:.3e} (bound {bound:.3e})")
                assert max(errs) <= bound, (step_index, kw, errs, bound)
                worst = max(worst, max(errs) / bound)
                # without noise the generator is out of the picture: bitwise what explicit zeros give
                assert torch.equal(d.ddpm_previous(xd, tsd, 0.05, ed, seed=seed, clip_offset=off, step_index=step_index, noise_scale=0.0, **kw),
                                   d.ddpm_previous(xd, tsd, 0.05, ed, noise=torch.zeros_like(xd), **kw))
    record(f"c generated-noise step vs oracle {schedule} T={T} (largest fraction of 2e-6 max(1, |want|) + 1.2e-5)", worst, 1.0)


# ---------------------------------------------------------------- d. the seeded sampler end to end
def test_seeded_sampler_end_to_end_vs_oracle(dev):
    """The oracle's sampler fed x_T = stream 1 and noises[i] = stream 0 at step i of the reference generator, against the HIP
    sampler given only the seed: fails if `ddpm_sample` numbers its steps or clips differently, or x_T shares a stream with a step."""
    B, T, steps, seed = 3, 4096, 10, 99
    model = DiffusionModel("unet", 32)
    det_init_(model.state_dict().items())
    model.eval()
    model.set_precision("fp32")
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def oracle(off):
        def f32(a):
            return torch.from_numpy(a.astype(np.float32)).view(B, 1, T)

        x_T = f32(philox_ref.randn(B, T, seed, off, philox_ref.STREAM_XT))
        noises = [f32(philox_ref.randn(B, T, seed, off, philox_ref.STREAM_STEP, step=i)) for i in range(steps)]
        return ref_cpu.ddpm_sample("exp", x_T, lambda a, b: ref_cpu.unet_predictor(sd, 32, a, b), steps, noises, constrain=True)

    got = model.diffusion.ddpm_sample(randn_clips(B, T, dev, seed, clip_offset=6), model.predictor, steps, constrain=True, seed=seed,
                                      clip_offset=6).cpu()
    name = "d seeded ddpm_sample unet32 fp32, clips 6..8, vs oracle on reference draws"
    record(name, gate(name, got, oracle(6), WAVE_RMS), WAVE_RMS)
    got = sample_clips(model, B, T, steps, seed, constrain=True, gather=False).cpu()
    name = "d seeded sample_clips unet32 fp32, clips 0..2, vs oracle on reference draws"
    record(name, gate(name, got, oracle(0), WAVE_RMS), WAVE_RMS)
