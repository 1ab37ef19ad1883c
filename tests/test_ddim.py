"""The DDIM sampler, host side: exports, declarations and argument checks of `vqvs_ddim_step` / `vqvs_ddim_step_windows`; the
float64 oracle tests/ddim_ref.py against the reference-pinned `oracle.ref_cpu.ddpm_previous` at eta = 1, and against itself
(inversion); the kernel's float32 arithmetic, restated in numpy, against the bound the GPU test applies; `ddim_invert`'s table walk and
the scripts' new flags (none of this needs a device)."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

import ddim_ref
import vq_voice_swap_amd
from oracle import ref_cpu
from vq_voice_swap_amd import _native
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

from util import flags_of, seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_REL = {"exp": 2e-6, "cos": 4e-6}  # the project's gates for the DDPM step's arithmetic (tests/test_longform_gpu.py)

STEP_ARGS = ["const float* d_x_t", "const float* d_eps", "const float* d_grad", "const float* d_noise", "const float* d_alpha_t",
             "const float* d_alpha_to", "float* d_x_to", "int B", "int T", "uint32_t flags", "float eta", "float noise_scale", "uint64_t seed",
             "uint64_t clip_offset", "uint32_t step_index", "void* stream"]
WINDOWS_ARGS = ["const float* d_x", "const float* d_eps", "const float* d_grad", "const float* d_noise", "const float* d_alpha_t",
                "const float* d_alpha_to", "float* d_x_to", "float* d_windows", "int n", "int W", "int H", "uint32_t flags", "float eta",
                "float noise_scale", "uint64_t seed", "uint64_t clip", "uint32_t step_index", "void* stream"]


# ---------------------------------------------------------------- 1. exports, declarations, refusals
def test_symbols_are_exported_and_declared(lib_built):
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    for name, want in (("vqvs_ddim_step", STEP_ARGS), ("vqvs_ddim_step_windows", WINDOWS_ARGS)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl, f"include/vqvs.h does not declare {name}"
        assert [a.strip() for a in " ".join(decl.group(1).split()).split(",")] == want
        assert len(getattr(lib_built, name).argtypes) == len(want)
    assert re.search(r"#define VQVS_DDIM_CONSTRAIN 2u", header) and re.search(r"#define VQVS_DDIM_INVERT 4u", header)
    assert (_native.DDIM_CONSTRAIN, _native.DDIM_INVERT) == (2, 4) and _native.DDIM_CONSTRAIN == _native.DDPM_CONSTRAIN
    for method in ("ddim_previous", "ddim_sample", "ddim_invert", "ddim_sample_windows"):
        assert callable(getattr(vq_voice_swap_amd.Diffusion, method))
    assert callable(vq_voice_swap_amd.VQVAE.invert)


def host_buffers(count, floats=64):
    bufs = [(C.c_float * floats)() for _ in range(count)]
    return bufs, [C.cast(b, C.c_void_p) for b in bufs]


def test_step_refuses_bad_arguments_without_a_device(lib_built):
    """Every refusal of include/vqvs.h: VQVS_ERR_ARG with host-only pointers, which a call that reached the device would fault on."""
    L = lib_built
    keep, (x, eps, grad, noise, a_t, a_to, out) = host_buffers(7)
    ok = dict(x=x, eps=eps, grad=grad, noise=noise, a_t=a_t, a_to=a_to, out=out, B=2, T=16, flags=0, eta=0.0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_ddim_step(a["x"], a["eps"], a["grad"], a["noise"], a["a_t"], a["a_to"], a["out"], a["B"], a["T"], a["flags"], a["eta"],
                                1.0, 1, 2, 3, None)

    inside = C.c_void_p(eps.value + 16)
    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_to=None), dict(out=None),
                dict(B=0), dict(B=-1), dict(T=0), dict(T=-4), dict(B=65536), dict(T=(1 << 30) + 1),
                dict(eta=-0.5), dict(eta=float("nan")), dict(eta=float("inf")),
                dict(flags=1), dict(flags=3), dict(flags=8), dict(flags=1 << 31),
                dict(flags=6),                    # INVERT with CONSTRAIN
                dict(flags=4, eta=0.5),           # INVERT with eta != 0
                dict(out=x), dict(out=eps), dict(out=grad), dict(out=noise), dict(out=inside),
                dict(grad=None, noise=None, x=None)):  # the optional arguments do not switch the checks off
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(flags=1) == -1 and b"flags" in L.vqvs_last_error()
    assert call(flags=6) == -1 and b"CONSTRAIN" in L.vqvs_last_error()
    assert call(flags=4, eta=0.5) == -1 and b"eta" in L.vqvs_last_error()
    assert call(out=eps) == -1 and b"overlap" in L.vqvs_last_error()
    assert call(eta=-0.5) == -1 and b"eta" in L.vqvs_last_error()


def test_windows_refuses_bad_arguments_without_a_device(lib_built):
    """The limits of `vqvs_ddpm_step_windows` (tests/test_longform.py) and the eta / flag rules of `vqvs_ddim_step`."""
    L = lib_built
    keep, (x, eps, grad, noise, a_t, a_to, out, win) = host_buffers(8)
    ok = dict(x=x, eps=eps, grad=grad, noise=noise, a_t=a_t, a_to=a_to, out=out, win=None, n=3, W=16, H=12, flags=2, eta=0.5)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_ddim_step_windows(a["x"], a["eps"], a["grad"], a["noise"], a["a_t"], a["a_to"], a["out"], a["win"], a["n"], a["W"], a["H"],
                                        a["flags"], a["eta"], 1.0, 1, 2, 3, None)

    inside = C.c_void_p(x.value + 16)
    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_to=None), dict(out=None),
                dict(n=0), dict(n=-1), dict(n=65536),
                dict(W=18, H=12), dict(W=16, H=10), dict(W=0, H=0), dict(W=16, H=0), dict(W=-16, H=-12), dict(W=16, H=-4),
                dict(W=12, H=16), dict(W=28, H=12),
                dict(n=65535, W=65536, H=32768), dict(n=40000, W=1 << 20, H=1 << 19),
                dict(out=x), dict(out=inside), dict(out=grad), dict(win=eps), dict(win=out),
                dict(eta=-1.0), dict(eta=float("nan")), dict(flags=1), dict(flags=3), dict(flags=16), dict(flags=6, eta=0.0),
                dict(flags=4, eta=0.5),
                dict(noise=None, grad=None, x=None), dict(win=win, n=0)):
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(n=65536) == -1 and b"65535" in L.vqvs_last_error()
    assert call(W=28, H=12) == -1 and b"overlap" in L.vqvs_last_error()
    assert call(x=None) == -1 and b"non-NULL" in L.vqvs_last_error()


# ---------------------------------------------------------------- 2. the oracle at eta = 1 is the pinned DDPM step
@pytest.mark.parametrize("schedule", ["exp", "cos"])
def test_oracle_at_eta_one_is_the_reference_ddpm_step(schedule):
    """eta = 1: sig^2 = (1 - a_t / a_to)(1 - a_to) / (1 - a_t) is the DDPM small sigma^2 and sqrt(a_to) x0 + sqrt(1 - a_to - sig^2) e is
    its mean, so the float64 oracle and the float32 `ref_cpu.ddpm_previous` differ by the latter's rounding alone: inside the project's
    gates for that arithmetic, 2e-6 (cos: 4e-6) * max(1, max |want|), at the t of tests/test_longform.py, plain and constrained.
    With a cond_fn the two do NOT agree and nothing is asserted: the DDPM path guides the posterior MEAN, with the gradient taken at
    (mean, t - step), while the DDIM step guides the prediction with the gradient at (x_t, t).  They coincide only to first order in
    the step."""
    W = 4352
    x, eps, noise = seeded((1, 1, W), 1), seeded((1, 1, W), 2), seeded((1, 1, W), 3)
    flat = [v.numpy().reshape(1, W) for v in (x, eps, noise)]
    for t, step in ((0.6, 0.02), (0.3, 0.02)):
        ts = torch.tensor([t], dtype=torch.float32)
        a_t, a_to = ref_cpu.schedule_alpha(schedule, ts).numpy(), ref_cpu.schedule_alpha(schedule, ts - step).numpy()
        for constrain in (False, True):
            want = ref_cpu.ddpm_previous(schedule, x, ts, step, eps, noise, constrain=constrain).reshape(-1).numpy()
            got, _, _ = ddim_ref.step(flat[0], flat[1], a_t, a_to, noise=flat[2], eta=1.0, constrain=constrain)
            err, bound = np.abs(got[0] - want).max(), STEP_REL[schedule] * max(1.0, np.abs(want).max())
            print(f"ddim_ref eta=1 vs ref_cpu {schedule} t={t} constrain={constrain}: max abs err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (schedule, t, constrain, err, bound)
            # ... and eta matters: the deterministic step is another one
            other, _, _ = ddim_ref.step(flat[0], flat[1], a_t, a_to, noise=flat[2], eta=0.0, constrain=constrain)
            assert np.abs(other[0] - want).max() > 1e3 * bound


def test_oracle_windows_forms_agree():
    """One window is the single-clip step; without overlap (and without CONSTRAIN) the windows are one long row; the window output is the
    state gathered; C is 16 exactly where two windows meet."""
    n, W, H = 3, 64, 48
    Np = (n - 1) * H + W
    long = n * W  # the rows without overlap are longer than Np
    x, noise = seeded((long,), 4).numpy(), seeded((long,), 5).numpy()
    eps, grad = seeded((n, W), 6).numpy(), seeded((n, W), 7).numpy()
    kw = dict(eta=0.5, noise=noise[:W], grad=grad[:1])
    for constrain in (False, True):
        one, win, M, Cn, _ = ddim_ref.step_windows(x[:W], eps[:1], 0.3, 0.4, 1, W, W, constrain=constrain, **kw)
        ref, Mr, _ = ddim_ref.step(x[None, :W], eps[:1], [0.3], [0.4], noise=noise[None, :W], grad=grad[:1], eta=0.5, constrain=constrain)
        assert np.array_equal(one, ref[0]) and np.array_equal(M, Mr[0]) and np.array_equal(win[0], one) and (Cn == ddim_ref.C_STEP).all()
    row, win, _, _, _ = ddim_ref.step_windows(x[:n * W], eps, 0.3, 0.4, n, W, W, eta=0.5, noise=noise[:n * W], grad=grad)
    ref, _, _ = ddim_ref.step(x[None, :n * W], eps.reshape(1, -1), [0.3], [0.4], noise=noise[None, :n * W], grad=grad.reshape(1, -1), eta=0.5)
    assert np.array_equal(row, ref[0]) and np.array_equal(win.reshape(-1), row)
    out, win, M, Cn, _ = ddim_ref.step_windows(x[:Np], eps, 0.3, 0.4, n, W, H, eta=0.5, noise=noise[:Np], grad=grad, constrain=True)
    assert np.array_equal(win, ddim_ref.window_view(out, n, W, H))
    two = np.zeros(Np, dtype=bool)
    for b in range(1, n):
        two[b * H:b * H + W - H] = True
    assert np.array_equal(Cn == ddim_ref.C_BLEND, two) and (M > 0).all()


# ---------------------------------------------------------------- 3. inversion is exact for a fixed prediction
@pytest.mark.parametrize("schedule", ["exp", "cos"])
def test_invert_then_step_returns_the_input(schedule):
    """INVERT from alpha_bar(t - step) to alpha_bar(t) and the eta = 0 step back with the SAME eps: x to 1e-12 relative in float64 (the
    two are one affine map of x and its inverse).  The way back divides by sqrt(alpha_bar(t)), which multiplies float64's 1.1e-16 by
    1 / sqrt(alpha_bar(t)): 316 at t = 1 under the exp schedule, still two orders inside 1e-12.  Under the cos schedule alpha_bar(1)
    is the float32 cosine of pi / 2 squared, 1.9e-15, and NO arithmetic returns x to 1e-12 through a factor of 2.3e7; the first pair
    is therefore (0.9, 0.1) there (1 / sqrt(alpha_bar) = 6.4), the other two are the kernel test's."""
    B, T = 2, 1000
    x, eps, _, _ = ddim_ref.case_inputs(B, T, seed=7)
    for t, step in ((1.0 if schedule == "exp" else 0.9, 0.1),) + tuple(ddim_ref.T_PAIRS[1:]):
        ts = torch.tensor([t] * B, dtype=torch.float32)
        a_hi_t, a_lo_t = ref_cpu.schedule_alpha(schedule, ts).numpy(), ref_cpu.schedule_alpha(schedule, ts - step).numpy()
        assert (a_hi_t < a_lo_t).all()
        up, _, sig = ddim_ref.step(x, eps, a_lo_t, a_hi_t, invert=True)
        assert (sig == 0).all() and np.abs(up - x).max() > 1e-3
        back, _, _ = ddim_ref.step(up, eps, a_hi_t, a_lo_t, eta=0.0)
        err, scale = np.abs(back - x).max(), np.abs(x).max()
        print(f"invert then step {schedule} t={t}: max abs err {err:.3e} (bound {1e-12 * scale:.3e})")
        assert err <= 1e-12 * scale, (schedule, t, err, scale)


# ---------------------------------------------------------------- 4. float32 arithmetic can meet the bound
@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("B,T", ddim_ref.SHAPES)
def test_float32_evaluation_meets_the_bound(schedule, B, T):
    """The kernel's operations in float32 numpy (ddim_ref.step_f32) against the float64 oracle, on the inputs, alphas and variants of
    tests/test_ddim_gpu.py::test_kernel_vs_oracle: within C_STEP * 2^-24 * M everywhere, so the bound can be met by the arithmetic as
    specified.  Largest fraction of the bound found here: 0.26."""
    x, eps, grad, noise = ddim_ref.case_inputs(B, T)
    worst = 0.0
    for first in range(3):
        a_t, a_to = ddim_ref.alphas(schedule, B, first)
        for constrain, eta, g in itertools.product((False, True), ddim_ref.ETAS, (None, grad)):
            kw = dict(grad=g, noise=noise, eta=eta, constrain=constrain)
            want, M, _ = ddim_ref.step(x, eps, a_t, a_to, **kw)
            frac = (np.abs(ddim_ref.step_f32(x, eps, a_t, a_to, **kw) - want) / ddim_ref.bound(M)).max()
            assert frac <= 1.0, (first, constrain, eta, g is not None, frac)
            worst = max(worst, frac)
        want, M, _ = ddim_ref.step(x, eps, a_to, a_t, invert=True)
        frac = (np.abs(ddim_ref.step_f32(x, eps, a_to, a_t, invert=True) - want) / ddim_ref.bound(M)).max()
        assert frac <= 1.0, ("invert", first, frac)
        worst = max(worst, frac)
    print(f"float32 evaluation {schedule} (B, T)=({B}, {T}): largest fraction of the bound {worst:.3f}")


# ---------------------------------------------------------------- 5. host logic
def test_ddim_invert_walks_the_tables_backwards(monkeypatch):
    steps, B = 4, 2
    d = Diffusion(make_schedule("exp"))
    ts_all, a_t_all, a_prev_all, ts_prev_all = d.step_tables(steps, B, None, torch.device("cpu"))
    calls = []

    def predictor(x, ts):
        calls.append(("pred", ts.clone(), x.clone()))
        return x * 0.5

    def stub_step(x_t, eps, a_t, a_to, ts, **kw):
        calls.append(("step", a_t.clone(), a_to.clone(), ts.clone(), kw))
        assert torch.equal(eps, x_t * 0.5)
        return x_t + 1

    monkeypatch.setattr(d, "_ddim_step", stub_step)
    out = d.ddim_invert(torch.zeros(B, 1, 8), predictor, steps)
    assert torch.equal(out, torch.full((B, 1, 8), float(steps)))
    assert [c[0] for c in calls] == ["pred", "step"] * steps
    for j in range(steps):
        row = steps - 1 - j  # the table's rows run t = 1 ... 1/steps: the walk starts at the last one
        pred, step = calls[2 * j], calls[2 * j + 1]
        assert torch.equal(pred[1], ts_prev_all[row]) and torch.equal(pred[2], torch.full((B, 1, 8), float(j)))  # the predictor sees the LOWER t
        assert torch.equal(step[1], a_prev_all[row]) and torch.equal(step[2], a_t_all[row]) and torch.equal(step[3], ts_prev_all[row])
        assert bool((step[2] < step[1]).all())  # towards larger t: alpha_bar falls
        assert step[4] == dict(invert=True)
    lower = [float(c[1][0]) for c in calls[::2]]
    assert lower == sorted(lower) and lower[0] == 0.0 and abs(lower[-1] - (1 - 1 / steps)) < 1e-6
    with pytest.raises(TypeError):
        d.ddim_invert(torch.zeros(B, 1, 8), predictor, steps, eta=0.0)  # no eta, constrain or noise argument


def test_sampler_argument_checks():
    from vq_voice_swap_amd.diffusion import check_sampler

    assert check_sampler("ddpm") == "ddpm" and check_sampler("ddim", 0.5) == "ddim"
    for bad in (("euler", 0.0), ("ddpm", 0.5)):
        with pytest.raises(ValueError):
            check_sampler(*bad)


def test_script_flags_and_refusals(capsys):
    sys.path.insert(0, ROOT)
    import sample_diffusion
    import sample_vqvae
    import sample_vqvae_uncond

    base = flags_of(sample_vqvae.arg_parser())
    assert flags_of(sample_vqvae.arg_parser(sampler_flags=True)) == sorted(base + ["--sampler", "--eta", "--source-label"])
    assert {"--sampler", "--eta"} <= set(flags_of(sample_diffusion.arg_parser())) and "--source-label" not in flags_of(sample_diffusion.arg_parser())
    assert {"--sampler", "--eta"} <= set(flags_of(sample_vqvae_uncond.arg_parser()))
    vq = ["--label", "2", "--input-file", "in.wav", "ck.pt", "out.wav"]
    a = sample_vqvae.parse_args(vq)
    assert (a.sampler, a.eta, a.source_label, a.whole_file, a.sample_steps) == ("ddpm", 0.0, None, False, 100)
    a = sample_vqvae.parse_args(["--sampler", "ddim", "--eta", "0.25", "--source-label", "1"] + vq)
    assert (a.sampler, a.eta, a.source_label) == ("ddim", 0.25, 1)
    assert sample_vqvae.parse_args(["--sampler", "ddim", "--whole-file"] + vq).whole_file
    for bad in (["--source-label", "1"], ["--sampler", "ddpm", "--source-label", "1"], ["--sampler", "ddim", "--source-label", "1", "--whole-file"],
                ["--sampler", "ddim", "--source-label", "1", "--no-vq"], ["--eta", "0.5"], ["--sampler", "ddim", "--eta", "-1"],
                ["--sampler", "heun"]):
        with pytest.raises(SystemExit):
            sample_vqvae.parse_args(bad + vq)
    a = sample_diffusion.parse_args([])
    assert (a.sampler, a.eta) == ("ddpm", 0.0)
    assert sample_diffusion.parse_args(["--sampler", "ddim", "--eta", "1"]).eta == 1.0
    un = ["--label", "1", "--input-file", "in.wav", "ck.pt", "out.wav"]
    assert (sample_vqvae_uncond.parse_args(un).sampler, sample_vqvae_uncond.parse_args(["--sampler", "ddim"] + un).sampler) == ("ddpm", "ddim")
    for mod, rest in ((sample_diffusion, []), (sample_vqvae_uncond, un)):
        for bad in (["--eta", "0.5"], ["--sampler", "ddim", "--eta", "-0.1"], ["--sampler", "x"]):
            with pytest.raises(SystemExit):
                mod.parse_args(bad + rest)
    capsys.readouterr()
