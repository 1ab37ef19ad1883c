"""The DPM-Solver++(2M) sampler, host side: exports, declarations and argument checks of `vqvs_dpmpp_step` /
`vqvs_dpmpp_step_windows`; the float64 oracle tests/dpmpp_ref.py against `ddim_ref.step(eta=0)` at first order; the kernel's float32
arithmetic, restated in numpy, against the bound the GPU test applies; the solver's order on a model with a closed-form solution;
the history logic of the sampling loops on stubbed kernels; the samplers' and scripts' argument surface (none of this needs a device)."""
import contextlib
import ctypes as C
import itertools
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

import ddim_ref
import dpmpp_ref
import vq_voice_swap_amd
from vq_voice_swap_amd import _native
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

from test_ddim import host_buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEP_ARGS = ["const float* d_x_t", "const float* d_eps", "const float* d_grad", "const float* d_x0_prev", "const float* d_alpha_from",
             "const float* d_alpha_t", "const float* d_alpha_to", "float* d_x_to", "float* d_x0_out", "int B", "int T", "uint32_t flags",
             "void* stream"]
WINDOWS_ARGS = ["const float* d_x", "const float* d_eps", "const float* d_grad", "const float* d_x0_prev", "const float* d_alpha_from",
                "const float* d_alpha_t", "const float* d_alpha_to", "float* d_x_to", "float* d_x0_out", "float* d_windows", "int n", "int W",
                "int H", "uint32_t flags", "void* stream"]


# ---------------------------------------------------------------- 1. exports, declarations, refusals
def test_symbols_are_exported_and_declared(lib_built):
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    for name, want in (("vqvs_dpmpp_step", STEP_ARGS), ("vqvs_dpmpp_step_windows", WINDOWS_ARGS)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl, f"include/vqvs.h does not declare {name}"
        assert [a.strip() for a in " ".join(decl.group(1).split()).split(",")] == want
        assert len(getattr(lib_built, name).argtypes) == len(want)
    for method in ("dpmpp_previous", "dpmpp_sample", "dpmpp_sample_windows"):
        assert callable(getattr(vq_voice_swap_amd.Diffusion, method))


def test_step_refuses_bad_arguments_without_a_device(lib_built):
    """Every refusal of include/vqvs.h: VQVS_ERR_ARG with host-only pointers, which a call that reached the device would fault on."""
    L = lib_built
    keep, (x, eps, grad, prev, a_from, a_t, a_to, out, x0) = host_buffers(9)
    ok = dict(x=x, eps=eps, grad=grad, prev=prev, a_from=a_from, a_t=a_t, a_to=a_to, out=out, x0=x0, B=2, T=16, flags=2)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_dpmpp_step(a["x"], a["eps"], a["grad"], a["prev"], a["a_from"], a["a_t"], a["a_to"], a["out"], a["x0"], a["B"], a["T"],
                                 a["flags"], None)

    inside = C.c_void_p(prev.value + 16)
    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_to=None), dict(out=None),
                dict(B=0), dict(B=-1), dict(T=0), dict(T=-4), dict(B=65536), dict(T=(1 << 30) + 1),
                dict(flags=1), dict(flags=3), dict(flags=4), dict(flags=6), dict(flags=8), dict(flags=1 << 31),
                dict(out=x), dict(out=eps), dict(out=grad), dict(out=prev), dict(out=a_t), dict(out=a_from), dict(out=x0),
                dict(x0=x), dict(x0=eps), dict(x0=grad), dict(x0=a_to), dict(x0=inside),  # a PART of the history is no alias
                dict(x0=prev, out=prev), dict(x0=prev, x=prev),                          # ... and the exact alias excuses nothing else
                dict(grad=None, prev=None, a_from=None, x0=None, x=None)):               # the optional arguments do not switch the checks off
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(flags=4) == -1 and b"flags" in L.vqvs_last_error()
    assert call(out=eps) == -1 and b"overlap" in L.vqvs_last_error()
    assert call(x0=inside) == -1 and b"x0_prev" in L.vqvs_last_error()
    assert call(x=None) == -1 and b"non-NULL" in L.vqvs_last_error()


def test_windows_refuses_bad_arguments_without_a_device(lib_built):
    """The limits of `vqvs_ddpm_step_windows` (tests/test_longform.py), the flag and aliasing rules of `vqvs_dpmpp_step`."""
    L = lib_built
    keep, (x, eps, grad, prev, a_from, a_t, a_to, out, x0, win) = host_buffers(10)
    ok = dict(x=x, eps=eps, grad=grad, prev=prev, a_from=a_from, a_t=a_t, a_to=a_to, out=out, x0=x0, win=None, n=3, W=16, H=12, flags=2)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_dpmpp_step_windows(a["x"], a["eps"], a["grad"], a["prev"], a["a_from"], a["a_t"], a["a_to"], a["out"], a["x0"], a["win"],
                                         a["n"], a["W"], a["H"], a["flags"], None)

    inside = C.c_void_p(prev.value + 16)
    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_to=None), dict(out=None),
                dict(n=0), dict(n=-1), dict(n=65536),
                dict(W=18, H=12), dict(W=16, H=10), dict(W=0, H=0), dict(W=16, H=0), dict(W=-16, H=-12), dict(W=16, H=-4),
                dict(W=12, H=16), dict(W=28, H=12),
                dict(n=65535, W=65536, H=32768), dict(n=40000, W=1 << 20, H=1 << 19),
                dict(flags=1), dict(flags=4), dict(flags=16),
                dict(out=x), dict(out=grad), dict(out=prev), dict(out=x0), dict(x0=inside), dict(x0=eps), dict(x0=prev, out=prev),
                dict(win=eps), dict(win=out), dict(win=x0), dict(win=prev), dict(win=prev, x0=prev),
                dict(grad=None, prev=None, a_from=None, x0=None, x=None), dict(win=win, n=0)):
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(n=65536) == -1 and b"65535" in L.vqvs_last_error()
    assert call(W=28, H=12) == -1 and b"overlap" in L.vqvs_last_error()
    assert call(x=None) == -1 and b"non-NULL" in L.vqvs_last_error()


# ---------------------------------------------------------------- 2. the oracle at first order is the DDIM oracle at eta = 0
def variants(grad):
    return (("plain", None, False), ("grad", grad, False), ("constrain", None, True))


@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("B,T", ddim_ref.SHAPES)
def test_first_order_is_the_ddim_oracle_at_eta_zero(schedule, B, T):
    """Without a history x_to = (sigma_to / sigma_t) x + (alpha_to - sigma_to alpha_t / sigma_t) x0 is algebraically
    sqrt(a_to) x0 + sqrt(1 - a_to) e' with e' = (x - sqrt(a_t) x0) / sqrt(1 - a_t): `ddim_ref.step(eta=0)`, un-constrained (e' = e) and
    constrained alike.  The two are evaluated in float64 in different orders, so they agree to a few float64 roundings of the terms
    that meet: 16 * 2^-53 * M (four roundings on either path would be the count; 16 leaves room for the cancellation in phi, whose two
    terms each carry the rounding of a square root and a division).  It ties this oracle to the one tests/test_ddim.py pins to the
    reference's `ddpm_previous`."""
    x, eps, grad, _ = ddim_ref.case_inputs(B, T)
    worst = 0.0
    for first in range(3):
        a_t, a_to = ddim_ref.alphas(schedule, B, first)
        for name, g, constrain in variants(grad):
            want, M_ddim, _ = ddim_ref.step(x, eps, a_t, a_to, grad=g, eta=0.0, constrain=constrain)
            got, x0, M, _ = dpmpp_ref.step(x, eps, a_t, a_to, grad=g, constrain=constrain)
            frac = (np.abs(got - want) / (16 * 2.0 ** -53 * np.maximum(M, M_ddim))).max()
            assert frac <= 1.0, (first, name, frac)
            worst = max(worst, frac)
            same, _, _, _ = dpmpp_ref.step(x, eps, a_t, a_to, grad=g, constrain=constrain, x0_prev=x0, a_from=None)
            assert np.array_equal(same, got)  # a history without its alpha_bar is no history
        last = np.asarray(a_to) == 1.0
        assert last.any() or B < 3
        got, x0, _, _ = dpmpp_ref.step(x, eps, a_t, a_to)
        assert np.array_equal(got[last], x0[last])  # at alpha_bar = 1 the step returns x0
    print(f"first order vs ddim_ref eta=0 {schedule} (B, T)=({B}, {T}): largest fraction of 16 * 2^-53 * M {worst:.3f}")


def test_oracle_windows_forms_agree():
    """One window is the single-clip step; without overlap (and without CONSTRAIN) the windows are one long row; the window output is the
    state gathered; the blend's counts stand exactly where two windows meet."""
    n, W, H = 3, 64, 48
    Np = (n - 1) * H + W
    rng = np.random.default_rng(4)
    x, prev = rng.standard_normal(n * W).astype(np.float32), (0.3 * rng.standard_normal(n * W)).astype(np.float32)
    eps, grad = rng.standard_normal((n, W)).astype(np.float32), rng.standard_normal((n, W)).astype(np.float32)
    al = dict(a_t=0.3, a_to=0.4)
    for constrain, hist in itertools.product((False, True), (False, True)):
        hw = dict(x0_prev=prev[:W], a_from=0.25) if hist else {}
        hc = dict(x0_prev=prev[None, :W], a_from=[0.25]) if hist else {}
        one, win, x0, M, x0m, Cn, C0 = dpmpp_ref.step_windows(x[:W], eps[:1], n=1, W=W, H=W, grad=grad[:1], constrain=constrain, **al, **hw)
        ref, ref0, Mr, x0mr = dpmpp_ref.step(x[None, :W], eps[:1], [0.3], [0.4], grad=grad[:1], constrain=constrain, **hc)
        assert np.array_equal(one, ref[0]) and np.array_equal(x0, ref0[0]) and np.array_equal(M, Mr[0]) and np.array_equal(x0m, x0mr[0])
        assert np.array_equal(win[0], one) and (Cn == dpmpp_ref.C_STEP).all() and (C0 == dpmpp_ref.C_X0).all()
    row, win, x0, _, _, _, _ = dpmpp_ref.step_windows(x, eps, n=n, W=W, H=W, grad=grad, x0_prev=prev, a_from=0.25, **al)
    ref, ref0, _, _ = dpmpp_ref.step(x[None], eps.reshape(1, -1), [0.3], [0.4], grad=grad.reshape(1, -1), x0_prev=prev[None], a_from=[0.25])
    assert np.array_equal(row, ref[0]) and np.array_equal(win.reshape(-1), row) and np.array_equal(x0, ref0[0])
    out, win, x0, M, x0m, Cn, C0 = dpmpp_ref.step_windows(x[:Np], eps, n=n, W=W, H=H, grad=grad, constrain=True, x0_prev=prev[:Np], a_from=0.25, **al)
    assert np.array_equal(win, ddim_ref.window_view(out, n, W, H))
    two = np.zeros(Np, dtype=bool)
    for b in range(1, n):
        two[b * H:b * H + W - H] = True
    assert np.array_equal(Cn == dpmpp_ref.C_BLEND, two) and np.array_equal(C0 == dpmpp_ref.C_X0_BLEND, two) and (M > 0).all()
    assert (np.abs(x0) <= 1.0).all()  # a blend of two clamped predictions


# ---------------------------------------------------------------- 3. float32 arithmetic can meet the bound
def check_f32(x, eps, a_t, a_to, tag, **kw):
    want, want0, M, x0m = dpmpp_ref.step(x, eps, a_t, a_to, **kw)
    got, got0 = dpmpp_ref.step_f32(x, eps, a_t, a_to, **kw)
    frac = (np.abs(got - want) / dpmpp_ref.bound(M)).max()
    frac0 = (np.abs(got0 - want0) / dpmpp_ref.bound(x0m, dpmpp_ref.C_X0)).max()
    assert frac <= 1.0 and frac0 <= 1.0, (tag, frac, frac0)
    return max(frac, frac0)


@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("B,T", ddim_ref.SHAPES)
def test_float32_evaluation_meets_the_bound(schedule, B, T):
    """The kernel's operations in float32 numpy (dpmpp_ref.step_f32) against the float64 oracle: x_to within C_STEP * 2^-24 * M and x0
    within C_X0 * 2^-24 * X0M everywhere -- without a history on the cases of tests/test_ddim.py, with one at the three (t_from, t, step)
    triples -- so the bound can be met by the arithmetic as specified."""
    x, eps, grad, _ = ddim_ref.case_inputs(B, T)
    prev = dpmpp_ref.history_input(B, T)
    worst = 0.0
    for first in range(3):
        a_t, a_to = ddim_ref.alphas(schedule, B, first)
        a_from, a_t3, a_to3 = dpmpp_ref.alphas(schedule, B, first)
        for name, g, constrain in variants(grad) + (("grad+constrain", grad, True),):
            worst = max(worst, check_f32(x, eps, a_t, a_to, (first, name), grad=g, constrain=constrain))
            worst = max(worst, check_f32(x, eps, a_t3, a_to3, (first, name, "history"), grad=g, constrain=constrain, x0_prev=prev, a_from=a_from))
    print(f"float32 evaluation {schedule} (B, T)=({B}, {T}): largest fraction of the bounds {worst:.3f}")


@pytest.mark.parametrize("schedule", ["exp", "cos"])
def test_order_rule(schedule):
    """Second order needs a history, its alpha_bar, 1 - a_to != 0 and h_prev > 0: the (0.04, 0.02, 0.02) triple steps to alpha_bar = 1
    and a_from == a_t has h_prev = 0 -- both come out first order, bit for bit the step without a history, in the oracle and in the
    float32 restatement; the other two triples do not."""
    B, T = 3, 8
    x, eps, _, _ = ddim_ref.case_inputs(B, T)
    prev = dpmpp_ref.history_input(B, T)
    a_from, a_t, a_to = dpmpp_ref.alphas(schedule, B, 0)
    k = dpmpp_ref.coef(a_t, a_to, a_from)
    assert a_to[2] == 1.0 and k["second"].tolist() == [True, True, False] and (k["q"][:2] > 0).all() and k["q"][2] == 0
    assert (k["c0"][:2] > k["phi"][:2]).all() and (k["c1"][:2] < 0).all() and k["c1"][2] == 0 and k["c0"][2] == 1.0 and k["cx"][2] == 0
    plain, plain32 = dpmpp_ref.step(x, eps, a_t, a_to), dpmpp_ref.step_f32(x, eps, a_t, a_to)
    with_h, with_h32 = dpmpp_ref.step(x, eps, a_t, a_to, x0_prev=prev, a_from=a_from), dpmpp_ref.step_f32(x, eps, a_t, a_to, x0_prev=prev, a_from=a_from)
    assert np.array_equal(with_h[0][2], plain[0][2]) and np.array_equal(with_h32[0][2], plain32[0][2])
    assert not np.array_equal(with_h[0][:2], plain[0][:2]) and not np.array_equal(with_h32[0][:2], plain32[0][:2])
    same = dpmpp_ref.step(x, eps, a_t, a_to, x0_prev=prev, a_from=a_t)  # a_from == a_t
    assert not dpmpp_ref.coef(a_t, a_to, a_t)["second"].any() and np.array_equal(same[0], plain[0])
    same32 = dpmpp_ref.step_f32(x, eps, a_t, a_to, x0_prev=prev, a_from=a_t)
    assert np.array_equal(same32[0], plain32[0])
    check_f32(x, eps, a_t, a_to, "a_from == a_t", x0_prev=prev, a_from=a_t)
    backwards = dpmpp_ref.coef(a_t, a_to, a_to)  # a history from a SMALLER t: h_prev < 0
    assert not backwards["second"][:2].any()
    nan_hist = np.full_like(prev, np.nan)  # the history is not read at first order
    assert np.isfinite(dpmpp_ref.step(x, eps, a_t, a_to, x0_prev=nan_hist, a_from=a_t)[0]).all()
    assert np.isfinite(dpmpp_ref.step_f32(x, eps, a_t, a_to, x0_prev=nan_hist, a_from=a_t)[0]).all()


# ---------------------------------------------------------------- 4. the analytic model: the solver is second order
def analytic_errors(schedule, power, B=2, T=16):
    _, a_t_all, a_to_all = dpmpp_ref.analytic_tables(schedule, power, B)
    x_T = np.random.default_rng(7).standard_normal((B, T))
    exact = dpmpp_ref.analytic_exact(x_T, a_t_all[0])
    predictor = lambda x, i: dpmpp_ref.analytic_scalar(a_t_all[i]).reshape(B, 1) * x
    errs = []
    for order in (1, 2):
        x_0, trace = dpmpp_ref.chain(x_T, a_t_all, a_to_all, predictor, order=order)
        errs.append(np.abs(x_0 - exact).max() / np.abs(exact).max())
        seconds = [bool(t["k"]["second"].all()) for t in trace]
        assert seconds == ([False] + [True] * (len(trace) - 2) + [False] if order == 2 else [False] * len(trace))
    return errs


def test_analytic_model_two_m_halves_the_first_order_error():
    """Data N(0, s^2) per sample, s = 0.3: eps*(x, t) = sqrt(1 - a) x / (a s^2 + 1 - a), and the probability-flow ODE maps x_T to
    x_0 = x_T s / sqrt(a_T s^2 + 1 - a_T).  The float64 chains run over `step_tables`' own float32 alphas at 40 steps on {exp, cos} x
    {t, t**2}; the 2M chain's relative error of x_0 is at most HALF the first-order (eta = 0 DDIM) chain's on all four grids.  A
    condition, not a measurement: nothing printed here is hard-coded."""
    for schedule, power in dpmpp_ref.GRIDS:
        first, second = analytic_errors(schedule, power)
        print(f"analytic model {schedule} / t**{power or 1}, {dpmpp_ref.ANALYTIC_STEPS} steps: first order {first:.3e}, 2M {second:.3e}, ratio {first / second:.2f}")
        assert second <= 0.5 * first, (schedule, power, first, second)


def test_chain_first_order_is_the_ddim_chain():
    """order=1 of the chain runner is the eta = 0 DDIM chain of `ddim_ref.step` (whose eps it rounds to float32: 2^-24 per step)."""
    B, T = 2, 16
    _, a_t_all, a_to_all = dpmpp_ref.analytic_tables("exp", None, B, steps=10)
    x_T = np.random.default_rng(8).standard_normal((B, T))
    predictor = lambda x, i: dpmpp_ref.analytic_scalar(a_t_all[i]).reshape(B, 1) * x
    got, _ = dpmpp_ref.chain(x_T, a_t_all, a_to_all, predictor, order=1)
    x = x_T
    for i in range(10):
        x, _, _ = ddim_ref.step(x, predictor(x, i), a_t_all[i], a_to_all[i], eta=0.0)
    assert np.abs(got - x).max() <= 1e-5 * np.abs(x).max()


# ---------------------------------------------------------------- 5. loop logic on stubbed kernels
@pytest.fixture
def host_loops(monkeypatch):
    monkeypatch.delenv("VQVS_FEW_STEP_PROMOTE", raising=False)
    monkeypatch.setattr(_native, "require_cuda", lambda *tensors: None)
    monkeypatch.setattr(_native, "_stream_ptr", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())


def test_clip_loop_hands_each_step_the_previous_x0(monkeypatch, host_loops):
    steps, B = 5, 2
    d = Diffusion(make_schedule("exp"))
    ts_all, a_t_all, a_to_all, _ = d.step_tables(steps, B, None, torch.device("cpu"))
    log = []

    def stub(x_t, eps, a_from, a_t, a_to, ts, *, x0_prev, constrain, cond_fn):
        assert torch.equal(eps, 0.5 * x_t)
        x0 = x_t * 2
        log.append(dict(kind="step", a_from=a_from, a_t=a_t, a_to=a_to, ts=ts, x0_prev=x0_prev, x0=x0, constrain=constrain, cond_fn=cond_fn))
        return x_t + 1, x0

    def keep_stub(x, source, keep, alpha, **kw):
        if keep is None:  # the start at a later step: the call writes EVERY sample of a state that is uninitialised memory until then
            x.copy_(source)
        log.append(dict(kind="keep", index=kw["index"], alpha=alpha, seed=kw["seed"], clip_offset=kw["clip_offset"]))

    def noise(i):
        raise AssertionError("the deterministic sampler asked for noise")

    def cond_fn(x, ts):
        return 0.1 * x

    monkeypatch.setattr(d, "_dpmpp_step", stub)
    monkeypatch.setattr(d, "_keep_", keep_stub)
    x_T = torch.zeros(B, 1, 8)
    source, keep = torch.ones_like(x_T), torch.zeros_like(x_T, dtype=torch.bool)
    keep[..., 3:6] = True
    for start in (0, 2, 0):  # (the third run: the same Diffusion starts again with no history)
        del log[:]
        out = d.dpmpp_sample(x_T, lambda x, ts: 0.5 * x, steps, constrain=True, cond_fn=cond_fn, noise=noise, seed=7, clip_offset=3,
                             source=source, keep=keep, start_step=start)
        assert out.shape == x_T.shape
        assert log[0]["kind"] == "keep" and log[0]["index"] == start and torch.equal(log[0]["alpha"], a_t_all[start])
        rest = log[1:]
        assert [e["kind"] for e in rest] == ["step", "keep"] * (steps - start)
        calls, keeps = rest[0::2], rest[1::2]
        assert calls[0]["x0_prev"] is None and calls[0]["a_from"] is None  # step `start_step` has no history
        for k, i in enumerate(range(start, steps)):
            c = calls[k]
            assert torch.equal(c["a_t"], a_t_all[i]) and torch.equal(c["a_to"], a_to_all[i]) and torch.equal(c["ts"], ts_all[i])
            assert c["constrain"] is True and c["cond_fn"] is cond_fn
            if k:
                assert c["x0_prev"] is calls[k - 1]["x0"] and torch.equal(c["a_from"], calls[k - 1]["a_t"])
                assert c["a_from"].data_ptr() == calls[k - 1]["a_t"].data_ptr()
            assert keeps[k]["index"] == i + 1 and torch.equal(keeps[k]["alpha"], a_to_all[i]) and (keeps[k]["seed"], keeps[k]["clip_offset"]) == (7, 3)


def test_window_loop_keeps_the_history_in_the_long_layout(monkeypatch, host_loops):
    from vq_voice_swap_amd import longform

    steps, n, W, H = 4, 3, 8, 4
    Np = (n - 1) * H + W
    d = Diffusion(make_schedule("exp"))
    _, a_t_all, a_to_all, _ = d.step_tables(steps, 2, None, torch.device("cpu"))  # window_batch = 2: two rows
    log = []

    def stub(x, eps, grad, x0_prev, a_from, a_t, a_to, x_to, x0_out, next_windows, n_, window, hop, flags, st):
        assert (n_, window, hop, flags) == (n, W, H, _native.DDIM_CONSTRAIN) and torch.equal(eps, 0.5 * longform.gather_windows(x, W, H))
        assert x0_out.shape == x.shape == x_to.shape == (1, 1, Np) and tuple(grad.shape) == (n, 1, W)
        assert torch.equal(grad, 0.1 * longform.gather_windows(x, W, H))  # the gradient AT the windows the predictor saw
        log.append(dict(kind="step", a_from=a_from, a_t=a_t, a_to=a_to, x0_prev=x0_prev, x0=x0_out))
        x_to.copy_(x + 1)
        next_windows.copy_(longform.gather_windows(x_to, W, H))

    def keep_stub(*args, **kw):
        if args[3] is None:  # the start at a later step: the call writes EVERY sample of a state that is uninitialised memory until then
            args[0].copy_(args[2])
        log.append(dict(kind="keep", index=kw["index"], alpha=args[-1]))

    monkeypatch.setattr(longform, "dpmpp_step_windows_", stub)
    monkeypatch.setattr(longform, "keep_windows_", keep_stub)
    x_T = torch.zeros(1, 1, Np)
    source, keep = torch.ones_like(x_T), torch.zeros_like(x_T, dtype=torch.bool)
    keep[..., 3:6] = True
    for start in (0, 2, 0):
        del log[:]
        out = d.dpmpp_sample_windows(x_T, lambda x, ts, first: 0.5 * x, steps, window=W, hop=H, window_batch=2, constrain=True,
                                     cond_fn=lambda x, ts, first: 0.1 * x, seed=7, clip_offset=3, source=source, keep=keep, start_step=start)
        assert out.shape == x_T.shape
        rest = log[1:]
        assert log[0]["kind"] == "keep" and [e["kind"] for e in rest] == ["step", "keep"] * (steps - start)
        calls, keeps = rest[0::2], rest[1::2]
        assert calls[0]["x0_prev"] is None and calls[0]["a_from"] is None
        for k, i in enumerate(range(start, steps)):
            assert torch.equal(calls[k]["a_t"], a_t_all[i]) and torch.equal(calls[k]["a_to"], a_to_all[i])
            if k:
                assert calls[k]["x0_prev"] is calls[k - 1]["x0"] and calls[k]["a_from"].data_ptr() == calls[k - 1]["a_t"].data_ptr()
            assert keeps[k]["index"] == i + 1 and torch.equal(keeps[k]["alpha"], a_to_all[i])


def test_few_unguided_steps_warn_for_this_sampler_too(monkeypatch, host_loops):
    d = Diffusion(make_schedule("exp"))
    monkeypatch.setattr(d, "_dpmpp_step", lambda x_t, eps, *a, **kw: (x_t + 1, x_t * 2))

    class HalfPredictor:
        precision = "fp16"

        @contextlib.contextmanager
        def precision_override(self, mode):
            raise AssertionError("an un-guided run is not promoted")
            yield

        def check_status(self):
            pass

        def __call__(self, x, ts):
            return 0.5 * x

    for steps, expect in ((3, 1), (10, 0)):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            d.dpmpp_sample(torch.zeros(2, 1, 8), HalfPredictor(), steps)
        kept = [w for w in rec if "the mode is kept" in str(w.message)]
        assert len(kept) == expect and all("dpmpp_sample:" in str(w.message) and w.filename == __file__ for w in kept)


# ---------------------------------------------------------------- 6. argument surface
def test_sampler_argument_checks():
    from vq_voice_swap_amd.diffusion import SAMPLERS, check_sampler, pick_sampler
    from vq_voice_swap_amd.sampler import sample_clips

    assert SAMPLERS == ("ddpm", "ddim", "dpmpp") and check_sampler("dpmpp") == "dpmpp" and check_sampler("dpmpp", 0.0) == "dpmpp"
    with pytest.raises(ValueError, match="deterministic"):
        check_sampler("dpmpp", eta=0.5)
    d = Diffusion(make_schedule("exp"))
    for windows, name in ((False, "dpmpp_sample"), (True, "dpmpp_sample_windows")):
        fn, kw = pick_sampler(d, "dpmpp", windows=windows)
        assert fn == getattr(d, name) and kw == {}
        assert pick_sampler(d, "dpmpp", sigma_large=False, windows=windows)[1] == {}
    with pytest.raises(ValueError):
        pick_sampler(d, "dpmpp", 0.5)
    assert pick_sampler(d, "ddim", 0.5)[1] == dict(eta=0.5) and pick_sampler(d, "ddpm", sigma_large=True)[1] == dict(sigma_large=True)

    class Model:
        diffusion = d

    with pytest.raises(ValueError, match="sigma_large"):
        sample_clips(Model(), 2, 8, 3, 0, sampler="dpmpp", sigma_large=True)
    with pytest.raises(ValueError, match="sigma_large"):
        sample_clips(Model(), 2, 8, 3, 0, sampler="ddim", sigma_large=True)


def test_script_flags_and_refusals(capsys):
    sys.path.insert(0, ROOT)
    import sample_diffusion
    import sample_vqvae
    import sample_vqvae_uncond

    vq = ["--label", "2", "--input-file", "in.wav", "ck.pt", "out.wav"]
    assert sample_diffusion.parse_args(["--sampler", "dpmpp"]).sampler == "dpmpp"
    assert sample_diffusion.parse_args(["--sampler", "dpmpp", "--eta", "0"]).eta == 0.0
    assert sample_vqvae_uncond.parse_args(["--sampler", "dpmpp"] + vq).sampler == "dpmpp"
    a = sample_vqvae.parse_args(["--sampler", "dpmpp", "--whole-file"] + vq)
    assert (a.sampler, a.eta, a.source_label, a.whole_file) == ("dpmpp", 0.0, None, True)
    a = sample_vqvae.parse_args(["--sampler", "dpmpp", "--strength", "0.6", "--keep", "0:0.5"] + vq)
    assert a.sampler == "dpmpp" and a.strength == 0.6 and a.keep
    for mod, rest in ((sample_diffusion, []), (sample_vqvae_uncond, vq), (sample_vqvae, vq)):
        with pytest.raises(SystemExit):
            mod.parse_args(["--sampler", "dpmpp", "--eta", "0.5"] + rest)
    with pytest.raises(SystemExit):
        sample_vqvae.parse_args(["--sampler", "dpmpp", "--source-label", "1"] + vq)
    assert "deterministic" in capsys.readouterr().err
