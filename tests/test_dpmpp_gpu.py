"""The DPM-Solver++(2M) sampler on the device: `vqvs_dpmpp_step` and `vqvs_dpmpp_step_windows` against the float64 oracle
tests/dpmpp_ref.py under its bounds C * 2^-24 * M (the roundings are counted in that file's docstring), both outputs; against each
other bit for bit where they coincide; the aliasing and argument rules; `Diffusion.dpmpp_sample` and the windows loop against the
same calls chained by hand, bit for bit; the analytic model of tests/test_dpmpp.py on the device; `VQVAE.decode` / `decode_long`
end to end.  fp32 mode throughout.

A run with VQVS_DPMPP_MARGINS=<file>.jsonl appends the largest fraction of its bound each test found; profiles/dpmpp_margins.jsonl
is such a run on an MI355X: the step used at most 0.54 of its bound, the windows form 0.50, the 40-step chain 0.005 of the carried
bound under the exp schedule (under cos the carried bound exceeds the result and shows nothing)."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

import ddim_ref
import dpmpp_ref
from test_keep_gpu import read_s16
from vq_voice_swap_amd import VQVAE, _native, longform, plan_windows
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

from util import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTRAIN = _native.DDIM_CONSTRAIN
VARIANTS = [("plain", False, 0), ("grad", True, 0), ("constrain", False, CONSTRAIN), ("grad+constrain", True, CONSTRAIN)]
WINDOW_SHAPES = [(1, 16, 16), (3, 16, 12), (3, 8200, 4104), (4, 8, 8)]  # one window; overlaps; an overlap over a mean chunk and more; V = 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(name, fraction):
    print(f"[margin] {name}: largest fraction of the bound {fraction:.3f}")
    path = os.environ.get("VQVS_DPMPP_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": name, "fraction_of_bound": float(fraction)}) + "\n")


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def guarded(size, dev):
    return torch.full((size + 64,), float("nan"), device=dev)


def unguard(buf, size):
    assert torch.isnan(buf[size:]).all(), "the kernel wrote past the end of an output"
    assert torch.isfinite(buf[:size]).all(), "the kernel left elements unwritten (or wrote non-finite values)"
    return buf[:size]


def step_call(x, eps, grad, prev, a_from, a_t, a_to, flags, want_x0=True, x0_into=None):
    """`vqvs_dpmpp_step` on [B, T] device tensors -> (x_to, x0); the outputs lie in front of NaN guards that the call must leave alone.
    `x0_into`: the buffer d_x0_out is to be (the history itself, for the in-place form)."""
    B, T = x.shape
    out = guarded(B * T, x.device)
    x0 = x0_into if x0_into is not None else (guarded(B * T, x.device) if want_x0 else None)
    _native.check(_native.lib().vqvs_dpmpp_step(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(prev), _native._ptr(a_from),
                                                a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), _native._ptr(x0), B, T, flags,
                                                _native._stream_ptr()))
    if x0 is not None and x0_into is None:
        x0 = unguard(x0, B * T).view(B, T)
    return unguard(out, B * T).view(B, T), x0


def windows_call(x, eps, grad, prev, a_from, a_t, a_to, n, W, H, flags, want_windows=True, x0_into=None):
    Np = (n - 1) * H + W
    assert x.numel() == Np and eps.numel() == n * W and (prev is None or prev.numel() == Np) and (grad is None or grad.numel() == n * W)
    out = guarded(Np, x.device)
    x0 = x0_into if x0_into is not None else guarded(Np, x.device)
    win = guarded(n * W, x.device) if want_windows else None
    _native.check(_native.lib().vqvs_dpmpp_step_windows(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(prev), _native._ptr(a_from),
                                                        a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), x0.data_ptr(), _native._ptr(win), n, W, H,
                                                        flags, _native._stream_ptr()))
    if x0_into is None:
        x0 = unguard(x0, Np)
    return unguard(out, Np), x0, None if win is None else unguard(win, n * W).view(n, W)


def fraction(got, want, bound):
    """max |got - want| / bound over the elements (a zero bound admits a zero error only)."""
    err = np.abs(got.detach().cpu().double().numpy().reshape(want.shape) - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


# ---------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("B,T", ddim_ref.SHAPES)
def test_kernel_vs_oracle(dev, schedule, B, T):
    """x_to within 9 * 2^-24 * M and x0 within 6 * 2^-24 * X0M per element (dpmpp_ref: C_STEP, C_X0): {no history, history} x {plain,
    grad, constrain, grad + constrain}, rows at the three (t_from, t, step) triples in turn -- the a_to = 1 row among them."""
    xs = ddim_ref.case_inputs(B, T)
    hist = dpmpp_ref.history_input(B, T)
    x, eps, grad, _ = (to_dev(a, dev) for a in xs)
    prev = to_dev(hist, dev)
    worst = 0.0
    for first in range(3):
        al = dpmpp_ref.alphas(schedule, B, first)
        a_from, a_t, a_to = (to_dev(a, dev) for a in al)
        for history, (name, guided, flags) in itertools.product((False, True), VARIANTS):
            want, want0, M, x0m = dpmpp_ref.step(xs[0], xs[1], al[1], al[2], grad=xs[2] if guided else None, constrain=bool(flags),
                                                 x0_prev=hist if history else None, a_from=al[0] if history else None)
            got, got0 = step_call(x, eps, grad if guided else None, prev if history else None, a_from if history else None, a_t, a_to, flags)
            frac = fraction(got, want, dpmpp_ref.bound(M))
            frac0 = fraction(got0, want0, dpmpp_ref.bound(x0m, dpmpp_ref.C_X0))
            print(f"dpmpp step {schedule} (B, T)=({B}, {T}) first={first} history={history} {name}: x_to {frac:.3f}, x0 {frac0:.3f} of the bound")
            assert frac <= 1.0 and frac0 <= 1.0, (first, history, name, frac, frac0)
            worst = max(worst, frac, frac0)
            last = torch.from_numpy(al[2] == 1.0).to(dev)
            assert torch.equal(got[last], got0[last])  # at alpha_bar = 1 the step returns x0
    record(f"1 dpmpp step vs oracle {schedule} (B, T)=({B}, {T})", worst)


# ---------------------------------------------------------------- 2. aliasing, optional arguments, access width, refusals
def test_history_in_place_optional_outputs_and_access_width(dev):
    B, T = 3, 4100  # (T % 4 == 0: the aligned buffers take the 16-byte path)
    xs = ddim_ref.case_inputs(B, T, seed=301)
    x, eps, grad, _ = (to_dev(a, dev) for a in xs)
    prev = to_dev(dpmpp_ref.history_input(B, T), dev)
    a_from, a_t, a_to = (to_dev(a, dev) for a in dpmpp_ref.alphas("exp", B, 0))
    poison = torch.full((B, T), float("nan"), device=dev)
    for name, guided, flags in VARIANTS:
        g = grad if guided else None
        out, x0 = step_call(x, eps, g, prev, a_from, a_t, a_to, flags)
        hist = prev.clone()
        out_ip, _ = step_call(x, eps, g, hist, a_from, a_t, a_to, flags, x0_into=hist)  # d_x0_out IS d_x0_prev
        assert torch.equal(out_ip, out) and torch.equal(hist, x0), name
        alone, none = step_call(x, eps, g, prev, a_from, a_t, a_to, flags, want_x0=False)  # NULL d_x0_out
        assert none is None and torch.equal(alone, out), name
        # first order reads no history: without d_alpha_from, without d_x0_prev, and with a_from == a_t a poisoned one changes nothing
        first, first0 = step_call(x, eps, g, None, None, a_t, a_to, flags)
        assert torch.equal(first0, x0) and not torch.equal(first, out), name
        for p, af in ((prev, None), (None, a_from), (poison, a_t)):
            again, again0 = step_call(x, eps, g, p, af, a_t, a_to, flags)
            assert torch.equal(again, first) and torch.equal(again0, x0), name
        # the same values one float off the 16-byte grid: the scalar path
        def off(t):
            if t is None:
                return None
            buf = torch.empty(t.numel() + 1, device=dev)
            buf[1:].copy_(t.reshape(-1))
            return buf[1:].view(t.shape)

        shifted, shifted0 = step_call(off(x), off(eps), off(g), off(prev), a_from, a_t, a_to, flags)
        assert torch.equal(shifted, out) and torch.equal(shifted0, x0), name


def test_refusals_return_before_launch(dev):
    """Every VQVS_ERR_ARG rule with device pointers: -1, and the outputs keep their NaN fill -- nothing was launched."""
    L = _native.lib()
    B, T = 2, 16
    bufs = {k: torch.zeros(B * T + 8, device=dev) for k in ("x", "eps", "grad", "prev")}
    al = {k: torch.full((B,), v, device=dev) for k, v in (("a_from", 0.2), ("a_t", 0.3), ("a_to", 0.4))}
    out, x0 = torch.full((B * T + 8,), float("nan"), device=dev), torch.full((B * T + 8,), float("nan"), device=dev)
    ok = dict(x=bufs["x"].data_ptr(), eps=bufs["eps"].data_ptr(), grad=bufs["grad"].data_ptr(), prev=bufs["prev"].data_ptr(),
              a_from=al["a_from"].data_ptr(), a_t=al["a_t"].data_ptr(), a_to=al["a_to"].data_ptr(), out=out.data_ptr(), x0=x0.data_ptr(),
              B=B, T=T, flags=CONSTRAIN)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_dpmpp_step(a["x"], a["eps"], a["grad"], a["prev"], a["a_from"], a["a_t"], a["a_to"], a["out"], a["x0"], a["B"], a["T"],
                                 a["flags"], _native._stream_ptr())

    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_to=None), dict(out=None), dict(B=0), dict(B=65536), dict(T=0),
                dict(T=(1 << 30) + 1), dict(flags=1), dict(flags=4), dict(flags=1 << 31),
                dict(out=ok["x"] + 16), dict(out=ok["prev"]), dict(x0=ok["prev"] + 16), dict(x0=ok["eps"]), dict(x0=ok["out"] + 32),
                dict(x0=ok["prev"], out=ok["prev"])):
        assert call(**bad) == -1, bad
        assert _native.last_error(), bad
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(x0).all()
    n, W, H = 2, 8, 4  # Np = 12, n * W = 16
    win = torch.full((n * W,), float("nan"), device=dev)

    def wcall(**kw):
        a = dict(ok, win=win.data_ptr(), n=n, W=W, H=H)
        a.update(kw)
        return L.vqvs_dpmpp_step_windows(a["x"], a["eps"], a["grad"], a["prev"], a["a_from"], a["a_t"], a["a_to"], a["out"], a["x0"], a["win"],
                                         a["n"], a["W"], a["H"], a["flags"], _native._stream_ptr())

    for bad in (dict(x=None), dict(out=None), dict(n=0), dict(W=10), dict(W=16, H=4), dict(flags=4), dict(out=ok["x"]),
                dict(x0=ok["prev"] + 16), dict(win=ok["eps"]), dict(win=ok["out"]), dict(win=ok["prev"], x0=ok["prev"])):
        assert wcall(**bad) == -1, bad
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(x0).all() and torch.isnan(win).all()
    assert call() == 0 and wcall(x0=ok["prev"]) == 0  # ... and the good calls, the in-place history among them, are taken
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 3. windows
def window_inputs(n, W, H, dev, seed=11):
    Np = (n - 1) * H + W
    host = [seeded((Np,), seed).numpy(), seeded((n, W), seed + 1).numpy(), (0.5 * seeded((n, W), seed + 2)).numpy(),
            (0.3 * seeded((Np,), seed + 3)).clamp(-1, 1).numpy()]
    return host, [to_dev(a, dev) for a in host]


def scalar(v, dev):
    return torch.tensor([float(v)], dtype=torch.float32, device=dev)


def test_one_window_is_the_single_clip_step_bit_for_bit(dev):
    n, W, H = WINDOW_SHAPES[0]
    _, (x, eps, grad, prev) = window_inputs(n, W, H, dev)
    a_from, a_t, a_to = scalar(0.25, dev), scalar(0.3, dev), scalar(0.37, dev)
    for history, (name, guided, flags) in itertools.product((False, True), VARIANTS):
        g, p, af = grad if guided else None, prev if history else None, a_from if history else None
        got, got0, win = windows_call(x, eps, g, p, af, a_t, a_to, n, W, H, flags)
        want, want0 = step_call(x.view(1, W), eps, g, None if p is None else p.view(1, W), af, a_t, a_to, flags)
        assert torch.equal(got, want[0]) and torch.equal(got0, want0[0]) and torch.equal(win[0], want[0]), (history, name)


def test_no_overlap_without_constrain_is_one_long_row_bit_for_bit(dev):
    n, W, H = WINDOW_SHAPES[3]
    _, (x, eps, grad, prev) = window_inputs(n, W, H, dev)
    a_from, a_t, a_to = scalar(0.25, dev), scalar(0.3, dev), scalar(0.37, dev)
    for history, guided in itertools.product((False, True), (False, True)):
        g, p, af = grad if guided else None, prev if history else None, a_from if history else None
        got, got0, win = windows_call(x, eps, g, p, af, a_t, a_to, n, W, H, 0)
        want, want0 = step_call(x.view(1, -1), eps.view(1, -1), None if g is None else g.view(1, -1), None if p is None else p.view(1, -1), af,
                                a_t, a_to, 0)
        assert torch.equal(got, want[0]) and torch.equal(got0, want0[0]) and torch.equal(win.view(-1), want[0]), (history, guided)


@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("n,W,H", WINDOW_SHAPES)
def test_windows_vs_oracle(dev, schedule, n, W, H):
    """The general case under the bounds of test 1, with C = 12 / 9 where two windows meet (dpmpp_ref: C_BLEND, C_X0_BLEND): {no history,
    history in the long layout} x the four variants x the three triples; the window output is the state gathered, the optional output
    changes nothing, and the history may be updated in place."""
    host, (x, eps, grad, prev) = window_inputs(n, W, H, dev, seed=21)
    worst = 0.0
    for first in range(3):
        al = dpmpp_ref.alphas(schedule, 1, first)
        a_from, a_t, a_to = (to_dev(a, dev) for a in al)
        for history, (name, guided, flags) in itertools.product((False, True), VARIANTS):
            want, want_win, want0, M, x0m, Cn, C0 = dpmpp_ref.step_windows(host[0], host[1], al[1], al[2], n, W, H, grad=host[2] if guided else None,
                                                                           constrain=bool(flags), x0_prev=host[3] if history else None,
                                                                           a_from=al[0] if history else None)
            g, p, af = grad if guided else None, prev if history else None, a_from if history else None
            got, got0, win = windows_call(x, eps, g, p, af, a_t, a_to, n, W, H, flags)
            frac, frac0 = fraction(got, want, dpmpp_ref.bound(M, Cn)), fraction(got0, want0, dpmpp_ref.bound(x0m, C0))
            print(f"dpmpp windows {schedule} (n, W, H)=({n}, {W}, {H}) first={first} history={history} {name}: x_to {frac:.3f}, x0 {frac0:.3f} of the bound")
            assert frac <= 1.0 and frac0 <= 1.0, (first, history, name, frac, frac0)
            assert torch.equal(win, got.unfold(0, W, H))  # d_windows[b, j] == d_x_to[b * H + j]
            assert fraction(win, want_win, ddim_ref.window_view(dpmpp_ref.bound(M, Cn), n, W, H)) <= 1.0
            worst = max(worst, frac, frac0)
            alone, alone0, _ = windows_call(x, eps, g, p, af, a_t, a_to, n, W, H, flags, want_windows=False)
            assert torch.equal(alone, got) and torch.equal(alone0, got0)
            if history:
                hist = prev.clone()
                in_place, _, _ = windows_call(x, eps, g, hist, af, a_t, a_to, n, W, H, flags, x0_into=hist)
                assert torch.equal(in_place, got) and torch.equal(hist, got0)
    record(f"3 dpmpp windows vs oracle {schedule} (n, W, H)=({n}, {W}, {H})", worst)


# ---------------------------------------------------------------- 4. the loops against hand-chained calls, bit for bit
def clip_predictor(x, ts):
    return torch.tanh(x) * 0.5 + ts.view(-1, 1, 1)


def clip_cond_fn(x, ts):
    return torch.sin(2 * x) * (0.2 + ts.view(-1, 1, 1))


@pytest.mark.parametrize("case", ["plain", "constrain", "cond_fn", "start_step+keep"])
def test_dpmpp_sample_is_the_hand_chained_calls(dev, case):
    B, T, steps, seed, clip = 2, 260, 6, 11, 5
    d = Diffusion(make_schedule("exp"))
    x_T = seeded((B, 1, T), 41).to(dev)
    constrain, cond_fn = case == "constrain", clip_cond_fn if case == "cond_fn" else None
    kw, start, source, keep = {}, 0, None, None
    if case == "start_step+keep":
        start, source = 2, (0.3 * seeded((B, 1, T), 42)).clamp(-1, 1).to(dev)
        keep = torch.zeros(B, 1, T, dtype=torch.bool, device=dev)
        keep[..., 50:131] = True
        kw = dict(source=source, keep=keep, start_step=start)
    seen = []

    def noise(i):
        seen.append(i)
        return torch.zeros_like(x_T)

    out = d.dpmpp_sample(x_T, clip_predictor, steps, constrain=constrain, cond_fn=cond_fn, noise=noise, seed=seed, clip_offset=clip, **kw)
    assert not seen and out.shape == x_T.shape and bool(torch.isfinite(out).all())
    ts_all, a_t_all, a_to_all, _ = d.step_tables(steps, B, None, dev)
    x, x0, ts_from = x_T, None, None
    if start:
        x = d.keep_region(torch.zeros_like(source), source, a_t_all[start], None, seed=seed, clip_offset=clip, index=start)
    for i in range(start, steps):
        x, x0 = d.dpmpp_previous(x, ts_all[i], 1 / steps, clip_predictor(x, ts_all[i]), x0_prev=x0, ts_from=ts_from, constrain=constrain,
                                 cond_fn=cond_fn)
        ts_from = ts_all[i]
        if keep is not None:
            x = d.keep_region(x, source, a_to_all[i], keep, seed=seed, clip_offset=clip, index=i + 1)
    assert torch.equal(out, x), (case, (out - x).abs().max().item())
    if keep is not None:
        assert torch.equal(out[keep], source[keep])  # alpha_bar = 1 after the last step: the source itself
    # the history matters: the run is not the eta = 0 DDIM run, and it is deterministic
    assert not torch.equal(out, d.ddim_sample(x_T, clip_predictor, steps, constrain=constrain, cond_fn=cond_fn, seed=seed, clip_offset=clip, **kw))
    assert torch.equal(out, d.dpmpp_sample(x_T, clip_predictor, steps, constrain=constrain, cond_fn=cond_fn, seed=seed, clip_offset=clip, **kw))


def test_dpmpp_sample_windows_is_the_hand_chained_calls(dev):
    n, W, H, steps = 3, 16, 12, 6
    Np = (n - 1) * H + W
    d = Diffusion(make_schedule("exp"))
    x_T = seeded((1, 1, Np), 43).to(dev)

    def predictor(w, ts, first):
        return torch.tanh(w) * 0.5 + ts.view(-1, 1, 1) + 0.01 * first

    def cond_fn(w, ts, first):
        return torch.sin(2 * w) * (0.2 + ts.view(-1, 1, 1))

    for constrain, guide, wb in ((False, None, 3), (True, cond_fn, 3), (True, cond_fn, 2)):
        out = d.dpmpp_sample_windows(x_T, predictor, steps, window=W, hop=H, window_batch=wb, constrain=constrain, cond_fn=guide)
        ts_all, a_t_all, a_to_all, _ = d.step_tables(steps, min(n, wb), None, dev)
        x, windows, x0, a_from = x_T.reshape(-1).contiguous(), longform.gather_windows(x_T, W, H), None, None
        for i in range(steps):
            eps, grad = torch.empty_like(windows), torch.empty_like(windows) if guide else None
            for b0 in range(0, n, wb):
                m = min(wb, n - b0)
                eps[b0:b0 + m] = predictor(windows[b0:b0 + m], ts_all[i, :m], b0)
                if guide:
                    grad[b0:b0 + m] = guide(windows[b0:b0 + m], ts_all[i, :m], b0)
            x, x0, windows = windows_call(x, eps, grad, x0, a_from, a_t_all[i], a_to_all[i], n, W, H, CONSTRAIN if constrain else 0)
            windows, a_from = windows.reshape(n, 1, W).contiguous(), a_t_all[i]
        assert torch.equal(out.reshape(-1), x), (constrain, guide is not None, wb)
        assert not torch.equal(out, d.ddim_sample_windows(x_T, predictor, steps, window=W, hop=H, window_batch=wb, constrain=constrain, cond_fn=guide))


# ---------------------------------------------------------------- 5. the analytic model on the device
@pytest.mark.parametrize("schedule,power", dpmpp_ref.GRIDS)
def test_analytic_model_on_the_device(dev, schedule, power):
    """The model of tests/test_dpmpp.py with the predictor ONE float32 multiply by a per-step scalar (float64, rounded once): at 40
    steps `dpmpp_sample`'s relative error of x_0 against the closed form is at most half `ddim_sample(eta=0)`'s, and the run agrees
    with the float64 chain inside the per-step bounds carried through the chain (dpmpp_ref.chain_bound)."""
    B, T, steps = 2, 64, dpmpp_ref.ANALYTIC_STEPS
    remap, a_t_all, a_to_all = dpmpp_ref.analytic_tables(schedule, power, B)
    d = Diffusion(make_schedule(schedule))
    x_T = seeded((B, 1, T), 61)
    scalars = [dpmpp_ref.analytic_scalar(a_t_all[i]) for i in range(steps)]
    table = torch.tensor(np.stack(scalars), dtype=torch.float32, device=dev)  # [steps, B]: rounded to float32 once

    def run(sample, **kw):
        calls = []

        def predictor(x, ts):
            calls.append(ts)
            return table[len(calls) - 1].view(B, 1, 1) * x

        out = sample(x_T.to(dev), predictor, steps, schedule=remap, **kw)
        assert len(calls) == steps
        return out.cpu().double().numpy().reshape(B, T)

    x64 = x_T.double().numpy().reshape(B, T)
    exact = dpmpp_ref.analytic_exact(x64, a_t_all[0])
    first = np.abs(run(d.ddim_sample, eta=0.0) - exact).max() / np.abs(exact).max()
    got = run(d.dpmpp_sample)
    second = np.abs(got - exact).max() / np.abs(exact).max()
    print(f"analytic model on the device {schedule} / t**{power or 1}, {steps} steps: ddim_sample {first:.3e}, dpmpp_sample {second:.3e}, ratio {first / second:.2f}")
    assert second <= 0.5 * first, (schedule, power, first, second)
    want, trace = dpmpp_ref.chain(x64, a_t_all, a_to_all, lambda x, i: scalars[i].reshape(B, 1) * x, order=2)
    E = dpmpp_ref.chain_bound(trace, scalars)
    err = np.abs(got - want)
    frac = float(np.max(np.where(err == 0, 0.0, err / np.maximum(E, 1e-300))))
    print(f"analytic model on the device {schedule} / t**{power or 1}: {frac:.3f} of the chained bound (largest bound {E.max():.3e}, largest |x_0| {np.abs(want).max():.3e})")
    assert frac <= 1.0, (schedule, power, frac)
    record(f"5 dpmpp_sample vs float64 chain, analytic model {schedule} / t**{power or 1}, chained bound", frac)


# ---------------------------------------------------------------- 6. end to end
@pytest.fixture(scope="module")
def vqvae(dev):
    m = VQVAE(base_channels=32, pred_name="unet", num_labels=3)
    det_init_(m.state_dict().items())
    m.eval()
    m.to(dev)
    m.set_precision("fp32")
    return m


def test_vqvae_decode_and_decode_long(dev, vqvae):
    W, H, steps = 2048, 1536, 4
    wave = (0.3 * seeded((1, 1, W), 72)).clamp(-1, 1).to(dev)
    codes = vqvae.encode(wave)
    dst = torch.tensor([2], device=dev)
    kw = dict(steps=steps, constrain=True, sampler="dpmpp")
    x_T = torch.randn(1, 1, W, generator=torch.Generator().manual_seed(3)).to(dev)
    fixed = vqvae.decode(codes, dst, x_T=x_T, seed=1, **kw)
    assert fixed.shape == (1, 1, W) and bool(torch.isfinite(fixed).all())
    assert torch.equal(fixed, vqvae.decode(codes, dst, x_T=x_T, seed=2, **kw))  # x_T alone decides
    assert not torch.equal(fixed, vqvae.decode(codes, dst, x_T=x_T, seed=1, **dict(kw, sampler="ddim")))
    with pytest.raises(ValueError):
        vqvae.decode(codes, dst, x_T=x_T, eta=0.5, **kw)
    guided = vqvae.decode_uncond_guidance(codes, torch.tensor([0], device=dev), steps=steps, vq_scale=1.5, x_T=x_T, sampler="dpmpp")
    assert guided.shape == (1, 1, W) and bool(torch.isfinite(guided).all())
    # two windows
    N = 3000
    n, padded = plan_windows(N, W, H)
    assert (n, padded) == (2, 3584)
    long_wave = (0.3 * seeded((1, 1, N), 73)).clamp(-1, 1).to(dev)
    long_codes = vqvae.encode_long(long_wave, W, H)
    lkw = dict(num_samples=N, window=W, hop=H, steps=steps, constrain=True, clip_offset=5, sampler="dpmpp")
    long_out = vqvae.decode_long(long_codes, dst, seed=9, window_batch=2, **lkw)
    assert long_out.shape == (1, 1, N) and bool(torch.isfinite(long_out).all())
    assert torch.equal(long_out, vqvae.decode_long(long_codes, dst, seed=9, window_batch=1, **lkw))
    assert not torch.equal(long_out, vqvae.decode_long(long_codes, dst, seed=9, **dict(lkw, sampler="ddim")))
    # one window: decode_long is decode, as for the other samplers
    assert torch.equal(vqvae.decode_long(codes, dst, seed=9, **dict(lkw, num_samples=W)), vqvae.decode(codes, dst, seed=9, clip_offset=5, **kw))


@pytest.mark.parametrize("whole_file", [False, True])
def test_sample_vqvae_with_the_new_sampler(dev, vqvae, tmp_path, whole_file):
    """`sample_vqvae.py --sampler dpmpp`, alone and with --keep / --strength, with and without --whole-file: the files are written, the
    plain run is repeatable and differs from DDIM's, and the kept range is the input on the writer's
    s16 grid (tests/test_keep_gpu.py)."""
    sys.path.insert(0, ROOT)
    import sample_vqvae

    ck, src, echo = (str(tmp_path / name) for name in ("v.pt", "in.wav", "echo.wav"))
    vqvae.save(ck)
    rate = 16000
    N = 8000 if whole_file else rate  # 0.5 s in windows of 0.128 s; or the first --seconds 1
    w = ChunkWriter(src, rate)
    w.write(0.3 * np.sin(np.arange(N) * 0.05).astype(np.float32))
    w.close()
    r = ChunkReader(src, rate)
    samples = r.read(N)
    r.close()
    w = ChunkWriter(echo, rate)
    w.write(samples)
    w.close()
    usable = N if whole_file else N // 256 * 256  # a single clip is cut to a multiple of the model's rate
    want = read_s16(echo)[:usable]
    a, b = round(0.1 * rate), round(0.25 * rate)
    common = ["--label", "2", "--input-file", src, "--sample-steps", "4", "--seed", "9"]
    common += ["--whole-file", "--window-seconds", "0.128", "--overlap-seconds", "0.032", "--window-batch", "2"] if whole_file else ["--seconds", "1"]
    outs = {}
    for name, flags in (("dpmpp", ["--sampler", "dpmpp"]), ("again", ["--sampler", "dpmpp"]), ("ddim", ["--sampler", "ddim"]),
                        ("kept", ["--sampler", "dpmpp", "--keep", "0.1:0.25", "--strength", "0.5"])):
        dst = str(tmp_path / f"{name}.wav")
        sample_vqvae.main(common + flags + [ck, dst])
        outs[name] = read_s16(dst)
        assert outs[name].shape == want.shape, name
    assert np.array_equal(outs["dpmpp"], outs["again"]) and not np.array_equal(outs["dpmpp"], outs["ddim"])
    assert np.array_equal(outs["kept"][a:b], want[a:b]) and not np.array_equal(outs["dpmpp"][a:b], want[a:b])
    rest = np.concatenate([outs["kept"][:a] != want[:a], outs["kept"][b:] != want[b:]])
    assert rest.mean() > 0.5, rest.mean()
