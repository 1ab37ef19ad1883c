"""float64 numpy restatement of `vqvs_dpmpp_step` and `vqvs_dpmpp_step_windows` (include/vqvs.h): the oracle of tests/test_dpmpp.py
and tests/test_dpmpp_gpu.py, in the manner of tests/ddim_ref.py, whose x0 prediction (`_x0_eps`), magnitudes and float32 helpers it
uses.  Inputs are float32 values (the alphas are rounded to float32 first, as the kernels receive them; a float64 state, prediction
or history is taken as it is, so that steps can be chained without a rounding between them) and ALL arithmetic is float64.  The
reference project has no such solver: tests/test_dpmpp.py ties this file, at first order, to `ddim_ref.step(eta=0)`, which
tests/test_ddim.py ties to the reference-pinned `oracle.ref_cpu.ddpm_previous`.

The step (Lu et al. 2022, "DPM-Solver++", Algorithm 2, in alpha_bar): alpha = sqrt(a), sigma = sqrt(1 - a),
lambda(a) = (log a - log1p(-a)) / 2, h = lambda(a_to) - lambda(a_t), h_prev = lambda(a_t) - lambda(a_from), q = h / (2 h_prev),
    x_to = c_x x + c0 x0 + c1 x0_prev,   c_x = sigma_to / sigma_t,  phi = alpha_to - sigma_to alpha_t / sigma_t,  c0 = phi (1 + q),  c1 = -phi q
and q = 0 -- first order, x0_prev not read -- without a history, at 1 - a_to == 0, when h_prev is not > 0 or q is not finite.

Besides the values every function returns M, per element: the sum of the absolute values of the terms that meet in the output, each
carried through the factors applied to it,
    M   = |c_x| |x| + |c0| X0M + |c1| |x0_prev|
    X0M = rsat * (|x| + sq1mat * (|eps| + sq1mat * |g|)) + |mean|                                     (ddim_ref's)
(c0 and c1 have opposite signs and |c0| = |phi| (1 + q) exceeds |phi|: M carries the two magnitudes, not phi), and where two windows
meet, with w on the right one, X0M = (1 + w) X0M_l + w X0M_r: the magnitudes of fmaf(w, right - left, left) as it is written.

The bound on x_to is |got - want| <= C * 2^-24 * M, C being the number of float32 roundings on the longest path from an input to the
output in the kernel AS WRITTEN (csrc/sampler_kernels.hip: dpmpp_coef, ddim_x0_eps, dpmpp_out), each use of a rounded coefficient
counted.  The longest path starts at the gradient and runs through x0:
     1  sq1mat (coefficient, fp64 -> fp32)        2  e = fmaf(-sq1mat, g, eps)
     3  sq1mat again                              4  fmaf(-sq1mat, e, x)
     5  rsat                                      6  x0 = fmaf(., rsat, -mean)  /  . * rsat      (the clamp does not round)
     7  c0                                        8  fmaf(c0, x0, c1 * x0_prev)  /  c0 * x0
     9  out = fmaf(c_x, x, .)
C_STEP = 9.  (The other paths are shorter: the mean is summed in fp64 and rounded once: mean, x0, c0, inner, out = 5; the history:
c1, c1 * x0_prev, inner fmaf, out = 4; x itself: c_x, out = 2.)  `d_x0_out` is x0 as it stands after rounding 6, under
|got - want| <= C_X0 * 2^-24 * X0M with C_X0 = 6.  Where two windows meet the path to x0 goes on through the blend: w = (u + 1/2) / V
(one division), right - left, fmaf: C_BLEND = 12 and C_X0_BLEND = 9.  These counts are a derivation, not a measurement.

A chain of steps on the analytic model of tests/test_dpmpp.py (eps = c_i x, ONE float32 multiply by a per-step scalar) is LINEAR in the
state, x0 = m_i x with m_i = (1 - sigma_t c_i) / alpha_t, so a device run is held to the float64 chain by carrying each step's own
bound through the later steps' coefficients (`chain_bound`):
    d0_i    = C_X0 * 2^-24 * X0M_i + 2 * 2^-24 * rsat sq1mat |c_i| |x_i|        x0 against m_i x AT THE DEVICE'S OWN x (the second term: c_i
                                                                                 rounded to float32, and the multiply)
    G_i     = |m_i| E_i + d0_i                                                   the history's error
    E_{i+1} = (|c_x| + |c0| |m_i|) E_i + |c1| G_{i-1} + C_STEP * 2^-24 * M_i + |c0| * 2 * 2^-24 * rsat sq1mat |c_i| |x_i|
with E_0 = 0 and the magnitudes taken at |x_i| + E_i."""
import numpy as np

import ddim_ref
from ddim_ref import D, F, U, fmaf, window_view

C_STEP, C_X0, C_BLEND, C_X0_BLEND = 9, 6, 12, 9


def lam(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 0.5 * (np.log(a) - np.log1p(-a))


def coef(a_t, a_to, a_from=None, history=True):
    """The per-row scalars, float64 arrays shaped like a_t (float32 alphas in, as the kernel receives them), and `second`, the rows
    that take the second-order form.  a_from None, or history False (no x0_prev): first order everywhere."""
    at, ato = np.asarray(a_t, dtype=F).astype(D), np.asarray(a_to, dtype=F).astype(D)
    k = {name: v for name, v in ddim_ref.coef(a_t, a_to).items() if name in ("sq1mat", "rsat", "sqat", "rs1mat")}  # (`_x0_eps` reads the four)
    with np.errstate(divide="ignore", invalid="ignore"):
        sig_to = np.sqrt(1.0 - ato)
        phi = np.sqrt(ato) - sig_to * np.sqrt(at) / k["sq1mat"]
        q, second = np.zeros_like(at), np.zeros(at.shape, dtype=bool)
        if a_from is not None and history:
            af = np.asarray(a_from, dtype=F).astype(D)
            h, h_prev = lam(ato) - lam(at), lam(at) - lam(af)
            q = h / (2.0 * h_prev)
            second = (1.0 - ato != 0.0) & (h_prev > 0.0) & np.isfinite(q)
            q = np.where(second, q, 0.0)
        k.update(cx=sig_to / k["sq1mat"], phi=phi, q=q, c0=phi * (1.0 + q), c1=-phi * q, second=second)
    return k


def _row_coef(a_t, a_to, a_from, history, B):
    flat = lambda a: None if a is None else np.reshape(a, B)
    return {name: v.reshape(B, 1) for name, v in coef(flat(a_t), flat(a_to), flat(a_from), history).items()}


def _combine(k, x, x0, x0m, x0_prev):
    """(x_to, M) of the output line; x0_prev is read only on the second-order rows."""
    p = np.zeros_like(x) if x0_prev is None else np.where(k["second"], np.asarray(x0_prev, dtype=D).reshape(x.shape), 0.0)
    return k["cx"] * x + k["c0"] * x0 + k["c1"] * p, np.abs(k["cx"]) * np.abs(x) + np.abs(k["c0"]) * x0m + np.abs(k["c1"]) * np.abs(p)


def step(x, eps, a_t, a_to, grad=None, constrain=False, x0_prev=None, a_from=None):
    """x, eps, grad, x0_prev [B, T]; a_t, a_to, a_from [B] -> (x_to, x0, M, X0M), float64."""
    x, eps = np.asarray(x, dtype=D), np.asarray(eps, dtype=D)
    B = x.shape[0]
    k = _row_coef(a_t, a_to, a_from, x0_prev is not None, B)
    grad = None if grad is None else np.asarray(grad, dtype=D)
    x0, _, x0m, _ = ddim_ref._x0_eps(k, x, eps, grad, constrain)
    out, M = _combine(k, x, x0, x0m, x0_prev)
    return out, x0, M, x0m


def step_windows(x, eps, a_t, a_to, n, W, H, grad=None, constrain=False, x0_prev=None, a_from=None):
    """x, x0_prev [Np], eps / grad [n, W], scalar alphas -> (x_to [Np], windows [n, W], x0 [Np], M, X0M, C, C0), float64: x0 is the
    BLENDED prediction, the history of the next step; C / C0 are C_BLEND / C_X0_BLEND where two windows meet and C_STEP / C_X0
    elsewhere."""
    V, Np = W - H, (n - 1) * H + W
    assert n >= 1 and W % 4 == 0 and H % 4 == 0 and 0 <= V <= H
    x, eps = np.asarray(x, dtype=D).reshape(Np), np.asarray(eps, dtype=D).reshape(n, W)
    grad = None if grad is None else np.asarray(grad, dtype=D).reshape(n, W)
    k = coef(np.reshape(a_t, ()), np.reshape(a_to, ()), None if a_from is None else np.reshape(a_from, ()), x0_prev is not None)
    per_window = ddim_ref._x0_eps(k, window_view(x, n, W, H), eps, grad, constrain)
    x0, x0m = np.empty(Np), np.empty(Np)
    two = np.zeros(Np, dtype=bool)
    w = (np.arange(V) + 0.5) / V if V else None
    for dst, src, mag in ((x0, per_window[0], False), (x0m, per_window[2], True)):
        dst[:W] = src[0]
        for b in range(1, n):  # window b is the RIGHT window of the overlap [b * H, b * H + V) and alone behind it
            lo = b * H
            if V:
                left, right = src[b - 1, H:], src[b, :V]
                dst[lo:lo + V] = (1 + w) * left + w * right if mag else left + w * (right - left)
                two[lo:lo + V] = True
            dst[lo + V:lo + W] = src[b, V:]
    out, M = _combine(k, x, x0, x0m, None if x0_prev is None else np.asarray(x0_prev, dtype=D).reshape(Np))
    return out, window_view(out, n, W, H), x0, M, x0m, np.where(two, float(C_BLEND), float(C_STEP)), np.where(two, float(C_X0_BLEND), float(C_X0))


def bound(M, C=C_STEP):
    """C * 2^-24 * M."""
    return np.asarray(C) * U * M


# ---- float32 evaluation of the specified formulas (what the kernel does, in numpy): tests/test_dpmpp.py holds it to the bound ----
def step_f32(x, eps, a_t, a_to, grad=None, constrain=False, x0_prev=None, a_from=None):
    """`step` in the kernel's arithmetic -> (x_to, x0) float32: coefficients rounded to float32 once, the per-sample operations of
    ddim_x0_eps / dpmpp_out in float32, the mean summed in float64 from the float32 inputs and rounded once."""
    x, eps = np.asarray(x, dtype=F), np.asarray(eps, dtype=F)
    B = x.shape[0]
    kd = _row_coef(a_t, a_to, a_from, x0_prev is not None, B)
    k = ddim_ref.rounded({name: kd[name] for name in ("sq1mat", "rsat", "cx", "c0", "c1")})
    e = eps
    if grad is not None:
        grad = np.asarray(grad, dtype=F)
        e = fmaf(-k["sq1mat"], grad, eps)
    if constrain:
        ed = eps.astype(D) - (kd["sq1mat"] * grad.astype(D) if grad is not None else 0.0)
        mean = ((x.astype(D) - kd["sq1mat"] * ed) * kd["rsat"]).mean(axis=-1, keepdims=True).astype(F)
        x0 = np.clip(fmaf(fmaf(-k["sq1mat"], e, x), k["rsat"], -mean), F(-1), F(1))
    else:
        x0 = fmaf(-k["sq1mat"], e, x) * k["rsat"]
    first = fmaf(k["cx"], x, k["c0"] * x0)
    out = first
    if x0_prev is not None:
        p = np.asarray(x0_prev, dtype=F).reshape(x.shape)
        with np.errstate(invalid="ignore", over="ignore"):
            out = np.where(kd["second"], fmaf(k["cx"], x, fmaf(k["c0"], x0, k["c1"] * p)), first)
    assert out.dtype == F and x0.dtype == F
    return out, x0


# ---- chains: the sampling loop on float64 states, and the bound of a device run of the linear model against it ----
def chain(x_T, a_t_all, a_to_all, predictor, order=2, constrain=False, cond_fn=None, start=0):
    """Steps start .. len - 1 of a run over the table rows a_t_all / a_to_all [steps, B] (`Diffusion.step_tables`), float64 throughout:
    `predictor(x, i)` -> eps, `cond_fn(x, i)` -> grad.  order 2 hands every step but the first the x0 and the a_t of the step before
    (the kernel's own rule makes the last one, to alpha_bar = 1, first order); order 1 hands none: the eta = 0 DDIM chain.
    Returns (x_0, [per step: dict(x, eps, x0_prev, x0, x_to, M, X0M, k)])."""
    x, x0_prev, a_from, trace = np.asarray(x_T, dtype=D), None, None, []
    B = x.shape[0]
    for i in range(start, len(a_t_all)):
        eps = np.asarray(predictor(x, i), dtype=D)
        g = None if cond_fn is None else cond_fn(x, i)
        hist = dict(x0_prev=x0_prev, a_from=a_from) if order == 2 else {}
        x_to, x0, M, x0m = step(x, eps, a_t_all[i], a_to_all[i], grad=g, constrain=constrain, **hist)
        trace.append(dict(x=x, eps=eps, x0_prev=hist.get("x0_prev"), x0=x0, x_to=x_to, M=M, X0M=x0m,
                          k=_row_coef(a_t_all[i], a_to_all[i], hist.get("a_from"), hist.get("x0_prev") is not None, B)))
        x, x0_prev, a_from = x_to, x0, a_t_all[i]
    return x, trace


def chain_bound(trace, scalars):
    """The bound E on |device - float64 chain| after the last step of `trace` (of `chain`, un-guided, un-constrained) when the
    predictor is eps = float32(c_i) * x in float32, `scalars[i]` = c_i in float64 per row [B]: the recursion of the docstring."""
    E = np.zeros_like(trace[0]["x"])
    G_prev = np.zeros_like(E)
    for t, c in zip(trace, scalars):
        k = t["k"]
        c = np.abs(np.asarray(c, dtype=D)).reshape(-1, 1)
        ax = np.abs(t["x"]) + E
        ae = c * ax
        x0m = k["rsat"] * (ax + k["sq1mat"] * ae)
        pred = 2 * U * k["rsat"] * k["sq1mat"] * ae
        m = np.abs((1.0 - k["sq1mat"] * c) * k["rsat"])
        hist_err = np.where(k["second"], G_prev, 0.0)  # (the history is read on the second-order rows alone)
        hist_mag = 0.0 if t["x0_prev"] is None else np.where(k["second"], np.abs(t["x0_prev"]) + G_prev, 0.0)
        M = np.abs(k["cx"]) * ax + np.abs(k["c0"]) * x0m + np.abs(k["c1"]) * hist_mag
        G = m * E + C_X0 * U * x0m + pred
        E = (np.abs(k["cx"]) + np.abs(k["c0"]) * m) * E + np.abs(k["c1"]) * hist_err + C_STEP * U * M + np.abs(k["c0"]) * pred
        G_prev = G
    return E


# ---- the cases of the kernel test, shared by the CPU and the GPU file ----
TRIPLES = [(1.0, 0.9, 0.1), (0.32, 0.3, 0.02), (0.04, 0.02, 0.02)]  # (t_from, t, step): an early step, a middle one, the last one (a_to = 1)


def alphas(schedule, B, first):
    """float32 (a_from, a_t, a_to) [B]: row b is at TRIPLES[(first + b) % 3], so every triple is met at every shape and rows differ."""
    import torch

    from oracle import ref_cpu

    cols = [torch.tensor([TRIPLES[(first + b) % 3][k] for b in range(B)], dtype=torch.float32) for k in range(3)]
    return tuple(ref_cpu.schedule_alpha(schedule, t).numpy() for t in (cols[0], cols[1], cols[1] - cols[2]))


def history_input(B, T, seed=105):
    """float32 numpy x0_prev [B, T] of the kernel test: a plausible earlier prediction, inside [-1, 1]."""
    import torch

    return torch.randn((B, T), generator=torch.Generator().manual_seed(seed)).mul(0.3).clamp(-1, 1).numpy()


# ---- the analytic model: data N(0, s^2) per sample, whose probability-flow ODE has a closed-form solution ----
S_DATA, ANALYTIC_STEPS = 0.3, 40
GRIDS = [("exp", None), ("exp", 2), ("cos", None), ("cos", 2)]  # (alpha_bar schedule, P of the sample-time remap t**P)


def analytic_scalar(a, s=S_DATA):
    """c with eps*(x, t) = c x: sqrt(1 - a) / (a s^2 + 1 - a), float64, from float32 alphas."""
    a = np.asarray(a, dtype=F).astype(D)
    return np.sqrt(1.0 - a) / (a * s * s + 1.0 - a)


def analytic_exact(x_T, a_T, s=S_DATA):
    """x_0 = x_T s / sqrt(a_T s^2 + 1 - a_T), float64."""
    a = np.asarray(a_T, dtype=F).astype(D).reshape(-1, *([1] * (np.ndim(x_T) - 1)))
    return np.asarray(x_T, dtype=D) * s / np.sqrt(a * s * s + 1.0 - a)


def analytic_tables(schedule, power, B, steps=ANALYTIC_STEPS):
    """(remap or None, a_t_all, a_to_all [steps, B] float32 numpy) of `Diffusion.step_tables` on the host."""
    import torch

    from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

    remap = None if power is None else (lambda t: t ** power)
    _, a_t_all, a_to_all, _ = Diffusion(make_schedule(schedule)).step_tables(steps, B, remap, torch.device("cpu"))
    return remap, a_t_all.numpy(), a_to_all.numpy()
