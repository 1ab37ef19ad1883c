"""float64 numpy restatement of `vqvs_ddim_step` and `vqvs_ddim_step_windows` (include/vqvs.h): the oracle of tests/test_ddim.py and
tests/test_ddim_gpu.py.  Inputs are float32 values (the alphas are rounded to float32 first, as the kernels receive them; a float64
state is taken as it is, so that two steps can be chained without a rounding between them) and ALL arithmetic is float64.  The
reference project has no DDIM: tests/test_ddim.py ties this file, at eta = 1, to the reference-pinned `oracle.ref_cpu.ddpm_previous`.

Besides the value every function returns M, per element: the sum of the absolute values of the terms that meet in the output, each
carried through the factors applied to it,
    M   = sqto * X0M + ce * E + sig * |noise_scale z|
    X0M = rsat * (|x| + sq1mat * (|eps| + sq1mat * |g|)) + |mean|
    E   = |eps| + sq1mat * |g|                 without CONSTRAIN
    E   = rs1mat * (|x| + sqat * |x0c|)        with CONSTRAIN (x0c: the clamped x0)
and where two windows meet, with w on the right one, X0M = (1 + w) X0M_l + w X0M_r and E likewise: the magnitudes of
fmaf(w, right - left, left) as it is written.

The bound on a kernel's output is |got - want| <= C * 2^-24 * M, C being the number of float32 roundings on the longest path from an
input to the output in the kernel AS WRITTEN (csrc/sampler_kernels.hip: ddim_coef, ddim_x0_eps, ddim_sample), each use of a rounded
coefficient counted.  The longest path starts at the gradient and runs through CONSTRAIN:
     1  sq1mat (coefficient, fp64 -> fp32)        2  e = fmaf(-sq1mat, g, eps)
     3  sq1mat again                              4  fmaf(-sq1mat, e, x)
     5  rsat                                      6  x0 = fmaf(., rsat, -mean)      (the clamp does not round)
     7  sqat                                      8  fmaf(-x0, sqat, x)
     9  rs1mat                                   10  e' = . * rs1mat
    11  ce                                       12  fmaf(ce, e', sig * nv)
    13  out = fmaf(sqto, x0, .)
C_STEP = 13.  (The other paths are shorter: x0 reaches the output through sqto as well, but an error d of x0 arrives as
(sqto - ce sqat rs1mat) d with 0 <= ce sqat rs1mat <= sqto whenever a_to >= a_t, so no more than sqto |d|, which M's first term carries;
the mean is summed in fp64 and rounded once: mean, x0, sqto, out = 4; the noise: sig, noise_scale * z, their product, two fmaf = 5.)
Where two windows meet the path goes on through the blend: w = (u + 1/2) / V (one division), right - left, fmaf: C_BLEND = 16.
With generated noise the generator's own tolerance is added: sig * (1.2e-5 + 3 * 2^-24 |z|) (tests/test_rng_gpu.py)."""
import numpy as np

F, D = np.float32, np.float64
U = 2.0 ** -24
C_STEP, C_BLEND = 13, 16
NORMAL_ABS = 1.2e-5
SUM_CHUNK = 4096


def coef(a_t, a_to, eta=0.0, invert=False):
    """The per-row scalars, float64 arrays shaped like a_t (float32 alphas in, as the kernel receives them; eta as float32)."""
    at, ato = np.asarray(a_t, dtype=F).astype(D), np.asarray(a_to, dtype=F).astype(D)
    om = 1.0 - at
    with np.errstate(divide="ignore", invalid="ignore"):
        sig = float(F(eta)) * np.sqrt(np.maximum((1.0 - ato) / om, 0.0)) * np.sqrt(np.maximum(1.0 - at / ato, 0.0))
        sig = np.where(np.logical_or(invert, om == 0.0), 0.0, sig)
        k = dict(sq1mat=np.sqrt(om), rsat=1.0 / np.sqrt(at), sqat=np.sqrt(at), rs1mat=1.0 / np.sqrt(om), sqto=np.sqrt(ato), sig=sig,
                 ce=np.sqrt(np.maximum(1.0 - ato - sig * sig, 0.0)))
    return k


def rounded(k):
    """The coefficients as the kernel holds them: each rounded to float32 once."""
    return {name: np.asarray(v, dtype=D).astype(F) for name, v in k.items()}


def _x0_eps(k, x, eps, grad, constrain):
    """(x0, e', X0M, E) of rows [R, T] under coefficients shaped [R, 1] (or scalars); float64."""
    ax, ae = np.abs(x), np.abs(eps)
    e = eps
    if grad is not None:
        e = eps - k["sq1mat"] * grad
        ae = ae + k["sq1mat"] * np.abs(grad)
    x0 = (x - k["sq1mat"] * e) * k["rsat"]
    x0m = k["rsat"] * (ax + k["sq1mat"] * ae)
    if not constrain:
        return x0, e, x0m, ae
    mean = x0.mean(axis=-1, keepdims=True)
    x0 = np.clip(x0 - mean, -1.0, 1.0)
    return x0, (x - x0 * k["sqat"]) * k["rs1mat"], x0m + np.abs(mean), k["rs1mat"] * (ax + k["sqat"] * np.abs(x0))


def step(x, eps, a_t, a_to, grad=None, noise=None, eta=0.0, constrain=False, invert=False, noise_scale=1.0):
    """x, eps, grad, noise [B, T]; a_t, a_to [B] -> (x_to, M, sig [B]), float64.  noise=None: zeros."""
    assert not (invert and (constrain or eta != 0))
    x, eps = np.asarray(x, dtype=D), np.asarray(eps, dtype=F).astype(D)
    B = x.shape[0]
    k = {name: v.reshape(B, 1) for name, v in coef(np.reshape(a_t, B), np.reshape(a_to, B), eta, invert).items()}
    grad = None if grad is None else np.asarray(grad, dtype=F).astype(D)
    x0, ep, x0m, em = _x0_eps(k, x, eps, grad, constrain)
    nv = np.zeros_like(x) if noise is None else np.asarray(noise, dtype=D) * float(F(noise_scale))
    out = k["sqto"] * x0 + k["ce"] * ep + k["sig"] * nv
    return out, k["sqto"] * x0m + k["ce"] * em + k["sig"] * np.abs(nv), k["sig"].reshape(B)


def window_view(x, n, W, H):
    return np.stack([x[b * H:b * H + W] for b in range(n)])


def step_windows(x, eps, a_t, a_to, n, W, H, grad=None, noise=None, eta=0.0, constrain=False, noise_scale=1.0):
    """x [Np], eps / grad [n, W], noise [Np] or None, scalar alphas -> (x_to [Np], windows [n, W], M [Np], C [Np], sig), float64;
    C is C_BLEND where two windows meet and C_STEP elsewhere."""
    V, Np = W - H, (n - 1) * H + W
    assert n >= 1 and W % 4 == 0 and H % 4 == 0 and 0 <= V <= H
    x, eps = np.asarray(x, dtype=D).reshape(Np), np.asarray(eps, dtype=F).astype(D).reshape(n, W)
    grad = None if grad is None else np.asarray(grad, dtype=F).astype(D).reshape(n, W)
    k = coef(np.reshape(a_t, ()), np.reshape(a_to, ()), eta)
    per_window = _x0_eps(k, window_view(x, n, W, H), eps, grad, constrain)
    x0, ep, x0m, em = (np.empty(Np) for _ in range(4))
    C = np.full(Np, float(C_STEP))
    w = (np.arange(V) + 0.5) / V if V else None
    for dst, src, mag in ((x0, per_window[0], False), (ep, per_window[1], False), (x0m, per_window[2], True), (em, per_window[3], True)):
        dst[:W] = src[0]
        for b in range(1, n):  # window b is the RIGHT window of the overlap [b * H, b * H + V) and alone behind it
            lo = b * H
            if V:
                left, right = src[b - 1, H:], src[b, :V]
                dst[lo:lo + V] = (1 + w) * left + w * right if mag else left + w * (right - left)
                C[lo:lo + V] = C_BLEND
            dst[lo + V:lo + W] = src[b, V:]
    nv = np.zeros(Np) if noise is None else np.asarray(noise, dtype=D).reshape(Np) * float(F(noise_scale))
    out = k["sqto"] * x0 + k["ce"] * ep + k["sig"] * nv
    M = k["sqto"] * x0m + k["ce"] * em + k["sig"] * np.abs(nv)
    return out, window_view(out, n, W, H), M, C, float(k["sig"])


def bound(M, C=C_STEP, sig=0.0, z=None):
    """C * 2^-24 * M, plus the generator's tolerance sig * (1.2e-5 + 3 * 2^-24 |z|) when the noise z was generated on the device."""
    b = np.asarray(C) * U * M
    if z is not None:
        b = b + np.reshape(sig, (-1,) + (1,) * (np.ndim(M) - 1)) * (NORMAL_ABS + 3 * U * np.abs(z))
    return b


# ---- float32 evaluation of the specified formulas (what the kernel does, in numpy): tests/test_ddim.py holds it to the bound ----
def fmaf(a, b, c):
    """fmaf of float32 arrays: the product is exact in float64 (24 + 24 bits), so this is the fused result but for a double rounding."""
    return (np.asarray(a, dtype=F).astype(D) * np.asarray(b, dtype=F).astype(D) + np.asarray(c, dtype=F).astype(D)).astype(F)


def step_f32(x, eps, a_t, a_to, grad=None, noise=None, eta=0.0, constrain=False, invert=False, noise_scale=1.0):
    """`step` in the kernel's arithmetic: coefficients rounded to float32 once, the per-sample operations of ddim_x0_eps / ddim_sample
    in float32, the mean summed in float64 from the float32 inputs and rounded once."""
    x, eps = np.asarray(x, dtype=F), np.asarray(eps, dtype=F)
    B = x.shape[0]
    kd = {name: v.reshape(B, 1) for name, v in coef(np.reshape(a_t, B), np.reshape(a_to, B), eta, invert).items()}
    k = rounded(kd)
    e = eps
    if grad is not None:
        grad = np.asarray(grad, dtype=F)
        e = fmaf(-k["sq1mat"], grad, eps)
    if constrain:
        ed = eps.astype(D) - (kd["sq1mat"] * grad.astype(D) if grad is not None else 0.0)
        mean = ((x.astype(D) - kd["sq1mat"] * ed) * kd["rsat"]).mean(axis=-1, keepdims=True).astype(F)
        x0 = np.clip(fmaf(fmaf(-k["sq1mat"], e, x), k["rsat"], -mean), F(-1), F(1))
        ep = fmaf(-x0, k["sqat"], x) * k["rs1mat"]
    else:
        x0 = fmaf(-k["sq1mat"], e, x) * k["rsat"]
        ep = e
    nv = np.zeros_like(x) if noise is None else np.asarray(noise, dtype=F) * F(noise_scale)
    out = fmaf(k["sqto"], x0, fmaf(k["ce"], ep, k["sig"] * nv))
    assert out.dtype == F and x0.dtype == F and ep.dtype == F
    return out


# ---- the cases of the kernel test, shared by the CPU and the GPU file ----
SHAPES = [(1, 4), (3, 4099), (2, 9216)]  # one quad; a ragged tail over two sum chunks; three sum chunks with a ragged last one
T_PAIRS = [(1.0, 0.1), (0.3, 0.02), (0.02, 0.02)]  # (t, step): the first step, a middle one, the last one (a_to = 1)
ETAS = [0.0, 0.5, 1.0]


def alphas(schedule, B, first):
    """float32 (a_t, a_to) [B]: row b is at T_PAIRS[(first + b) % 3], so every pair is met at every shape and rows differ."""
    import torch

    from oracle import ref_cpu

    t = torch.tensor([T_PAIRS[(first + b) % 3][0] for b in range(B)], dtype=torch.float32)
    s = torch.tensor([T_PAIRS[(first + b) % 3][1] for b in range(B)], dtype=torch.float32)
    return ref_cpu.schedule_alpha(schedule, t).numpy(), ref_cpu.schedule_alpha(schedule, t - s).numpy()


def case_inputs(B, T, seed=101):
    """float32 numpy (x, eps, grad, noise) [B, T] of the kernel test."""
    import torch

    def draw(s, scale=1.0):
        return (torch.randn((B, T), generator=torch.Generator().manual_seed(s)) * scale).numpy()

    return draw(seed), draw(seed + 1), draw(seed + 2, 0.5), draw(seed + 3)
