"""float32 numpy restatement of `vqvs_ddpm_step_windows` (include/vqvs.h), one operation after the other in the stated order, with
explicit noise: the oracle of tests/test_longform.py and tests/test_longform_gpu.py.  tests/test_longform.py ties it, at one window,
to the reference-pinned `oracle.ref_cpu.ddpm_previous`.

Two places are not float32 roundings of the kernel's own: the window means are sums in float64 (per 4096 samples, added in chunk
order, as the kernel's; the order inside a chunk moves a float64 sum of <= 4096 float32 values by ~1e-13 relative, far below the
float32 rounding of the mean), and fmaf(w, d, e) is evaluated in float64 and rounded once (w * d is exact there)."""
import numpy as np

F = np.float32
SUM_CHUNK = 4096


def step_coef(a_t, a_prev, sigma_large):
    """The per-step scalars in the operation order of step_coef (csrc/sampler_kernels.hip)."""
    a_t, a_prev, one = F(a_t), F(a_prev), F(1)
    alphas = a_t / a_prev
    betas = one - alphas
    om = one - a_t
    k = {"c1": one / np.sqrt(alphas), "c2": betas * (one / np.sqrt(om))}
    sig2 = betas if sigma_large else betas * (one - a_prev) / om
    k.update(sig=np.sqrt(sig2), sq1mat=np.sqrt(om), rsat=one / np.sqrt(a_t), sqat=np.sqrt(a_t), rs1mat=one / np.sqrt(om), c3=sig2,
             alphas=alphas, betas=betas)
    assert all(v.dtype == F for v in k.values())
    return k


def geometry(n, W, H):
    V = W - H
    assert n >= 1 and W % 4 == 0 and H % 4 == 0 and 0 <= V <= H
    return V, (n - 1) * H + W


def window_view(x, n, W, H):
    """[Np] -> [n, W], window b = x[b * H : b * H + W] (a copy)."""
    return np.stack([x[b * H:b * H + W] for b in range(n)])


def window_eps(k, xw, eps, constrain):
    """e_b of every window [n, W]: the prediction, or with constrain its re-derivation about the window's own mean of x0."""
    if not constrain:
        return eps
    x0 = (xw - k["sq1mat"] * eps) * k["rsat"]
    W = x0.shape[1]
    mean = np.zeros(len(x0), dtype=np.float64)
    for c in range(0, W, SUM_CHUNK):
        mean += x0[:, c:c + SUM_CHUNK].astype(np.float64).sum(axis=1)
    mean = (mean / float(W)).astype(F)[:, None]
    x0 = np.minimum(np.maximum(x0 - mean, F(-1)), F(1))
    return (xw - x0 * k["sqat"]) * k["rs1mat"]


def step_windows(x, eps, noise, a_t, a_prev, n, W, H, sigma_large=False, constrain=False, noise_scale=1.0):
    """x [Np], eps [n, W], noise [Np] or None (zeros) -> (x_prev [Np], windows [n, W]), all float32."""
    V, Np = geometry(n, W, H)
    x, eps = np.asarray(x, dtype=F).reshape(Np), np.asarray(eps, dtype=F).reshape(n, W)
    k = step_coef(a_t, a_prev, sigma_large)
    eb = window_eps(k, window_view(x, n, W, H), eps, constrain)
    e = np.empty(Np, dtype=F)
    e[:W] = eb[0]
    for b in range(1, n):  # window b is the RIGHT window of the overlap [b * H, b * H + V) and alone behind it
        lo = b * H
        if V:
            w = ((np.arange(V, dtype=F) + F(0.5)) / F(V)).astype(F)
            e_l, e_r = eb[b - 1, H:], eb[b, :V]
            d = e_r - e_l
            e[lo:lo + V] = (w.astype(np.float64) * d.astype(np.float64) + e_l.astype(np.float64)).astype(F)
        e[lo + V:lo + W] = eb[b, V:]
    nv = np.zeros(Np, dtype=F)
    if noise is not None and noise_scale != 0:
        nv = np.asarray(noise, dtype=F).reshape(Np) * F(noise_scale)
    x_prev = k["c1"] * (x - k["c2"] * e) + k["sig"] * nv
    assert x_prev.dtype == F
    return x_prev, window_view(x_prev, n, W, H)


def guided_eps(xw, eps, grad_fn, a_t, a_prev, sigma_large=False):
    """The two half-steps around a cond_fn on a window batch [n, W], in the order of ddpm_mean_kernel / ddpm_guided_eps_kernel:
    mean = c1 (x - c2 eps); m = mean + sigma^2 grad_fn(mean); eps' = (-m sqrt(alphas) + x) sqrt(1 - a_t) / betas."""
    k = step_coef(a_t, a_prev, sigma_large)
    xw, eps = np.asarray(xw, dtype=F), np.asarray(eps, dtype=F)
    mean = k["c1"] * (xw - k["c2"] * eps)
    m = mean + k["c3"] * np.asarray(grad_fn(mean), dtype=F)
    out = (-m * np.sqrt(k["alphas"]) + xw) * k["sq1mat"] / k["betas"]
    assert out.dtype == F
    return out
