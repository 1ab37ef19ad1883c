"""The keep-region operation of the library (include/vqvs.h "Keep region"), restated in float64 numpy: the reference that
tests/test_keep.py checks against itself and tests/test_keep_gpu.py compares the kernels with.  It does not import the library.

Kept samples of a state are put back on the forward process of a source at alpha_bar = alpha:
    x[p] = ca * x0[p] + cn * (noise_scale * z),   ca = sqrt(alpha), cn = sqrt(max(1 - alpha, 0))
with ca and cn computed in float64 from the float32 alpha and rounded to float32 ONCE -- the coefficients are the library's own, so
the comparison sees the per-sample arithmetic alone -- and everything after that in float64.  Nothing is drawn when cn == 0 or
noise_scale == 0.  Drawn noise is the generator of tests/philox_ref.py on stream 3.
"""
import numpy as np

import philox_ref

STREAM_KEEP = 3  # csrc/philox.hpp PHILOX_STREAM_KEEP: apart from the step noise (0), x_T (1) and the loss noise (2)


def coefficients(alpha):
    """(ca, cn) as float32 scalars from a float32 alpha."""
    a = np.float64(np.float32(alpha))
    return np.float32(np.sqrt(a)), np.float32(np.sqrt(max(1.0 - a, 0.0)))


def keep_region(x, x0, keep, noise, alpha, noise_scale=1.0, seed=0, clip_offset=0, index=0):
    """x, x0 [B, T]; keep [B, T] (nonzero: kept) or None (all); noise [B, T] or None (drawn); alpha [B] -> float64 [B, T].
    Also returns the per-sample magnitude |ca x0| + |cn z| that the rounding bound of the kernel is stated in."""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    B, T = x.shape
    out, mag = x.copy(), np.zeros_like(x)
    for b in range(B):
        ca, cn = coefficients(np.asarray(alpha).reshape(-1)[b])
        z = np.zeros(T)
        if cn != 0 and noise_scale != 0:
            z = philox_ref.randn(1, T, seed, clip_offset + b, STREAM_KEEP, step=index)[0] if noise is None else np.asarray(noise, dtype=np.float64)[b]
            z = np.float64(noise_scale) * z
        new = np.float64(ca) * x0[b] + np.float64(cn) * z
        kept = np.ones(T, dtype=bool) if keep is None else np.asarray(keep)[b] != 0
        out[b, kept] = new[kept]
        mag[b] = np.abs(np.float64(ca) * x0[b]) + np.abs(np.float64(cn) * z)
    return out, mag


def keep_region_windows(x, windows, x0, keep, noise, alpha, n, W, H, noise_scale=1.0, seed=0, clip=0, index=0):
    """The windows geometry as a plain loop over absolute positions: x, x0 [Np], keep [Np] or None, noise [Np] or None, ONE alpha;
    windows [n, W] or None.  Returns (x [Np], windows [n, W] or None, magnitude [Np]): a kept sample is written to the long state and
    to its copy in every window that covers it."""
    Np = (n - 1) * H + W
    x, x0 = np.asarray(x, dtype=np.float64).copy(), np.asarray(x0, dtype=np.float64)
    assert x.shape == (Np,) and x0.shape == (Np,)
    windows = None if windows is None else np.asarray(windows, dtype=np.float64).copy()
    ca, cn = coefficients(alpha)
    noisy = cn != 0 and noise_scale != 0
    if noisy and noise is None:
        noise = philox_ref.randn(1, Np, seed, clip, STREAM_KEEP, step=index)[0]
    mag = np.zeros(Np)
    for p in range(Np):
        z = np.float64(noise_scale) * np.float64(noise[p]) if noisy else 0.0
        mag[p] = abs(np.float64(ca) * x0[p]) + abs(np.float64(cn) * z)
        if keep is not None and not keep[p]:
            continue
        v = np.float64(ca) * x0[p] + np.float64(cn) * z
        x[p] = v
        if windows is not None:
            for b in range(n):
                if 0 <= p - b * H < W:
                    windows[b, p - b * H] = v
    return x, windows, mag
