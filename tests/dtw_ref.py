"""Float64 numpy restatement of `vqvs_mel_cepstra` and `vqvs_dtw_distance` (include/vqvs.h), written from the definitions.

`cepstra_ref`: per row the frames of the recording ALONE -- centred, reflect-padded about its own ends -- through the emulated
front end of spectral_ref (float32 roundings at the points the header names, everything else float64, numpy's FFT in place of the
direct DFT), zeros from the row's own frame count on.

`dtw_ref`: the local cost in float64 from the float32 cepstra with the terms added in index order as single operations (numpy does
not contract), then the recurrence cell by cell in Python floats, which are IEEE doubles: D(i,j) = d(i,j) + min over the existing
predecessors, ties to the first of (diagonal, i-1, j-1), every cell carrying its chosen predecessor's steps, both, vuv, sum l and
sum l^2 plus its own.  It also reports the smallest RELATIVE MARGIN between the best and the second-best predecessor over all
cells with more than one, (second - best) / second (0 where both are 0): where that is far above the rounding error of an
accumulated cost, no correct implementation can choose differently.

`brute_force` enumerates every monotone path; `dtw_inputs` builds the seeded inputs the CPU and the GPU tests share."""
import functools
import math

import numpy as np

import spectral_ref as sr

DB = 10.0 / math.log(10.0)
CFG_SMALL, CFG_DEFAULT = (64, 16, 8, 5), (400, 160, 40, 13)   # (n_fft, hop, n_mels, n_ceps)
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 3), (5, 5), (17, 9), (64, 65), (129, 70), (257, 300))
BATCH_ORDER = (8, 0, 1, 2, 3, 4, 5, 6, 7, 8)  # rows of the mixed batch: the largest shape first and last
MARGIN_FACTOR = 1000.0


def bound_factor(n_ceps: int, Fa: int, Fb: int) -> float:
    """The relative bound on |cost - ref|: the same algorithm on the same float32 inputs differs by the rounding of the square root
    and of the local cost's n_ceps + 2 operations and by the summation of at most Fa + Fb - 1 non-negative terms, each a relative
    2^-53; the minimum over paths is 1-Lipschitz in these perturbations.  Doubled."""
    return 2.0 * (n_ceps + Fa + Fb + 4) * 2.0 ** -53


def cepstra_ref(x, lengths, cfg, eps=sr.EPS, logmel=False):
    """x [B, T] float32, lengths [B] -> (ceps float64 [B, T // hop + 1, n_ceps] (, logmel [B, Fmax, n_mels]), frames [B])."""
    x = np.asarray(x, dtype=np.float32)
    n_fft, hop, n_mels, n_ceps = cfg
    win, fb, dct, _ = (np.asarray(c, dtype=np.float64) for c in sr.constants(cfg))
    r32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)  # noqa: E731
    eps = float(np.float32(eps))
    Fmax = x.shape[1] // hop + 1
    ceps, mel_out, frames = np.zeros((len(x), Fmax, n_ceps)), np.zeros((len(x), Fmax, n_mels)), []
    for b, n in enumerate(lengths):
        n = min(max(int(n), n_fft // 2 + 1), x.shape[1])
        row = np.pad(x[b, :n].astype(np.float64), n_fft // 2, mode="reflect")
        F = n // hop + 1
        idx = (np.arange(F) * hop)[:, None] + np.arange(n_fft)[None]
        power = r32(np.abs(np.fft.rfft(r32(row[idx] * win), axis=-1)) ** 2)
        L = r32(np.log(r32(r32(power @ fb) + eps)))
        ceps[b, :F], mel_out[b, :F] = r32(L @ dct), L
        frames.append(F)
    return (ceps, mel_out, np.array(frames)) if logmel else (ceps, np.array(frames))


def local_cost(ca, cb):
    """ca [Fa, n_ceps], cb [Fb, n_ceps] float32 -> d [Fa, Fb] float64; coefficient 0 is left out."""
    ca, cb = np.asarray(ca, dtype=np.float32).astype(np.float64), np.asarray(cb, dtype=np.float32).astype(np.float64)
    s = np.zeros((ca.shape[0], cb.shape[0]))
    for c in range(1, ca.shape[1]):
        diff = ca[:, None, c] - cb[None, :, c]
        s = s + diff * diff
    return DB * np.sqrt(2.0 * s)


def cell_terms(ta, tb, i, j):
    """(both, vuv, l) of cell (i, j): l = tb[j] - ta[i] where both tracks are finite."""
    if ta is None:
        return 0, 0, 0.0
    ha, hb = math.isfinite(ta[i]), math.isfinite(tb[j])
    if ha and hb:
        return 1, 0, float(tb[j]) - float(ta[i])
    return 0, int(ha != hb), 0.0


def dtw_ref(ca, cb, ta=None, tb=None):
    """One pair -> {"cost", "steps", "both", "vuv", "s1", "s2", "margin"}; ta [Fa], tb [Fb] float64 with NaN for no value, or None."""
    d = local_cost(ca, cb).tolist()
    Fa, Fb = len(d), len(d[0])
    ta, tb = (None, None) if ta is None else (np.asarray(ta, dtype=np.float64).tolist(), np.asarray(tb, dtype=np.float64).tolist())
    prev, margin = None, math.inf
    for i in range(Fa):
        row = []
        for j in range(Fb):
            preds = []  # in tie-break order
            if i > 0 and j > 0:
                preds.append(prev[j - 1])
            if i > 0:
                preds.append(prev[j])
            if j > 0:
                preds.append(row[j - 1])
            both, vuv, l = cell_terms(ta, tb, i, j)
            if not preds:
                row.append((d[i][j], 1, both, vuv, 0.0 + l if both else 0.0, l * l if both else 0.0))
                continue
            best = preds[0]
            for p in preds[1:]:
                if p[0] < best[0]:
                    best = p
            if len(preds) > 1:
                lo, second = sorted(p[0] for p in preds)[:2]
                margin = min(margin, (second - lo) / second if second > 0 else 0.0)
            s1, s2 = (best[4] + l, best[5] + l * l) if both else (best[4], best[5])
            row.append((d[i][j] + best[0], best[1] + 1, best[2] + both, best[3] + vuv, s1, s2))
        prev = row
    cost, steps, both, vuv, s1, s2 = prev[-1]
    return {"cost": cost, "steps": steps, "both": both, "vuv": vuv, "s1": s1, "s2": s2, "margin": margin}


def brute_force(ca, cb, ta=None, tb=None):
    """Every monotone path from (0, 0) to (Fa-1, Fb-1), each summed in path order -> [(cost, steps, both, vuv, s1, s2)]."""
    d = local_cost(ca, cb).tolist()
    Fa, Fb = len(d), len(d[0])
    ta, tb = (None, None) if ta is None else (np.asarray(ta, dtype=np.float64).tolist(), np.asarray(tb, dtype=np.float64).tolist())
    out = []

    def walk(i, j, carry):
        both, vuv, l = cell_terms(ta, tb, i, j)
        first = carry is None
        cost, steps, nb, nv, s1, s2 = (0.0, 0, 0, 0, 0.0, 0.0) if first else carry
        carry = (d[i][j] if first else d[i][j] + cost, steps + 1, nb + both, nv + vuv, s1 + l if both else s1, s2 + l * l if both else s2)
        if (i, j) == (Fa - 1, Fb - 1):
            out.append(carry)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < Fa and j + dj < Fb:
                walk(i + di, j + dj, carry)

    walk(0, 0, None)
    return out


def noise_cepstra(F: int, n_ceps: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((F, n_ceps)).astype(np.float32)


def noise_track(F: int, seed: int) -> np.ndarray:
    """Semitone-like values around 90 with about a third of the frames unvoiced (NaN); frame 0, on every path, is voiced."""
    g = np.random.default_rng(seed)
    t = 90.0 + 5.0 * g.standard_normal(F)
    t[1:][g.random(F - 1) < 0.35] = np.nan
    return t


LONG_SHAPES = ((2048, 3), (3, 2048))  # the longest side the kernel takes: its largest LDS rings, and eight rows per thread


@functools.lru_cache(maxsize=None)
def dtw_inputs(n_ceps: int = CFG_SMALL[3], shapes=SHAPES):
    """Per shape: (ca, cb, ta, tb, reference with tracks).  Computed once, shared, never modified by the tests."""
    out = []
    for k, (Fa, Fb) in enumerate(shapes):
        ca, cb = noise_cepstra(Fa, n_ceps, 100 + 2 * k), noise_cepstra(Fb, n_ceps, 101 + 2 * k)
        ta, tb = noise_track(Fa, 300 + 2 * k), noise_track(Fb, 301 + 2 * k)
        for arr in (ca, cb, ta, tb):
            arr.setflags(write=False)
        out.append((ca, cb, ta, tb, dtw_ref(ca, cb, ta, tb)))
    return tuple(out)
