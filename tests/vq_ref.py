"""The float64 nearest-code reference that the VQ search (`vq_search` in csrc/sampler_kernels.hip, behind `vqvs_vq_argmin` and
`vqvs_vq_quantize`) is held to, the bound on the kernel's fp32 distance, and the cases both test files walk
(tests/test_vq_search.py on the host, tests/test_vq_search_gpu.py on the device).  Plain numpy: no device, no library.

The reference.  D[b,t,k] = sum_c (z[b,c,t] - d[k,c])^2 in float64, formed from the float32 inputs as differences (never the
expanded formula, so nothing cancels), and best64 = argmin_k D with the first index on ties.

The bound.  The kernel computes dist[k] = ((-2 <x, e_k>) + |e_k|^2) + |x|^2 in fp32, which cancels: the answer cannot be held to
"equals best64".  What can be derived:
  * the dot product <x, e_k>, |e_k|^2 and |x|^2 are each an fmaf chain of Cd terms (zero padding adds exact terms): every
    product of a chain passes through at most Cd roundings, so each chain is off by at most gamma_Cd times the sum of its terms'
    magnitudes, gamma_n = n u / (1 - n u), u = 2^-24;
  * -2 * acc is exact (a power of two);
  * the two additions round twice (once if the compiler contracts -2 acc + en into one fmaf);
  * so |dist_fp32[k] - D[k]| <= gamma_(Cd+2) * (2 sum|x_c e_c| + sum e_c^2 + sum x_c^2) = gamma_(Cd+2) * S[k] with
    S[b,t,k] = sum_c (|z[b,c,t]| + |d[k,c]|)^2;
  * written E[b,t,k] = (Cd + 3) * u * S[b,t,k]: the third unit absorbs the 1 / (1 - n u) factor (n u < 2^-14 for Cd <= 1024).
The bound is derived, not measured: no test may widen it.  If the kernel breaks it with no defect, the derivation above is what
has to be corrected.

The search rule.  For a kernel answer g at position (b,t):
  (1) D[g] - D[best64] <= E[g] + E[best64]     (the kernel's fp32 distance of g is no greater than that of best64, and each is
                                                within E of its float64 value);
  (2) g is the smallest index among the dictionary rows that are bitwise equal to row g (equal rows give bitwise-equal fp32
      distances in this kernel -- same operands, same fmaf order in every slot --, so the first index must win exactly);
  (3) a position of z that holds a NaN gets code 0 (no `d < best` ever fires; torch.argmin returns 0 for an all-NaN row).
`undecided(z, d)` marks the positions where (1) and (2) allow more than one answer; the host test caps its share per case.
"""
from functools import lru_cache

import numpy as np
import torch

from util import seeded

U = 2.0 ** -24
VQ_TILE, VQ_KC = 128, 64  # the kernel's tile: codes per tile, channels per chunk


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _rows(z):
    """float32 [B,Cd,T] -> float64 rows [B*T, Cd]"""
    z = _np(z)
    return np.ascontiguousarray(z.transpose(0, 2, 1)).reshape(-1, z.shape[1]).astype(np.float64)


def _pairwise(z, d, term):
    """sum_c term(x_c, e_c) in float64 for every (position, code): [B,T,K], in blocks of codes to bound the memory."""
    z, d = _np(z), _np(d)
    assert z.dtype == np.float32 and d.dtype == np.float32 and z.ndim == 3 and d.ndim == 2 and z.shape[1] == d.shape[1]
    x, e = _rows(z), d.astype(np.float64)
    out = np.empty((x.shape[0], e.shape[0]), dtype=np.float64)
    step = max(1, (1 << 22) // max(1, x.shape[0] * x.shape[1]))
    for k0 in range(0, e.shape[0], step):
        out[:, k0:k0 + step] = term(x[:, None, :], e[None, k0:k0 + step, :]).sum(-1)
    return out.reshape(z.shape[0], z.shape[2], e.shape[0])


def dist64(z, d):
    """D[b,t,k] = sum_c (z[b,c,t] - d[k,c])^2 in float64, as differences of the float32 inputs."""
    return _pairwise(z, d, lambda x, e: (x - e) ** 2)


def mag64(z, d):
    """S[b,t,k] = sum_c (|z[b,c,t]| + |d[k,c]|)^2 in float64."""
    return _pairwise(z, d, lambda x, e: (np.abs(x) + np.abs(e)) ** 2)


def err_bound(z, d):
    """E[b,t,k] = (Cd + 3) * 2^-24 * S[b,t,k] (the derivation is in the module docstring)."""
    return (_np(z).shape[1] + 3) * U * mag64(z, d)


def first_equal_row(d):
    """first[k] = the smallest index whose dictionary row is bitwise equal to row k"""
    d = np.ascontiguousarray(_np(d))
    seen, first = {}, np.empty(d.shape[0], dtype=np.int64)
    for k in range(d.shape[0]):
        first[k] = seen.setdefault(d[k].tobytes(), k)
    return first


class Reference:
    """Everything the rule needs of one (z, d), computed once and never modified."""

    def __init__(self, z, d):
        z, d = _np(z), _np(d)
        self.shape = (z.shape[0], z.shape[2])
        self.K = d.shape[0]
        self.nan = np.isnan(z).any(axis=1)  # [B,T]: positions that hold a NaN
        self.D, self.E = dist64(z, d), err_bound(z, d)
        self.first = first_equal_row(d)
        self.best = np.where(self.nan, 0, np.argmin(np.where(self.nan[..., None], 0.0, self.D), axis=-1))
        for a in (self.D, self.E, self.first, self.best, self.nan):
            a.setflags(write=False)

    def _at(self, a, idx):
        return np.take_along_axis(a, idx[..., None], axis=-1)[..., 0]

    def slack(self, g):
        """(D[g] - D[best64], E[g] + E[best64]) per position, NaN positions as (0, 1)"""
        g = _np(g).astype(np.int64)
        gap = self._at(self.D, g) - self._at(self.D, self.best)
        room = self._at(self.E, g) + self._at(self.E, self.best)
        return np.where(self.nan, 0.0, gap), np.where(self.nan, 1.0, room)

    def violations(self, g):
        """The positions (b, t, code, reason) at which the answer g breaks the search rule: empty means g passes."""
        g = _np(g)
        assert g.shape == self.shape, (g.shape, self.shape)
        g = g.astype(np.int64)
        out = []
        outside = (g < 0) | (g >= self.K)
        gc = np.clip(g, 0, self.K - 1)
        gap, room = self.slack(gc)
        far = ~self.nan & ~outside & ~(gap <= room)
        later = ~self.nan & ~outside & (self.first[gc] != gc)
        nan_bad = self.nan & (g != 0)
        for mask, why in ((outside, "index outside 0..K-1"), (far, "D[g] - D[best64] > E[g] + E[best64]"),
                          (later, "a later copy of an equal row"), (nan_bad, "NaN position is not code 0")):
            out += [(int(b), int(t), int(g[b, t]), why) for b, t in zip(*np.nonzero(mask))]
        return out

    def undecided(self):
        """[B,T] bool: some k != best64 has D[k] - D[best64] <= E[k] + E[best64] and row k is not bitwise equal to row best64."""
        Db, Eb = self._at(self.D, self.best)[..., None], self._at(self.E, self.best)[..., None]
        with np.errstate(invalid="ignore"):
            close = (self.D - Db) <= (self.E + Eb)
        close &= self.first[None, None, :] != self.first[self.best][..., None]
        return close.any(axis=-1) & ~self.nan

    def margins(self, g):
        """(largest fraction of the bound used, positions where g != best64): recorded by the device test, not gated"""
        g = _np(g).astype(np.int64)
        gap, room = self.slack(g)
        return float((gap / room).max()), int((g != self.best).sum())


def best64(z, d):
    return Reference(z, d).best


def undecided(z, d):
    return Reference(z, d).undecided()


def search_f32(z, d, *, skip_partial_tile=False, skip_tail_channels=False, last_on_ties=False, norms_of=None, skip_slot=None):
    """An honest float32 implementation of the kernel's formula in numpy: float32 matmul, float32 norms, the kernel's bracket
    order ((-2 dot + |e|^2) + |x|^2), first index on ties.  Not bit-identical to the kernel and never compared with it: it shows
    that the rule is satisfiable -- and, through the keyword arguments, that it can fail.  Each keyword is one defect a tiled
    search could have:
      skip_partial_tile   the codes of a partial last 128-code tile (behind at least one full tile) are never scored
      skip_tail_channels  the channels past the last full 64-channel chunk are left out of the dot product and of |x|^2
      last_on_ties        equal distances go to the later index
      norms_of            |e|^2 is taken from this dictionary instead (stale norms in the scratch buffer)
      skip_slot           the codes with k % 128 == skip_slot are never chosen"""
    z, d = _np(z), _np(d)
    B, Cd, T = z.shape
    K = d.shape[0]
    x = np.ascontiguousarray(z.transpose(0, 2, 1)).reshape(-1, Cd)
    c_used = (Cd // VQ_KC) * VQ_KC if skip_tail_channels and Cd > VQ_KC else Cd
    dots = x[:, :c_used] @ np.ascontiguousarray(d[:, :c_used].T)
    en_src = d if norms_of is None else _np(norms_of)
    en = (en_src * en_src).sum(-1, dtype=np.float32)
    xn = (x[:, :c_used] * x[:, :c_used]).sum(-1, dtype=np.float32)
    assert dots.dtype == np.float32 and en.dtype == np.float32 and xn.dtype == np.float32
    with np.errstate(invalid="ignore"):
        dist = (np.float32(-2.0) * dots + en[None, :]) + xn[:, None]
    assert dist.dtype == np.float32
    dead = np.zeros(K, dtype=bool)
    if skip_partial_tile and K > VQ_TILE and K % VQ_TILE:
        dead[(K // VQ_TILE) * VQ_TILE:] = True
    if skip_slot is not None:
        dead |= np.arange(K) % VQ_TILE == skip_slot
    if dead.all():
        dead[:] = False
    dist = np.where(dead[None, :], np.float32(np.inf), dist)
    nan = np.isnan(dist).any(-1)
    dist = np.where(nan[:, None], np.float32(0), dist)  # `d < best` never fires on a NaN: code 0
    idx = K - 1 - np.argmin(dist[:, ::-1], axis=-1) if last_on_ties else np.argmin(dist, axis=-1)
    return np.where(nan, 0, idx).reshape(B, T).astype(np.int64)


MUTANTS = {
    "partial last tile ignored": dict(skip_partial_tile=True),
    "channels past the last full 64-channel chunk ignored": dict(skip_tail_channels=True),
    "last index on ties": dict(last_on_ties=True),
    "norms of a different dictionary": "norms",  # resolved per case in mutant_answer
    "slot k % 128 == 37 never chosen": dict(skip_slot=37),
}


def mutant_answer(name, case):
    kw = MUTANTS[name]
    if kw == "norms":
        kw = dict(norms_of=seeded(tuple(case.d.shape), 99000 + case.K + case.Cd, float(case.d.std())))
    return search_f32(case.z, case.d, **kw)


# ---------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """One (z [B,Cd,T1], dictionary [K,Cd]) pair of float32 CPU tensors, never modified.  `expected` (int64 [B,T1] or None) is the
    exact answer of the families where the rule leaves nothing open; `nan_at` lists the (b, t) that hold a NaN."""

    def __init__(self, family, name, z, d, expected=None, nan_at=()):
        self.family, self.name, self.z, self.d, self.expected, self.nan_at = family, name, z.contiguous(), d.contiguous(), expected, tuple(nan_at)
        self.B, self.Cd, self.T1 = self.z.shape
        self.K = self.d.shape[0]
        assert self.d.shape[1] == self.Cd and self.Cd % 4 == 0 and self.B * self.T1 <= 600

    def __repr__(self):
        return self.name


EXACT_FAMILIES = ("every slot", "ties")  # `undecided` must be empty; the kernel's answer must equal `expected`
UNDECIDED_CAP = 0.02  # of a case's positions, every other family (a condition on the cases: change a seed, never the cap)

GRID_CD, GRID_K, GRID_T1, GRID_B = (4, 60, 64, 68, 128, 512), (1, 15, 17, 127, 128, 129, 130, 257, 512), (1, 31, 32, 33, 70), (1, 3)
# Seeds that replace the rule-given one of a case, so that `undecided` stays within the cap (test_vq_search.py checks it).
RESEED = {"grid Cd=512 K=257 T1=32 B=1": 5042}  # the rule-given 5040 leaves 1 of its 32 positions undecided (3.1 %)


def _seed(name, base):
    return RESEED.get(name, base)


def _grid_cases():
    """Every (Cd, K) pair once -- 54 cases, the fewest that cover all pairs of these two factors --, T1 and B walked so that every
    pair of values of any two factors occurs (test_vq_search.py checks the covering): T1 by (i + j) mod 5, B by (i + j) mod 2."""
    out = []
    for i, Cd in enumerate(GRID_CD):
        for j, K in enumerate(GRID_K):
            T1, B = GRID_T1[(i + j) % 5], GRID_B[(i + j) % 2]
            name = f"grid Cd={Cd} K={K} T1={T1} B={B}"
            scale = 0.35 if Cd == 512 else 1.0  # the golden fixture's dictionary scale (its z has RMS 0.34)
            s = _seed(name, 4000 + 20 * (i * len(GRID_K) + j))
            out.append(Case("grid", name, seeded((B, Cd, T1), s, scale), seeded((K, Cd), s + 1, scale)))
    return out


def _slot_cases():
    out = []
    for n, (Cd, K) in enumerate(((4, 130), (68, 130), (68, 512))):
        for order in ("identity", "reversed"):
            name = f"every slot Cd={Cd} K={K} {order}"
            s = _seed(name, 5000 + 20 * n)
            d = seeded((K, Cd), s)
            perm = np.arange(K) if order == "identity" else np.arange(K)[::-1].copy()
            z = d[perm].t()[None] + 1e-3 * seeded((1, Cd, K), s + 1)  # column t is dict[perm[t]] + noise
            out.append(Case("every slot", name, z, d, expected=perm[None].astype(np.int64)))
    return out


TIE_COPIES = {2: (5,), 3: (40,), 7: (135,), 120: (130,), 9: (200, 256)}  # first index -> its copies (same thread; other code group; other tile, same slot; earlier tile, higher code group; a triple ending in the 1-code last tile)


def _tie_cases():
    out = []
    firsts = np.array(sorted(TIE_COPIES), dtype=np.int64)
    for n, Cd in enumerate((4, 68)):
        name = f"ties Cd={Cd} K=257"
        s = _seed(name, 6000 + 20 * n)
        d = seeded((257, Cd), s)
        for first, copies in TIE_COPIES.items():
            for c in copies:
                d[c] = d[first]
        rows = d[firsts].t()[None]  # [1, Cd, 5]: the duplicated rows themselves ...
        z = torch.cat([rows, rows + 1e-3 * seeded(tuple(rows.shape), s + 1)], dim=2)  # ... and the same plus noise
        out.append(Case("ties", name, z, d, expected=np.concatenate([firsts, firsts])[None]))
    return out


def _cancel_cases():
    out = []
    for n, (Cd, K, T1) in enumerate(((32, 512, 64), (68, 130, 64))):
        for m, (tag, offset, scale) in enumerate((("offset 3.0", 3.0, 1.0), ("scale 1e3", 0.0, 1e3), ("scale 1e-3", 0.0, 1e-3))):
            name = f"cancellation Cd={Cd} K={K} T1={T1} {tag}"
            s = _seed(name, 7000 + 100 * n + 20 * m)
            out.append(Case("cancellation", name, seeded((2, Cd, T1), s, scale) + offset, seeded((K, Cd), s + 1, scale) + offset))
    return out


def _nan_cases():
    name = "nan Cd=68 K=130 T1=32"
    s = _seed(name, 8000)
    z = seeded((1, 68, 32), s)
    z[0, 41, 13] = float("nan")  # one channel of one position
    return [Case("nan", name, z, seeded((130, 68), s + 1), nan_at=((0, 13),))]


CASES = _grid_cases() + _slot_cases() + _tie_cases() + _cancel_cases() + _nan_cases()
FAMILIES = ("grid", "every slot", "ties", "cancellation", "nan")
assert len({c.name for c in CASES}) == len(CASES)


@lru_cache(maxsize=None)
def reference(i):
    """The Reference of CASES[i]: computed once per process, shared by every test that needs it."""
    return Reference(CASES[i].z, CASES[i].d)
