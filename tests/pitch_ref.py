"""Reference of `vqvs_pitch_distance` (include/vqvs.h), written from the definition: two waveform batches
[B, T] -> per clip and frame the YIN period in samples (0.0 = unvoiced), and per clip the voicing counts and the sums of the
frame-wise pitch distance in semitones and of its square.

Steps 1-3 are integers: the samples a 16-bit WAV would hold, zero-padded frames of W + tau_max samples, the difference function
d(tau) and its running sum c(tau).  Every square is below 2^32 and every sum below 2^53 (asserted on every call), so d is the same
integer in any order of addition, in int64 or in float64; the squares are added in float64 (numpy's fastest exact path; tests/
test_pitch.py holds the result to a plain integer loop) and held as int64 from there.  Steps 4-6 are single float64 operations in
the stated order; the clip sums are `math.fsum`s of the frame terms.

`mutant=...` applies ONE deliberate error (MUTANTS); used on the CPU to show that the device test's gates (bitwise periods, equal
counts, sums within SUM_FACTOR roundings) would reject a subtly wrong kernel.  `case` builds every input the CPU and the GPU tests
share, once: a clip is tracked once per (family, T, configuration) and the pairings index into that."""
import functools
import math

import numpy as np
import torch
from numpy.lib.stride_tricks import sliding_window_view

from mfcc_ref import FAMILIES as MFCC_FAMILIES, make_batch

SAMPLE_RATE = 16000
THRESHOLD = 0.15
CONFIGS = ((400, 160, 32, 266), (64, 16, 4, 40), (1024, 256, 16, 1023))  # (window, hop, tau_min, tau_max)
FAMILIES = MFCC_FAMILIES + ("nonfinite", "voiced")
PAIRINGS = ("roll", "perturb", "same")
TRACKING_MUTANTS = ("truncate", "clamp_32768", "start_off_by_one", "mean_from_tau_min", "global_min", "no_walk", "no_parabola")
COMPARE_MUTANTS = ("natural_log", "sign_flipped", "factor_12_dropped")
MUTANTS = TRACKING_MUTANTS + COMPARE_MUTANTS
PD_FR = 4          # frames per workgroup of pitch_distance_kernel (csrc/pitch_kernels.hip)
SUM_FACTOR = 20    # roundings allowed on a frame term beyond the n - 1 additions (tests/test_pitch_gpu.py)
LIMIT = 2 ** 53


def lengths(cfg):
    """1 (one frame, all padding but one sample); 800; 1119, no multiple of any hop; 4000; 9600; and the frame counts 2 PD_FR and
    2 PD_FR + 1, the two sides of a workgroup seam (the kernel has one path otherwise)."""
    hop = cfg[1]
    return (1, 800, 1119, 4000, 9600, hop * (2 * PD_FR - 1), hop * 2 * PD_FR)


def quantise(x, mutant=None):
    """float32 [..., T] -> int64: clamp(rint(x * 32768), -32768, 32767), NaN -> 0, +-inf saturate."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = x * np.float32(32768.0)   # exact: a power of two (overflow gives +-inf, which saturates)
        r = np.trunc(p) if mutant == "truncate" else np.rint(p)  # rint: round half to even
        r = np.where(np.isnan(r), np.float32(0.0), r)
        r = np.clip(r, -32768.0, 32768.0 if mutant == "clamp_32768" else 32767.0)
    return r.astype(np.int64)


def difference(q, cfg, mutant=None):
    """q [B, T] int64 -> d [B, F, tau_max + 1] int64 with d[..., 0] = 0: step 2 and the first line of step 3."""
    W, hop, _, tau_max = cfg
    B, T = q.shape
    F, S = T // hop + 1, W + tau_max
    left = S // 2 + (1 if mutant == "start_off_by_one" else 0)
    qp = np.zeros((B, left + (F - 1) * hop + S), dtype=np.float64)   # zero padding; float64 holds a 17-bit integer exactly
    qp[:, left:left + T] = q
    d = np.zeros((B, F, tau_max + 1), dtype=np.int64)
    step = max(1, (1 << 22) // (W * tau_max))                        # frames per pass: at most 32 MB of differences
    for b in range(B):
        spans = sliding_window_view(qp[b], S)[::hop][:F]             # [F, S]: frame f reads q[f hop - S // 2 ...)
        lagged = sliding_window_view(spans, W, axis=1)               # [F, tau_max + 1, W]: lagged[f, tau, j] = span[f, j + tau]
        for f in range(0, F, step):
            diff = lagged[f:f + step, :1] - lagged[f:f + step, 1:]   # |diff| <= 65535: the square is below 2^32
            dd = np.einsum("ftw,ftw->ft", diff, diff)                # a sum of W such squares: below 2^53, exact in any order
            assert dd.max(initial=0.0) < LIMIT
            d[b, f:f + step, 1:] = dd.astype(np.int64)
    return d


def track(x, cfg, threshold=THRESHOLD, mutant=None):
    """x [B, T] float32 -> period [B, F] float64 (0.0 = unvoiced): steps 1 to 6."""
    assert mutant is None or mutant in TRACKING_MUTANTS, mutant
    W, hop, tau_min, tau_max = cfg
    assert 16 <= W <= 2048 and 2 <= tau_min < tau_max <= 1023 and W * tau_max <= 1 << 20 and 1 <= hop <= W
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    d = difference(quantise(x, mutant), cfg, mutant)
    tau = np.arange(tau_max + 1, dtype=np.int64)
    c = np.cumsum(d, axis=-1)
    num = d * tau
    assert d.max() < LIMIT and c.max() < LIMIT and num.max() < LIMIT   # the exactness argument, on every case
    if mutant == "mean_from_tau_min":   # the running mean started at tau_min instead of 1
        c = c - c[..., tau_min - 1:tau_min]
        num = d * (tau - (tau_min - 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        dn = np.where(c == 0, 1.0, num.astype(np.float64) / c.astype(np.float64))   # one correctly rounded division
    B, F = d.shape[:2]
    period = np.zeros((B, F), dtype=np.float64)
    for b in range(B):
        for f in range(F):
            y = dn[b, f]
            if mutant == "global_min":
                t = tau_min + int(np.argmin(y[tau_min:tau_max + 1]))
                if not y[t] < threshold:
                    continue
            else:
                below = np.flatnonzero(y[tau_min:tau_max + 1] < threshold)
                if below.size == 0:
                    continue
                t = tau_min + int(below[0])
                if mutant != "no_walk":
                    while t + 1 <= tau_max and y[t + 1] < y[t]:
                        t += 1
            p = float(t)
            if t < tau_max and mutant != "no_parabola":
                y0, y1, y2 = float(y[t - 1]), float(y[t]), float(y[t + 1])
                den = (y0 - y1) + (y2 - y1)
                if den > 0:
                    p = t + min(max((0.5 * (y0 - y2)) / den, -1.0), 1.0)
            period[b, f] = p
    return period


def compare(pa, pb, mutant=None):
    """Step 7 for period tracks [B, F]: {"counts" int64 [B, 4], "sums" float64 [B, 2], "abs" float64 [B, 2], "n"}: the sums by
    `math.fsum`, "abs" the sums of |term| the device test's bound is made of."""
    assert mutant is None or mutant in COMPARE_MUTANTS, mutant
    B = pa.shape[0]
    counts, sums, mags = np.zeros((B, 4), dtype=np.int64), np.zeros((B, 2)), np.zeros((B, 2))
    log = (lambda v: math.log(v)) if mutant == "natural_log" else (lambda v: math.log2(v))
    factor = 1.0 if mutant == "factor_12_dropped" else 12.0
    for b in range(B):
        va, vb = pa[b] > 0, pb[b] > 0
        counts[b] = (va.sum(), vb.sum(), (va & vb).sum(), (va != vb).sum())
        terms = []
        for x, y in zip(pa[b][va & vb], pb[b][va & vb]):
            hi, lo = (x, y) if x >= y else (y, x)
            mag = factor * log(hi / lo)
            terms.append(mag if (x >= y) != (mutant == "sign_flipped") else -mag)
        sums[b] = (math.fsum(terms), math.fsum(t * t for t in terms))
        mags[b] = (math.fsum(abs(t) for t in terms), math.fsum(t * t for t in terms))
    return {"counts": counts, "sums": sums, "abs": mags, "n": counts[:, 2].copy()}


def voice(f0, T, harmonics=5, amp=0.5):
    """A `harmonics`-partial voice whose fundamental follows f0 [T] (Hz), partial k at amplitude 1 / k, peak about `amp`."""
    phase = 2 * np.pi * np.cumsum(np.asarray(f0, dtype=np.float64)) / SAMPLE_RATE
    k = np.arange(1, harmonics + 1)[:, None]
    w = (np.sin(k * phase[None]) / k).sum(0)
    return amp * w / (1.0 / np.arange(1, harmonics + 1)).sum()


def glide(T, lo, hi, semitones=0.0):
    """The five-harmonic voice gliding geometrically from lo to hi Hz over the clip, shifted by `semitones`."""
    t = np.arange(T, dtype=np.float64) / max(T - 1, 1)
    return voice(lo * (hi / lo) ** t * 2.0 ** (semitones / 12.0), T)


def make_family(family: str, T: int) -> torch.Tensor:
    """[B, T] float32, seeded; the four families of mfcc_ref.make_batch, "nonfinite" (a voice with a NaN, a +inf and a -inf sample
    and the same voice without them) and "voiced" (four clips)."""
    if family in MFCC_FAMILIES:
        return make_batch(family, T)
    g = np.random.default_rng(T * 7 + 3)
    t = np.arange(T, dtype=np.float64)
    if family == "nonfinite":
        clean = voice(np.full(T, 220.0), T, harmonics=3)
        bad = clean.copy()
        for pos, v in ((T // 5, np.nan), (T // 2, np.inf), ((4 * T) // 5, -np.inf)):
            bad[pos] = v
        return torch.from_numpy(np.stack([bad, clean]).astype(np.float32))
    if family == "voiced":
        vibrato = voice(200.0 * 2.0 ** (0.5 / 12.0 * np.sin(2 * np.pi * 5.0 * t / SAMPLE_RATE)), T) + 0.005 * g.standard_normal(T)
        gate = (t // 800) % 2 == 0   # 50 ms on, 50 ms off
        alternating = np.where(gate, voice(np.full(T, 150.0), T), 0.1 * g.standard_normal(T))
        clipped = np.clip(6.0 * voice(np.full(T, 123.0), T), -1.2, 1.2)   # amplitude 3, beyond the 16-bit range: the clamp binds
        return torch.from_numpy(np.stack([glide(T, 90.0, 360.0), vibrato, alternating, clipped]).astype(np.float32))
    raise ValueError(family)


def make_pair(family: str, T: int, pairing: str):
    """(a, b) [B, T] float32: b is a rolled by one clip, a + 1e-3 roll(a), or a itself."""
    a = make_family(family, T)
    if pairing == "roll":
        return a, a.roll(1, 0)
    if pairing == "perturb":
        return a, a + 1e-3 * a.roll(1, 0)
    if pairing == "same":
        return a, a
    raise ValueError(pairing)


@functools.lru_cache(maxsize=None)
def tracked(family: str, T: int, cfg, perturbed: bool, mutant=None) -> np.ndarray:
    a, b = make_pair(family, T, "perturb" if perturbed else "same")
    return track(b if perturbed else a, cfg, mutant=mutant)


class Case:
    """One (a, b) pair with the reference's periods, counts and sums."""

    def __init__(self, family, T, cfg, pairing):
        self.family, self.T, self.cfg, self.pairing = family, T, cfg, pairing
        self.a, self.b = make_pair(family, T, pairing)
        self.frames = T // cfg[1] + 1
        self.period_a, self.period_b = self.periods()
        self.__dict__.update(compare(self.period_a, self.period_b))

    def periods(self, mutant=None):
        pa = tracked(self.family, self.T, self.cfg, False, mutant)
        if self.pairing == "roll":
            return pa, np.roll(pa, 1, axis=0)
        return pa, (pa if self.pairing == "same" else tracked(self.family, self.T, self.cfg, True, mutant))

    def mutant(self, name):
        """(period_a, period_b, compare(...)) with the one error `name` applied."""
        pa, pb = self.periods(name) if name in TRACKING_MUTANTS else (self.period_a, self.period_b)
        return pa, pb, compare(pa, pb, name if name in COMPARE_MUTANTS else None)


@functools.lru_cache(maxsize=None)
def case(family: str, T: int, cfg, pairing: str) -> Case:
    return Case(family, T, cfg, pairing)
