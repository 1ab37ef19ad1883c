"""Float64 reference of `vqvs_spectral_distance` (include/vqvs.h), written from the definitions: two waveform batches [B, T] ->
per clip the SUM over the F = T // hop + 1 frames of

    mcd = (10 / ln 10) sqrt(2 sum_{j=1}^{n_ceps-1} (c_a[j] - c_b[j])^2)        lsd = (10 / ln 10) sqrt(mean_m (L_a[m] - L_b[m])^2)

with L = log(mel + eps) and c = L @ dct of a centred, reflect-padded, Hann-windowed power spectrum.  `constants` derives its own
window, HTK filter bank and orthonormal DCT-II (the formulation of mfcc_ref.numpy_mfcc, not the package's `spectral_constants`);
the kernel reads them as float32 tables and eps as a float32, so the reference uses those float32 values, exactly, in float64.

Two switches, as in mfcc_ref.front_end_ref:
  * emulate=True rounds to float32 at the points a float32-in kernel with float64 accumulation rounds at (windowed sample, power,
    mel value, mel + eps, its logarithm, cepstral coefficient) and keeps everything else float64.  It is built from the
    definitions, not from any kernel's output: |emulated - exact| is the error such a kernel owes (E_model).
  * mutant=... applies ONE deliberate error (MUTANTS); used on the CPU to show that the gate would reject a subtly wrong kernel.

`case` builds every input the CPU and the GPU tests share, once: reference, emulation and gate per clip and per output."""
import functools
import math

import numpy as np
import torch

from mfcc_ref import FAMILIES, GATE_FACTOR, make_batch

SAMPLE_RATE = 16000
EPS = 1e-6
CONFIGS = ((400, 160, 40, 13), (64, 16, 8, 4), (512, 128, 80, 20))  # (n_fft, hop, n_mels, n_ceps)
PAIRINGS = ("roll", "perturb", "same")
MUTANTS = ("c0_included", "factor_2_dropped", "log10", "zero_pad", "hop_off_by_one", "symmetric_window", "mean_over_frames", "eps_1e-10")
MUTANT_OUTPUTS = {"c0_included": ("mcd",), "factor_2_dropped": ("mcd",)}  # the others change both outputs
SD_FR = 4           # frames per workgroup of spectral_distance_kernel (csrc/spectral_kernels.hip)
CAP_PER_FRAME = 1e-3  # dB: no clip's gate may exceed CAP_PER_FRAME * frames
DB = 10.0 / math.log(10.0)


def lengths(cfg):
    """The smallest accepted T; 800; 1119, no multiple of the hop; 9600; 19360; and frame counts 2 SD_FR and 2 SD_FR + 1, the two
    sides of a workgroup seam (the kernel has one path otherwise: the rows-per-item choice depends on n_fft alone)."""
    n_fft, hop = cfg[0], cfg[1]
    return (n_fft // 2 + 1, 800, 1119, 9600, 19360, hop * (2 * SD_FR - 1), hop * 2 * SD_FR)


@functools.lru_cache(maxsize=None)
def constants(cfg, symmetric_window=False):
    """window [n_fft], fb [n_freqs, n_mels], dct [n_mels, n_ceps] as float32 arrays and the float64 twiddle table [n_fft, 2]."""
    n_fft, _, n_mels, n_ceps = cfg
    n = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / (n_fft - 1 if symmetric_window else n_fft))
    hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)  # noqa: E731
    mel2hz = lambda m: 700.0 * (10 ** (m / 2595.0) - 1.0)  # noqa: E731
    freqs = np.linspace(0, SAMPLE_RATE // 2, n_fft // 2 + 1)
    pts = mel2hz(np.linspace(hz2mel(0.0), hz2mel(SAMPLE_RATE // 2), n_mels + 2))
    fb = np.zeros((len(freqs), n_mels))
    for m in range(n_mels):
        lo, ce, hi = pts[m], pts[m + 1], pts[m + 2]
        fb[:, m] = np.maximum(0.0, np.minimum((freqs - lo) / (ce - lo), (hi - freqs) / (hi - ce)))
    k = np.arange(n_ceps)[:, None]
    dct = np.cos(np.pi / n_mels * (np.arange(n_mels)[None] + 0.5) * k) * np.sqrt(2.0 / n_mels)
    dct[0] *= 1.0 / math.sqrt(2.0)
    tw = np.stack([np.cos(2 * np.pi * n / n_fft), np.sin(2 * np.pi * n / n_fft)], axis=1)
    return win.astype(np.float32), fb.astype(np.float32), dct.T.astype(np.float32).copy(), tw


def spectral_ref(a, b, cfg, eps=EPS, emulate=False, mutant=None):
    """a, b [B, T] float32 (numpy or torch) -> (mcd [B], lsd [B]) float64, the clips' sums over frames."""
    assert mutant is None or mutant in MUTANTS, mutant
    r32 = (lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)) if emulate else (lambda v: v)
    f64 = lambda t: np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)  # noqa: E731
    n_fft, hop, n_mels, n_ceps = cfg
    win, fb, dct, _ = (f64(c) for c in constants(cfg, mutant == "symmetric_window"))
    eps = 1e-10 if mutant == "eps_1e-10" else float(np.float32(eps))
    half, shift = n_fft // 2, 1 if mutant == "hop_off_by_one" else 0

    def log_mel_and_cepstrum(x):
        x = f64(x)
        T = x.shape[1]
        x = np.pad(x, ((0, 0), (half, half + shift)), mode="constant" if mutant == "zero_pad" else "reflect")
        frames = T // hop + 1
        idx = (np.arange(frames) * hop + shift)[:, None] + np.arange(n_fft)[None]
        xw = r32(x[:, idx] * win)                                     # [B, frames, n_fft]
        power = r32(np.abs(np.fft.rfft(xw, axis=-1)) ** 2)
        mel = r32(power @ fb)                                         # [B, frames, n_mels]
        log = np.log10 if mutant == "log10" else np.log
        L = r32(log(r32(mel + eps)))
        return L, r32(L @ dct)                                        # [B, frames, n_ceps]

    (La, ca), (Lb, cb) = log_mel_and_cepstrum(a), log_mel_and_cepstrum(b)
    first = 0 if mutant == "c0_included" else 1
    two = 1.0 if mutant == "factor_2_dropped" else 2.0
    mcd = DB * np.sqrt(two * ((ca[..., first:] - cb[..., first:]) ** 2).sum(-1))   # [B, frames]
    lsd = DB * np.sqrt(((La - Lb) ** 2).sum(-1) / n_mels)
    if mutant == "mean_over_frames":
        return mcd.mean(-1), lsd.mean(-1)
    return mcd.sum(-1), lsd.sum(-1)


def make_pair(family: str, T: int, pairing: str, cfg=CONFIGS[0]):
    """(a, b) [3, T] float32: b is a rolled by one clip, a + 1e-3 roll(a), or a itself.  The perturbation takes the previous clip;
    under the third configuration it takes the NEXT one: there the pure tone of "loud_quiet_tone" plus a millionth of noise breaks
    the cap at T = 800 (8 E_model = 1.14 caps: in the 80 narrow mel bands the tone's leakage lies near eps, where the logarithm
    amplifies the float32 rounding of the windowed samples), and an input that breaks the cap is changed, not the cap.  One clip
    of "tone_silence_square" gets silence added either way: its b equals its a, and its distance must be exactly 0."""
    a = make_batch(family, T)
    if pairing == "roll":
        return a, a.roll(1, 0)
    if pairing == "perturb":
        return a, a + 1e-3 * a.roll(-1 if cfg == CONFIGS[2] else 1, 0)
    if pairing == "same":
        return a, a
    raise ValueError(pairing)


class Case:
    """One (a, b) pair with the yardstick: per output ("mcd", "lsd") and per clip the reference `ref`, E_model = |emulated - ref|
    and the gate GATE_FACTOR * E_model, capped at CAP_PER_FRAME * frames."""

    def __init__(self, family, T, cfg, pairing):
        self.family, self.T, self.cfg, self.pairing = family, T, cfg, pairing
        self.a, self.b = make_pair(family, T, pairing, cfg)
        self.frames = T // cfg[1] + 1
        self.cap = CAP_PER_FRAME * self.frames
        ref = spectral_ref(self.a, self.b, cfg)
        emu = spectral_ref(self.a, self.b, cfg, emulate=True)
        self.ref = dict(zip(("mcd", "lsd"), ref))
        self.e_model = {k: np.abs(e - r) for k, e, r in zip(("mcd", "lsd"), emu, ref)}
        self.gate = {k: np.minimum(GATE_FACTOR * v, self.cap) for k, v in self.e_model.items()}

    def mutant(self, name):
        return dict(zip(("mcd", "lsd"), spectral_ref(self.a, self.b, self.cfg, mutant=name)))


@functools.lru_cache(maxsize=None)
def case(family: str, T: int, cfg, pairing: str) -> Case:
    return Case(family, T, cfg, pairing)
