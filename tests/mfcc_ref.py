"""Float64 reference of ConvMFCCEncoder's whole front end (reference models/conv_encoder.py:42-58, 96-104, 123-133 and the
published algorithm of torchaudio.transforms.MFCC): waveform [B, T] -> the 39 feature rows [B, 39, T // hop + 1] the convolution
stack reads (13 coefficients, their deltas, their delta-deltas).

`front_end_ref` is plain numpy in float64 and takes the checkpoint's own window, filter bank and DCT matrix.  Two switches:
  * emulate=True rounds to float32 at the rounding points a float32-in / float32-out kernel with float64 accumulation cannot
    avoid (windowed sample, power, mel value, log / dB value and floor, the 13 coefficients, each delta) and keeps everything else
    float64.  It is built from the algorithm, not from any kernel's output: max|emulated - exact| is the error such a kernel owes.
  * mutant=... applies ONE deliberate error (MUTANTS).  Used on the CPU only, to show that the gate the GPU test applies
    would reject a subtly wrong kernel.

`numpy_mfcc` is a second, independent derivation (it builds its own window, filter bank and DCT matrix) for one clip.
`make_batch` builds every input the CPU and the GPU tests share; `front_end_case` computes reference, emulation, oracle and the
per-case gate once per (family, T, version, mu-law) and caches it."""
import functools
import math

import numpy as np
import torch

from oracle import ref_cpu

from util import seeded

MUTANTS = ("per_clip_floor", "top_db_100", "no_floor", "zero_pad", "symmetric_window", "hop_off_by_one", "delta_zero_edge",
           "natural_log_db")
FLOOR_MUTANTS = ("per_clip_floor", "top_db_100", "no_floor")

FAMILIES = ("noise", "loud_quiet_tone", "tone_silence_square", "fullscale")
# frame counts 6 7 8 9 | 59 60 61 62 62 | 121 122: both sides of the 8-frame (log-mel) and 60-frame (features) workgroup seams and
# of the 2-frame delta halo; 800 is the smallest accepted length, 1119 and 9919 are no multiples of the hop
LENGTHS = (800, 1119, 1120, 1280, 9280, 9440, 9600, 9760, 9919, 19200, 19360)
GATE_FACTOR = 8.0   # device logf / log10f are a few ulp off where the emulation rounds once; the accumulation order differs
GATE_CAP = 1e-4     # no case's bound may exceed GATE_CAP * max(1, max|ref|)


def make_batch(family: str, T: int) -> torch.Tensor:
    """[3, T] float32, seeded.  (Built in float64 where a formula is involved, so the tensor does not depend on the thread count.)"""
    t = np.arange(T, dtype=np.float64)
    tone = torch.from_numpy((0.5 * np.sin(2 * np.pi * 440 * t / 16000)).astype(np.float32))
    if family == "noise":  # equal loudness: no log-mel value ever reaches the dB floor
        return (0.4 * seeded((3, T), 101)).clamp(-1, 1)
    if family == "loud_quiet_tone":
        return torch.stack([(0.4 * seeded((T,), 102)).clamp(-1, 1), 1e-3 * seeded((T,), 103), tone])
    if family == "tone_silence_square":  # exact zeros: log(1e-6), the 1e-10 clamp and sign(0) = 0 in the mu-law expansion
        square = torch.from_numpy((0.9 * np.sign(np.sin(2 * np.pi * 100 * t / 16000))).astype(np.float32))
        return torch.stack([tone, torch.zeros(T), square])
    if family == "fullscale":  # the mu-law end points
        levels = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])
        return levels[torch.randint(0, 5, (3, T), generator=torch.Generator().manual_seed(104))]
    raise ValueError(family)


def _deltas(seq: np.ndarray, zero_edge: bool) -> np.ndarray:
    """conv_encoder.py:123-129 on the last axis, same order of operations."""
    first, last = (np.zeros_like(seq[..., :1]),) * 2 if zero_edge else (seq[..., :1], seq[..., -1:])
    right_shifted = np.concatenate([first, seq[..., :-1]], axis=-1)
    left_shifted = np.concatenate([seq[..., 1:], last], axis=-1)
    return ((right_shifted - seq) + (seq - left_shifted)) / 2


def front_end_ref(wave, bufs, cfg, input_ulaw, emulate=False, mutant=None, details=None):
    """wave [B, T] float32 (numpy or torch) -> [B, 39, frames] float64.  `bufs` holds the checkpoint's buffers under the
    reference's names (ref_cpu.mfcc_buffers or the "mfcc." entries of a ConvMFCCEncoder state dict).  `details`, a dict,
    receives the unfloored log-mel / dB values [B, frames, n_mels] and the floor."""
    assert mutant is None or mutant in MUTANTS, mutant
    r32 = (lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)) if emulate else (lambda a: a)
    f64 = lambda t: np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)  # noqa: E731
    n_fft, hop = cfg["n_fft"], cfg["hop"]
    x = f64(wave)
    B, T = x.shape
    if input_ulaw:  # conv_encoder.py:132-133
        x = np.sign(x) * (1.0 / 255.0) * ((1.0 + 255.0) ** np.abs(x) - 1.0)
    half, shift = n_fft // 2, 1 if mutant == "hop_off_by_one" else 0
    x = np.pad(x, ((0, 0), (half, half + shift)), mode="constant" if mutant == "zero_pad" else "reflect")
    frames = T // hop + 1
    idx = (np.arange(frames) * hop + shift)[:, None] + np.arange(n_fft)[None]
    win = f64(bufs["mfcc.MelSpectrogram.spectrogram.window"])
    if mutant == "symmetric_window":  # hann(N, periodic=False)
        win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / (n_fft - 1))
    xw = r32(x[:, idx] * win)                                           # [B, frames, n_fft]
    power = np.abs(np.fft.rfft(xw, axis=-1)) ** 2
    if cfg["normalized"]:                                               # Spectrogram(normalized=True): spec / sqrt(sum w^2)
        power = power * (1.0 / (win ** 2).sum())
    power = r32(power)
    mel = r32(power @ f64(bufs["mfcc.MelSpectrogram.mel_scale.fb"]))    # [B, frames, n_mels]
    floor = None
    if cfg["log_mels"]:
        lm = r32(np.log(mel + 1e-6))
        floored = lm
    else:
        logf = np.log if mutant == "natural_log_db" else np.log10
        lm = r32(10.0 * logf(np.maximum(mel, 1e-10)))
        top_db = 100.0 if mutant == "top_db_100" else 80.0
        peak = lm.max(axis=(1, 2), keepdims=True) if mutant == "per_clip_floor" else lm.max()  # ONE maximum over the batch
        floor = r32(peak - top_db)
        floored = lm if mutant == "no_floor" else np.maximum(lm, floor)
    if details is not None:
        details["logmel"], details["floor"] = lm, floor
    coef = r32(floored @ f64(bufs["mfcc.dct_mat"])).transpose(0, 2, 1)  # [B, 13, frames]
    d1 = r32(_deltas(coef, mutant == "delta_zero_edge"))
    d2 = r32(_deltas(d1, mutant == "delta_zero_edge"))
    return np.concatenate([coef, d1, d2], axis=1)


def oracle_features(wave: torch.Tensor, bufs, cfg, input_ulaw) -> torch.Tensor:
    """The oracle's feature rows (ref_cpu.conv_mfcc_encoder up to its "features" probe), float32."""
    x = ref_cpu.invert_ulaw(wave) if input_ulaw else wave
    h = ref_cpu.mfcc_transform(x, bufs, cfg)
    d = ref_cpu.deltas(h)
    return torch.cat([h, d, ref_cpu.deltas(d)], dim=1)


class Case:
    """One input with everything the gate is derived from.  gate = GATE_FACTOR * max(E_oracle, E_model): the project claims
    its float64 DFT is closer to the exact transform than the oracle's float32 FFT, so the oracle's own error is the yardstick;
    E_model covers the cases where the float32 rounding points no kernel can avoid exceed it."""

    def __init__(self, wave: torch.Tensor, version: int, input_ulaw: bool, bufs=None):
        self.wave, self.version, self.input_ulaw = wave, version, input_ulaw
        self.cfg = ref_cpu.mfcc_config(version)
        self.bufs = bufs if bufs is not None else buffers(version)
        self.details = {}
        self.ref = front_end_ref(wave, self.bufs, self.cfg, input_ulaw, details=self.details)
        self.oracle = oracle_features(wave, self.bufs, self.cfg, input_ulaw)
        self.e_oracle = float(np.abs(self.oracle.double().numpy() - self.ref).max())
        self.e_model = float(np.abs(front_end_ref(wave, self.bufs, self.cfg, input_ulaw, emulate=True) - self.ref).max())
        self.ref_max = float(np.abs(self.ref).max())
        self.gate = GATE_FACTOR * max(self.e_oracle, self.e_model)
        self.cap = GATE_CAP * max(1.0, self.ref_max)

    def mutant(self, name: str) -> np.ndarray:
        return front_end_ref(self.wave, self.bufs, self.cfg, self.input_ulaw, mutant=name)

    def floored_fraction(self, clip=None) -> float:
        lm = self.details["logmel"] if clip is None else self.details["logmel"][clip]
        return float((lm < self.details["floor"]).mean())

    def error(self, got: torch.Tensor):
        """(max|got - ref|, "clip c row r frame f" of the worst element) for [B, 39, frames] feature rows."""
        d = np.abs(got.double().numpy() - self.ref)
        c, r, f = np.unravel_index(int(d.argmax()), d.shape)
        return float(d.max()), f"clip {c} row {r} frame {f} of {d.shape[2]}"


@functools.lru_cache(maxsize=None)
def buffers(version: int):
    return ref_cpu.mfcc_buffers(ref_cpu.mfcc_config(version))


@functools.lru_cache(maxsize=None)
def front_end_case(family: str, T: int, version: int, input_ulaw: bool) -> Case:
    return Case(make_batch(family, T), version, input_ulaw)


def numpy_mfcc(wave: np.ndarray, cfg: dict) -> np.ndarray:
    """Independent restatement of torchaudio.transforms.MFCC for one [T] waveform (float64 throughout); builds its own periodic
    Hann window, HTK filter bank and orthonormal DCT-II instead of reading the checkpoint's."""
    n_fft, hop, n_mels, sr = cfg["n_fft"], cfg["hop"], cfg["n_mels"], cfg["sample_rate"]
    x = np.pad(wave.astype(np.float64), n_fft // 2, mode="reflect")
    frames = 1 + (len(x) - n_fft) // hop
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)  # periodic Hann
    spec = np.stack([np.fft.rfft(x[f * hop:f * hop + n_fft] * win) for f in range(frames)], axis=1)  # [freq, frames]
    if cfg["normalized"]:
        spec = spec / np.sqrt((win ** 2).sum())
    power = np.abs(spec) ** 2
    # HTK mel filter bank, norm=None
    hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)  # noqa: E731
    mel2hz = lambda m: 700.0 * (10 ** (m / 2595.0) - 1.0)  # noqa: E731
    freqs = np.linspace(0, sr // 2, n_fft // 2 + 1)
    pts = mel2hz(np.linspace(hz2mel(0.0), hz2mel(sr // 2), n_mels + 2))
    fb = np.zeros((len(freqs), n_mels))
    for m in range(n_mels):
        lo, ce, hi = pts[m], pts[m + 1], pts[m + 2]
        fb[:, m] = np.maximum(0.0, np.minimum((freqs - lo) / (ce - lo), (hi - freqs) / (hi - ce)))
    mel = fb.T @ power
    if cfg["log_mels"]:
        mel = np.log(mel + 1e-6)
    else:
        mel = 10.0 * np.log10(np.maximum(mel, 1e-10))
        mel = np.maximum(mel, mel.max() - 80.0)
    k = np.arange(cfg["n_mfcc"])[:, None]
    dct = np.cos(np.pi / n_mels * (np.arange(n_mels)[None] + 0.5) * k) * np.sqrt(2.0 / n_mels)
    dct[0] *= 1.0 / math.sqrt(2.0)
    return dct @ mel
