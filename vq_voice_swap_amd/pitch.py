"""
Pitch scores of a finished conversion: per frame the YIN period of two waveforms, per clip the voicing counts and the sums of the
frame-wise pitch distance in semitones and of its square, through `vqvs_pitch_distance` (one fused kernel, csrc/pitch_kernels.hip;
definition in include/vqvs.h and DESIGN.md section 3.14).  The samples are quantised to 16 bits first, so the difference function
is integer arithmetic and the periods are the definition's bit for bit.  The conversion preserves timing, so the recordings are
compared frame for frame without alignment.
"""

from __future__ import annotations

import math
from typing import Dict

import torch

from . import _native


class PitchDistance:
    """`PitchDistance()(a, b)` -> {"voiced_a", "voiced_b", "voiced_both", "vuv": int64 [B], "shift_sum", "shift_sq_sum": float64 [B],
    "frames": F}: per clip the frames voiced in a, in b and in both, the frames whose voicing differs, and over the frames voiced
    in both the sum of l_f = 12 log2(f0_b / f0_a) (semitones by which b is higher than a) and of l_f^2.  `.track(x)` ->
    {"period", "f0": float64 [B, F]}: samples per period and Hz, 0 where unvoiced.  `a`, `b` and `x` are float32 tensors [B,1,T] or
    [B,T] on one ROCm device.  The lags searched are tau_min = ceil(sample_rate / fmax) .. tau_max = floor(sample_rate / fmin).
    All values are deterministic: a clip scores the same whatever batch it is in, b = a gives sums of exactly 0 and swapping the
    arguments negates shift_sum."""

    def __init__(self, sample_rate: int = 16000, window: int = 400, hop: int = 160, fmin: float = 60.0, fmax: float = 500.0,
                 threshold: float = 0.15):
        if not (sample_rate > 0 and math.isfinite(fmin) and math.isfinite(fmax) and 0 < fmin < fmax):
            raise ValueError(f"sample_rate={sample_rate}, fmin={fmin}, fmax={fmax}: need sample_rate > 0 and 0 < fmin < fmax")
        tau_min, tau_max = math.ceil(sample_rate / fmax), math.floor(sample_rate / fmin)
        if not 16 <= window <= 2048:
            raise ValueError(f"window={window} outside 16..2048")
        if not 1 <= hop <= window:
            raise ValueError(f"hop={hop} outside 1..window={window}")
        if not 2 <= tau_min < tau_max <= 1023:
            raise ValueError(f"fmin={fmin}, fmax={fmax} at sample_rate={sample_rate} give lags {tau_min}..{tau_max}: outside 2 <= tau_min < tau_max <= 1023")
        if window * tau_max > 1 << 20:
            raise ValueError(f"window={window} times tau_max={tau_max} is more than 2^20")
        if not (math.isfinite(threshold) and 0.0 < threshold <= 1.0):
            raise ValueError(f"threshold={threshold} must lie in (0, 1]")
        self.sample_rate, self.window, self.hop, self.fmin, self.fmax = sample_rate, int(window), int(hop), float(fmin), float(fmax)
        self.tau_min, self.tau_max, self.threshold = tau_min, tau_max, float(threshold)

    def frames(self, T: int) -> int:
        return T // self.hop + 1

    def _waveforms(self, *xs):
        """[B,1,T] or [B,T] float32 tensors of one shape on one ROCm device -> contiguous [B,T] tensors, B, T."""
        if not all(torch.is_tensor(x) for x in xs):
            raise ValueError("the waveforms must be tensors")
        if any(x.shape != xs[0].shape for x in xs):
            raise ValueError(f"a and b differ in shape: {[tuple(x.shape) for x in xs]}")
        if xs[0].dim() == 3 and xs[0].shape[1] == 1:
            xs = tuple(x[:, 0] for x in xs)
        if xs[0].dim() != 2:
            raise ValueError(f"expected waveforms of shape [B, 1, T] or [B, T], got {tuple(xs[0].shape)}")
        if any(x.dtype != torch.float32 for x in xs):
            raise ValueError(f"the waveforms must be float32, got {[x.dtype for x in xs]}")
        B, T = int(xs[0].shape[0]), int(xs[0].shape[1])
        if not (1 <= B <= 65535 and 1 <= T <= 2 ** 30):
            raise ValueError(f"B={B}, T={T} outside the limits 1..65535, 1..2^30")
        _native.require_cuda(*xs)
        if any(x.device != xs[0].device for x in xs):
            raise ValueError("a and b must be on one device")
        return tuple(x.detach().contiguous() for x in xs), B, T

    def _call(self, a, b, period_a, period_b, counts, sums, B, T):
        with torch.cuda.device(a.device):
            _native.check(_native.lib().vqvs_pitch_distance(
                a.data_ptr(), _native._ptr(b), _native._ptr(period_a), _native._ptr(period_b), _native._ptr(counts), _native._ptr(sums),
                B, T, self.window, self.hop, self.tau_min, self.tau_max, self.threshold, _native._stream_ptr()))

    def __call__(self, a: torch.Tensor, b: torch.Tensor) -> Dict[str, object]:
        (a, b), B, T = self._waveforms(a, b)
        counts = torch.empty(B, 4, device=a.device, dtype=torch.int64)
        sums = torch.empty(B, 2, device=a.device, dtype=torch.float64)
        self._call(a, b, None, None, counts, sums, B, T)
        return {"voiced_a": counts[:, 0], "voiced_b": counts[:, 1], "voiced_both": counts[:, 2], "vuv": counts[:, 3],
                "shift_sum": sums[:, 0], "shift_sq_sum": sums[:, 1], "frames": self.frames(T)}

    def track(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        (x,), B, T = self._waveforms(x)
        period = torch.empty(B, self.frames(T), device=x.device, dtype=torch.float64)
        self._call(x, None, period, None, None, None, B, T)
        f0 = torch.where(period > 0, self.sample_rate / period.clamp_min(1.0), torch.zeros_like(period))
        return {"period": period, "f0": f0}
