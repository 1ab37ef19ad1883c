"""
Scores against a PARALLEL recording -- the target speaker reading the same sentence --, which differs from the converted one in
timing: the two are aligned by dynamic time warping under the mel-cepstral cost and the distortion is summed along the warping
path ("MCD-DTW").  `SpectralDistance.cepstra` (vqvs_mel_cepstra) gives the per-frame cepstra of recordings of different lengths,
`dtw_distance` (vqvs_dtw_distance, one workgroup per pair, csrc/dtw_kernels.hip) the path's cost and length and, with per-frame
pitch tracks, the voicing counts and the sums of the pitch distance over the path's cells.  Definitions: include/vqvs.h and
DESIGN.md section 3.18.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _native
from .pitch import PitchDistance
from .spectral import SpectralDistance, check_lengths

MAX_FRAMES = 2048  # per side (20 s at the default hop)


def _counts(frames, B: int, Fmax: int, what: str) -> torch.Tensor:
    if torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.int32 and frames.dim() == 1 and frames.shape[0] == B:
        return frames.contiguous()  # (device data: the kernel clamps it into 1..Fmax)
    return check_lengths(frames, B, 1, Fmax, what)


def dtw_distance(ceps_a: torch.Tensor, frames_a, ceps_b: torch.Tensor, frames_b, track_a: Optional[torch.Tensor] = None,
                 track_b: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """`vqvs_dtw_distance` on float32 cepstra [B, Fa_max, n_ceps] and [B, Fb_max, n_ceps] with frame counts [B] (an int32 tensor on
    the device is passed through as it is; anything else is checked against 1..F_max on the host) -> {"cost": float64 [B], "steps":
    int32 [B]}; with float64 tracks [B, Fa_max] and [B, Fb_max] (NaN: no value) also {"both", "vuv": int64 [B], "shift_sum",
    "shift_sq_sum": float64 [B]} over the path's cells, the shift being track_b - track_a."""
    if not (torch.is_tensor(ceps_a) and torch.is_tensor(ceps_b)):
        raise ValueError("the cepstra must be tensors")
    if ceps_a.dim() != 3 or ceps_b.dim() != 3 or ceps_a.shape[0] != ceps_b.shape[0] or ceps_a.shape[2] != ceps_b.shape[2]:
        raise ValueError(f"expected cepstra [B, Fa, n_ceps] and [B, Fb, n_ceps], got {tuple(ceps_a.shape)} and {tuple(ceps_b.shape)}")
    if ceps_a.dtype != torch.float32 or ceps_b.dtype != torch.float32:
        raise ValueError(f"the cepstra must be float32, got {ceps_a.dtype} and {ceps_b.dtype}")
    B, Fa, n_ceps = (int(n) for n in ceps_a.shape)
    Fb = int(ceps_b.shape[1])
    if not (1 <= B <= 65535 and 1 <= Fa <= MAX_FRAMES and 1 <= Fb <= MAX_FRAMES and 2 <= n_ceps <= 64):
        raise ValueError(f"B={B}, Fa_max={Fa}, Fb_max={Fb}, n_ceps={n_ceps} outside the limits 1..65535, 1..{MAX_FRAMES}, 1..{MAX_FRAMES}, 2..64")
    if (track_a is None) != (track_b is None):
        raise ValueError("the tracks come together: both or neither")
    tracks = track_a is not None
    if tracks:
        if not (torch.is_tensor(track_a) and torch.is_tensor(track_b)) or track_a.dtype != torch.float64 or track_b.dtype != torch.float64:
            raise ValueError("the tracks must be float64 tensors")
        if tuple(track_a.shape) != (B, Fa) or tuple(track_b.shape) != (B, Fb):
            raise ValueError(f"expected tracks {(B, Fa)} and {(B, Fb)}, got {tuple(track_a.shape)} and {tuple(track_b.shape)}")
    fa, fb = _counts(frames_a, B, Fa, "frames_a"), _counts(frames_b, B, Fb, "frames_b")
    used = [ceps_a, ceps_b] + ([track_a, track_b] if tracks else [])
    _native.require_cuda(*used)
    dev = ceps_a.device
    if any(t.device != dev for t in used):
        raise ValueError("cepstra and tracks must be on one device")
    fa, fb = fa.to(dev), fb.to(dev)
    ceps_a, ceps_b = ceps_a.detach().contiguous(), ceps_b.detach().contiguous()
    if tracks:
        track_a, track_b = track_a.detach().contiguous(), track_b.detach().contiguous()
    cost = torch.empty(B, device=dev, dtype=torch.float64)
    steps = torch.empty(B, device=dev, dtype=torch.int32)
    counts = torch.empty(B, 2, device=dev, dtype=torch.int64) if tracks else None
    sums = torch.empty(B, 2, device=dev, dtype=torch.float64) if tracks else None
    with torch.cuda.device(dev):
        _native.check(_native.lib().vqvs_dtw_distance(
            ceps_a.data_ptr(), ceps_b.data_ptr(), fa.data_ptr(), fb.data_ptr(), _native._ptr(track_a), _native._ptr(track_b), cost.data_ptr(),
            steps.data_ptr(), _native._ptr(counts), _native._ptr(sums), B, Fa, Fb, n_ceps, _native._stream_ptr()))
    out = {"cost": cost, "steps": steps}
    if tracks:
        out.update(both=counts[:, 0], vuv=counts[:, 1], shift_sum=sums[:, 0], shift_sq_sum=sums[:, 1])
    return out


class AlignedDistance:
    """`AlignedDistance(spectral, pitch)(a, len_a, b, len_b)` -> {"cost": float64 [B], "steps": int32 [B], "frames_a", "frames_b":
    int32 [B]}: recording b of every pair aligned to recording a by dynamic time warping; cost is the mel-cepstral distortion (dB)
    summed over the path's `steps` cells.  `a` [B,1,Ta] or [B,Ta] and `b` [B,1,Tb] or [B,Tb] are float32 on one ROCm device and hold
    recordings of len_a[i] and len_b[i] samples; what lies beyond a recording's length is never used.  With a `PitchDistance` also
    {"both", "vuv": int64 [B], "shift_sum", "shift_sq_sum": float64 [B]}: the path's cells voiced in both recordings and in exactly
    one, and over the former the sum of l = 12 log2(f0_b / f0_a) (semitones by which b is higher than a, the convention of
    `PitchDistance`) and of l^2.  A pair scores the same whatever batch it is in and however far its rows are padded."""

    def __init__(self, spectral: Optional[SpectralDistance] = None, pitch: Optional[PitchDistance] = None):
        self.spectral = SpectralDistance() if spectral is None else spectral
        self.pitch = pitch
        if pitch is not None and (pitch.hop != self.spectral.hop or pitch.sample_rate != self.spectral.sample_rate):
            raise ValueError(f"the pitch hop and rate ({pitch.hop}, {pitch.sample_rate}) must equal the spectral ones "
                             f"({self.spectral.hop}, {self.spectral.sample_rate}): one track value per cepstral frame")

    def max_samples(self) -> int:
        """The longest recording the alignment takes: 2048 frames."""
        return MAX_FRAMES * self.spectral.hop - 1

    def _semitones(self, x: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """12 log2(f0) per frame in float64, NaN where unvoiced.  `PitchDistance.track` knows one length for the whole batch and reads
        zeros outside it, so every row is zeroed beyond its own length first: its frames below its own count are then those of the
        recording tracked alone (the alignment reads no others)."""
        if x.dim() == 3:
            x = x[:, 0]
        inside = torch.arange(x.shape[1], device=x.device)[None, :] < lengths.to(x.device)[:, None]
        f0 = self.pitch.track(torch.where(inside, x, torch.zeros_like(x)))["f0"]
        return torch.where(f0 > 0, 12.0 * torch.log2(f0.clamp_min(1e-300)), torch.full_like(f0, float("nan")))

    def __call__(self, a: torch.Tensor, len_a, b: torch.Tensor, len_b) -> Dict[str, torch.Tensor]:
        if not (torch.is_tensor(a) and torch.is_tensor(b)):
            raise ValueError("a and b must be tensors")
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"a and b hold {a.shape[0]} and {b.shape[0]} recordings")
        if a.device != b.device:
            raise ValueError("a and b must be on one device")
        for x in (a, b):
            if x.shape[-1] > self.max_samples():
                raise ValueError(f"rows of {x.shape[-1]} samples are more than {MAX_FRAMES} frames")
        ca, cb = self.spectral.cepstra(a, len_a), self.spectral.cepstra(b, len_b)
        ta = tb = None
        if self.pitch is not None:
            half = self.spectral.n_fft // 2 + 1
            ta = self._semitones(a, check_lengths(len_a, a.shape[0], half, a.shape[-1], "len_a"))
            tb = self._semitones(b, check_lengths(len_b, b.shape[0], half, b.shape[-1], "len_b"))
        out = dtw_distance(ca["ceps"], ca["frames"], cb["ceps"], cb["frames"], ta, tb)
        out.update(frames_a=ca["frames"], frames_b=cb["frames"])
        return out
