"""
Objective scores of a finished conversion: per clip, the sum over frames of the mel-cepstral distortion (MCD, dB) and of the
log-mel spectral distance (LSD, dB) between two waveforms, frame for frame, through `vqvs_spectral_distance` (one fused kernel,
csrc/spectral_kernels.hip; definitions in include/vqvs.h and DESIGN.md section 3.13).  The conversion preserves timing, so the
recordings are compared without alignment.  `SpectralDistance.cepstra` (`vqvs_mel_cepstra`, the same front end) writes the per-frame
cepstra of recordings of different lengths out, for the aligned comparison with a parallel recording (dtw.py, section 3.18).
"""

from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _native


def spectral_constants(sample_rate: int, n_fft: int, n_mels: int, n_ceps: int) -> Dict[str, np.ndarray]:
    """The four constant tables of `vqvs_spectral_distance`, built in float64 numpy: "window" [n_fft], the periodic Hann window;
    "fb" [n_fft/2+1, n_mels], the HTK mel filter bank (triangles of height 1, norm=None) from 0 to sample_rate / 2; "dct"
    [n_mels, n_ceps], the orthonormal DCT-II; "twiddle" [n_fft, 2], cos and sin of 2 pi i / n_fft.  The first three are rounded to
    float32; the twiddle table stays float64."""
    if n_fft < 2 or n_fft % 2 or n_mels < 1 or not 1 <= n_ceps <= n_mels or sample_rate <= 0:
        raise ValueError(f"bad constants request: sample_rate={sample_rate} n_fft={n_fft} n_mels={n_mels} n_ceps={n_ceps}")
    i = np.arange(n_fft, dtype=np.float64)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / n_fft)
    twiddle = np.stack([np.cos(2.0 * np.pi * i / n_fft), np.sin(2.0 * np.pi * i / n_fft)], axis=1)
    # HTK mel scale; filter m rises from point m to point m + 1 and falls to point m + 2
    freqs = np.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1)
    mel_max = 2595.0 * np.log10(1.0 + (sample_rate / 2.0) / 700.0)
    pts = 700.0 * (10.0 ** (np.linspace(0.0, mel_max, n_mels + 2) / 2595.0) - 1.0)
    width = np.diff(pts)
    slopes = pts[None, :] - freqs[:, None]                       # [n_freqs, n_mels + 2]
    fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / width[:-1], slopes[:, 2:] / width[1:]))
    m = np.arange(n_mels, dtype=np.float64)
    dct = np.cos(np.pi / n_mels * (m[:, None] + 0.5) * np.arange(n_ceps, dtype=np.float64)[None, :]) * np.sqrt(2.0 / n_mels)
    dct[:, 0] *= np.sqrt(0.5)
    return {"window": window.astype(np.float32), "fb": fb.astype(np.float32), "dct": dct.astype(np.float32), "twiddle": twiddle}


class SpectralDistance:
    """`SpectralDistance()(a, b)` -> {"mcd": float64 [B], "lsd": float64 [B], "frames": F}: the clips' SUMS over their F = T // hop + 1
    frames (divide by F for a per-frame mean in dB).  `a` and `b` are float32 tensors [B,1,T] or [B,T] on one ROCm device.  The sums
    are deterministic float64: a clip scores the same whatever batch it is in, d(a, a) is exactly 0 and d(a, b) == d(b, a)."""

    def __init__(self, sample_rate: int = 16000, n_fft: int = 400, hop: int = 160, n_mels: int = 40, n_ceps: int = 13, eps: float = 1e-6):
        if n_fft % 2 or not 16 <= n_fft <= 512:
            raise ValueError(f"n_fft={n_fft} must be even and in 16..512")
        if not 1 <= hop <= n_fft:
            raise ValueError(f"hop={hop} outside 1..n_fft={n_fft}")
        if not 1 <= n_mels <= 128 or not 2 <= n_ceps <= min(n_mels, 64):
            raise ValueError(f"n_mels={n_mels} outside 1..128 or n_ceps={n_ceps} outside 2..min(n_mels, 64)")
        if not (np.isfinite(eps) and eps > 0):
            raise ValueError(f"eps={eps} must be finite and positive")
        self.sample_rate, self.n_fft, self.hop, self.n_mels, self.n_ceps, self.eps = sample_rate, n_fft, hop, n_mels, n_ceps, float(eps)
        self._host = spectral_constants(sample_rate, n_fft, n_mels, n_ceps)
        self._device = {}

    def constants(self, device) -> Dict[str, torch.Tensor]:
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = {k: torch.from_numpy(v).contiguous().to(device) for k, v in self._host.items()}
        return self._device[device]

    def frames(self, T: int) -> int:
        return T // self.hop + 1

    def __call__(self, a: torch.Tensor, b: torch.Tensor) -> Dict[str, object]:
        if not (torch.is_tensor(a) and torch.is_tensor(b)):
            raise ValueError("a and b must be tensors")
        if a.shape != b.shape:
            raise ValueError(f"a and b differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
        if a.dim() == 3 and a.shape[1] == 1:
            a, b = a[:, 0], b[:, 0]
        if a.dim() != 2:
            raise ValueError(f"expected waveforms of shape [B, 1, T] or [B, T], got {tuple(a.shape)}")
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise ValueError(f"a and b must be float32, got {a.dtype} and {b.dtype}")
        B, T = int(a.shape[0]), int(a.shape[1])
        if not (1 <= B <= 65535 and self.n_fft // 2 < T <= 2 ** 30):
            raise ValueError(f"B={B}, T={T} outside the limits 1..65535, {self.n_fft // 2 + 1}..2^30")
        _native.require_cuda(a, b)
        if a.device != b.device:
            raise ValueError("a and b must be on one device")
        a, b = a.detach().contiguous(), b.detach().contiguous()
        c = self.constants(a.device)
        mcd = torch.empty(B, device=a.device, dtype=torch.float64)
        lsd = torch.empty(B, device=a.device, dtype=torch.float64)
        with torch.cuda.device(a.device):
            _native.check(_native.lib().vqvs_spectral_distance(
                a.data_ptr(), b.data_ptr(), c["window"].data_ptr(), c["twiddle"].data_ptr(), c["fb"].data_ptr(), c["dct"].data_ptr(),
                mcd.data_ptr(), lsd.data_ptr(), B, T, self.n_fft, self.hop, self.n_mels, self.n_ceps, self.eps, _native._stream_ptr()))
        return {"mcd": mcd, "lsd": lsd, "frames": self.frames(T)}

    def cepstra(self, x: torch.Tensor, lengths, logmel: bool = False) -> Dict[str, torch.Tensor]:
        """The per-frame values behind the distances, through `vqvs_mel_cepstra`: `x` [B,1,T] or [B,T] float32 holds recordings of
        `lengths[b]` samples (n_fft / 2 < length <= T; what lies beyond is never read) -> {"ceps": float32 [B, T // hop + 1, n_ceps],
        "frames": int32 [B], the rows' own frame counts length // hop + 1} and with `logmel` also {"logmel": float32 [B, T // hop + 1,
        n_mels]}.  Frames at or beyond a row's count are 0.  A row's values are those of the recording alone."""
        if not torch.is_tensor(x):
            raise ValueError("x must be a tensor")
        if x.dim() == 3 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 2:
            raise ValueError(f"expected waveforms of shape [B, 1, T] or [B, T], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"x must be float32, got {x.dtype}")
        B, T = int(x.shape[0]), int(x.shape[1])
        if not (1 <= B <= 65535 and self.n_fft // 2 < T <= 2 ** 30):
            raise ValueError(f"B={B}, T={T} outside the limits 1..65535, {self.n_fft // 2 + 1}..2^30")
        lengths = check_lengths(lengths, B, self.n_fft // 2 + 1, T, "lengths")
        _native.require_cuda(x)
        x = x.detach().contiguous()
        c = self.constants(x.device)
        F = self.frames(T)
        d_len = lengths.to(x.device)
        ceps = torch.empty(B, F, self.n_ceps, device=x.device, dtype=torch.float32)
        mel = torch.empty(B, F, self.n_mels, device=x.device, dtype=torch.float32) if logmel else None
        frames = torch.empty(B, device=x.device, dtype=torch.int32)
        with torch.cuda.device(x.device):
            _native.check(_native.lib().vqvs_mel_cepstra(
                x.data_ptr(), d_len.data_ptr(), c["window"].data_ptr(), c["twiddle"].data_ptr(), c["fb"].data_ptr(), c["dct"].data_ptr(),
                ceps.data_ptr(), _native._ptr(mel), frames.data_ptr(), B, T, self.n_fft, self.hop, self.n_mels, self.n_ceps, self.eps,
                _native._stream_ptr()))
        out = {"ceps": ceps, "frames": frames}
        if logmel:
            out["logmel"] = mel
        return out


def check_lengths(lengths, B: int, lo: int, hi: int, what: str) -> torch.Tensor:
    """`lengths` (a sequence of integers or an integer tensor) as a host int32 tensor [B] with every entry in lo..hi, or ValueError."""
    if torch.is_tensor(lengths):
        if lengths.dtype not in (torch.int32, torch.int64) or lengths.dim() != 1:
            raise ValueError(f"{what} must be a one-dimensional int32 or int64 tensor, got {lengths.dtype} {tuple(lengths.shape)}")
        values = lengths.detach().cpu().tolist()
    else:
        try:
            values = list(lengths)
        except TypeError:
            raise ValueError(f"{what} must be a sequence of integers") from None
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in values):
            raise ValueError(f"{what} must be integers, got {values}")
    if len(values) != B:
        raise ValueError(f"{len(values)} {what} for {B} rows")
    if any(not lo <= int(v) <= hi for v in values):
        raise ValueError(f"{what} {values} outside {lo}..{hi}")
    return torch.tensor([int(v) for v in values], dtype=torch.int32)
