"""
Pauses of a pack of recordings (the reference has nothing of the kind): `pause_mask` says which samples of
the padded source rows lie in a pause -- the uint8 mask the keep region takes (`vqvs_pause_mask`, csrc/pause_kernels.hip) -- and
`windows_kept` which windows a mask covers whole (`vqvs_windows_kept`), the windows whose forward cannot reach the result.

The detector is integer arithmetic on the 16-bit values a WAV would hold: a frame is quiet iff its energy is at most
`threshold_energy(db)` per sample, a pause is a run of at least `min_pause_frames` quiet frames, and `guard_frames` are trimmed
off each end that touches speech.  The mask equals its definition (include/vqvs.h, tests/pause_ref.py) bit for bit, and a
recording's mask does not depend on the pack it is in.
"""

from __future__ import annotations

import math
from typing import Sequence

import torch

from . import _native
from .longform import pack_table

FULL_SCALE_ENERGY = 1 << 30  # the energy per sample of a full-scale square wave: 32768^2


def threshold_energy(db: float) -> int:
    """A level in dB re full scale as the detector's integer energy per sample: floor(2^30 * 10^(db / 10)), in float64."""
    db = float(db)
    if not math.isfinite(db) or db > 0.0:
        raise ValueError(f"threshold_db={db!r} must be a finite level at or below 0 dBFS")
    return int(math.floor(FULL_SCALE_ENERGY * 10.0 ** (db / 10.0)))


def pause_mask(rows: torch.Tensor, counts: Sequence[int], window: int, hop: int, *, threshold_db: float, frame: int = 160,
               min_pause_frames: int = 30, guard_frames: int = 5, return_counts: bool = False):
    """rows [1,1,total] float32: the padded source rows of a pack of recordings of `counts` windows each, end to end (`plan_pack`) ->
    the uint8 mask [1,1,total] of the samples that lie in a pause.  With `return_counts` also an int64 [R,2] tensor: kept samples
    and pauses per recording."""
    _native.require_cuda(rows)
    first, R, _, _, total = pack_table(counts, window, hop, rows.device)
    if rows.dim() != 3 or rows.shape[0] != 1 or rows.shape[1] != 1 or rows.shape[2] != total:
        raise ValueError(f"rows must be [1, 1, {total}] (recordings of {list(counts)} windows of {window} every {hop}), got {tuple(rows.shape)}")
    x = rows.detach().to(torch.float32).contiguous()
    keep = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    stats = torch.empty(R, 2, dtype=torch.int64, device=x.device) if return_counts else None
    with torch.cuda.device(x.device):
        _native.check(_native.lib().vqvs_pause_mask(x.data_ptr(), keep.data_ptr(), _native._ptr(stats), first.data_ptr(), R, int(window), int(hop),
                                                    int(frame), threshold_energy(threshold_db), int(min_pause_frames), int(guard_frames),
                                                    _native._stream_ptr()))
    return (keep, stats) if return_counts else keep


def windows_kept(keep: torch.Tensor, counts: Sequence[int], window: int, hop: int) -> torch.Tensor:
    """keep [1,1,total] bool or uint8 in pack layout -> uint8 [N]: 1 for a window whose every sample is kept."""
    _native.require_cuda(keep)
    first, R, N, _, total = pack_table(counts, window, hop, keep.device)
    if keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"keep must be a bool or uint8 tensor, got {keep.dtype}")
    if keep.numel() != total:
        raise ValueError(f"keep must hold {total} samples (recordings of {list(counts)} windows of {window} every {hop}), got {keep.numel()}")
    mask = keep.detach().to(torch.uint8).contiguous()
    out = torch.empty(N, dtype=torch.uint8, device=mask.device)
    with torch.cuda.device(mask.device):
        _native.check(_native.lib().vqvs_windows_kept(mask.data_ptr(), out.data_ptr(), first.data_ptr(), R, int(window), int(hop),
                                                      _native._stream_ptr()))
    return out
