"""
Vector-quantisation layer, inference and evaluation halves (reference vq_voice_swap/vq.py:36-51, 74-143, 199-243):
nearest-codeword search and embedding gather run as HIP kernels (`vqvs_vq_argmin`, `vqvs_vq_embed`); `VQ.quantize` runs the
search, the embedding, the per-clip quantisation error and the code counts as ONE kernel (`vqvs_vq_quantize`), which is what
`StandardVQLoss.from_sq_err` and `code_usage` read.  `ReviveVQLoss`, the usage tracker and dead-code revival (vq.py:54-71,
145-196) stay out of scope: they are training regularisers, and nothing here trains.
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _native


class VQLoss(nn.Module):
    """A loss of a VQ layer: (inputs [N,C,...], embedded like inputs, dictionary [D,C]) -> scalar (vq.py:17-33)."""

    def forward(self, inputs: torch.Tensor, embedded: torch.Tensor, dictionary: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError


class StandardVQLoss(VQLoss):
    """The standard VQ-VAE loss IN VALUE (vq.py:36-51): codebook term + commitment * commitment term, which are the same
    number mean((inputs - embedded)^2) once nothing is differentiated.  Evaluation only: no gradients are recorded."""

    def __init__(self, commitment: float = 0.25):
        super().__init__()
        self.commitment = commitment

    def forward(self, inputs: torch.Tensor, embedded: torch.Tensor, dictionary: torch.Tensor) -> torch.Tensor:
        _ = dictionary
        with torch.no_grad():
            codebook_loss = ((inputs.detach() - embedded.detach()) ** 2).mean()
            comm_loss = ((inputs.detach() - embedded.detach()) ** 2).mean()
            return codebook_loss + self.commitment * comm_loss

    def from_sq_err(self, sq_err, numel: int) -> torch.Tensor:
        """The same number from `VQ.quantize`'s per-clip sums: (1 + commitment) * sum(sq_err) / numel, in float64."""
        total = sq_err.detach().to(torch.float64).sum() if torch.is_tensor(sq_err) else torch.tensor(float(np.sum(sq_err)), dtype=torch.float64)
        return (1.0 + self.commitment) * total / float(numel)


def code_usage(hist) -> Dict[str, float]:
    """{"used_codes": bins that are not empty, "perplexity": exp(-sum p ln p) over them} of a code histogram, on the host in
    float64.  An all-zero histogram gives 0 and 0.0."""
    h = hist.detach().cpu().numpy() if torch.is_tensor(hist) else np.asarray(hist)
    h = h.astype(np.float64).reshape(-1)
    if (h < 0).any():
        raise ValueError("a histogram has no negative counts")
    nz = h[h > 0]
    if nz.size == 0:
        return {"used_codes": 0, "perplexity": 0.0}
    p = nz / nz.sum()
    return {"used_codes": int(nz.size), "perplexity": float(math.exp(-float(np.sum(p * np.log(p)))))}


class VQ(nn.Module):
    def __init__(self, num_channels: int, num_codes: int, dead_rate: int = 100):
        super().__init__()
        self.num_channels = num_channels
        self.num_codes = num_codes
        self.dead_rate = dead_rate
        self.dictionary = nn.Parameter(torch.randn(num_codes, num_channels))
        self.register_buffer("usage_count", dead_rate * torch.ones(num_codes).long())

    def embed(self, idxs: torch.Tensor) -> torch.Tensor:
        """int [N, ...] -> float [N, C, ...] (vq.py:98-110)."""
        _native.require_cuda(idxs)
        n = idxs.shape[0]
        flat = idxs.detach().reshape(n, -1).to(torch.int64).contiguous()
        _native.check_index_range(flat, self.num_codes, "VQ codes")
        d = self.dictionary.detach().to(device=flat.device, dtype=torch.float32).contiguous()
        out = torch.empty(n, self.num_channels, flat.shape[1], device=flat.device, dtype=torch.float32)
        with torch.cuda.device(flat.device):
            _native.check(_native.lib().vqvs_vq_embed(flat.data_ptr(), d.data_ptr(), out.data_ptr(), n, self.num_channels,
                                                      flat.shape[1], self.num_codes, _native._stream_ptr()))
        return out.reshape(n, self.num_channels, *idxs.shape[1:])

    def encode(self, inputs: torch.Tensor) -> torch.Tensor:
        """float [N, C, ...] -> int64 [N, ...] nearest code, first index on ties (vq.py:127-131)."""
        _native.require_cuda(inputs)
        n, c = inputs.shape[:2]
        if c != self.num_channels:
            raise ValueError(f"expected {self.num_channels} channels, got {c}")
        z = inputs.detach().to(torch.float32).reshape(n, c, -1).contiguous()
        d = self.dictionary.detach().to(device=z.device, dtype=torch.float32).contiguous()
        idx = torch.empty(n, z.shape[2], device=z.device, dtype=torch.int64)
        with torch.cuda.device(z.device):
            _native.check(_native.lib().vqvs_vq_argmin(z.data_ptr(), d.data_ptr(), idx.data_ptr(), n, c, z.shape[2], self.num_codes,
                                                       _native._stream_ptr()))
        return idx.reshape(n, *inputs.shape[2:])

    def quantize(self, inputs: torch.Tensor, *, hist: Optional[torch.Tensor] = None, embedded: bool = True) -> Dict[str, Optional[torch.Tensor]]:
        """One fused pass over float [N, C, ...]: {"idxs": int64 [N, ...] (what `encode` returns, bit for bit), "embedded":
        float32 [N, C, ...] (what `embed(idxs)` returns; None when `embedded=False`), "sq_err": float64 [N], the clip's
        sum of (inputs - embedded)^2}.  `hist`, a caller-owned int64 [num_codes] tensor on the inputs' device, has every
        position's code counted into it IN PLACE: zero it once and pass it to every call of an evaluation pass."""
        _native.require_cuda(inputs, hist)
        n, c = inputs.shape[:2]
        if c != self.num_channels:
            raise ValueError(f"expected {self.num_channels} channels, got {c}")
        z = inputs.detach().to(torch.float32).reshape(n, c, -1).contiguous()
        if hist is not None and (hist.dtype != torch.int64 or tuple(hist.shape) != (self.num_codes,) or not hist.is_contiguous()
                                 or hist.device != z.device):
            raise ValueError(f"hist must be a contiguous int64 [{self.num_codes}] tensor on {z.device}, got {hist.dtype} "
                             f"{tuple(hist.shape)} on {hist.device}")
        d = self.dictionary.detach().to(device=z.device, dtype=torch.float32).contiguous()
        idx = torch.empty(n, z.shape[2], device=z.device, dtype=torch.int64)
        emb = torch.empty_like(z) if embedded else None
        sq_err = torch.empty(n, device=z.device, dtype=torch.float64)
        with torch.cuda.device(z.device):
            _native.check(_native.lib().vqvs_vq_quantize(z.data_ptr(), d.data_ptr(), idx.data_ptr(), _native._ptr(emb), sq_err.data_ptr(),
                                                         _native._ptr(hist), n, c, z.shape[2], self.num_codes, _native._stream_ptr()))
        return {"idxs": idx.reshape(n, *inputs.shape[2:]), "embedded": emb.reshape(inputs.shape) if embedded else None, "sq_err": sq_err}

    def forward(self, inputs: torch.Tensor) -> Dict[str, torch.Tensor]:
        if self.training:
            raise RuntimeError("VQ training (usage tracking / revival, vq.py:145-196) is outside the accelerated path; call .eval()")
        idxs = self.encode(inputs)
        embedded = self.embed(idxs)
        return {"embedded": embedded, "passthrough": embedded, "idxs": idxs}
