"""
Denoising-loss evaluation: the per-quartile loss averages of the reference's eval_diffusion.py (its LossTracker,
vq_voice_swap/loss_tracker.py:8-41) and the speaker search of voice_search_vqvae.py:68-103, both on
`Diffusion.denoising_losses` (the fused noising / squared-error kernels); and the scores of the two guidance models
(`classification_scores`: the NLL the reference logs at train_loop.py:551-561 and :602-613, with accuracy, top-k and confusion
counts, from one fused kernel).
"""

from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import _native


def _as_f64(v) -> np.ndarray:
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.asarray(v).astype(np.float64).reshape(-1)


class _Window:
    """The last `cap` values pushed, oldest first: a ring buffer that starts small and doubles until it holds `cap`."""

    def __init__(self, cap: int):
        self.cap = cap
        self.buf = np.empty(min(cap, 1024), dtype=np.float64)
        self.n = 0      # values held
        self.head = 0   # position of the oldest one once the buffer is full at `cap`

    def push(self, vals: np.ndarray) -> None:
        vals = vals[-self.cap:] if self.cap else vals[:0]
        room = self.cap - self.n
        fill, rest = vals[:room], vals[room:]
        if fill.size:
            need = self.n + fill.size
            if need > self.buf.size:
                grown = np.empty(min(self.cap, max(need, 2 * self.buf.size)), dtype=np.float64)
                grown[:self.n] = self.buf[:self.n]
                self.buf = grown
            self.buf[self.n:need] = fill
            self.n = need
        if rest.size:  # full: overwrite the oldest values
            pos = (self.head + np.arange(rest.size)) % self.cap
            self.buf[pos] = rest
            self.head = int((self.head + rest.size) % self.cap)

    def values(self) -> np.ndarray:
        if self.n < self.cap or self.head == 0:
            return self.buf[:self.n]
        return np.concatenate((self.buf[self.head:self.n], self.buf[:self.head]))


class LossTracker:
    """Sliding averages of a loss per quantile of t.  A value at time t belongs to bucket int(t * (quantiles - 1e-8)); every
    bucket keeps its last `avg_size` values; `log_dict()` names the buckets that hold any `{prefix}q{i}`.  The averages are
    numpy means of the window in arrival order, i.e. the same floats as the reference's list-based tracker gives."""

    def __init__(self, quantiles: int = 4, avg_size: int = 1000, prefix: str = ""):
        self.quantiles = quantiles
        self.avg_size = avg_size
        self.prefix = prefix
        self._windows = [_Window(avg_size) for _ in range(quantiles)]

    def add(self, ts, mses) -> None:
        t, m = _as_f64(ts), _as_f64(mses)
        if t.shape != m.shape:
            raise ValueError(f"ts and mses differ in length: {t.size} and {m.size}")
        bucket = (t * (self.quantiles - 1e-8)).astype(np.int64)
        if t.size and (bucket.min() < 0 or bucket.max() >= self.quantiles):
            raise IndexError(f"ts outside [0, 1]: {t.min()} .. {t.max()}")
        for i, w in enumerate(self._windows):
            sel = m[bucket == i]
            if sel.size:
                w.push(sel)

    def merge(self, other: "LossTracker") -> "LossTracker":
        """Append another tracker's windows (say, another rank's) to this one's, bucket by bucket."""
        if other.quantiles != self.quantiles:
            raise ValueError(f"cannot merge trackers of {other.quantiles} and {self.quantiles} quantiles")
        for w, o in zip(self._windows, other._windows):
            w.push(o.values().copy())
        return self

    def counts(self) -> List[int]:
        return [w.n for w in self._windows]

    def quantile_averages(self) -> List[Optional[float]]:
        return [float(np.mean(w.values())) if w.n else None for w in self._windows]

    def log_dict(self) -> Dict[str, float]:
        return {f"{self.prefix}q{i}": avg for i, avg in enumerate(self.quantile_averages()) if avg is not None}


def speaker_search_losses(model, target: torch.Tensor, encoded: torch.Tensor, labels: torch.Tensor, ts: torch.Tensor,
                          batch_size: int, num_seeds: int = 1, seed: int = 0, *, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Denoising loss of ONE clip under every (label, t) pair, averaged over `num_seeds` noise draws: [len(labels)] float32
    (reference voice_search_vqvae.py:68-103).  `target` is [1,1,T], `encoded` its [1,C,T1] conditioning sequence.  Draw k
    is the same noise for every pair -- generator index k, or row k of `noise` [num_seeds,1,T] when given -- so pairs differ by
    label and t alone.  Per micro-batch only ts, labels and the conditioning rows are batch-sized: the clip and the noise
    stay single rows."""
    if target.dim() != 3 or target.shape[0] != 1 or encoded.shape[0] != 1:
        raise ValueError(f"expected one clip [1,1,T] and its conditioning [1,C,T1], got {tuple(target.shape)} and {tuple(encoded.shape)}")
    if labels.shape != ts.shape or labels.dim() != 1:
        raise ValueError(f"labels and ts must be vectors of one length, got {tuple(labels.shape)} and {tuple(ts.shape)}")
    if batch_size < 1 or num_seeds < 1:
        raise ValueError("batch_size and num_seeds must be at least 1")
    if noise is not None and noise.shape[0] != num_seeds:
        raise ValueError(f"noise has {noise.shape[0]} rows for {num_seeds} seeds")
    dev = target.device
    labels, ts = labels.to(dev), ts.to(dev)
    draw = [torch.full((batch_size,), k, dtype=torch.int64, device=dev) for k in range(num_seeds)]
    alpha = model.diffusion.schedule(ts.cpu()).to(dev)  # on the host, once for every pair: the micro-batches below never synchronise
    out = []
    for i in range(0, len(labels), batch_size):
        labels_mb, ts_mb, alpha_mb = labels[i:i + batch_size], ts[i:i + batch_size], alpha[i:i + batch_size]
        n = len(ts_mb)
        cond = encoded.expand(n, -1, -1)  # (the native forward reads one conditioning row per clip: T/256 long, the only copy made)
        per_seed = []
        for k in range(num_seeds):
            kw = dict(noise=noise[k:k + 1]) if noise is not None else dict(seed=seed, noise_index=draw[k][:n])
            per_seed.append(model.diffusion.denoising_losses(target, model.predictor, ts_mb, alpha=alpha_mb, check=False, cond=cond,
                                                             labels=labels_mb, **kw))
        out.append(torch.stack(per_seed).mean(0))
    model.predictor.check_status()  # range guard of the decoder's mode, once per search
    return torch.cat(out)


def classification_scores(logits: torch.Tensor, targets: torch.Tensor, *, topk: Optional[int] = None,
                          confusion: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """Scores of classification logits against integer targets through `vqvs_xent_score`, on the current stream.

    `logits` is float32 [B, K] with `targets` int64 [B] (a classifier), or [B, K, L] with targets [B, L] (an encoder predictor).
    Returns {"nll": float64 [B], the clip's SUMMED negative log-likelihood; "top1": int64 [B], positions whose target holds the
    first maximum; "topk": int64 [B], positions whose target ranks among the first `topk` (None when topk is None);
    "positions": L}.  `confusion`, an int64 [K, K] tensor on the logits' device, gets [target, argmax] += 1 per position: zero it
    once and pass it to every call of a pass.  Sums are deterministic float64 and counts exact, so a clip scores the same
    whatever batch it is in.  Targets outside 0..K-1 raise IndexError before anything is launched."""
    if not (torch.is_tensor(logits) and torch.is_tensor(targets)):
        raise ValueError("logits and targets must be tensors")
    if logits.dim() not in (2, 3):
        raise ValueError(f"expected logits of shape [B, K] or [B, K, L], got {tuple(logits.shape)}")
    B, K = int(logits.shape[0]), int(logits.shape[1])
    L = int(logits.shape[2]) if logits.dim() == 3 else 1
    want = (B, L) if logits.dim() == 3 else (B,)
    if tuple(targets.shape) != want:
        raise ValueError(f"expected targets of shape {want} for logits of shape {tuple(logits.shape)}, got {tuple(targets.shape)}")
    if logits.dtype != torch.float32:
        raise ValueError(f"logits must be float32, got {logits.dtype}")
    if targets.dtype != torch.int64:
        raise ValueError(f"targets must be int64, got {targets.dtype}")
    if not (1 <= B <= 65535 and 1 <= K <= 8192 and 1 <= L <= 2 ** 24):
        raise ValueError(f"B={B}, K={K}, L={L} outside the limits 1..65535, 1..8192, 1..2^24")
    if topk is not None and not 1 <= int(topk) <= K:
        raise ValueError(f"topk={topk} outside 1..{K}")
    if confusion is not None:
        if not torch.is_tensor(confusion) or confusion.dtype != torch.int64 or tuple(confusion.shape) != (K, K) or not confusion.is_contiguous():
            raise ValueError(f"confusion must be a contiguous int64 tensor of shape {(K, K)}")
    _native.require_cuda(logits, targets, confusion)
    if targets.device != logits.device or (confusion is not None and confusion.device != logits.device):
        raise ValueError("logits, targets and confusion must be on one device")
    logits, targets = logits.detach().contiguous(), targets.detach().contiguous()
    _native.check_index_range(targets, K, "classification_scores: targets")
    nll = torch.empty(B, device=logits.device, dtype=torch.float64)
    top1 = torch.empty(B, device=logits.device, dtype=torch.int64)
    topk_out = torch.empty(B, device=logits.device, dtype=torch.int64) if topk is not None else None
    with torch.cuda.device(logits.device):
        _native.check(_native.lib().vqvs_xent_score(logits.data_ptr(), targets.data_ptr(), nll.data_ptr(), top1.data_ptr(),
                                                    _native._ptr(topk_out), int(topk or 0), _native._ptr(confusion), B, K, L,
                                                    _native._stream_ptr()))
    return {"nll": nll, "top1": top1, "topk": topk_out, "positions": L}
