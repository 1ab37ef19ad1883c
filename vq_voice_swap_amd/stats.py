"""
Sample-quality statistics: the classifier-feature moments, class score and Frechet distance of the reference's
stat_generate.py / stat_compare.py.

`FeatureStats` accumulates the first and second moments of classifier features on the device, batch by batch
(`vqvs_feature_moments`: f64 MFMA, deterministic), about a shift K -- the first feature row it sees -- so that f64
sums stay exact enough when the features share a large common offset.  States with different shifts combine by
Chan's pairwise formula over central moments (`merge`, `all_reduce`), and `save` writes the reference's npz keys
(mean, cov, probs, class_score), so either side's stat_compare.py reads the other's files.

`class_score` and `frechet_distance` are host float64 restatements of stat_generate.py:47-52 and
stat_compare.py:20-53; the matrix square root comes from symmetric eigendecompositions (numpy only, no scipy).
"""

from __future__ import annotations

import numpy as np
import torch

from . import _native
from .audio import decode_to_linear


def class_score(probs) -> float:
    """exp(mean_i KL(p_i || mean_j p_j)) in float64 (stat_generate.py:47-52, the Inception score's formula); 0 log 0 = 0."""
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] < 1:
        raise ValueError(f"expected probabilities of shape [N, num_labels], got {p.shape}")
    pbar = p.mean(axis=0, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.where(p > 0, p * (np.log(p) - np.log(pbar)), 0.0)
    return float(np.exp(np.mean(np.sum(kl, axis=1))))


def _rounding_floor(w: np.ndarray) -> float:
    """Eigenvalues below this are rounding noise of a symmetric eigensolver (n * eps * the largest magnitude)."""
    return w.size * np.finfo(np.float64).eps * float(np.abs(w).max(initial=0.0))


def _psd_sqrt(s: np.ndarray) -> np.ndarray:
    w, v = np.linalg.eigh(s)
    w = np.where(w > _rounding_floor(w), w, 0.0)  # (the square root would lift noise of 1e-16 to 1e-8)
    return (v * np.sqrt(w)) @ v.T


def _trace_sqrt_product(s1: np.ndarray, s2: np.ndarray):
    """tr sqrt(s1 s2) from the eigenvalues of s1^1/2 s2 s1^1/2 (similar to s1 s2, symmetric PSD), or None when the product is not
    PSD beyond rounding (what makes scipy's sqrtm return non-finite values in the reference)."""
    r = _psd_sqrt(s1)
    m = r @ s2 @ r
    ev = np.linalg.eigvalsh((m + m.T) * 0.5)
    if not np.isfinite(ev).all():
        return None
    if ev.min(initial=0.0) < -1e-10 * float(np.abs(ev).max(initial=0.0)):
        return None
    return float(np.sqrt(np.where(ev > _rounding_floor(ev), ev, 0.0)).sum())


def frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """|mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr sqrt(sigma1 sigma2) in float64 (stat_compare.py:20-53).  A product that
    is not positive semi-definite beyond rounding is retried with eps * I added to both covariances, as the reference does."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    tr = _trace_sqrt_product(sigma1, sigma2)
    if tr is None:
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        tr = _trace_sqrt_product(sigma1 + offset, sigma2 + offset)
        if tr is None:
            raise ValueError("the covariance product is not positive semi-definite, even with eps * I added")
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2.0 * tr)


def wav_roundtrip(x: torch.Tensor, encoding: str) -> torch.Tensor:
    """What a sample becomes when ChunkWriter writes it and ChunkReader reads it back (audio.py): clip to [-1, 1], decode to
    linear, truncate x * 32767 to int16, divide by 32768.  In-line statistics of a sampling run see what the file route sees."""
    x = x.detach().to(torch.float32).clamp(-1.0, 1.0)
    if encoding == "ulaw":
        mu = 255.0
        x = torch.sign(x) * (1 / mu) * (torch.pow(torch.tensor(1 + mu, dtype=torch.float32, device=x.device), x.abs()) - 1)
    else:
        decode_to_linear(np.zeros(0, dtype=np.float32), encoding)  # (raises for an unknown encoding, as ChunkWriter does)
    return (x * (2 ** 15 - 1)).to(torch.int16).to(torch.float32) / 2 ** 15


class FeatureStats:
    """Running mean / covariance (and softmax probabilities) of classifier features.

    State: n rows, a shift K (float32-representable, so the device kernel takes it as f32), s1 = sum (f - K) and
    s2 = sum (f - K)(f - K)^T in float64 on `device`; probabilities are kept on the host."""

    def __init__(self, dim: int, device=None):
        if not 1 <= int(dim) <= 8192:
            raise ValueError(f"feature width {dim} outside 1..8192")
        self.dim = int(dim)
        device = torch.device("cuda") if device is None else torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.n = 0
        self._shift = torch.zeros(self.dim, dtype=torch.float32, device=self.device)
        self._s1 = torch.zeros(self.dim, dtype=torch.float64, device=self.device)
        self._s2 = torch.zeros(self.dim, self.dim, dtype=torch.float64, device=self.device)
        self._probs = []

    # ---- accumulation
    def update(self, feat: torch.Tensor) -> "FeatureStats":
        """Add a device batch of features [B, dim] (`vqvs_feature_moments`)."""
        _native.require_cuda(feat)
        if feat.dim() != 2 or feat.shape[1] != self.dim:
            raise ValueError(f"expected features of shape [B, {self.dim}], got {tuple(feat.shape)}")
        if feat.device != self.device:
            raise ValueError(f"features on {feat.device}, statistics on {self.device}")
        B = int(feat.shape[0])
        if B == 0:
            return self
        feat = feat.detach().to(torch.float32).contiguous()
        if self.n == 0:
            self._shift.copy_(feat[0])
        with torch.cuda.device(self.device):
            _native.check(_native.lib().vqvs_feature_moments(feat.data_ptr(), B, self.dim, self._shift.data_ptr(), self._s1.data_ptr(),
                                                            self._s2.data_ptr(), _native._stream_ptr()))
        self.n += B
        return self

    def add_probs(self, probs) -> "FeatureStats":
        p = probs.detach().cpu().numpy() if isinstance(probs, torch.Tensor) else np.asarray(probs)
        if p.ndim != 2:
            raise ValueError(f"expected probabilities of shape [B, num_labels], got {p.shape}")
        self._probs.append(p.astype(np.float32, copy=False))
        return self

    @property
    def probs(self) -> np.ndarray:
        if not self._probs:
            return np.zeros((0, 0), dtype=np.float32)
        return np.concatenate(self._probs, axis=0)

    # ---- moments (host float64)
    def moments(self):
        """(n, K, s1, s2) as float64 numpy."""
        return (self.n, self._shift.cpu().numpy().astype(np.float64), self._s1.cpu().numpy(), self._s2.cpu().numpy())

    def _central(self):
        n, k, s1, s2 = self.moments()
        return n, k + s1 / n, s2 - np.outer(s1, s1) / n

    def mean(self) -> np.ndarray:
        if self.n < 1:
            raise ValueError("no features accumulated")
        n, k, s1, _ = self.moments()
        return k + s1 / n

    def cov(self) -> np.ndarray:
        """Sample covariance, ddof = 1 (np.cov(features, rowvar=False))."""
        if self.n < 2:
            raise ValueError(f"a covariance needs at least two rows, have {self.n}")
        n, _, s1, s2 = self.moments()
        return (s2 - np.outer(s1, s1) / n) / (n - 1)

    def class_score(self) -> float:
        return class_score(self.probs)

    # ---- combination
    def _set_central(self, n: int, mean: np.ndarray, m2: np.ndarray) -> None:
        """Store central moments (mean, m2 = sum (f - mean)(f - mean)^T) about the float32 rounding of the mean."""
        k = mean.astype(np.float32).astype(np.float64)
        d = mean - k
        s1 = n * d
        s2 = m2 + n * np.outer(d, d)
        self.n = int(n)
        self._shift.copy_(torch.from_numpy(k.astype(np.float32)))
        self._s1.copy_(torch.from_numpy(s1))
        self._s2.copy_(torch.from_numpy(s2))

    @classmethod
    def from_moments(cls, n: int, shift, s1, s2, probs=None, device="cpu") -> "FeatureStats":
        """A state from host moments about any shift: n rows, s1 = sum (f - shift), s2 = sum (f - shift)(f - shift)^T."""
        shift, s1, s2 = (np.asarray(a, dtype=np.float64) for a in (shift, s1, s2))
        st = cls(shift.shape[0], device=device)
        if s1.shape != shift.shape or s2.shape != shift.shape * 2:
            raise ValueError(f"moment shapes {s1.shape} / {s2.shape} do not match the shift {shift.shape}")
        if n > 0:
            st._set_central(int(n), shift + s1 / n, s2 - np.outer(s1, s1) / n)
        if probs is not None:
            st.add_probs(probs)
        return st

    def merge(self, other: "FeatureStats") -> "FeatureStats":
        """Add another state's rows (Chan et al.'s pairwise update of central moments: the two states may carry different
        shifts); probabilities are appended after this state's own."""
        if other.dim != self.dim:
            raise ValueError(f"feature widths differ: {self.dim} and {other.dim}")
        if other.n > 0:
            nb, mb, m2b = other._central()
            if self.n == 0:
                self._set_central(nb, mb, m2b)
            else:
                na, ma, m2a = self._central()
                n = na + nb
                delta = mb - ma
                self._set_central(n, ma + delta * (nb / n), m2a + m2b + np.outer(delta, delta) * (na * nb / n))
        self._probs.extend(p.copy() for p in other._probs)
        return self

    def all_reduce(self, group=None) -> "FeatureStats":
        """Merge the states of every rank of `group` (any torch.distributed backend; gloo gathers host tensors, as
        sampler.gather_clips).  Every rank ends with the same state: the ranks' states merged in rank order."""
        import torch.distributed as dist

        world = dist.get_world_size(group)
        F = self.dim
        flat = torch.cat([torch.tensor([float(self.n)], dtype=torch.float64, device=self.device), self._shift.to(torch.float64),
                          self._s1, self._s2.reshape(-1)])
        if dist.get_backend(group) == "gloo":
            flat = flat.cpu()
        elif self.device.type != "cuda":
            flat = flat.to(torch.device("cuda", torch.cuda.current_device()))
        bufs = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(bufs, flat, group=group)
        probs = [None] * world
        dist.all_gather_object(probs, self.probs, group=group)
        self.n = 0
        self._s1.zero_()
        self._s2.zero_()
        self._probs = []
        for buf, p in zip(bufs, probs):
            buf = buf.cpu().numpy()
            part = FeatureStats(F, device="cpu")
            part.n = int(buf[0])
            part._shift.copy_(torch.from_numpy(buf[1:1 + F].astype(np.float32)))
            part._s1.copy_(torch.from_numpy(buf[1 + F:1 + 2 * F]))
            part._s2.copy_(torch.from_numpy(buf[1 + 2 * F:].reshape(F, F)))
            if p is not None and p.size:
                part._probs.append(p)
            self.merge(part)
        return self

    def save(self, path: str) -> None:
        """npz with the reference's keys (stat_generate.py:54): mean, cov, probs, class_score."""
        probs = self.probs
        score = class_score(probs) if probs.size else float("nan")
        np.savez(path, mean=self.mean(), cov=self.cov(), probs=probs, class_score=np.float64(score))
