"""
Whole recordings: ONE long diffusion state, predicted through overlapping windows of the trained length ("Long-form
conversion").  The reference converts a single clip and has nothing of the kind.

Every reverse step cuts the long x_t into windows of `window` samples, one every `hop`, runs the predictor on the batch of
windows, and `vqvs_ddpm_step_windows` does the rest in one pass: each window's `constrain` with its own mean, the predictions of
the two windows of an overlap cross-faded, ONE noise draw per absolute sample position, the long state and the next forward's
window batch written together.  Means are blended and the noise is shared, so the windows agree on their common samples at every
step and the step has the variance a single clip's has.

`Diffusion.ddpm_sample_windows`, `VQVAE.encode_long` and `VQVAE.decode_long` are the functions below; `Diffusion.ddim_sample_windows`
is the same walk with the DDIM step `vqvs_ddim_step_windows`, `Diffusion.dpmpp_sample_windows` with the
DPM-Solver++(2M) step `vqvs_dpmpp_step_windows` (section 3.12).

Pauses (section 3.21): `pack_source=` / `pack_keep=` / `pack_start_step=` are the keep region of a pack, `skip=` leaves the windows that a
mask covers whole out of the forwards, and `decode_long(_batch)(keep_pauses=, skip_kept=)` find the pauses (pauses.py) and do both.

A corpus is converted in PACKS (section 3.17): with `counts=` the three loops run several recordings' rows laid end to end, their
windows in one batch that fills the forwards, and the step is the `..._packed` entry point, which keeps the recordings apart.
`VQVAE.encode_long_batch` / `decode_long_batch` are below as well; recording r of a pack is, bit for bit, what `decode_long` returns
for it alone at clip_offset + r.

So on the host ONE recording is the pack of one -- `pack_layout([n], W, H)` is offsets [0] and `plan_windows`' length -- and everything
here is written once, over (offsets, counts): the layout `_Windows`, the gather that starts a run, the body of the three loops
(`_window_run`), `encode_long` as `encode_long_batch` of one, `decode_long` and `decode_long_batch` over `_decode`.  The two forms
differ in what the kernels are told alone (`_entry`): n and the `..._windows` entry points without `counts=`, the table and the
`..._windows_packed` ones with it.
"""

from __future__ import annotations

import functools
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _native

MAX_WINDOWS = 65535  # the limits of vqvs_ddpm_step_windows (include/vqvs.h)


def plan_windows(num_samples: int, window: int, hop: int) -> Tuple[int, int]:
    """(n, padded_len): the number of windows of `window` samples, one every `hop`, that cover `num_samples`, and the length
    (n - 1) * hop + window of the signal they span.  The overlap window - hop lies in 0..hop: at most two windows cover a sample."""
    num_samples, window, hop = int(num_samples), int(window), int(hop)
    if num_samples < 1:
        raise ValueError(f"num_samples={num_samples} must be at least 1")
    if window < 4 or hop < 4 or window % 4 or hop % 4:
        raise ValueError(f"window={window} and hop={hop} must be positive multiples of 4")
    overlap = window - hop
    if overlap < 0 or overlap > hop:
        raise ValueError(f"overlap {overlap} (window {window} - hop {hop}) must lie in 0..hop: at most two windows may cover a sample")
    n = 1 if num_samples <= window else -(-(num_samples - overlap) // hop)
    padded_len = (n - 1) * hop + window
    if n > MAX_WINDOWS or padded_len >= 2 ** 31:
        raise ValueError(f"{num_samples} samples need {n} windows spanning {padded_len} samples: more than {MAX_WINDOWS} windows or 2^31 samples")
    return n, padded_len


def pack_layout(counts: Sequence[int], window: int, hop: int) -> Tuple[List[int], List[int], int]:
    """(first, offsets, total) of a pack of recordings of `counts` windows each, their long rows laid end to end (include/vqvs.h,
    "Packed window steps"): first [R + 1] the prefix sums of the counts, offsets[r] = first[r] * hop + r * (window - hop) the first
    sample of recording r, total = N * hop + R * (window - hop).  Refused: no recording, a count below 1, more than MAX_WINDOWS
    windows or recordings, 2^31 samples or more."""
    counts = [int(c) for c in counts]
    plan_windows(1, window, hop)  # (the rules on window and hop)
    if not counts or min(counts) < 1:
        raise ValueError(f"counts={counts} must hold at least one recording, each of at least 1 window")
    first = [0]
    for c in counts:
        first.append(first[-1] + c)
    overlap = int(window) - int(hop)
    offsets = [first[r] * int(hop) + r * overlap for r in range(len(counts))]
    total = first[-1] * int(hop) + len(counts) * overlap
    if first[-1] > MAX_WINDOWS or total >= 2 ** 31:
        raise ValueError(f"a pack of {len(counts)} recordings holds {first[-1]} windows and {total} samples: more than {MAX_WINDOWS} windows or 2^31 samples")
    return first, offsets, total


def plan_pack(num_samples_list: Sequence[int], window: int, hop: int) -> Tuple[List[int], List[int], int]:
    """(counts, offsets, total) of the pack of recordings of `num_samples_list` samples: each recording's `plan_windows` count, the
    first sample of its padded row in the concatenation, and the concatenation's length (`pack_layout`)."""
    counts = [plan_windows(n, window, hop)[0] for n in num_samples_list]
    _, offsets, total = pack_layout(counts, window, hop)
    return counts, offsets, total


def pack_table(counts: Sequence[int], window: int, hop: int, device) -> Tuple[torch.Tensor, int, int, List[int], int]:
    """(d_first, R, N, offsets, total) of a pack (`pack_layout`): the prefix sums `first` uploaded as the int32 [R + 1] table that every
    packed entry point reads, the numbers of recordings and of windows, each recording's first sample and the samples in all."""
    first, offsets, total = pack_layout(counts, window, hop)
    return torch.tensor(first, dtype=torch.int32, device=device), len(first) - 1, first[-1], offsets, total


def pack_rows(t: torch.Tensor, offsets: Sequence[int], counts: Sequence[int], window: int, hop: int):
    """Each recording's padded row t[..., o : o + (c - 1) * hop + window] of a tensor in pack layout, as views."""
    for o, c in zip(offsets, counts):
        yield t[..., o:o + (c - 1) * hop + window]


def _cat(tensors: List[torch.Tensor], dim: int = 0) -> torch.Tensor:
    """`torch.cat`, without its copy where there is one tensor (one recording)."""
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, dim=dim)


def gather_windows(x: torch.Tensor, window: int, hop: int) -> torch.Tensor:
    """[1,1,Np] -> the contiguous window batch [n,1,window] (a copy; the step kernel writes the later ones itself)."""
    return x.reshape(-1).unfold(0, window, hop).unsqueeze(1).contiguous()


def _entry(name: str, geom):
    """The C entry point of a window kernel and its geometry arguments: `geom` is the window count n of one recording, or the `_Windows`
    of a pack -- the packed form takes (d_first, R) where the single one takes n."""
    if isinstance(geom, int):
        return getattr(_native.lib(), name), (geom,)
    return getattr(_native.lib(), name + "_packed"), (geom.first.data_ptr(), geom.R)


def keep_windows_(x: torch.Tensor, windows: Optional[torch.Tensor], source: torch.Tensor, keep: Optional[torch.Tensor], alpha: torch.Tensor, *,
                  geom, window: int, hop: int, seed: int, clip_offset: int, index: int) -> None:
    """`vqvs_keep_region_windows` IN PLACE on the long state x [Np] and (unless None) on the window batch [n,1,window] gathered from
    it: the kept samples (keep None: all) are put back on the source's forward process at alpha[0].  For a pack (`_entry`) the
    packed form: the same on every recording's own slices, recording r keyed clip_offset + r, in one launch."""
    fn, geom = _entry("vqvs_keep_region_windows", geom)
    _native.check(fn(x.data_ptr(), _native._ptr(windows), source.data_ptr(), _native._ptr(keep), None, alpha.data_ptr(), *geom, window, hop, 1.0,
                     int(seed), int(clip_offset), int(index), _native._stream_ptr()))


def start_windows(x_T_long: torch.Tensor, source, keep, alpha, *, start_step: int, geom, offsets: Sequence[int], counts: Sequence[int],
                  window: int, hop: int, seed: int, clip_offset: int):
    """(long state, window batch) a windowed run starts from: x_T as it is, x_T with the kept samples replaced, or -- `start_step` > 0
    -- the source noised to that step's alpha_bar (Diffusion._keep_start, on the long state).  The batch is gathered recording by
    recording: no window spans two."""
    x = x_T_long.detach().to(torch.float32).contiguous()
    if source is not None and (start_step > 0 or keep is not None):
        x = torch.empty_like(x) if start_step > 0 else x.clone()
        with torch.cuda.device(x.device):
            keep_windows_(x, None, source, None if start_step > 0 else keep, alpha, geom=geom, window=window, hop=hop, seed=seed,
                          clip_offset=clip_offset, index=start_step)
    return x, _cat([gather_windows(row, window, hop) for row in pack_rows(x, offsets, counts, window, hop)])


def pad_source_keep(source: Optional[torch.Tensor], keep: Optional[torch.Tensor], num_samples: int, padded_len: int):
    """`decode_long`'s `source` / `keep` [1,1,num_samples] at the length of the long state: the source zero-padded as `encode_long`
    pads the encoder's input, the mask padded with zeros (the padding is cut off the result and never kept)."""
    for name, t in (("source", source), ("keep", keep)):
        if t is not None and tuple(t.shape) != (1, 1, num_samples):
            raise ValueError(f"{name} must be [1, 1, {num_samples}], got {tuple(t.shape)}")
    pad = (0, padded_len - num_samples)
    if source is not None:
        source = torch.nn.functional.pad(source, pad)
    if keep is not None:
        if keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"keep must be a bool or uint8 tensor, got {keep.dtype}")
        keep = torch.nn.functional.pad(keep.to(torch.uint8), pad)
    return source, keep


def _ddpm_fill(rule, xw, e, tables, i, b0, cond_fn, eps, grad, st) -> None:
    """The DDPM rule on one slice of windows: the prediction `e`, or -- guided -- the two half-steps of `Diffusion._step` around
    cond_fn, written straight into the slice's rows of `eps`."""
    m, window = xw.shape[0], xw.shape[-1]
    e = e.detach().to(torch.float32).contiguous()
    if cond_fn is None:
        eps[b0:b0 + m].copy_(e)
        return
    L = _native.lib()
    a_t, a_prev = tables[1][i, :m], tables[2][i, :m]
    mean = torch.empty_like(xw)
    _native.check(L.vqvs_ddpm_mean(xw.data_ptr(), e.data_ptr(), a_t.data_ptr(), a_prev.data_ptr(), mean.data_ptr(), m, window, st))
    g = cond_fn(mean, tables[3][i, :m], first=b0).detach().to(torch.float32).contiguous()
    _native.check(L.vqvs_ddpm_guided_eps(xw.data_ptr(), mean.data_ptr(), g.data_ptr(), a_t.data_ptr(), a_prev.data_ptr(),
                                         eps[b0:b0 + m].data_ptr(), m, window, rule.flags, st))


def _ddim_fill(rule, xw, e, tables, i, b0, cond_fn, eps, grad, st) -> None:
    """The DDIM rule on one slice of windows: the prediction into `eps` and cond_fn's gradient AT the windows the predictor saw
    into `grad`, which the step kernel applies per window."""
    m = xw.shape[0]
    eps[b0:b0 + m].copy_(e.detach())
    if cond_fn is not None:
        g = cond_fn(xw, tables[0][i, :m], first=b0)
        _native.require_cuda(g)
        if tuple(g.shape) != tuple(xw.shape):
            raise ValueError(f"cond_fn returned shape {tuple(g.shape)} for windows of shape {tuple(xw.shape)}")
        grad[b0:b0 + m].copy_(g.detach())


def _ddpm_step_windows(rule, x, eps, grad, nz, a_t, a_to, x_to, next_windows, n, window, hop, noise_scale, seed, clip_offset, step_index, st) -> None:
    fn, geom = _entry("vqvs_ddpm_step_windows", n)
    _native.check(fn(x.data_ptr(), eps.data_ptr(), _native._ptr(nz), a_t.data_ptr(), a_to.data_ptr(), x_to.data_ptr(), next_windows.data_ptr(),
                     *geom, window, hop, rule.flags, noise_scale, int(seed), int(clip_offset), step_index, st))


def _ddim_step_windows(rule, x, eps, grad, nz, a_t, a_to, x_to, next_windows, n, window, hop, noise_scale, seed, clip_offset, step_index, st) -> None:
    fn, geom = _entry("vqvs_ddim_step_windows", n)
    _native.check(fn(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(nz), a_t.data_ptr(), a_to.data_ptr(), x_to.data_ptr(),
                     next_windows.data_ptr(), *geom, window, hop, rule.flags, float(rule.eta), noise_scale, int(seed), int(clip_offset),
                     step_index, st))


def dpmpp_step_windows_(x, eps, grad, x0_prev, a_from, a_t, a_to, x_to, x0_out, next_windows, n, window, hop, flags, st) -> None:
    """`vqvs_dpmpp_step_windows` on the long state x [Np] and the window batches eps / grad [n,1,window]: x_to and x0_out [Np] and the
    next forward's windows are written; x0_prev / a_from None: no history.  (n the layout of a pack: the packed form, `_entry`.)"""
    fn, geom = _entry("vqvs_dpmpp_step_windows", n)
    _native.check(fn(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(x0_prev), _native._ptr(a_from), a_t.data_ptr(), a_to.data_ptr(),
                     x_to.data_ptr(), x0_out.data_ptr(), next_windows.data_ptr(), *geom, window, hop, flags, st))


def _dpmpp_step_windows(rule, x, eps, grad, nz, a_t, a_to, x_to, next_windows, n, window, hop, noise_scale, seed, clip_offset, step_index, st) -> None:
    """The 2M rule's window step.  The history is the rule's: the blended x0 of the long row that the step before wrote, and that step's
    alpha_bar (`a_t` is the table row of a slice, one value per window, all equal: the kernel reads the first)."""
    x0 = torch.empty_like(x)
    dpmpp_step_windows_(x, eps, grad, rule.x0_prev, rule.a_from, a_t, a_to, x_to, x0, next_windows, n, window, hop, rule.flags, st)
    rule.x0_prev, rule.a_from = x0, a_t


class _Windows:
    """The state layout of the window loops for `Diffusion._sample`: the long row [Np], with its window batch [n,1,window] kept
    beside it.  The predictor and cond_fn see slices of at most `window_batch` windows, with `first=`; `fill` and `step` are the
    rule's window forms above.  `skip` (bool [n], checked by `_check_skip`) names windows that are not predicted: the slices then
    run over the ACTIVE windows, gathered, with `first=idx[0], rows=idx`, and the skipped rows of eps and grad stay zero.

    `counts` makes it a pack of recordings of that many windows each (`pack_layout`): the long rows end to end in one [total] state,
    the windows of all of them in one batch, so the predictor's slices run across recordings.  One recording is the pack of one, rows
    (0, n) of the same walk; only what the kernels are told differs (`geom`): n and the single entry points, or the table `first` and
    the packed ones, which key recording r by clip_offset + r and blend nothing across recordings."""

    def __init__(self, rule, predictor: Callable, cond_fn: Optional[Callable], window: int, hop: int, window_batch: int, fill, step,
                 skip: Optional[torch.Tensor] = None, counts: Optional[Sequence[int]] = None):
        self.rule, self.predictor, self.cond_fn, self.fill, self.step_windows = rule, predictor, cond_fn, fill, step
        self.window, self.hop, self.window_batch = window, hop, window_batch
        self.skip, self.active, self.pack = skip, None, counts

    def plan_skip(self, device) -> None:
        """The slices of active windows as (first index, index tensor [m]); the tensors stay the same objects for the whole run (a
        callee may key a cache by them).  None when no window is skipped."""
        if self.skip is None:
            return
        if self.skip.numel() != self.n:
            raise ValueError(f"skip must hold one entry per window ({self.n}), got {self.skip.numel()}")
        idx = (~self.skip.to(device)).nonzero().reshape(-1)  # (one synchronisation per run)
        if idx.numel() < self.n:
            firsts = idx[::self.mb].tolist()
            self.active = [(firsts[k], idx[a0:a0 + self.mb].contiguous()) for k, a0 in enumerate(range(0, idx.numel(), self.mb))]

    def rows(self, x_T_long) -> int:
        """The input checks and the geometry; the tables hold one row per window of a slice."""
        if x_T_long.dim() != 3 or x_T_long.shape[0] != 1 or x_T_long.shape[1] != 1:
            raise ValueError(f"x_T_long must be [1, 1, Np], got {tuple(x_T_long.shape)}")
        got, W, H = x_T_long.shape[2], self.window, self.hop
        if self.pack is None:
            self.n, self.Np = plan_windows(got, W, H)
            self.counts, self.offsets, self.geom = [self.n], [0], self.n  # (geom: what the entry points are told, `_entry`)
            laid = f"{self.n} windows of {W} every {H} span {self.Np} (see plan_windows)"
        else:
            self.first, self.R, self.n, self.offsets, self.Np = pack_table(self.pack, W, H, x_T_long.device)
            self.counts, self.geom = list(self.pack), self
            laid = f"recordings of {self.counts} windows of {W} every {H} are {self.Np} laid end to end (see plan_pack)"
        if got != self.Np:
            raise ValueError(f"x_T_long has {got} samples: {laid}")
        if self.window_batch < 1:
            raise ValueError(f"window_batch={self.window_batch} must be at least 1")
        self.mb = min(self.n, int(self.window_batch))
        self.plan_skip(x_T_long.device)
        return self.mb

    def start(self, x_T_long, source, keep, alpha, **kw):
        x, self.windows = self.gather(x_T_long, source, keep, alpha, **kw)
        fresh = torch.empty_like if self.active is None else torch.zeros_like  # (rows of skipped windows: zero, filled once)
        self.eps = fresh(self.windows)
        self.grad = fresh(self.windows) if self.cond_fn is not None and self.rule.name != "ddpm" else None
        return x

    def gather(self, x_T_long, source, keep, alpha, **kw):
        return start_windows(x_T_long, source, keep, alpha, geom=self.geom, offsets=self.offsets, counts=self.counts, window=self.window,
                             hop=self.hop, **kw)

    def predict(self, x, tables, i) -> None:
        self.st = _native._stream_ptr()  # (of this step: the slices' kernels and the step kernel)
        if self.active is not None:
            return self.predict_active(tables, i)
        for b0 in range(0, self.n, self.mb):
            m = min(self.mb, self.n - b0)
            xw = self.windows[b0:b0 + m]
            e = self.predictor(xw, tables[0][i, :m], first=b0)
            _native.require_cuda(e)
            if tuple(e.shape) != tuple(xw.shape):
                raise ValueError(f"the predictor returned shape {tuple(e.shape)} for windows of shape {tuple(xw.shape)}")
            self.fill(self.rule, xw, e, tables, i, b0, self.cond_fn, self.eps, self.grad, self.st)

    def predict_active(self, tables, i) -> None:
        """`predict` under a skip list: each slice of active windows is gathered, predicted with `first=idx[0], rows=idx`, filled as a
        batch of its own (the rule's `fill` at row 0 of [m,1,window] buffers, cond_fn bound to the slice), and its eps and grad rows
        scattered back."""
        for first, idx in self.active:
            m = idx.numel()
            xw = self.windows.index_select(0, idx)
            e = self.predictor(xw, tables[0][i, :m], first=first, rows=idx)
            _native.require_cuda(e)
            if tuple(e.shape) != tuple(xw.shape):
                raise ValueError(f"the predictor returned shape {tuple(e.shape)} for windows of shape {tuple(xw.shape)}")
            cond = None
            if self.cond_fn is not None:
                def cond(x_, ts_, first=0, at=first, idx=idx):  # (`first` is the row in the slice's own buffers: 0)
                    return self.cond_fn(x_, ts_, first=at, rows=idx)
            eps, grad = torch.empty_like(xw), None if self.grad is None else torch.empty_like(xw)
            self.fill(self.rule, xw, e, tables, i, 0, cond, eps, grad, self.st)
            self.eps.index_copy_(0, idx, eps)
            if grad is not None:
                self.grad.index_copy_(0, idx, grad)

    def step(self, x, _, nz, tables, i, *, noise_scale, seed, clip_offset):
        if nz is not None:
            _native.require_cuda(nz)
            nz = nz.detach().to(torch.float32).contiguous()
            if nz.numel() != self.Np:
                raise ValueError(f"noise of step {i} has {nz.numel()} values: expected [1, 1, {self.Np}]")
        x_to, next_windows = torch.empty_like(x), torch.empty_like(self.windows)
        self.step_windows(self.rule, x, self.eps, self.grad, nz, tables[1][i], tables[2][i], x_to, next_windows, self.geom, self.window, self.hop,
                          noise_scale, seed, clip_offset, i, self.st)
        self.windows = next_windows
        return x_to

    def keep(self, x, source, keep, alpha, **kw) -> None:
        keep_windows_(x, self.windows, source, keep, alpha, geom=self.geom, window=self.window, hop=self.hop, **kw)


def _check_skip(skip, keep, counts, window: int, hop: int):
    """The `skip=` keyword of the window loops as a bool [n] tensor.  A window may be skipped only when the keep mask covers it
    whole -- then every sample it covers is overwritten after every step, and its forward cannot reach the result.  One reduction
    over the mask's windows, once per run, on whatever device the mask is on."""
    if skip is None:
        return None
    if not torch.is_tensor(skip) or skip.dtype not in (torch.bool, torch.uint8) or skip.dim() != 1:
        raise ValueError("skip must be a bool or uint8 tensor [n]: the windows not to predict")
    if keep is None:
        raise ValueError("skip= needs a keep mask: only a window whose every sample is kept may be skipped")
    if keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"keep must be a bool or uint8 tensor, got {keep.dtype}")
    flat = keep.detach().reshape(-1)
    counts = [plan_windows(flat.numel(), window, hop)[0]] if counts is None else list(counts)
    first, offsets, total = pack_layout(counts, window, hop)
    if flat.numel() != total or skip.numel() != first[-1]:
        raise ValueError(f"skip of {skip.numel()} windows and a keep mask of {flat.numel()} samples do not match {first[-1]} windows of {window} "
                         f"every {hop} spanning {total} samples")
    whole = torch.cat([row.unfold(0, window, hop).ne(0).all(dim=1) for row in pack_rows(flat, offsets, counts, window, hop)])
    skip = skip.detach().ne(0).to(whole.device)
    if bool((skip & ~whole).any()):
        raise ValueError("skip= names a window that the keep mask does not cover whole: its forward would be missed")
    return skip


def _window_run(diffusion, what: str, x_T_long, steps, counts, skip, one, pack, *layout, **run):
    """The body of the three `..._sample_windows` functions, as the `Diffusion._sample` call for its caller to make (it is made
    there because `_sample` addresses its warnings by stack depth, to the caller of the public function).  `layout` is `_Windows`'
    arguments, the rule first.  One recording takes one = (`source`, `keep`, `start_step`); with `counts` a pack takes them in pack
    layout as pack = (`pack_source`, `pack_keep`, `pack_start_step`); each refuses the other's.  `skip` is checked against the mask of
    either (`_check_skip`)."""
    if counts is None:
        if pack[0] is not None or pack[1] is not None or pack[2]:
            raise ValueError("pack_source, pack_keep and pack_start_step belong to a pack of recordings (counts=): one recording takes source, "
                             "keep and start_step")
        source, keep, start_step = one
    else:
        if one[0] is not None or one[1] is not None or one[2]:
            raise ValueError("source, keep and start_step are one recording's: a pack of recordings (counts=) takes pack_source, pack_keep and "
                             "pack_start_step, the same in pack layout [1,1,total]")
        source, keep, start_step = pack
    windows = _Windows(*layout, skip=_check_skip(skip, keep, counts, layout[3], layout[4]), counts=counts)
    return functools.partial(diffusion._sample, what, windows, x_T_long, steps, source=source, keep=keep, start_step=start_step, **run)


def ddpm_sample_windows(diffusion, x_T_long: torch.Tensor, predictor: Callable, steps: int, *, window: int, hop: int,
                        window_batch: int = 64, constrain: bool = False, sigma_large: bool = False, cond_fn: Optional[Callable] = None,
                        schedule: Optional[Callable] = None, noise=None, seed: Optional[int] = None, clip_offset: int = 0,
                        progress: bool = False, source: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                        start_step: int = 0, counts: Optional[Sequence[int]] = None, pack_source: Optional[torch.Tensor] = None,
                        pack_keep: Optional[torch.Tensor] = None, pack_start_step: int = 0,
                        skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`Diffusion.ddpm_sample` for one long state x_T_long [1,1,Np], Np = (n - 1) * hop + window (`plan_windows`): the same
    host-side tables of t and alpha_bar(t), the same step numbering, zero noise on the last step.

    `predictor(windows [m,1,window], ts [m], first=b0)` is called on slices of at most `window_batch` windows; `first` is the
    index of the slice's first window, for a callee that slices its conditioning.  `cond_fn(mean [m,1,window], ts_prev [m],
    first=b0)` guides each slice through `vqvs_ddpm_mean` / `vqvs_ddpm_guided_eps`, as in the single-clip step, before the
    windows' predictions meet in `vqvs_ddpm_step_windows`.  `noise` is a list or callable giving [1,1,Np] per step; None draws in the
    kernel from (seed, clip_offset, step): the draws of row `clip_offset` of a batch of clips of length Np.
    `source`, `keep` ([1,1,Np]) and `start_step` are `ddpm_sample`'s, applied by `vqvs_keep_region_windows` to the long state and to
    both window copies of an overlap sample.

    `counts` makes the run a PACK of recordings of that many windows each: x_T_long (and `noise` per step) is their rows end to end,
    [1,1,total] (`plan_pack`), recording r is keyed clip_offset + r, and the predictor's and cond_fn's slices run across recordings
    (`first` indexes the pack's window batch).  Recording r's slice of the result is what the run of that recording alone returns at
    clip_offset + r, bit for bit.  A pack takes `pack_source`, `pack_keep` ([1,1,total], the rows end to end) and `pack_start_step` in
    the place of `source`, `keep` and `start_step`, which raise ValueError with `counts`; they are applied by
    `vqvs_keep_region_windows_packed`, recording r at clip_offset + r.

    `skip` (bool or uint8 [n], with or without `counts`) names windows that are NOT predicted.  It is refused unless the keep mask
    covers every skipped window whole: such a window's samples are all overwritten after every step, so the result is the same bit
    for bit and only the forwards are saved.  The predictor and cond_fn are then called on gathered slices of the active windows as
    `predictor(windows [m,1,window], ts [m], first=idx[0], rows=idx)`, idx the int64 [m] indices of the slice's windows; without
    `skip` (or with nothing skipped) `first=` alone is passed, as ever."""
    from .diffusion import _Ddpm

    return _window_run(diffusion, "ddpm_sample_windows", x_T_long, steps, counts, skip, (source, keep, start_step), (pack_source, pack_keep, pack_start_step),
                       _Ddpm(sigma_large, constrain), predictor, cond_fn, window, hop, window_batch, _ddpm_fill, _ddpm_step_windows,
                       schedule=schedule, noise=noise, seed=seed, clip_offset=clip_offset, progress=progress)()


def ddim_sample_windows(diffusion, x_T_long: torch.Tensor, predictor: Callable, steps: int, *, window: int, hop: int,
                        window_batch: int = 64, eta: float = 0.0, constrain: bool = False, cond_fn: Optional[Callable] = None,
                        schedule: Optional[Callable] = None, noise=None, seed: Optional[int] = None, clip_offset: int = 0,
                        progress: bool = False, source: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                        start_step: int = 0, counts: Optional[Sequence[int]] = None, pack_source: Optional[torch.Tensor] = None,
                        pack_keep: Optional[torch.Tensor] = None, pack_start_step: int = 0,
                        skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`Diffusion.ddim_sample` for one long state x_T_long [1,1,Np]: `ddpm_sample_windows` with `vqvs_ddim_step_windows` as the step.
    `predictor` and `noise` are as there.  `cond_fn(x [m,1,window], ts [m], first=b0)` is evaluated on each slice of windows AT the
    windows the predictor saw and at their t; its gradients fill a [n, window] batch that the step kernel applies per window, before
    the windows' predictions are blended -- one kernel after the forwards, no half-steps.  `source`, `keep` and `start_step` are as
    there, the kept samples replaced at the alpha_bar stepped TO; `counts` (a pack of recordings), the `pack_...` keywords and `skip` are
    as there."""
    from .diffusion import _Ddim

    return _window_run(diffusion, "ddim_sample_windows", x_T_long, steps, counts, skip, (source, keep, start_step), (pack_source, pack_keep, pack_start_step),
                       _Ddim(eta, constrain), predictor, cond_fn, window, hop, window_batch, _ddim_fill, _ddim_step_windows,
                       schedule=schedule, noise=noise, seed=seed, clip_offset=clip_offset, progress=progress)()


def dpmpp_sample_windows(diffusion, x_T_long: torch.Tensor, predictor: Callable, steps: int, *, window: int, hop: int,
                         window_batch: int = 64, constrain: bool = False, cond_fn: Optional[Callable] = None,
                         schedule: Optional[Callable] = None, noise=None, seed: Optional[int] = None, clip_offset: int = 0,
                         progress: bool = False, source: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                         start_step: int = 0, counts: Optional[Sequence[int]] = None, pack_source: Optional[torch.Tensor] = None,
                         pack_keep: Optional[torch.Tensor] = None, pack_start_step: int = 0,
                         skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`Diffusion.dpmpp_sample` for one long state x_T_long [1,1,Np]: `ddim_sample_windows` at eta = 0 with `vqvs_dpmpp_step_windows` as
    the step.  `predictor` and `cond_fn` are as there (the gradient is taken at the windows the predictor saw and applied per window,
    before the blend); the history is the BLENDED x0 of the long row, one value per absolute position, kept by the rule.  `noise` is
    accepted and never asked for anything; `source`, `keep` and `start_step` are as there and leave the history alone; `counts` (a
    pack of recordings) is as there, the history the pack's rows end to end; the `pack_...` keywords and `skip` are as there (a kept
    position of the history never reaches a sample that is not kept)."""
    from .diffusion import _Dpmpp

    return _window_run(diffusion, "dpmpp_sample_windows", x_T_long, steps, counts, skip, (source, keep, start_step), (pack_source, pack_keep, pack_start_step),
                       _Dpmpp(constrain), predictor, cond_fn, window, hop, window_batch, _ddim_fill, _dpmpp_step_windows,
                       schedule=schedule, noise=noise, seed=seed, clip_offset=clip_offset, progress=progress)()


def encode_long(model, wave: torch.Tensor, window: int, hop: int, window_batch: int = 64) -> torch.Tensor:
    """[1,1,N] waveform -> codes [n, window / rate] of its n windows (`plan_windows`), the tail zero-padded: `encode_long_batch` of the
    one recording, without the counts."""
    if wave.dim() != 3 or wave.shape[0] != 1 or wave.shape[1] != 1:
        raise ValueError(f"wave must be [1, 1, N], got {tuple(wave.shape)}")
    return encode_long_batch(model, [wave], window, hop, window_batch)[0]


def encode_long_batch(model, waves: Sequence[torch.Tensor], window: int, hop: int, window_batch: int = 64) -> Tuple[torch.Tensor, List[int]]:
    """Several recordings [1,1,N_r] -> (codes [N, window / rate], counts), the windows of recording r -- zero-padded to its own
    `plan_windows` length -- at rows sum(counts[:r]) ... of the codes.  Windows are encoded in slices of `window_batch` that run across
    recordings; behind the version-2 (dB) MFCC front end, which floors at the maximum over the BATCH, one at a time, so that the codes
    depend neither on `window_batch` nor on the pack: they are `encode_long`'s of each recording."""
    if not len(waves):
        raise ValueError("waves must hold at least one recording")
    for w in waves:
        if w.dim() != 3 or w.shape[0] != 1 or w.shape[1] != 1:
            raise ValueError(f"every wave must be [1, 1, N], got {tuple(w.shape)}")
    check_rate(model, window, hop)
    counts, _, _ = plan_pack([w.shape[2] for w in waves], window, hop)
    windows = _cat([gather_windows(torch.nn.functional.pad(w, (0, (c - 1) * hop + window - w.shape[2])), window, hop)
                    for w, c in zip(waves, counts)])
    mb = 1 if getattr(model.encoder, "version", 1) == 2 else max(1, int(window_batch))
    return torch.cat([model.encode(windows[b0:b0 + mb]) for b0 in range(0, windows.shape[0], mb)]), counts


def check_rate(model, window: int, hop: int) -> None:
    rate = model.downsample_rate
    if window % rate or hop % rate:
        raise ValueError(f"window={window} and hop={hop} must be multiples of the model's downsample rate {rate}")


def _per_window(rows: torch.Tensor, n: int, counts: Optional[Sequence[int]], what: str) -> torch.Tensor:
    """The `labels` [k] or the explicit conditioning vectors [k,E] (speakers.py) of a window batch -> one row per window [n, ...]: one
    for every window, one per window, or -- with the `counts` of a pack -- one per recording."""
    if rows.shape[0] == 1:
        rows = rows.expand(n, *rows.shape[1:])
    elif counts is not None and rows.shape[0] == len(counts) != n:
        rows = rows.repeat_interleave(torch.tensor(list(counts), device=rows.device), dim=0)
    if rows.shape[0] != n:
        per = f", one per recording ({len(counts)})" if counts is not None else ""
        raise ValueError(f"{what}s must hold one {what}{per} or one per window ({n}), got {rows.shape[0]}")
    return rows.contiguous()


def _conditioned(model, cond_seq, labels, enc_pred, enc_pred_scale, guidance=None, vectors=None):
    """(predictor, cond_fn) of a window batch: each slice of windows (`first=`, or the gathered `rows=` of a run that skips windows)
    sees its own rows of the conditioning [n,C,T1], of `labels` [n]
    or `vectors` [n,E] (or neither) and -- with `enc_pred` -- guidance towards its own codes (VQVAE.decode).  `guidance` (label_scale, vq_scale) makes the
    predictor the guided one of `VQVAE.decode_uncond_guidance` (vq_vae.guided_predictor): labels are then NOT offset by the caller."""
    cond_fn = None
    if enc_pred is not None:
        targets = model.vq.encode(cond_seq)

        def cond_fn(x, ts, first, rows=None):
            return enc_pred.guidance_grad(x, ts, targets[first:first + x.shape[0]] if rows is None else targets[rows], enc_pred_scale)

        cond_fn.native_modules = (enc_pred,)

    if guidance is not None:
        from .vq_vae import guided_predictor

        return guided_predictor(model, cond_seq, labels, *guidance, vectors=vectors)[0], cond_fn

    def predictor(xs, ts, first, rows=None):
        sl = slice(first, first + xs.shape[0]) if rows is None else rows  # (rows: the windows of a gathered slice, `_Windows.predict_active`)
        return model.predictor(xs, ts, cond=cond_seq[sl], labels=None if labels is None else labels[sl],
                               vectors=None if vectors is None else vectors[sl])

    return predictor, cond_fn


def _pause_keep_and_skip(source, keep, counts, window, hop, keep_pauses, skip_kept, num_samples, stats):
    """(mask, skip list) of a pack's padded rows `source` [1,1,total]: the user's mask `keep` (uint8 or None) OR-ed, once, on the device,
    with the pause mask of the rows when `keep_pauses` holds the detector's settings; the windows the result covers whole when
    `skip_kept` (None when there are none).  `stats` (a dict or None) receives kept_samples (of the un-padded recordings), windows and
    skipped_windows."""
    from .pauses import pause_mask, windows_kept

    if keep_pauses is not None:
        _native.require_cuda(source)
        found = pause_mask(source, counts, window, hop, **keep_pauses)
        keep = found if keep is None else torch.bitwise_or(keep.ne(0).to(torch.uint8), found)
    skip = None
    if skip_kept and keep is not None and keep.is_cuda:
        skip = windows_kept(keep, counts, window, hop)
    if stats is not None or skip is not None:
        skipped = 0 if skip is None else int(skip.sum())  # (one synchronisation per pack)
        if skip is not None and skipped == 0:
            skip = None
        if stats is not None:
            rows = () if keep is None else pack_rows(keep, pack_layout(counts, window, hop)[1], counts, window, hop)
            kept = sum(int(row[..., :n].ne(0).sum()) for row, n in zip(rows, num_samples))
            stats.update(kept_samples=kept, windows=sum(counts), skipped_windows=skipped)
    return keep, skip


def _decode(model, codes, labels, counts, num_samples, single, sources, keeps, start_step, sampler_kwargs, *, window, hop, steps, progress,
            constrain, enc_pred, enc_pred_scale, seed, clip_offset, window_batch, sampler, eta, guidance, vectors, keep_pauses, skip_kept, stats):
    """`decode_long` (`single`: the pack of one recording, `counts` None, run on the single entry points with `sampler_kwargs` passed
    through, the result a view) and `decode_long_batch` (the result one clone per recording).  `sources` / `keeps` are None or hold one
    entry per recording; `start_step` is what the caller made of `strength`."""
    from .diffusion import fresh_seed, pick_sampler, randn_clips
    from .vq_vae import one_voice

    cond_seq = model.cond_sequence(codes)
    check_rate(model, window, hop)
    num_samples = [int(n) for n in num_samples]
    planned, offsets, _ = plan_pack(num_samples, window, hop)
    if not single and planned != [int(c) for c in counts]:
        raise ValueError(f"recordings of {num_samples} samples in windows of {window} every {hop} are {planned} windows, not counts={list(counts)}")
    counts, N, R = planned, sum(planned), len(planned)
    if cond_seq.shape[0] != N:
        raise ValueError(f"{num_samples} samples in windows of {window} every {hop} are {counts} windows; codes hold {cond_seq.shape[0]}")
    if codes.shape[-1] * model.encoder.downsample_rate != window:
        raise ValueError(f"codes of length {codes.shape[-1]} describe {codes.shape[-1] * model.encoder.downsample_rate} samples, not window={window}")
    one_voice(labels, vectors)
    if vectors is not None:
        vectors = _per_window(vectors.reshape(-1, vectors.shape[-1]), N, None if single else counts, "vector")
    if labels is not None:
        labels = _per_window(labels.reshape(-1), N, None if single else counts, "label")
    predictor, cond_fn = _conditioned(model, cond_seq, labels, enc_pred, enc_pred_scale, guidance, vectors)
    if seed is None:
        seed = fresh_seed()
    padded = [(c - 1) * hop + window for c in counts]
    run = dict(sampler_kwargs) if single else dict(counts=counts)
    if sources is not None:
        if len(sources) != R or (keeps is not None and len(keeps) != R):
            raise ValueError(f"sources (and keeps) must hold one entry per recording ({R})")
        rows = [pad_source_keep(sources[r], None if keeps is None else keeps[r], num_samples[r], padded[r]) for r in range(R)]
        source = _cat([s for s, _ in rows], dim=-1)
        keep = None
        if any(k is not None for _, k in rows):
            keep = _cat([torch.zeros(1, 1, padded[r], dtype=torch.uint8, device=source.device) if k is None else k
                         for r, (_, k) in enumerate(rows)], dim=-1)
        keep, skip = _pause_keep_and_skip(source, keep, counts, window, hop, keep_pauses, skip_kept, num_samples, stats)
        names = ("source", "keep", "start_step") if single else ("pack_source", "pack_keep", "pack_start_step")
        run.update(zip(names, (source, keep, start_step)), skip=skip)
    x_T = _cat([randn_clips(1, padded[r], codes.device, seed, clip_offset + r) for r in range(R)], dim=-1)
    sample, sampler_kw = pick_sampler(model.diffusion, sampler, eta, windows=True)
    out = sample(x_T, predictor, steps, window=window, hop=hop, window_batch=window_batch, constrain=constrain, cond_fn=cond_fn, seed=seed,
                 clip_offset=clip_offset, progress=progress, **sampler_kw, **run)
    model.predictor.check_status()  # range guard of the decoder's mode (once per sample)
    outs = [row[..., :n] for row, n in zip(pack_rows(out, offsets, counts, window, hop), num_samples)]
    return outs[0] if single else [o.clone() for o in outs]


def decode_long(model, codes: torch.Tensor, labels: Optional[torch.Tensor] = None, *, num_samples: int, window: int, hop: int,
                steps: int = 100, progress: bool = False, constrain: bool = False, enc_pred=None, enc_pred_scale: float = 1.0,
                seed: Optional[int] = None, clip_offset: int = 0, window_batch: int = 64, sampler: str = "ddpm", eta: float = 0.0,
                source: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, strength: float = 1.0,
                guidance: Optional[Tuple[float, float]] = None, vectors: Optional[torch.Tensor] = None,
                keep_pauses: Optional[dict] = None, skip_kept: bool = True, stats: Optional[dict] = None, **kwargs) -> torch.Tensor:
    """Window codes [n,T1] int or [n,C,T1] float (`encode_long`) -> [1,1,num_samples] waveform: `VQVAE.decode` on one long state.
    x_T is ONE row of (n - 1) * hop + window samples keyed by `clip_offset`; `labels` is one label for every window, or [n];
    `vectors` in their place is one conditioning vector [E] for every window, or [n,E] (a morph: speakers.morph_vectors).
    With one window the result is `decode`'s, bit for bit, at the same seed and clip_offset.  `sampler` "ddim" runs
    `ddim_sample_windows` with `eta` instead of `ddpm_sample_windows`, "dpmpp" `dpmpp_sample_windows`.  `source` [1,1,num_samples] (the recording itself), `keep`
    (bool / uint8, [1,1,num_samples]: samples that stay the source's) and `strength` in (0, 1] (below 1: start from the noised
    source, `strength_to_start_step`) are `VQVAE.decode`'s.  `guidance` (label_scale, vq_scale) is what
    `VQVAE.decode_long_uncond_guidance` passes: the guided window predictor of `_conditioned`, labels not offset by the caller.
    `keep_pauses` (the detector's settings: `pauses.pause_mask`'s keywords, at least threshold_db) also keeps the pauses of `source`,
    found on the zero-padded row and OR-ed with `keep`; `skip_kept` leaves the windows that the mask covers whole out of the
    forwards, which changes no bit of the result; `stats` (a dict) receives kept_samples, windows and skipped_windows.  Further
    keywords (`schedule=` ...) go to the sampler."""
    from .diffusion import source_start_step

    if keep_pauses is not None and source is None:
        raise ValueError("keep_pauses= needs source=, the waveform whose pauses are kept")
    start_step = source_start_step(source, keep, strength, steps)
    return _decode(model, codes, labels, None, [num_samples], True, None if source is None else [source], [keep], start_step, kwargs,
                   window=window, hop=hop, steps=steps, progress=progress, constrain=constrain, enc_pred=enc_pred, enc_pred_scale=enc_pred_scale,
                   seed=seed, clip_offset=clip_offset, window_batch=window_batch, sampler=sampler, eta=eta, guidance=guidance, vectors=vectors,
                   keep_pauses=keep_pauses, skip_kept=skip_kept, stats=stats)


def decode_long_batch(model, codes: torch.Tensor, labels: Optional[torch.Tensor] = None, *, counts: Sequence[int], num_samples: Sequence[int],
                      window: int, hop: int, steps: int = 100, progress: bool = False, constrain: bool = False, enc_pred=None,
                      enc_pred_scale: float = 1.0, seed: Optional[int] = None, clip_offset: int = 0, window_batch: int = 64,
                      sampler: str = "ddpm", eta: float = 0.0, guidance: Optional[Tuple[float, float]] = None,
                      vectors: Optional[torch.Tensor] = None, sources: Optional[Sequence[torch.Tensor]] = None,
                      keeps: Optional[Sequence[Optional[torch.Tensor]]] = None, strength: float = 1.0, keep_pauses: Optional[dict] = None,
                      skip_kept: bool = True, stats: Optional[dict] = None) -> List[torch.Tensor]:
    """`decode_long` for a pack of recordings (`encode_long_batch`): codes [N,T1] or [N,C,T1] of all their windows, `counts` windows and
    `num_samples` samples per recording -> one [1,1,num_samples[r]] waveform each.  The windows of all recordings fill the forwards
    together (`window_batch` at a time) and one packed step kernel follows, so many short recordings cost what one long one does.
    `labels` is one label, one per recording, or one per window; `vectors` in their place one [E], [R,E] or [N,E].  x_T is each recording's own row keyed clip_offset + r, and recording
    r's result is what `decode_long` returns for it alone at clip_offset + r, bit for bit, whatever else is in the pack and whatever
    `window_batch` is.  `sources` and `keeps` are `decode_long`'s `source` and `keep`, one per recording ([1,1,num_samples[r]]; an entry
    of `keeps` may be None), `strength`, `keep_pauses`, `skip_kept` and `stats` are `decode_long`'s: rows are zero-padded as there, the
    detector sees the padded rows, and the kept samples are replaced by `vqvs_keep_region_windows_packed`.  `guidance` (label_scale,
    vq_scale) is `decode_long`'s, what `VQVAE.decode_long_batch_uncond_guidance` passes."""
    from .diffusion import strength_to_start_step

    start_step = strength_to_start_step(strength, steps)
    if sources is None and (keeps is not None or start_step or keep_pauses is not None):
        raise ValueError("keeps=, strength < 1 and keep_pauses= need sources=, the waveforms whose samples are kept or noised")
    return _decode(model, codes, labels, counts, num_samples, False, sources, keeps, start_step, {},
                   window=window, hop=hop, steps=steps, progress=progress, constrain=constrain, enc_pred=enc_pred, enc_pred_scale=enc_pred_scale,
                   seed=seed, clip_offset=clip_offset, window_batch=window_batch, sampler=sampler, eta=eta, guidance=guidance, vectors=vectors,
                   keep_pauses=keep_pauses, skip_kept=skip_kept, stats=stats)
