"""
Speaker enrolment: learn `class_embed` rows for new speakers of a trained class-conditional model, everything else frozen
(reference train_vqvae_add.py, `VQVAEAddClassesTrainLoop`, train_loop.py:438-485: `add_labels(n)`, freeze all but
`predictor.label_parameters()`, AdamW on the noise-prediction MSE).

Nothing here runs torch autograd or a torch optimiser: the gradient of every clip's MSE with respect to its conditioning vector comes
from `UNetPredictor.embedding_grad` (`vqvs_unet_embed_grad`: the predictor's forward schedule and an explicit backward schedule that
reaches only the FiLM coefficients), and the batch mean, the sum over clips that share a speaker and the AdamW update are one kernel,
`vqvs_embed_adamw`.  The model itself is not touched until `finish()`.

`ClassifierEnroller` does the same for the speaker `Classifier`, the other model that knows the label set: new speakers are new rows of
its head, GELU -> Linear(F, num_labels) on the stem's feature vector.  With the stem and the old rows frozen the gradient of the NLL
of the label (the reference's `ClassifierTrainLoop.compute_losses`, train_loop.py:551-561) is closed-form in the new rows,
(softmax[K + j] - [y = K + j]) * gelu(feat), so a step is the stem's forward (`vqvs_classifier_features`), `vqvs_head_xent_grad` and
`vqvs_head_adamw`: no backward schedule, no autograd, no torch optimiser.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch

from . import _native
from .classifier import Classifier
from .diffusion import Diffusion, fresh_seed, make_schedule, randn_clips
from .diffusion_model import DiffusionModel


def init_rows(old: torch.Tensor, num_new: int, init: Union[str, int], seed: int) -> torch.Tensor:
    """The starting rows [num_new, E], float32 on the CPU.  "normal": N(0, 1), what a fresh nn.Embedding holds (the reference's
    `add_labels`), from a generator seeded by `seed`; "mean": the mean of the existing rows; an integer: that speaker's row."""
    old = old.detach().to(device="cpu", dtype=torch.float32)
    E = old.shape[1]
    if isinstance(init, bool):
        raise ValueError(f"init={init!r}: use 'normal', 'mean' or the index of an existing speaker")
    if isinstance(init, int):
        if not 0 <= init < old.shape[0]:
            raise IndexError(f"init={init}: the model has speakers 0..{old.shape[0] - 1}")
        return old[init].clone().expand(num_new, E).contiguous()
    if init == "normal":
        return torch.randn(num_new, E, generator=torch.Generator().manual_seed(int(seed)))
    if init == "mean":
        return old.double().mean(dim=0).float().expand(num_new, E).contiguous()
    raise ValueError(f"init={init!r}: use 'normal', 'mean' or the index of an existing speaker")


def adamw_step(rows: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grads: torch.Tensor, row_of_clip: torch.Tensor, step: int,
               lr: float, betas: Tuple[float, float], eps: float, weight_decay: float) -> None:
    """`vqvs_embed_adamw` in place on rows / m / v [n, E] from per-clip gradients [B, E]: the mean over the batch, summed per named row."""
    n, E = rows.shape
    B = grads.shape[0]
    _native.check_index_range(row_of_clip, n, "new speaker labels")
    with torch.cuda.device(rows.device):
        _native.check(_native.lib().vqvs_embed_adamw(rows.data_ptr(), m.data_ptr(), v.data_ptr(), grads.data_ptr(), row_of_clip.data_ptr(),
                                                     n, B, E, int(step), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                     float(weight_decay), _native._stream_ptr()))


class SpeakerEnroller:
    """Rows, AdamW moments and step count of `num_new` new speakers of `model`, a class-conditional `VQVAE` or `DiffusionModel` in
    `eval()`.  `step()` takes one optimiser step on a batch; `finish()` grows the model by the rows; `state_dict()` /
    `load_state_dict()` resume.  New speaker k is row k here and label `first_label + k` of the finished model."""

    front = False  # (NullLabelEnroller: the row goes in FRONT of the table; its state_dict says so and a resume of the other kind is refused)

    def __init__(self, model: DiffusionModel, num_new: int, lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, init: Union[str, int] = "normal", seed: int = 0):
        if not isinstance(model, DiffusionModel) or model.num_labels is None:
            raise ValueError("SpeakerEnroller needs a class-conditional VQVAE or DiffusionModel (num_labels is None)")
        if model.training:
            raise RuntimeError("SpeakerEnroller: the model's own parameters stay frozen; call .eval()")
        if int(num_new) != num_new or num_new < 1:
            raise ValueError(f"num_new={num_new!r} must be a positive integer")
        self.model = model
        self.num_new = int(num_new)
        self.first_label = int(model.num_labels)
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        old = model.predictor.class_embed.weight
        self.rows = init_rows(old, self.num_new, init, seed).to(old.device)
        self.exp_avg = torch.zeros_like(self.rows)
        self.exp_avg_sq = torch.zeros_like(self.rows)
        self.steps = 0
        self.finished = False

    def _cond(self, inputs: torch.Tensor) -> Optional[torch.Tensor]:
        """The decoder's conditioning of a batch: encode and quantise as `VQVAE.losses` does; None for a plain DiffusionModel."""
        if not hasattr(self.model, "encoder"):
            return None
        with torch.no_grad():
            return self.model.vq.quantize(self.model.encoder(inputs))["embedded"]

    def losses(self, inputs: torch.Tensor, new_labels: torch.Tensor, *, ts: Optional[torch.Tensor] = None,
               noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, clip_offset: int = 0):
        """(mses [B], grads [B, E], ts) of a batch under the current rows, without an optimiser step."""
        _native.require_cuda(inputs, noise)
        if self.finished:
            raise RuntimeError("SpeakerEnroller.finish() was called: the rows are part of the model now")
        if inputs.dim() != 3:
            raise ValueError(f"expected inputs of shape [N, 1, T], got {tuple(inputs.shape)}")
        x0 = inputs.detach().to(torch.float32).contiguous()
        B, T = x0.shape[0], x0.shape[-1]
        labels = new_labels.detach().to(device=x0.device, dtype=torch.int64).contiguous()
        if labels.shape != (B,):
            raise ValueError(f"expected new_labels of shape [{B}], got {tuple(labels.shape)}")
        _native.check_index_range(labels, self.num_new, "new speaker labels")
        if seed is None:
            seed = fresh_seed()
        diffusion = self.model.diffusion
        if ts is None:
            ts = diffusion.draw_ts(B, seed, clip_offset)
        ts = ts.detach().to(device=x0.device, dtype=torch.float32).contiguous()
        if ts.shape != (B,):
            raise ValueError(f"expected ts of shape [{B}], got {tuple(ts.shape)}")
        # the noise of clip clip_offset + b from the counter-based generator's loss stream: what `sample_q_seeded` draws in-kernel
        eps = randn_clips(B, T, x0.device, seed, clip_offset, _native.STREAM_LOSS) if noise is None else noise.detach().to(torch.float32).contiguous()
        if tuple(eps.shape) != tuple(x0.shape):
            raise ValueError(f"noise of shape {tuple(eps.shape)} does not match inputs of shape {tuple(x0.shape)}")
        alpha = diffusion.schedule(ts.cpu()).to(device=x0.device, dtype=torch.float32).contiguous()
        x_t = torch.empty_like(x0)
        with torch.cuda.device(x0.device):
            _native.check(_native.lib().vqvs_ddpm_noise(x0.data_ptr(), B, alpha.data_ptr(), eps.data_ptr(), B, None, x_t.data_ptr(), B, T,
                                                        int(seed), int(clip_offset), _native._stream_ptr()))
        mses, grads = self.model.predictor.embedding_grad(x_t, ts, eps, self.rows[labels], cond=self._cond(x0))
        return mses, grads, ts, labels

    def step(self, inputs: torch.Tensor, new_labels: torch.Tensor, *, ts: Optional[torch.Tensor] = None,
             noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, clip_offset: int = 0) -> Dict[str, torch.Tensor]:
        """One AdamW step on the batch `inputs` [B, 1, T] whose clips belong to new speakers `new_labels` [B] (0 .. num_new - 1).
        `ts` and `noise` as given, else drawn from (`seed`, `clip_offset` + b) as `Diffusion.denoising_losses` draws them.
        Returns {"loss": the batch mean BEFORE the step, "mses" [B], "ts" [B]}."""
        mses, grads, ts, labels = self.losses(inputs, new_labels, ts=ts, noise=noise, seed=seed, clip_offset=clip_offset)
        self.steps += 1
        adamw_step(self.rows, self.exp_avg, self.exp_avg_sq, grads, labels, self.steps, self.lr, self.betas, self.eps, self.weight_decay)
        return {"loss": mses.mean(), "mses": mses, "ts": ts}

    def finish(self) -> DiffusionModel:
        """`model.add_labels(num_new)` with the learned rows behind the checkpoint's own, which stay bit for bit; returns the model."""
        if self.finished:
            raise RuntimeError("SpeakerEnroller.finish() was already called")
        self.model.add_labels(self.num_new)
        with torch.no_grad():
            w = self.model.predictor.class_embed.weight
            w[self.first_label:].copy_(self.rows.to(w.device))
        self.model.predictor.invalidate()
        self.finished = True
        return self.model

    def checkpoint(self) -> Dict[str, object]:
        """The {"kwargs", "state_dict"} checkpoint of the model grown by the rows as they stand, without touching the model: what
        `finish()` followed by `save_dict()` would hold.  `VQVAE.load` / `DiffusionModel.load` read it."""
        if self.finished:
            return self.model.save_dict()
        state = self.model.save_dict()
        kwargs = dict(state["kwargs"], num_labels=self.first_label + self.num_new)
        sd = {k: v.detach().cpu().clone() for k, v in state["state_dict"].items()}
        key = "predictor.class_embed.weight"
        sd[key] = torch.cat([sd[key], self.rows.detach().cpu().to(sd[key].dtype)], dim=0)
        return {"kwargs": kwargs, "state_dict": sd}

    def state_dict(self) -> Dict[str, object]:
        return {"rows": self.rows.detach().cpu().clone(), "exp_avg": self.exp_avg.detach().cpu().clone(),
                "exp_avg_sq": self.exp_avg_sq.detach().cpu().clone(), "steps": self.steps, "first_label": self.first_label}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        front = bool(state.get("front", False))
        if front != self.front:
            kinds = {True: "the null label (NullLabelEnroller, a row in front of the table)", False: "new speakers (SpeakerEnroller, rows behind the table)"}
            raise ValueError(f"state was made by an enroller of {kinds[front]}, this one learns {kinds[self.front]}")
        rows = state["rows"]
        if tuple(rows.shape) != tuple(self.rows.shape):
            raise ValueError(f"state holds rows of shape {tuple(rows.shape)}, this enroller has {tuple(self.rows.shape)}")
        if int(state["first_label"]) != self.first_label:
            raise ValueError(f"state was made for a model of {state['first_label']} speakers, this one has {self.first_label}")
        dev = self.rows.device
        self.rows = rows.to(device=dev, dtype=torch.float32).clone()
        self.exp_avg = state["exp_avg"].to(device=dev, dtype=torch.float32).clone()
        self.exp_avg_sq = state["exp_avg_sq"].to(device=dev, dtype=torch.float32).clone()
        self.steps = int(state["steps"])


class NullLabelEnroller(SpeakerEnroller):
    """The unconditional ("null") label of a class-conditional model, learned with everything else frozen: ONE row, trained by every
    clip of a batch whatever its speaker, that `finish()` puts in FRONT of the table -- `add_labels(1, end=False)`, the layout of the
    reference's `VQVAEUncondTrainLoop.load_from_pretrained`: label 0 is the null label, old speaker k is label k + 1, its row bit for
    bit.  That is the model `VQVAE.decode_uncond_guidance` and sample_vqvae_uncond.py expect.

    The reference (train_vqvae_uncond.py) gives a clip label 0 with probability `--no-class-prob` and fine-tunes every parameter; with
    all but row 0 frozen the clips that keep their label have zero gradient, so training every clip on row 0 is the reference's
    gradient for that row up to the factor no_class_prob, a learning-rate scale.  What a frozen model cannot learn is the reference's
    code dropout (`--no-vq-prob`): guidance towards the codes stays meaningful only for models the reference fine-tuned itself.

    The interface is `SpeakerEnroller`'s with `num_new` = 1; `step(inputs)` and `losses(inputs)` need no labels."""

    front = True

    def __init__(self, model: DiffusionModel, lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, init: Union[str, int] = "normal", seed: int = 0):
        super().__init__(model, 1, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, init=init, seed=seed)

    @staticmethod
    def _row_zero(inputs: torch.Tensor, new_labels: Optional[torch.Tensor]) -> torch.Tensor:
        if new_labels is not None:
            return new_labels
        if inputs.dim() != 3:
            raise ValueError(f"expected inputs of shape [N, 1, T], got {tuple(inputs.shape)}")
        return torch.zeros(inputs.shape[0], dtype=torch.int64, device=inputs.device)

    def losses(self, inputs: torch.Tensor, new_labels: Optional[torch.Tensor] = None, **kwargs):
        """`SpeakerEnroller.losses` with every clip on the one row (`new_labels`, if given at all, is all zeros)."""
        return super().losses(inputs, self._row_zero(inputs, new_labels), **kwargs)

    def step(self, inputs: torch.Tensor, new_labels: Optional[torch.Tensor] = None, **kwargs) -> Dict[str, torch.Tensor]:
        """`SpeakerEnroller.step` with every clip on the one row: the row's gradient is the mean over the batch."""
        return super().step(inputs, self._row_zero(inputs, new_labels), **kwargs)

    def finish(self) -> DiffusionModel:
        """`model.add_labels(1, end=False)` with the learned row at index 0; the checkpoint's own rows stay bit for bit, one up."""
        if self.finished:
            raise RuntimeError("NullLabelEnroller.finish() was already called")
        self.model.add_labels(1, end=False)
        with torch.no_grad():
            w = self.model.predictor.class_embed.weight
            w[:1].copy_(self.rows.to(w.device))
        self.model.predictor.invalidate()
        self.finished = True
        return self.model

    def checkpoint(self) -> Dict[str, object]:
        """`SpeakerEnroller.checkpoint` with the row in front of the old rows."""
        if self.finished:
            return self.model.save_dict()
        state = self.model.save_dict()
        kwargs = dict(state["kwargs"], num_labels=self.first_label + 1)
        sd = {k: v.detach().cpu().clone() for k, v in state["state_dict"].items()}
        key = "predictor.class_embed.weight"
        sd[key] = torch.cat([self.rows.detach().cpu().to(sd[key].dtype), sd[key]], dim=0)
        return {"kwargs": kwargs, "state_dict": sd}

    def state_dict(self) -> Dict[str, object]:
        return dict(super().state_dict(), front=True)


# ---- the classifier's head ----------------------------------------------------------------------------------------------------------
def init_head_rows(weight: torch.Tensor, bias: torch.Tensor, num_new: int, init: Union[str, int]) -> torch.Tensor:
    """The starting rows [num_new, F + 1] (column F is the bias), float32 on the CPU.  "zeros": what a fresh head holds (the reference
    zero-scales it); "mean": the float64 mean of the old rows and biases; an integer: that speaker's row and bias."""
    old = torch.cat([weight.detach().to(device="cpu", dtype=torch.float32), bias.detach().to(device="cpu", dtype=torch.float32)[:, None]], dim=1)
    W = old.shape[1]
    if isinstance(init, bool):
        raise ValueError(f"init={init!r}: use 'zeros', 'mean' or the index of an existing speaker")
    if isinstance(init, int):
        if not 0 <= init < old.shape[0]:
            raise IndexError(f"init={init}: the classifier has speakers 0..{old.shape[0] - 1}")
        return old[init].clone().expand(num_new, W).contiguous()
    if init == "zeros":
        return torch.zeros(num_new, W)
    if init == "mean":
        return old.double().mean(dim=0).float().expand(num_new, W).contiguous()
    raise ValueError(f"init={init!r}: use 'zeros', 'mean' or the index of an existing speaker")


def head_xent_grad(feat: torch.Tensor, w_old: torch.Tensor, b_old: torch.Tensor, rows: torch.Tensor, targets: torch.Tensor, *,
                   want_logits: bool = True) -> Dict[str, torch.Tensor]:
    """`vqvs_head_xent_grad` on stem features [B, F]: {"nll" f64 [B], "top1" int64 [B], "new_mass" f64 [B], "coef" f64 [B, n],
    "act" f32 [B, F], "logits" f32 [B, K + n] or None} of the head `w_old` [K, F], `b_old` [K] grown by `rows` [n, F + 1].  Targets
    outside 0 .. K + n - 1 raise IndexError before anything is launched."""
    _native.require_cuda(feat, w_old, b_old, rows, targets)
    B, F = feat.shape
    K, n = w_old.shape[0], rows.shape[0]
    if tuple(w_old.shape) != (K, F) or tuple(b_old.shape) != (K,) or tuple(rows.shape) != (n, F + 1):
        raise ValueError(f"head of shape {tuple(w_old.shape)} / {tuple(b_old.shape)} and rows {tuple(rows.shape)} do not fit features [{B}, {F}]")
    for t in (feat, w_old, b_old, rows):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("features, head and rows must be contiguous float32")
    if targets.dtype != torch.int64 or targets.device != feat.device or not targets.is_contiguous():  # (else the same object: checked once)
        targets = targets.detach().to(device=feat.device, dtype=torch.int64).contiguous()
    if tuple(targets.shape) != (B,):
        raise ValueError(f"expected targets of shape [{B}], got {tuple(targets.shape)}")
    _native.check_index_range(targets, K + n, "labels of the grown classifier")
    dev = feat.device
    out = {"nll": torch.empty(B, device=dev, dtype=torch.float64), "top1": torch.empty(B, device=dev, dtype=torch.int64),
           "new_mass": torch.empty(B, device=dev, dtype=torch.float64), "coef": torch.empty(B, n, device=dev, dtype=torch.float64),
           "act": torch.empty(B, F, device=dev, dtype=torch.float32),
           "logits": torch.empty(B, K + n, device=dev, dtype=torch.float32) if want_logits else None}
    with torch.cuda.device(dev):
        _native.check(_native.lib().vqvs_head_xent_grad(feat.data_ptr(), w_old.data_ptr(), b_old.data_ptr(), rows.data_ptr(), targets.data_ptr(),
                                                        out["act"].data_ptr(), _native._ptr(out["logits"]), out["nll"].data_ptr(),
                                                        out["top1"].data_ptr(), out["new_mass"].data_ptr(), out["coef"].data_ptr(), B, F, K, n,
                                                        _native._stream_ptr()))
    return out


def head_adamw_step(rows: torch.Tensor, m: torch.Tensor, v: torch.Tensor, act: torch.Tensor, coef: torch.Tensor, step: int, lr: float,
                    betas: Tuple[float, float], eps: float, weight_decay: float) -> None:
    """`vqvs_head_adamw` in place on rows / m / v [n, F + 1] from `act` [B, F] and `coef` [B, n] of `head_xent_grad`."""
    _native.require_cuda(rows, m, v, act, coef)
    n, W = rows.shape
    B, F = act.shape
    if W != F + 1 or tuple(coef.shape) != (B, n) or tuple(m.shape) != (n, W) or tuple(v.shape) != (n, W):
        raise ValueError(f"rows {tuple(rows.shape)}, act {tuple(act.shape)} and coef {tuple(coef.shape)} do not fit each other")
    if coef.dtype != torch.float64 or any(t.dtype != torch.float32 for t in (rows, m, v, act)) or not all(t.is_contiguous() for t in (rows, m, v, act, coef)):
        raise ValueError("rows, m, v and act must be contiguous float32, coef contiguous float64")
    with torch.cuda.device(rows.device):
        _native.check(_native.lib().vqvs_head_adamw(rows.data_ptr(), m.data_ptr(), v.data_ptr(), act.data_ptr(), coef.data_ptr(), n, B, F,
                                                    int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                                    _native._stream_ptr()))


class ClassifierEnroller:
    """Head rows, AdamW moments and step count of `num_new` new speakers of `classifier`, a `Classifier` in `eval()`; the interface of
    `SpeakerEnroller`.  `rows` is [num_new, F + 1], column F the bias.  Labels given to `losses` / `step` are labels of the GROWN
    model: `first_label + k` is new speaker k, anything below `first_label` is a replay clip of an old speaker, which only pushes the
    new logits down.  The classifier is untouched until `finish()`."""

    def __init__(self, classifier: Classifier, num_new: int, schedule_name: str = "exp", lr: float = 1e-4,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, init: Union[str, int] = "zeros",
                 seed: int = 0):
        if not isinstance(classifier, Classifier):
            raise ValueError("ClassifierEnroller needs a Classifier")
        if classifier.training:
            raise RuntimeError("ClassifierEnroller: the classifier's own parameters stay frozen; call .eval()")
        if int(num_new) != num_new or num_new < 1:
            raise ValueError(f"num_new={num_new!r} must be a positive integer")
        if classifier.num_labels + int(num_new) > 8192:
            raise ValueError(f"{classifier.num_labels} + {num_new} labels: the head kernels take at most 8192")
        self.classifier = classifier
        self.num_new = int(num_new)
        self.first_label = int(classifier.num_labels)
        self.diffusion = Diffusion(make_schedule(schedule_name))
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.seed = int(seed)  # (no init mode draws from it; kept for the interface of SpeakerEnroller)
        head = classifier.out[1]
        self.rows = init_head_rows(head.weight, head.bias, self.num_new, init).to(head.weight.device)
        self.exp_avg = torch.zeros_like(self.rows)
        self.exp_avg_sq = torch.zeros_like(self.rows)
        self.steps = 0
        self.finished = False

    def _old_head(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        head = self.classifier.out[1]
        return (head.weight.detach().to(device=device, dtype=torch.float32).contiguous(),
                head.bias.detach().to(device=device, dtype=torch.float32).contiguous())

    def losses(self, inputs: torch.Tensor, labels: torch.Tensor, *, ts: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
               seed: Optional[int] = None, clip_offset: int = 0) -> Dict[str, torch.Tensor]:
        """{"nll", "top1", "new_mass", "coef", "act", "logits", "ts", "x_t"} of a batch under the current rows, without a step: `ts` as
        given, else `Diffusion.draw_ts`; the noise of clip `clip_offset` + b from (`seed`, STREAM_LOSS) unless given; the stem's
        features under the classifier's own precision mode; `vqvs_head_xent_grad`."""
        _native.require_cuda(inputs, noise)
        if self.finished:
            raise RuntimeError("ClassifierEnroller.finish() was called: the rows are part of the classifier now")
        if inputs.dim() != 3:
            raise ValueError(f"expected inputs of shape [N, 1, T], got {tuple(inputs.shape)}")
        x0 = inputs.detach().to(torch.float32).contiguous()
        B, T = x0.shape[0], x0.shape[-1]
        if labels.dtype != torch.int64 or labels.device != x0.device or not labels.is_contiguous():  # (else the same object: checked once)
            labels = labels.detach().to(device=x0.device, dtype=torch.int64).contiguous()
        if labels.shape != (B,):
            raise ValueError(f"expected labels of shape [{B}], got {tuple(labels.shape)}")
        _native.check_index_range(labels, self.first_label + self.num_new, "labels of the grown classifier")
        if seed is None:
            seed = fresh_seed()
        if ts is None:
            ts = self.diffusion.draw_ts(B, seed, clip_offset)
        ts = ts.detach().to(device=x0.device, dtype=torch.float32).contiguous()
        if ts.shape != (B,):
            raise ValueError(f"expected ts of shape [{B}], got {tuple(ts.shape)}")
        eps = randn_clips(B, T, x0.device, seed, clip_offset, _native.STREAM_LOSS) if noise is None else noise.detach().to(torch.float32).contiguous()
        if tuple(eps.shape) != tuple(x0.shape):
            raise ValueError(f"noise of shape {tuple(eps.shape)} does not match inputs of shape {tuple(x0.shape)}")
        alpha = self.diffusion.schedule(ts.cpu()).to(device=x0.device, dtype=torch.float32).contiguous()
        x_t = torch.empty_like(x0)
        with torch.cuda.device(x0.device):
            _native.check(_native.lib().vqvs_ddpm_noise(x0.data_ptr(), B, alpha.data_ptr(), eps.data_ptr(), B, None, x_t.data_ptr(), B, T,
                                                        int(seed), int(clip_offset), _native._stream_ptr()))
        feat = self.classifier.features(x_t, ts)
        w_old, b_old = self._old_head(x0.device)
        out = head_xent_grad(feat, w_old, b_old, self.rows, labels)
        out.update(ts=ts, x_t=x_t)
        return out

    def step(self, inputs: torch.Tensor, labels: torch.Tensor, *, ts: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
             seed: Optional[int] = None, clip_offset: int = 0) -> Dict[str, torch.Tensor]:
        """One AdamW step on the batch `inputs` [B, 1, T] with labels of the grown model.  Returns {"loss": the batch-mean NLL, "nlls"
        [B], "acc": the share of clips whose label holds the first maximum, "new_mass" [B], "ts" [B]} as they stood BEFORE the step."""
        out = self.losses(inputs, labels, ts=ts, noise=noise, seed=seed, clip_offset=clip_offset)
        self.steps += 1
        head_adamw_step(self.rows, self.exp_avg, self.exp_avg_sq, out["act"], out["coef"], self.steps, self.lr, self.betas, self.eps,
                        self.weight_decay)
        return {"loss": out["nll"].mean(), "nlls": out["nll"], "acc": out["top1"].double().mean(), "new_mass": out["new_mass"], "ts": out["ts"]}

    def finish(self) -> Classifier:
        """`classifier.add_labels(num_new)` with the learned rows behind the checkpoint's own, which stay bit for bit; returns it."""
        if self.finished:
            raise RuntimeError("ClassifierEnroller.finish() was already called")
        self.classifier.add_labels(self.num_new)
        head = self.classifier.out[1]
        with torch.no_grad():
            rows = self.rows.to(head.weight.device)
            head.weight[self.first_label:].copy_(rows[:, :-1])
            head.bias[self.first_label:].copy_(rows[:, -1])
        self.classifier.invalidate()
        self.finished = True
        return self.classifier

    def checkpoint(self) -> Dict[str, object]:
        """The {"kwargs", "state_dict"} checkpoint of the classifier grown by the rows as they stand, without touching it: what
        `finish()` followed by `save_dict()` would hold.  `Classifier.load` reads it."""
        if self.finished:
            return self.classifier.save_dict()
        state = self.classifier.save_dict()
        kwargs = dict(state["kwargs"], num_labels=self.first_label + self.num_new)
        sd = {k: v.detach().cpu().clone() for k, v in state["state_dict"].items()}
        rows = self.rows.detach().cpu()
        sd["out.1.weight"] = torch.cat([sd["out.1.weight"], rows[:, :-1].to(sd["out.1.weight"].dtype)], dim=0)
        sd["out.1.bias"] = torch.cat([sd["out.1.bias"], rows[:, -1].to(sd["out.1.bias"].dtype)], dim=0)
        return {"kwargs": kwargs, "state_dict": sd}

    def state_dict(self) -> Dict[str, object]:
        return {"rows": self.rows.detach().cpu().clone(), "exp_avg": self.exp_avg.detach().cpu().clone(),
                "exp_avg_sq": self.exp_avg_sq.detach().cpu().clone(), "steps": self.steps, "first_label": self.first_label}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        rows = state["rows"]
        if tuple(rows.shape) != tuple(self.rows.shape):
            raise ValueError(f"state holds rows of shape {tuple(rows.shape)}, this enroller has {tuple(self.rows.shape)}")
        if int(state["first_label"]) != self.first_label:
            raise ValueError(f"state was made for a classifier of {state['first_label']} speakers, this one has {self.first_label}")
        dev = self.rows.device
        self.rows = rows.to(device=dev, dtype=torch.float32).clone()
        self.exp_avg = state["exp_avg"].to(device=dev, dtype=torch.float32).clone()
        self.exp_avg_sq = state["exp_avg_sq"].to(device=dev, dtype=torch.float32).clone()
        self.steps = int(state["steps"])
