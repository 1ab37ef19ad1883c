"""
VQVAE facade: UNet encoder + VQ + conditional diffusion decoder
(reference vq_voice_swap/vq_vae.py:10-240).  encode / decode keep the reference's
signatures; every stage runs in libvqvs_hip.so.
"""

from __future__ import annotations

import contextlib
from typing import Any, Dict, Optional

import torch

from .diffusion import fresh_seed, guidance_mix, pick_sampler, randn_clips, source_start_step
from .diffusion_model import DiffusionModel
from .conv_encoder import ConvMFCCEncoder
from .unet import UNetEncoder
from .vq import VQ


def make_encoder(enc_name: str, base_channels: int = 32, cond_mult: int = 16):
    """reference models/make.py:41-84: the UNet encoder and the three ConvMFCCEncoder variants are built."""
    if enc_name == "unet":
        return UNetEncoder(base_channels=base_channels, out_channels=base_channels * cond_mult)
    if enc_name == "conv-mfcc-ulaw":
        return ConvMFCCEncoder(base_channels=base_channels, out_channels=base_channels * cond_mult)
    if enc_name == "conv-mfcc-ulaw-v2":
        return ConvMFCCEncoder(base_channels=base_channels, out_channels=base_channels * cond_mult, version=2)
    if enc_name == "conv-mfcc-linear":
        return ConvMFCCEncoder(base_channels=base_channels, out_channels=base_channels * cond_mult, input_ulaw=False)
    raise ValueError(f"encoder {enc_name!r} is outside the accelerated hot path (SURVEY.md section 2a): "
                     "'unet' and the 'conv-mfcc-*' encoders are built")


def _guided(labels, label_scale: float, vq_scale: float) -> bool:
    """Whether a guidance call extrapolates at all: a label scale counts only with labels (or vectors in their place)."""
    return bool(vq_scale) or (labels is not None and bool(label_scale))


def one_voice(labels, vectors) -> None:
    """A voice is named by labels or given as vectors (speakers.py), never both."""
    if labels is not None and vectors is not None:
        raise ValueError("give labels or vectors, not both: a vector stands in for class_embed(labels)")


def guided_predictor(model, cond_seq: torch.Tensor, labels: Optional[torch.Tensor], label_scale: float, vq_scale: float,
                     vectors: Optional[torch.Tensor] = None):
    """(predictor(xs, ts, first=0), guided) of classifier-free-style guidance on the rows of `cond_seq` [n,C,T1] and `labels` [n] (not
    offset; None: no labels).  A slice of m rows starting at `first` runs the decoder's predictor on the reps-fold batch
    [own cond, labels + 1 | zero cond, labels + 1 | own cond, label 0] -- a block only for a non-zero scale (reference
    vq_vae.py:188-214, whose always-tripled batch lines up only when both are) -- and `vqvs_guidance_mix` extrapolates in place over
    block 0.  The batches of a slice are built once and kept: the sampling loop asks for the same slices at every step.  `rows=` (an
    int64 [m] index tensor, what a window loop that skips windows passes) names the slice's rows in the place of first .. first + m;
    its batch is keyed by the tensor itself, which the loop keeps for the whole run.
    `vectors` [n,E] in place of labels (NOT offset: they are the voices themselves) run as [own cond, vectors | zero cond, vectors |
    own cond, row 0 of the table as a vector]: with vectors = class_embed.weight[labels + 1] the labels run, bit for bit."""
    one_voice(labels, vectors)
    key = "labels" if vectors is None else "vectors"
    voice = vectors if vectors is not None else (None if labels is None else labels + 1)
    use_vq = bool(vq_scale)
    use_label = voice is not None and bool(label_scale)
    reps = 1 + int(use_vq) + int(use_label)
    scales = [float(s) for flag, s in ((use_vq, vq_scale), (use_label, label_scale)) if flag] + [0.0, 0.0]
    batches = {}

    def null_voice(like):
        if vectors is None:
            return torch.zeros_like(like)
        return model.predictor.class_embed.weight[0].detach().to(like).expand(like.shape[0], -1)

    def batch(first: int, m: int, rows=None):
        key_ = (first, m) if rows is None else ("rows", id(rows))  # (a gathered slice: the run passes the same index tensor every step)
        if key_ not in batches:
            sl = slice(first, first + m) if rows is None else rows
            conds = [cond_seq[sl]]
            voices = [voice[sl]] if voice is not None else None
            if use_vq:
                conds.append(torch.zeros_like(cond_seq[sl]))
                if voices is not None:
                    voices.append(voice[sl])
            if use_label:
                conds.append(cond_seq[sl])
                voices.append(null_voice(voice[sl]))
            batches[key_] = (torch.cat(conds, dim=0), torch.cat(voices, dim=0) if voices is not None else None, rows)
        return batches[key_][:2]

    def predictor(xs, ts, first: int = 0, rows=None):
        cond_batch, voice_batch = batch(int(first), xs.shape[0], rows)
        outs = model.predictor(torch.cat([xs] * reps, dim=0), torch.cat([ts] * reps, dim=0), cond=cond_batch, **{key: voice_batch})
        return guidance_mix(outs, reps, scales[0], scales[1])

    return predictor, reps > 1


class VQVAE(DiffusionModel):
    def __init__(self, base_channels: int, enc_name: str = "unet", cond_mult: int = 16, dictionary_size: int = 512, **kwargs):
        encoder = make_encoder(enc_name, base_channels=base_channels, cond_mult=cond_mult)
        kwargs["cond_channels"] = base_channels * cond_mult
        super().__init__(base_channels=base_channels, **kwargs)
        self.enc_name = enc_name
        self.cond_mult = cond_mult
        self.dictionary_size = dictionary_size
        self.encoder = encoder
        self.vq = VQ(self.cond_channels, dictionary_size)

    def set_precision(self, precision: str, encoder_precision: str = "fp32"):
        """Precision of the diffusion decoder; the encoder stays in the fp32 mode unless asked otherwise, because VQ code
        indices have to be bit-exact (a 2-byte encoder flips near-tie codes: 23/500 in bf16) and it runs once per clip."""
        self.predictor.set_precision(precision)
        self.encoder.set_precision(encoder_precision)  # (ConvMFCCEncoder accepts fp32 only)
        return self

    def cond_sequence(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [N,T1] int (embedded here) or [N,C,T1] float (taken as they are) -> the decoder's conditioning sequence [N,C,T1]."""
        if codes.dim() == 2:
            return self.vq.embed(codes)
        if codes.dim() == 3:
            return codes
        raise ValueError(f"unsupported codes shape: {codes.shape}")

    def _seed_and_x_T(self, codes: torch.Tensor, x_T: Optional[torch.Tensor], kwargs: dict):
        """(seed, x_T) of a decode: `seed` taken out of the sampler's keywords or drawn, x_T drawn from it at their `clip_offset`."""
        seed = kwargs.pop("seed", None)
        if seed is None:
            seed = fresh_seed()
        if x_T is None:
            T = codes.shape[-1] * self.encoder.downsample_rate
            x_T = randn_clips(codes.shape[0], T, codes.device, seed, kwargs.get("clip_offset", 0))
        return seed, x_T

    def encode(self, inputs: torch.Tensor) -> torch.Tensor:
        """[N,1,T] waveform -> [N,T/256] int64 codes (vq_vae.py:82-90)."""
        with torch.no_grad():
            return self.vq.encode(self.encoder(inputs))

    def code_agreement(self, codes: torch.Tensor, audio: torch.Tensor) -> torch.Tensor:
        """codes [N,T1] int64 against `encode(audio)` of a [N,1,T] waveform (say, a conversion decoded from them): the int64 [N]
        count of positions whose code survived the round trip."""
        again = self.encode(audio)
        if again.shape != codes.shape:
            raise ValueError(f"codes of shape {tuple(codes.shape)} against audio that encodes to {tuple(again.shape)}")
        return (again == codes.to(again.device)).sum(dim=1)

    def losses(self, vq_loss, inputs: torch.Tensor, labels: Optional[torch.Tensor] = None, jitter: float = 0.0, no_vq_prob: float = 0.0,
               *, ts: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
               clip_offset: int = 0, hist: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The losses of reference vq_vae.py:34-80 as an EVALUATION: {"vq_loss", "mse", "ts", "mses"} as there, plus "idxs"
        [N,T1], "sq_err" [N] float64 (the clip's sum of (z - e)^2) and "embedded" [N,C,T1] (the conditioning, for a caller
        that scores the decoder again).  Encoder (its own mode, fp32 unless `set_precision` was told otherwise) ->
        `VQ.quantize` (one kernel: codes, embedding, error sums, counts into `hist`) -> `Diffusion.denoising_losses` with the
        embedding as conditioning: the embedding is computed once and serves both losses.  `ts`, `noise`, `seed` and
        `clip_offset` are those of `denoising_losses`; the t of a clip comes back unchanged.  `vq_loss` is a `StandardVQLoss`
        (read from the kernel's sums) or any callable (inputs, embedded, dictionary) -> scalar.  `jitter` and `no_vq_prob`
        are training-only regularisers and must be zero; a module in training mode is refused."""
        if jitter or no_vq_prob:
            raise ValueError(f"jitter={jitter!r} and no_vq_prob={no_vq_prob!r} are training-only regularisers (reference vq_vae.py:58-72); "
                             "VQVAE.losses here is an evaluation and accepts only 0 for both")
        if self.training or self.vq.training:
            raise RuntimeError("VQVAE.losses is evaluation-only (no gradients, no usage tracking / revival); call .eval()")
        from . import _native

        _native.require_cuda(inputs, labels, noise, hist)
        if seed is None:
            seed = fresh_seed()
        if ts is None:
            ts = self.diffusion.draw_ts(inputs.shape[0], seed, clip_offset)
        with torch.no_grad():
            z = self.encoder(inputs)
            q = self.vq.quantize(z, hist=hist)
            if hasattr(vq_loss, "from_sq_err"):
                vq_value = vq_loss.from_sq_err(q["sq_err"], z.numel())
            else:
                vq_value = vq_loss(z, q["embedded"], self.vq.dictionary.detach().to(z))
            mses = self.diffusion.denoising_losses(inputs, self.predictor, ts, noise=noise, seed=seed, clip_offset=clip_offset,
                                                   cond=q["embedded"], labels=labels)
        return {"vq_loss": vq_value, "mse": mses.mean(), "ts": ts, "mses": mses, "idxs": q["idxs"], "sq_err": q["sq_err"],
                "embedded": q["embedded"]}

    def decode(self, codes: torch.Tensor, labels: Optional[torch.Tensor] = None, steps: int = 100, progress: bool = False,
               constrain: bool = False, enc_pred=None, enc_pred_scale: float = 1.0, x_T: Optional[torch.Tensor] = None,
               sampler: str = "ddpm", eta: float = 0.0, source: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
               strength: float = 1.0, vectors: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """codes [N,T1] int or [N,C,T1] float -> [N,1,T1*256] waveform (vq_vae.py:92-145).  `vectors` [N,E] in place of `labels`
        gives every clip's voice as an explicit conditioning vector (speakers.py).  `sampler` "ddim" runs
        `Diffusion.ddim_sample` with `eta` (0: the result depends on x_T alone) instead of `ddpm_sample`, "dpmpp" the deterministic
        second-order `Diffusion.dpmpp_sample`.
        `source` [N,1,T] is the waveform being converted: the samples `keep` marks (bool / uint8, [N,1,T]) stay the source's, bit for
        bit, and are shown to the predictor at every noise level; `strength` in (0, 1] below 1 starts from the source noised to step
        `strength_to_start_step(strength, steps)` instead of from x_T."""
        one_voice(labels, vectors)
        start_step = source_start_step(source, keep, strength, steps)
        if source is not None:
            kwargs.update(source=source, keep=keep, start_step=start_step)
        cond_seq = self.cond_sequence(codes)
        cond_fn = None
        if enc_pred is not None:  # vq_vae.py:123-130: guidance towards the codes, gradient from the native backward schedule
            targets = self.vq.encode(cond_seq)
            cond_fn = enc_pred.guidance_fn(targets, enc_pred_scale)

        seed, x_T = self._seed_and_x_T(codes, x_T, kwargs)
        sample, sampler_kw = pick_sampler(self.diffusion, sampler, eta)
        out = sample(
            x_T, lambda xs, ts, **kw: self.predictor(xs, ts, cond=cond_seq, labels=labels, vectors=vectors, **kw),
            steps=steps, progress=progress, constrain=constrain, cond_fn=cond_fn, seed=seed, **sampler_kw, **kwargs)
        self.predictor.check_status()  # range guard of the decoder's mode (once per sample)
        return out

    def invert(self, inputs: torch.Tensor, labels: Optional[torch.Tensor] = None, steps: int = 100, codes: Optional[torch.Tensor] = None,
               vectors: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """[N,1,T] waveform -> the x_T [N,1,T] that the DDIM sampler at eta = 0 maps back towards it under ITS OWN codes (encoded here
        unless `codes`, [N,T1] int or [N,C,T1] float, is given) and its own `labels`: `Diffusion.ddim_invert` with the decoder's
        predictor.  `decode(codes, other_labels, steps=steps, sampler="ddim", x_T=...)` then converts the voice from the source's
        latent instead of a fresh draw.  `vectors` [N,E] in place of `labels`: the source's voice as explicit vectors."""
        one_voice(labels, vectors)
        if codes is None:
            codes = self.encode(inputs)
        cond_seq = self.cond_sequence(codes)
        T = codes.shape[-1] * self.encoder.downsample_rate
        if inputs.dim() != 3 or inputs.shape[0] != cond_seq.shape[0] or inputs.shape[-1] != T:
            raise ValueError(f"inputs of shape {tuple(inputs.shape)} do not match codes for {cond_seq.shape[0]} clips of {T} samples")
        out = self.diffusion.ddim_invert(inputs, lambda xs, ts: self.predictor(xs, ts, cond=cond_seq, labels=labels, vectors=vectors), steps, **kwargs)
        self.predictor.check_status()
        return out

    def encode_long(self, wave: torch.Tensor, window: int, hop: int, window_batch: int = 64) -> torch.Tensor:
        """[1,1,N] waveform of any length -> codes [n, window / rate] of its overlapping windows (longform.encode_long)."""
        from .longform import encode_long

        return encode_long(self, wave, window, hop, window_batch)

    def decode_long(self, codes: torch.Tensor, labels: Optional[torch.Tensor] = None, *, vectors: Optional[torch.Tensor] = None,
                    **kwargs) -> torch.Tensor:
        """Window codes [n,T1] or [n,C,T1] -> [1,1,num_samples] waveform: `decode` on one long state whose windows are blended at
        every step (longform.decode_long; keywords num_samples, window, hop, steps, constrain, enc_pred, seed, window_batch, sampler,
        eta, source, keep, strength ...).  `vectors` [n,E] (or one [E]) in place of `labels`: a voice per window, e.g. a morph."""
        from .longform import decode_long

        return decode_long(self, codes, labels, vectors=vectors, **kwargs)

    def encode_long_batch(self, waves, window: int, hop: int, window_batch: int = 64):
        """Several recordings [1,1,N_r] -> (codes [N, window / rate] of all their windows, counts per recording)
        (longform.encode_long_batch)."""
        from .longform import encode_long_batch

        return encode_long_batch(self, waves, window, hop, window_batch)

    def decode_long_batch(self, codes: torch.Tensor, labels: Optional[torch.Tensor] = None, *, vectors: Optional[torch.Tensor] = None,
                          **kwargs):
        """The codes of a pack of recordings -> one [1,1,num_samples[r]] waveform each, the windows of all of them packed into the
        same forwards (longform.decode_long_batch; keywords counts, num_samples, window, hop, steps, sampler, eta, constrain, enc_pred,
        enc_pred_scale, seed, clip_offset, window_batch, progress).  `vectors` in place of `labels`: one [E], one per recording [R,E]
        or one per window [N,E]."""
        from .longform import decode_long_batch

        return decode_long_batch(self, codes, labels, vectors=vectors, **kwargs)

    def decode_uncond_guidance(self, codes: torch.Tensor, labels: Optional[torch.Tensor] = None, steps: int = 100,
                               progress: bool = False, constrain: bool = False, label_scale: float = 0.0, vq_scale: float = 0.0,
                               x_T: Optional[torch.Tensor] = None, sampler: str = "ddpm", eta: float = 0.0,
                               source: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, strength: float = 1.0,
                               vectors: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """Decode with classifier-free-style guidance towards the VQ codes and/or the label (reference
        vq_vae.py:147-220): the predictor runs on a 1x-3x batch [conditional | codes dropped | label dropped] and the
        prediction is base + scale * (base - dropped), mixed by `vqvs_guidance_mix`.  Labels are NOT offset by the caller: label 0 is
        the unconditional label of such a model, so `labels + 1` is used as in the reference.  `source`, `keep` and `strength` are
        `decode`'s.  `vectors` [N,E] in place of `labels` are the voices themselves (not offset); the dropped label is row 0 of the table."""
        one_voice(labels, vectors)
        start_step = source_start_step(source, keep, strength, steps)
        if source is not None:
            kwargs.update(source=source, keep=keep, start_step=start_step)
        cond_seq = self.cond_sequence(codes)
        seed, x_T = self._seed_and_x_T(codes, x_T, kwargs)
        pred_fn, guided = guided_predictor(self, cond_seq, labels, label_scale, vq_scale, vectors)
        sample, sampler_kw = pick_sampler(self.diffusion, sampler, eta)
        with self.guidance_precision(guided, "decode_uncond_guidance"):
            out = sample(x_T, pred_fn, steps=steps, progress=progress, constrain=constrain, seed=seed, **sampler_kw, **kwargs)
            self.predictor.check_status()
        return out

    @contextlib.contextmanager
    def guidance_precision(self, guided: bool, what: str, stacklevel: int = 4):
        """The decoder's mode for a guided call: the extrapolation base + s_vq (base - a) + s_label (base - b) multiplies the predictor's
        rounding error by up to 1 + 2 (s_vq + s_label), and a 2-byte decoder mode does not hold the 1e-3 waveform contract there
        (fixtures F11 / F11b), so the guided predictor runs in the fp32 mode for the call, whatever mode the decoder is set to.
        (precision_override keeps the decoder's own handle and arena; the fp32 handle is cached beside it for the next call.)"""
        prev = self.predictor.precision
        promote = guided and prev != "fp32"
        if promote:
            import warnings

            warnings.warn(f"{what}: the predictor runs in the fp32 mode for this call (decoder mode {prev!r} does not "
                          "meet the 1e-3 waveform contract under guidance extrapolation)", stacklevel=stacklevel)
        with self.predictor.precision_override("fp32" if promote else prev):
            yield

    def decode_long_uncond_guidance(self, codes: torch.Tensor, labels: Optional[torch.Tensor] = None, *, label_scale: float = 0.0,
                                    vq_scale: float = 0.0, vectors: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """`decode_uncond_guidance` on one long state: `decode_long` (its keywords: num_samples, window, hop, steps, constrain, seed,
        clip_offset, window_batch, sampler, eta, source, keep, strength ...) whose window predictor is the guided one -- each slice of
        windows runs as [own cond, labels + 1 | zero cond, labels + 1 | own cond, label 0] and is mixed by `vqvs_guidance_mix`.
        Labels are NOT offset by the caller.  With one window the result is `decode_uncond_guidance`'s, bit for bit."""
        from .longform import decode_long

        return self._decode_long_guided(decode_long, "decode_long_uncond_guidance", codes, labels, label_scale, vq_scale, vectors, kwargs)

    def decode_long_batch_uncond_guidance(self, codes: torch.Tensor, labels: Optional[torch.Tensor] = None, *, label_scale: float = 0.0,
                                          vq_scale: float = 0.0, vectors: Optional[torch.Tensor] = None, **kwargs):
        """`decode_long_uncond_guidance` for a pack of recordings: `decode_long_batch` (its keywords: counts, num_samples, window, hop
        ...) with the guided window predictor.  Recording r is what `decode_long_uncond_guidance` returns for it alone at
        clip_offset + r, bit for bit."""
        from .longform import decode_long_batch

        return self._decode_long_guided(decode_long_batch, "decode_long_batch_uncond_guidance", codes, labels, label_scale, vq_scale, vectors, kwargs)

    def _decode_long_guided(self, decode, what: str, codes, labels, label_scale, vq_scale, vectors, kwargs):
        """`decode` (longform.decode_long or decode_long_batch) with the guided window predictor, in the precision a guided call takes;
        `what` names the caller in the precision warning (stacklevel 5: addressed to that caller's caller)."""
        one_voice(labels, vectors)
        with self.guidance_precision(_guided(vectors if labels is None else labels, label_scale, vq_scale), what, stacklevel=5):
            return decode(self, codes, labels, vectors=vectors, guidance=(label_scale, vq_scale), **kwargs)

    @property
    def downsample_rate(self) -> int:
        import math

        a, b = self.predictor.downsample_rate, self.encoder.downsample_rate
        return a * b // math.gcd(a, b)

    def save_kwargs(self) -> Dict[str, Any]:
        res = super().save_kwargs()
        res.update(dict(enc_name=self.enc_name, cond_mult=self.cond_mult, dictionary_size=self.dictionary_size))
        return res
