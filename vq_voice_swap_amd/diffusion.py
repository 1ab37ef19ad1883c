"""
Continuous-time DDPM process with the reverse step running as fused HIP kernels.

Mirrors the reference's `Diffusion` / `Schedule` API (reference
vq_voice_swap/diffusion/diffusion.py:9-151, schedule.py:7-41, make.py:4-13).  The
sampler loop and `ddpm_previous` call `vqvs_ddpm_step` (one fused kernel instead of
~20 full-size elementwise ops with materialised broadcasts, diffusion.py:62-90,154-157).

Additions over the reference (it has no seeding):
  * `noise=` may be passed explicitly to `ddpm_sample` as a list / callable, which is how
    the parity tests drive oracle and HIP path with identical draws;
  * otherwise noise comes from an in-kernel counter-based generator keyed by
    (seed, global clip index, step), so results do not depend on how a batch is sharded.
"""

from __future__ import annotations

import contextlib
import math
import operator
from typing import Callable, List, Optional, Sequence, Union

import torch

from . import _native


class Schedule:
    def __call__(self, t: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError


class ExpSchedule(Schedule):
    """alpha_bar(t) = exp(-k t^2), k = -ln(alpha_final) (schedule.py:15-31)."""

    def __init__(self, alpha_final: float = 1e-5):
        self.alpha_final = alpha_final
        self.k = -math.log(alpha_final)

    def __call__(self, t: torch.Tensor) -> torch.Tensor:
        return torch.exp(-self.k * (t ** 2))


class CosSchedule(Schedule):
    """alpha_bar(t) = cos(pi t / 2)^2 (schedule.py:34-41)."""

    def __call__(self, t: torch.Tensor) -> torch.Tensor:
        return torch.cos(t * math.pi / 2) ** 2


def make_schedule(name: str) -> Schedule:
    if name == "exp":
        return ExpSchedule()
    if name == "cos":
        return CosSchedule()
    raise ValueError(f"unknown schedule: {name}")


def _rows(v: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return v.to(like).reshape(-1, *([1] * (like.dim() - 1)))


NoiseSource = Union[None, Sequence[torch.Tensor], Callable[[int], torch.Tensor]]

FEW_GUIDED_STEPS = 10  # a guided run of fewer steps is promoted to the fp32 mode (ddpm_sample)


def _native_modules(fn) -> list:
    """The native (precision-mode) modules behind a predictor / cond_fn callable: the module itself, the target of a
    functools.partial (`UNetPredictor.condition`), the owner of a bound method, or what a closure advertises as `native_modules`
    (`Classifier.guidance_fn`).  Anything else -- a plain Python function -- has none: nothing is promoted."""
    seen, out = set(), []

    def add(m):
        if m is not None and hasattr(m, "precision_override") and id(m) not in seen:
            seen.add(id(m))
            out.append(m)

    add(fn)
    add(getattr(fn, "func", None))
    add(getattr(fn, "__self__", None))
    add(getattr(getattr(fn, "func", None), "__self__", None))
    for m in getattr(fn, "native_modules", ()) or ():
        add(m)
    return out


def predictor_check_status(predictor):
    """The range guard of a native predictor -- its own `check_status`, or that of the first native module behind the callable --
    or None for a plain Python function."""
    chk = getattr(predictor, "check_status", None)
    if chk is None:
        mods = _native_modules(predictor)
        chk = mods[0].check_status if mods else None
    return chk


def fresh_seed() -> int:
    """The seed of a call that was given none: one draw from torch's global generator."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _progress(its: range, progress: bool):
    """`its`, under tqdm when asked."""
    if not progress:
        return its
    from tqdm.auto import tqdm

    return tqdm(its, total=len(its))


def few_guided_steps_promotion(what: str, steps: int, predictor, cond_fn, stacklevel: int = 3):
    """Few guided steps in a 2-byte mode: the first reverse step multiplies the predictor's rounding error by 1 / sqrt(alpha_bar(1))
    and a guided run adds the classifier gradient's own; fewer than FEW_GUIDED_STEPS iterations never average that out (measured:
    config 5 at 3 steps 1.05e-3 in fp16 against the 1e-3 waveform contract, profiles/r05_parity_margins.jsonl).  The call is then
    promoted to the fp32 mode -- predictor and guidance model -- through precision_override, which keeps each module's own
    handle; VQVAE.decode_uncond_guidance does the same for its extrapolation.  (VQVS_FEW_STEP_PROMOTE=0: warn only.)
    Returns None, or an ExitStack holding the overrides: the sampler `what` runs its loop inside it.  `stacklevel` is the warnings'
    (3: the caller of the function that called this one)."""
    if cond_fn is None or steps >= FEW_GUIDED_STEPS:
        return None
    promote = [m for m in _native_modules(predictor) + _native_modules(cond_fn) if getattr(m, "precision", "fp32") != "fp32"]
    if not promote:
        return None
    import os
    import warnings

    modes = sorted({m.precision for m in promote})
    if os.environ.get("VQVS_FEW_STEP_PROMOTE", "1") == "0":
        warnings.warn(f"{what}: {steps} guided steps in the {modes} mode(s) are outside the 1e-3 waveform contract "
                      f"(fewer than {FEW_GUIDED_STEPS} steps); VQVS_FEW_STEP_PROMOTE=0 keeps the mode", RuntimeWarning, stacklevel=stacklevel)
        return None
    warnings.warn(f"{what}: {steps} guided steps (fewer than {FEW_GUIDED_STEPS}): predictor / guidance model run in the fp32 "
                  f"mode for this call (their {modes} mode(s) do not hold the 1e-3 waveform contract at so few steps)",
                  RuntimeWarning, stacklevel=stacklevel)
    stack = contextlib.ExitStack()
    for m in promote:
        stack.enter_context(m.precision_override("fp32"))
    return stack


SAMPLERS = ("ddpm", "ddim", "dpmpp")


def check_sampler(sampler: str, eta: float = 0.0) -> str:
    """The `sampler=` / `eta=` pair of the sampling entry points: eta belongs to the DDIM sampler alone."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler={sampler!r}: expected one of {SAMPLERS}")
    if sampler == "ddpm" and eta:
        raise ValueError(f"eta={eta!r} has no meaning for sampler='ddpm' (the DDIM sampler at eta = 1 is its small-sigma step)")
    if sampler == "dpmpp" and eta:
        raise ValueError(f"eta={eta!r} has no meaning for sampler='dpmpp': the DPM-Solver++(2M) sampler is deterministic")
    return sampler


def pick_sampler(diffusion, sampler: str, eta: float = 0.0, *, sigma_large: Optional[bool] = None, windows: bool = False):
    """(sampling method of `diffusion`, its keywords) for a `sampler=` / `eta=` pair: `eta` goes to the DDIM sampler alone and
    `sigma_large` (None: not the caller's to pass) to the DDPM sampler alone; the DPM-Solver++ sampler takes neither.  `windows`: the
    `..._sample_windows` forms."""
    fn = getattr(diffusion, check_sampler(sampler, eta) + ("_sample_windows" if windows else "_sample"))
    if sampler == "ddim":
        return fn, dict(eta=eta)
    if sampler == "dpmpp":
        return fn, {}
    return fn, {} if sigma_large is None else dict(sigma_large=sigma_large)


def warn_few_unguided_steps(what: str, steps: int, predictor, cond_fn, stacklevel: int = 3) -> None:
    """An UN-guided DDIM or DPM-Solver++ run of fewer than FEW_GUIDED_STEPS steps in a 2-byte mode: the first step's 1 / sqrt(alpha_bar(1)) acts on
    the predictor's rounding error just the same, but nothing has been measured for it, so the run keeps its mode and only warns.
    (Guided runs are promoted by few_guided_steps_promotion; the DDPM samplers are not touched.)"""
    if cond_fn is not None or steps >= FEW_GUIDED_STEPS:
        return
    modes = sorted({m.precision for m in _native_modules(predictor) if getattr(m, "precision", "fp32") != "fp32"})
    if modes:
        import warnings

        warnings.warn(f"{what}: {steps} steps (fewer than {FEW_GUIDED_STEPS}) in the {modes} mode(s): the 1e-3 waveform contract is not "
                      "established for so few steps; the mode is kept", RuntimeWarning, stacklevel=stacklevel)


def strength_to_start_step(strength: float, steps: int) -> int:
    """The first step of a partial-noise start: a conversion of `strength` in (0, 1] runs the last ceil(strength * steps) of the
    `steps` steps, from the source noised to that step's alpha_bar.  1 is the whole run, from x_T."""
    strength, steps = float(strength), int(steps)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength={strength!r} must lie in (0, 1]")
    if steps < 1:
        raise ValueError(f"steps={steps} must be at least 1")
    return min(max(steps - math.ceil(strength * steps), 0), steps - 1)


def source_start_step(source, keep, strength: float, steps: int) -> int:
    """The `source=` / `keep=` / `strength=` keywords of `VQVAE.decode` and `decode_long`: the step the run starts at."""
    start_step = strength_to_start_step(strength, steps)
    if source is None and (keep is not None or start_step):
        raise ValueError("keep= and strength < 1 need source=, the waveform whose samples are kept or noised")
    return start_step


def check_keep_args(state: torch.Tensor, source: Optional[torch.Tensor], keep: Optional[torch.Tensor], start_step: int, steps: int):
    """The `source=` / `keep=` / `start_step=` keywords of the four sampling loops, checked before anything touches the device:
    (source, mask) as contiguous float32 / uint8 tensors, or (None, None) when the loop runs as it always has.  `keep` is a bool or
    uint8 tensor shaped like the state (nonzero: kept); without one no sample is kept and `source` only serves a `start_step` > 0."""
    try:
        start_step = operator.index(start_step)
    except TypeError:
        raise ValueError(f"start_step={start_step!r} must be an integer") from None
    if not 0 <= start_step < max(int(steps), 1):
        raise ValueError(f"start_step={start_step} outside 0..{int(steps) - 1} (steps={steps})")
    if source is None:
        if keep is not None:
            raise ValueError("keep= needs source=: the kept samples are taken from it")
        if start_step:
            raise ValueError("start_step > 0 needs source=: the run starts from the noised source")
        return None, None
    if tuple(source.shape) != tuple(state.shape):
        raise ValueError(f"source of shape {tuple(source.shape)} does not match the state's {tuple(state.shape)}")
    if keep is not None:
        if keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"keep must be a bool or uint8 tensor, got {keep.dtype}")
        if tuple(keep.shape) != tuple(state.shape):
            raise ValueError(f"keep of shape {tuple(keep.shape)} does not match the state's {tuple(state.shape)}")
        keep = keep.detach().to(torch.uint8).contiguous()
    return source.detach().to(torch.float32).contiguous(), keep


class Diffusion:
    def __init__(self, schedule: Schedule):
        self.schedule = schedule

    # ---- light helpers (training side; plain tensor expressions) -----------------------
    def sample_q(self, x_0: torch.Tensor, ts: torch.Tensor, epsilon: Optional[torch.Tensor] = None) -> torch.Tensor:
        if epsilon is None:
            epsilon = torch.randn_like(x_0)
        a = _rows(self.schedule(ts), x_0)
        return a.sqrt() * x_0 + (1 - a).sqrt() * epsilon

    def eps_to_x0(self, x_t: torch.Tensor, ts: torch.Tensor, epsilon_prediction: torch.Tensor) -> torch.Tensor:
        a = _rows(self.schedule(ts), x_t)
        return (x_t - (1 - a).sqrt() * epsilon_prediction) * a.rsqrt()

    def x0_to_eps(self, x_t: torch.Tensor, ts: torch.Tensor, x_0: torch.Tensor) -> torch.Tensor:
        a = _rows(self.schedule(ts), x_t)
        return (x_t - x_0 * a.sqrt()) * (1 - a).rsqrt()

    def ddpm_losses(self, x, predictor, ts=None, noise=None) -> torch.Tensor:
        if ts is None:
            ts = torch.rand(len(x), device=x.device)
        if noise is None:
            noise = torch.randn_like(x)
        pred = predictor(self.sample_q(x, ts, epsilon=noise), ts)
        return ((noise - pred) ** 2).flatten(1).mean(dim=1)

    # ---- denoising loss (evaluation side; fused HIP kernels) ---------------------------------
    @staticmethod
    def draw_ts(n: int, seed: int, clip_offset: int = 0) -> torch.Tensor:
        """n uniform times in [0, 1) from a host generator seeded by (seed, clip_offset): what `denoising_losses(ts=None)` uses."""
        g = torch.Generator().manual_seed((int(seed) + 0x9E3779B97F4A7C15 * (int(clip_offset) + 1)) % (2 ** 63))
        return torch.rand(n, generator=g)

    def sample_q_seeded(self, x_0: torch.Tensor, ts: torch.Tensor, *, seed: int, clip_offset: int = 0) -> torch.Tensor:
        """`sample_q` with the noise drawn inside `vqvs_ddpm_noise` from the counter-based generator keyed by (seed, clip_offset +
        row): the noising half of `denoising_losses`.  Row b is clip number clip_offset + b of a pass, so a clip's x_t does not
        depend on the batch it is noised in.  alpha_bar(t) is evaluated on the host, as there."""
        _native.require_cuda(x_0)
        if x_0.dim() < 2:
            raise ValueError("x_0 must be [N, ..., T]")
        x0 = x_0.detach().to(torch.float32).contiguous()
        B, T = x0.shape[0], x0[0].numel()
        ts = ts.detach().to(dtype=torch.float32)
        if ts.shape != (B,):
            raise ValueError(f"expected ts of shape [{B}], got {tuple(ts.shape)}")
        alpha = self.schedule(ts.cpu()).to(device=x0.device, dtype=torch.float32).contiguous()
        x_t = torch.empty_like(x0)
        with torch.cuda.device(x0.device):
            _native.check(_native.lib().vqvs_ddpm_noise(x0.data_ptr(), B, alpha.data_ptr(), None, 0, None, x_t.data_ptr(), B, T,
                                                        int(seed), int(clip_offset), _native._stream_ptr()))
        return x_t

    def denoising_losses(self, x_0: torch.Tensor, predictor: Callable, ts: Optional[torch.Tensor] = None, *,
                         noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                         noise_index: Optional[torch.Tensor] = None, clip_offset: int = 0, alpha: Optional[torch.Tensor] = None,
                         check: bool = True, **predictor_kwargs) -> torch.Tensor:
        """Per-row noise-prediction MSE, [B] float32: what `ddpm_losses` computes (reference diffusion.py:135-151), as
        `vqvs_ddpm_noise` -> `predictor(x_t, ts, **predictor_kwargs)` -> `vqvs_ddpm_sqerr`.

        `x_0` is [B, ..., T], or [1, ..., T] with `ts` of length B: one clip scored at B settings without B copies of it.
        `noise` is a tensor of B rows or of one (broadcast); `noise=None` draws it in the kernels from the counter-based
        generator keyed by (seed, noise_index[b]) -- `noise_index=None` means clip_offset + b, the GLOBAL clip index, so a clip's
        loss does not depend on the batch it is scored in -- and the loss kernel regenerates it instead of reading it back.
        `ts=None` draws B uniform values from a host generator seeded by (seed, clip_offset).
        A caller that scores many micro-batches in a row (`speaker_search_losses`) passes `alpha` = schedule(ts) of the rows, evaluated
        once for all of them, and `check=False`, and calls the predictor's `check_status()` itself once at the end: neither the
        host-side schedule nor the range guard then synchronises per micro-batch."""
        _native.require_cuda(x_0, noise, noise_index)
        if x_0.dim() < 2:
            raise ValueError("x_0 must be [N, ..., T]")
        if seed is None:
            seed = fresh_seed()
        x0 = x_0.detach().to(torch.float32).contiguous()
        if ts is None:
            ts = self.draw_ts(x0.shape[0], seed, clip_offset)
        ts = ts.detach().to(device=x0.device, dtype=torch.float32).contiguous()
        if ts.dim() != 1 or ts.numel() < 1:
            raise ValueError(f"ts must be a non-empty vector, got shape {tuple(ts.shape)}")
        B, T = ts.numel(), x0[0].numel()
        if x0.shape[0] not in (1, B):
            raise ValueError(f"x_0 has {x0.shape[0]} rows: expected {B} (one per entry of ts) or 1")
        eps, eps_rows = None, 0
        if noise is not None:
            eps = noise.detach().to(torch.float32).contiguous()
            eps_rows = eps.shape[0]
            if eps_rows not in (1, B) or tuple(eps.shape[1:]) != tuple(x0.shape[1:]):
                raise ValueError(f"noise of shape {tuple(eps.shape)} does not match {B} (or 1) rows of {tuple(x0.shape[1:])}")
        idx = None
        if noise_index is not None:
            idx = noise_index.detach().to(device=x0.device, dtype=torch.int64).contiguous()
            if idx.shape != (B,):
                raise ValueError(f"expected noise_index of shape [{B}], got {tuple(idx.shape)}")
        # alpha_bar(t) on the HOST, as ddpm_sample evaluates its tables: the reference's float32 expressions on the CPU's own exp / cos
        if alpha is None:
            alpha = self.schedule(ts.cpu())
        alpha = alpha.detach().to(device=x0.device, dtype=torch.float32).contiguous()
        if alpha.shape != (B,):
            raise ValueError(f"expected alpha of shape [{B}], got {tuple(alpha.shape)}")
        x_t = torch.empty((B,) + tuple(x0.shape[1:]), device=x0.device, dtype=torch.float32)
        loss = torch.empty(B, device=x0.device, dtype=torch.float32)
        L = _native.lib()
        with torch.cuda.device(x0.device):
            _native.check(L.vqvs_ddpm_noise(x0.data_ptr(), x0.shape[0], alpha.data_ptr(), _native._ptr(eps), eps_rows, _native._ptr(idx),
                                            x_t.data_ptr(), B, T, int(seed), int(clip_offset), _native._stream_ptr()))
            with torch.no_grad():
                pred = predictor(x_t, ts, **predictor_kwargs)
            _native.require_cuda(pred)
            if tuple(pred.shape) != tuple(x_t.shape):
                raise ValueError(f"the predictor returned shape {tuple(pred.shape)} for an input of shape {tuple(x_t.shape)}")
            pred = pred.detach().to(torch.float32).contiguous()
            _native.check(L.vqvs_ddpm_sqerr(pred.data_ptr(), _native._ptr(eps), eps_rows, _native._ptr(idx), loss.data_ptr(), B, T,
                                            int(seed), int(clip_offset), _native._stream_ptr()))
        chk = predictor_check_status(predictor) if check else None  # range guard of a native predictor, as in check_sample
        if chk is not None:
            chk()
        return loss

    # ---- hot path -------------------------------------------------------------------------
    def ddpm_previous(
        self,
        x_t: torch.Tensor,
        ts: torch.Tensor,
        step,
        epsilon_prediction: torch.Tensor,
        noise: Optional[torch.Tensor] = None,
        sigma_large: bool = False,
        constrain: bool = False,
        cond_fn: Optional[Callable] = None,
        *,
        seed: int = 0,
        clip_offset: int = 0,
        step_index: int = 0,
        noise_scale: float = 1.0,
    ) -> torch.Tensor:
        """x_{t-step} ~ p(. | x_t) (reference diffusion.py:48-90).  `noise=None` draws from the
        in-kernel generator keyed by (seed, clip_offset + row, step_index)."""
        _native.require_cuda(x_t, epsilon_prediction, noise)
        ts = ts.detach().to(device=x_t.device, dtype=torch.float32)
        if not torch.is_tensor(step):
            step = torch.full_like(ts, float(step))
        step = step.to(ts)
        return self._step(x_t, epsilon_prediction, self.schedule(ts).contiguous(), self.schedule(ts - step).contiguous(), ts - step,
                          noise=noise, sigma_large=sigma_large, constrain=constrain, cond_fn=cond_fn, seed=seed, clip_offset=clip_offset,
                          step_index=step_index, noise_scale=noise_scale)

    def _step(self, x_t, epsilon_prediction, a_t, a_prev, ts_prev, *, noise, sigma_large, constrain, cond_fn, seed, clip_offset,
              step_index, noise_scale) -> torch.Tensor:
        """The reverse step given alpha_bar(t) and alpha_bar(t - step) as [B] device tensors."""
        if x_t.dim() < 2:
            raise ValueError("x_t must be [N, ..., T]")
        B = x_t.shape[0]
        T = x_t[0].numel()
        x = x_t.detach().to(torch.float32).contiguous()
        eps = epsilon_prediction.detach().to(torch.float32).contiguous()
        flags = (_native.DDPM_SIGMA_LARGE if sigma_large else 0) | (_native.DDPM_CONSTRAIN if constrain else 0)
        L = _native.lib()
        st = _native._stream_ptr()
        with torch.cuda.device(x.device):
            if cond_fn is not None:  # diffusion.py:80-83
                mean = torch.empty_like(x)
                _native.check(L.vqvs_ddpm_mean(x.data_ptr(), eps.data_ptr(), a_t.data_ptr(), a_prev.data_ptr(), mean.data_ptr(), B, T, st))
                grad = cond_fn(mean.view_as(x_t), ts_prev).detach().to(torch.float32).contiguous()
                eps2 = torch.empty_like(x)
                _native.check(L.vqvs_ddpm_guided_eps(x.data_ptr(), mean.data_ptr(), grad.data_ptr(), a_t.data_ptr(), a_prev.data_ptr(),
                                                     eps2.data_ptr(), B, T, flags, st))
                eps = eps2
            if noise is not None:
                noise = noise.detach().to(torch.float32).contiguous()
            out = torch.empty_like(x)
            _native.check(L.vqvs_ddpm_step(x.data_ptr(), eps.data_ptr(), _native._ptr(noise), a_t.data_ptr(), a_prev.data_ptr(),
                                           out.data_ptr(), B, T, flags, float(noise_scale), int(seed), int(clip_offset),
                                           int(step_index), st))
        return out.view_as(x_t)

    def step_tables(self, steps: int, B: int, schedule: Optional[Callable], device):
        """Per-step scalars of a sampling run, t = steps/steps ... 1/steps: the reference's float32 tensor expressions
        (diffusion.py:107-118, schedule.py:30-41), evaluated once on the HOST -- the same arithmetic as the CPU reference -- and
        uploaded as four [steps, B] tables (t, alpha_bar(t), alpha_bar(t - step), t - step), instead of ~20 device micro-kernels per
        step."""
        rows = []
        for t in [(i + 1) / steps for i in range(steps)][::-1]:
            ts = torch.tensor([t] * B, dtype=torch.float32)
            t_step = 1 / steps
            if schedule is not None:
                t_step = schedule(ts) - schedule(ts - 1 / steps)
                ts = schedule(ts)
            step = t_step if torch.is_tensor(t_step) else torch.full_like(ts, float(t_step))
            rows.append((ts, self.schedule(ts), self.schedule(ts - step), ts - step))
        return tuple(torch.stack([r[k] for r in rows]).to(torch.float32).contiguous().to(device) for k in range(4))

    @staticmethod
    def check_sample(predictor, x_t: torch.Tensor, what: str) -> None:
        """The end of a sampling run: the range guard of a native predictor (once per sample, not per step) and the sample's
        finiteness."""
        chk = predictor_check_status(predictor)
        if chk is not None:
            chk()
            # The library's guard sees the tensors that feed a GroupNorm.  The network's output and x_t are fp32 in every mode and cannot
            # overflow a storage type, but a non-finite value can still reach them (an inf / NaN in x_T, in the conditioning or in a
            # cond_fn's gradient): the finished sample is checked here, on the sync check_status() has just paid for.
            if not bool(torch.isfinite(x_t).all()):
                raise _native.NativeError(f"{what}: the sample holds non-finite values (a non-finite x_T, conditioning tensor or "
                                          "guidance gradient, or an overflow the range guard reported as a warning)")

    # ---- keep region (the replacement method; not in the reference): DESIGN.md section 3.11 -------------
    def keep_region(self, x: torch.Tensor, source: torch.Tensor, alpha, keep: Optional[torch.Tensor] = None, *,
                    noise: Optional[torch.Tensor] = None, noise_scale: float = 1.0, seed: int, clip_offset: int = 0,
                    index: int) -> torch.Tensor:
        """A copy of the state `x` [N, ..., T] whose kept samples (`keep` nonzero, bool or uint8 shaped like x; None: every sample)
        lie on the forward process of `source` at alpha_bar = `alpha` ([N] or one value): sqrt(alpha) source + sqrt(1 - alpha) z
        (`vqvs_keep_region`).  `noise=None` draws z from the generator's stream 3 keyed by (seed, clip_offset + row, index); a sampler
        passes the number of the step that will consume the state as `index`.  At alpha = 1 the kept samples are the source."""
        if x.dim() < 2:
            raise ValueError("x must be [N, ..., T]")
        source, keep = check_keep_args(x, source, keep, 0, 1)
        _native.require_cuda(x, source, keep, noise)
        if noise is not None:
            if tuple(noise.shape) != tuple(x.shape):
                raise ValueError(f"noise of shape {tuple(noise.shape)} does not match the state's {tuple(x.shape)}")
            noise = noise.detach().to(torch.float32).contiguous()
        if not torch.is_tensor(alpha):
            alpha = torch.full((x.shape[0],), float(alpha), dtype=torch.float32)
        alpha = alpha.detach().to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
        if alpha.numel() == 1:
            alpha = alpha.expand(x.shape[0]).contiguous()
        if alpha.shape != (x.shape[0],):
            raise ValueError(f"alpha must hold one value or one per row ({x.shape[0]}), got {alpha.numel()}")
        out = x.detach().to(torch.float32).contiguous().clone()
        self._keep_(out, source, keep, alpha, noise=noise, noise_scale=noise_scale, seed=seed, clip_offset=clip_offset, index=index)
        return out.view_as(x)

    @staticmethod
    def _keep_(x, source, keep, alpha, *, noise=None, noise_scale=1.0, seed, clip_offset, index) -> None:
        """`vqvs_keep_region` IN PLACE on a contiguous float32 state the caller owns; alpha is a [B] device tensor."""
        B, T = x.shape[0], x[0].numel()
        with torch.cuda.device(x.device):
            _native.check(_native.lib().vqvs_keep_region(x.data_ptr(), source.data_ptr(), _native._ptr(keep), _native._ptr(noise),
                                                         alpha.data_ptr(), B, T, float(noise_scale), int(seed), int(clip_offset), int(index),
                                                         _native._stream_ptr()))

    def _keep_start(self, x_T, source, keep, alpha, *, start_step, seed, clip_offset) -> torch.Tensor:
        """The state a run with `source` starts from: the source noised to the first step's alpha_bar (start_step > 0; x_T is not
        used), or x_T with its kept samples replaced."""
        if start_step > 0:
            x, keep = torch.empty_like(source), None
        elif keep is None:
            return x_T
        else:
            x = x_T.detach().to(torch.float32).contiguous().clone()
        self._keep_(x, source, keep, alpha, seed=seed, clip_offset=clip_offset, index=start_step)
        return x.view_as(x_T)

    # ---- the sampling loop of ddpm_sample, ddim_sample, dpmpp_sample and their window forms (longform.py) --------------
    def _sample(self, what: str, layout, x_T: torch.Tensor, steps: int, *, schedule, noise: NoiseSource, seed, clip_offset, progress, source,
                keep, start_step) -> torch.Tensor:
        """The one reverse loop.  `layout` (`_Clips` here, `longform._Windows`) holds the state, calls the predictor and cond_fn and
        launches its form of the kernels of `layout.rule` (`_Ddpm` / `_Ddim` / `_Dpmpp`); everything the entry points share is here: the
        `source` / `keep` / `start_step` checks, the default seed, the few-steps promotion and warning, the tables, steps
        start_step .. steps - 1 with no noise on the last one, the keep region at the alpha_bar stepped to, the final guard."""
        source, keep = check_keep_args(x_T, source, keep, start_step, steps)
        _native.require_cuda(x_T, source, keep)
        rows = layout.rows(x_T)
        if seed is None:
            seed = fresh_seed()
        key = dict(seed=seed, clip_offset=clip_offset)
        rule, predictor, cond_fn = layout.rule, layout.predictor, layout.cond_fn
        stack = few_guided_steps_promotion(what, steps, predictor, cond_fn, stacklevel=4)  # (4: the caller of the entry point)
        with stack if stack is not None else contextlib.nullcontext():
            if rule.name != "ddpm":
                warn_few_unguided_steps(what, steps, predictor, cond_fn, stacklevel=4)
            tables = self.step_tables(steps, rows, schedule, x_T.device)  # t, alpha_bar(t), alpha_bar(t - step), t - step
            x_t = layout.start(x_T, source, keep, tables[1][start_step], start_step=start_step, **key)
            with torch.no_grad(), torch.cuda.device(x_T.device):
                for i in _progress(range(start_step, steps), progress):
                    last = i + 1 == steps
                    eps = layout.predict(x_t, tables, i)
                    nz = None
                    if not last and noise is not None and rule.draws_noise:
                        nz = noise(i) if callable(noise) else noise[i]
                    x_t = layout.step(x_t, eps, nz, tables, i, noise_scale=0.0 if last else 1.0, **key)
                    if keep is not None:  # (the step's output is a fresh float32 tensor of this loop's)
                        layout.keep(x_t, source, keep, tables[2][i], index=i + 1, **key)
            x_t = x_t.view_as(x_T)
            self.check_sample(predictor, x_t, what)
        return x_t

    def ddpm_sample_windows(self, x_T_long: torch.Tensor, predictor: Callable, steps: int, **kwargs) -> torch.Tensor:
        """`ddpm_sample` for one long state [1,1,Np] predicted through overlapping windows (longform.ddpm_sample_windows)."""
        from .longform import ddpm_sample_windows

        return ddpm_sample_windows(self, x_T_long, predictor, steps, **kwargs)

    def ddpm_sample(
        self,
        x_T: torch.Tensor,
        predictor: Callable[[torch.Tensor, torch.Tensor], torch.Tensor],
        steps: int,
        progress: bool = False,
        sigma_large: bool = False,
        constrain: bool = False,
        cond_fn: Optional[Callable] = None,
        schedule: Optional[Callable] = None,
        *,
        noise: NoiseSource = None,
        seed: Optional[int] = None,
        clip_offset: int = 0,
        source: Optional[torch.Tensor] = None,
        keep: Optional[torch.Tensor] = None,
        start_step: int = 0,
    ) -> torch.Tensor:
        """Reverse diffusion from x_T (reference diffusion.py:92-133): t runs steps/steps ... 1/steps,
        optional sample-time remap `schedule`, zero noise on the last iteration.

        `source` (shaped like x_T) with `keep` (bool / uint8, shaped like x_T) keeps the masked samples of the source: before the
        first step and after every step they are put back on the source's forward process at the alpha_bar the state has just
        reached (`keep_region`, indexed by the step that consumes the state), so the result holds the source there, bit for bit.
        `start_step` > 0 runs steps start_step .. steps - 1 of the same tables from the source noised to a_t[start_step], instead
        of from x_T.  Step numbers, and with them the step noise, are unchanged."""
        return self._sample("ddpm_sample", _Clips(self, _Ddpm(sigma_large, constrain), predictor, cond_fn), x_T, steps, schedule=schedule,
                            noise=noise, seed=seed, clip_offset=clip_offset, progress=progress, source=source, keep=keep,
                            start_step=start_step)

    # ---- DDIM (Song et al. 2020; not in the reference): DESIGN.md section 3.10 -----------------------
    def ddim_previous(
        self,
        x_t: torch.Tensor,
        ts: torch.Tensor,
        step,
        epsilon_prediction: torch.Tensor,
        noise: Optional[torch.Tensor] = None,
        eta: float = 0.0,
        constrain: bool = False,
        cond_fn: Optional[Callable] = None,
        *,
        seed: int = 0,
        clip_offset: int = 0,
        step_index: int = 0,
        noise_scale: float = 1.0,
    ) -> torch.Tensor:
        """The DDIM step from ts to ts - step (`vqvs_ddim_step`): deterministic at eta = 0, the small-sigma `ddpm_previous` at
        eta = 1.  `cond_fn(x_t, ts)` -- the callable the DDPM path takes -- is evaluated AT (x_t, ts) and its result handed to the
        kernel, which subtracts sqrt(1 - alpha_bar(ts)) times it from the prediction.  `noise=None` draws from the in-kernel
        generator keyed by (seed, clip_offset + row, step_index), the words `ddpm_previous` draws."""
        _native.require_cuda(x_t, epsilon_prediction, noise)
        ts = ts.detach().to(device=x_t.device, dtype=torch.float32)
        if not torch.is_tensor(step):
            step = torch.full_like(ts, float(step))
        step = step.to(ts)
        return self._ddim_step(x_t, epsilon_prediction, self.schedule(ts).contiguous(), self.schedule(ts - step).contiguous(), ts,
                               noise=noise, eta=eta, constrain=constrain, cond_fn=cond_fn, seed=seed, clip_offset=clip_offset,
                               step_index=step_index, noise_scale=noise_scale)

    def _ddim_step(self, x_t, epsilon_prediction, a_t, a_to, ts, *, noise=None, eta=0.0, constrain=False, cond_fn=None, invert=False,
                   seed=0, clip_offset=0, step_index=0, noise_scale=1.0) -> torch.Tensor:
        """One `vqvs_ddim_step` given alpha_bar of the time the state is at and of the time stepped to, as [B] device tensors."""
        if x_t.dim() < 2:
            raise ValueError("x_t must be [N, ..., T]")
        B = x_t.shape[0]
        T = x_t[0].numel()
        x = x_t.detach().to(torch.float32).contiguous()
        eps = epsilon_prediction.detach().to(torch.float32).contiguous()
        flags = (_native.DDIM_CONSTRAIN if constrain else 0) | (_native.DDIM_INVERT if invert else 0)
        with torch.cuda.device(x.device):
            grad = None
            if cond_fn is not None:
                grad = cond_fn(x.view_as(x_t), ts).detach().to(torch.float32).contiguous()
                _native.require_cuda(grad)
                if grad.numel() != x.numel():
                    raise ValueError(f"cond_fn returned shape {tuple(grad.shape)} for a state of shape {tuple(x_t.shape)}")
            if noise is not None:
                noise = noise.detach().to(torch.float32).contiguous()
            out = torch.empty_like(x)
            _native.check(_native.lib().vqvs_ddim_step(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(noise), a_t.data_ptr(),
                                                       a_to.data_ptr(), out.data_ptr(), B, T, flags, float(eta), float(noise_scale),
                                                       int(seed), int(clip_offset), int(step_index), _native._stream_ptr()))
        return out.view_as(x_t)

    def ddim_sample(
        self,
        x_T: torch.Tensor,
        predictor: Callable[[torch.Tensor, torch.Tensor], torch.Tensor],
        steps: int,
        eta: float = 0.0,
        progress: bool = False,
        constrain: bool = False,
        cond_fn: Optional[Callable] = None,
        schedule: Optional[Callable] = None,
        *,
        noise: NoiseSource = None,
        seed: Optional[int] = None,
        clip_offset: int = 0,
        source: Optional[torch.Tensor] = None,
        keep: Optional[torch.Tensor] = None,
        start_step: int = 0,
    ) -> torch.Tensor:
        """`ddpm_sample` with the DDIM step: the same tables of t and alpha_bar(t) (`step_tables`), the same step numbering and noise
        words, zero noise on the last iteration -- which, stepping to alpha_bar(0) = 1, returns x0 itself.  At eta = 0 the result
        depends on x_T alone -- and, with `source` / `keep` / `start_step` (as in `ddpm_sample`; the kept samples are replaced at the
        alpha_bar stepped TO), on the seed of the replacement noise."""
        return self._sample("ddim_sample", _Clips(self, _Ddim(eta, constrain), predictor, cond_fn), x_T, steps, schedule=schedule,
                            noise=noise, seed=seed, clip_offset=clip_offset, progress=progress, source=source, keep=keep,
                            start_step=start_step)

    def ddim_invert(self, x_0: torch.Tensor, predictor: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], steps: int,
                    schedule: Optional[Callable] = None, progress: bool = False) -> torch.Tensor:
        """x_0 -> the x_T that `ddim_sample(x_T, predictor, steps, eta=0)` maps back towards it: the rows of `step_tables` walked
        BACKWARDS.  Iteration j takes the row of t = (j + 1) / steps, evaluates the predictor at the row's t - step -- where the state
        is -- and steps from alpha_bar(t - step) to alpha_bar(t) with VQVS_DDIM_INVERT.  Each step inverts the forward one exactly for a
        FIXED prediction; the forward run predicts at t, not at t - step, so a round trip returns x_0 only up to that discretisation
        error."""
        x_t = x_0
        _, a_t_all, a_prev_all, ts_prev_all = self.step_tables(steps, x_0.shape[0], schedule, x_0.device)
        for i in _progress(range(steps - 1, -1, -1), progress):
            with torch.no_grad():
                eps = predictor(x_t, ts_prev_all[i])
                x_t = self._ddim_step(x_t, eps, a_prev_all[i], a_t_all[i], ts_prev_all[i], invert=True)
        self.check_sample(predictor, x_t, "ddim_invert")
        return x_t

    def ddim_sample_windows(self, x_T_long: torch.Tensor, predictor: Callable, steps: int, **kwargs) -> torch.Tensor:
        """`ddim_sample` for one long state [1,1,Np] predicted through overlapping windows (longform.ddim_sample_windows)."""
        from .longform import ddim_sample_windows

        return ddim_sample_windows(self, x_T_long, predictor, steps, **kwargs)


    # ---- DPM-Solver++(2M) (Lu et al. 2022; not in the reference): DESIGN.md section 3.12 -----------------------
    def dpmpp_previous(
        self,
        x_t: torch.Tensor,
        ts: torch.Tensor,
        step,
        epsilon_prediction: torch.Tensor,
        x0_prev: Optional[torch.Tensor] = None,
        ts_from: Optional[torch.Tensor] = None,
        constrain: bool = False,
        cond_fn: Optional[Callable] = None,
    ):
        """The DPM-Solver++(2M) step from ts to ts - step (`vqvs_dpmpp_step`): returns (x_to, x0), x0 being the guided, constrained
        data prediction the step formed -- the `x0_prev` of the next call, with this call's `ts` as its `ts_from`.  Without both the
        step is first order: the eta = 0 `ddim_previous`.  `cond_fn(x_t, ts)` is evaluated AT (x_t, ts), as there.  No noise is
        drawn.  alpha_bar is evaluated on the HOST, as `step_tables` evaluates it, so the calls of a run chained by hand reproduce
        `dpmpp_sample` bit for bit (a `ts` on the device costs one copy back)."""
        _native.require_cuda(x_t, epsilon_prediction, x0_prev)
        ts_host = ts.detach().to(device="cpu", dtype=torch.float32)
        if not torch.is_tensor(step):
            step = torch.full_like(ts_host, float(step))
        step = step.detach().to(ts_host)

        def alpha(t):
            return self.schedule(t).to(device=x_t.device, dtype=torch.float32).contiguous()

        a_from = None
        if x0_prev is not None and ts_from is not None:
            if not torch.is_tensor(ts_from):
                ts_from = torch.full_like(ts_host, float(ts_from))
            a_from = alpha(ts_from.detach().to(ts_host))
        return self._dpmpp_step(x_t, epsilon_prediction, a_from, alpha(ts_host), alpha(ts_host - step), ts_host.to(x_t.device),
                                x0_prev=x0_prev if a_from is not None else None, constrain=constrain, cond_fn=cond_fn)

    def _dpmpp_step(self, x_t, epsilon_prediction, a_from, a_t, a_to, ts, *, x0_prev=None, constrain=False, cond_fn=None):
        """One `vqvs_dpmpp_step` given alpha_bar of the step before (None: no history), of the time the state is at and of the time
        stepped to, as [B] device tensors: (x_to, x0), both fresh tensors shaped like x_t."""
        if x_t.dim() < 2:
            raise ValueError("x_t must be [N, ..., T]")
        B = x_t.shape[0]
        T = x_t[0].numel()
        x = x_t.detach().to(torch.float32).contiguous()
        eps = epsilon_prediction.detach().to(torch.float32).contiguous()
        if eps.numel() != x.numel():
            raise ValueError(f"the prediction has shape {tuple(epsilon_prediction.shape)} for a state of shape {tuple(x_t.shape)}")
        if a_from is None or x0_prev is None:
            a_from = x0_prev = None
        else:
            x0_prev = x0_prev.detach().to(torch.float32).contiguous()
            if x0_prev.numel() != x.numel():
                raise ValueError(f"x0_prev of shape {tuple(x0_prev.shape)} does not match the state's {tuple(x_t.shape)}")
        with torch.cuda.device(x.device):
            grad = None
            if cond_fn is not None:
                grad = cond_fn(x.view_as(x_t), ts).detach().to(torch.float32).contiguous()
                _native.require_cuda(grad)
                if grad.numel() != x.numel():
                    raise ValueError(f"cond_fn returned shape {tuple(grad.shape)} for a state of shape {tuple(x_t.shape)}")
            out, x0 = torch.empty_like(x), torch.empty_like(x)
            _native.check(_native.lib().vqvs_dpmpp_step(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(x0_prev),
                                                        _native._ptr(a_from), a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), x0.data_ptr(),
                                                        B, T, _native.DDIM_CONSTRAIN if constrain else 0, _native._stream_ptr()))
        return out.view_as(x_t), x0.view_as(x_t)

    def dpmpp_sample(
        self,
        x_T: torch.Tensor,
        predictor: Callable[[torch.Tensor, torch.Tensor], torch.Tensor],
        steps: int,
        progress: bool = False,
        constrain: bool = False,
        cond_fn: Optional[Callable] = None,
        schedule: Optional[Callable] = None,
        *,
        noise: NoiseSource = None,
        seed: Optional[int] = None,
        clip_offset: int = 0,
        source: Optional[torch.Tensor] = None,
        keep: Optional[torch.Tensor] = None,
        start_step: int = 0,
    ) -> torch.Tensor:
        """`ddim_sample` at eta = 0 with the DPM-Solver++(2M) step: the same tables, one forward per step, and the previous step's x0
        prediction as the only extra state.  The first executed step (step `start_step`) has no history and is first order -- the DDIM
        step --, and so is the last one, which steps to alpha_bar(0) = 1 and returns x0.  The result depends on x_T alone: `noise` is
        accepted and never asked for anything, and `seed` only feeds the replacement noise of `source` / `keep` / `start_step` (as in
        `ddpm_sample`; the history holds x0 predictions and is not touched by the replacement)."""
        return self._sample("dpmpp_sample", _Clips(self, _Dpmpp(constrain), predictor, cond_fn), x_T, steps, schedule=schedule,
                            noise=noise, seed=seed, clip_offset=clip_offset, progress=progress, source=source, keep=keep,
                            start_step=start_step)

    def dpmpp_sample_windows(self, x_T_long: torch.Tensor, predictor: Callable, steps: int, **kwargs) -> torch.Tensor:
        """`dpmpp_sample` for one long state [1,1,Np] predicted through overlapping windows (longform.dpmpp_sample_windows)."""
        from .longform import dpmpp_sample_windows

        return dpmpp_sample_windows(self, x_T_long, predictor, steps, **kwargs)


class _Ddpm:
    """The DDPM step rule of `Diffusion._sample`: `vqvs_ddpm_step`, guided -- inside `Diffusion._step` -- by `cond_fn(mean, t - step)`
    between `vqvs_ddpm_mean` and `vqvs_ddpm_guided_eps`."""
    name, draws_noise = "ddpm", True

    def __init__(self, sigma_large: bool, constrain: bool):
        self.sigma_large, self.constrain = sigma_large, constrain
        self.flags = (_native.DDPM_SIGMA_LARGE if sigma_large else 0) | (_native.DDPM_CONSTRAIN if constrain else 0)

    def step(self, diffusion, x_t, eps, tables, i, **kw):
        _, a_t, a_prev, ts_prev = tables
        return diffusion._step(x_t, eps, a_t[i], a_prev[i], ts_prev[i], sigma_large=self.sigma_large, constrain=self.constrain, **kw)


class _Ddim:
    """The DDIM step rule: `vqvs_ddim_step` at `eta` (0: no noise is drawn or asked for), guided by `cond_fn(x_t, t)` handed to the
    kernel."""
    name = "ddim"

    def __init__(self, eta: float, constrain: bool):
        self.eta, self.constrain, self.draws_noise = eta, constrain, bool(eta)
        self.flags = _native.DDIM_CONSTRAIN if constrain else 0

    def step(self, diffusion, x_t, eps, tables, i, **kw):
        ts, a_t, a_to, _ = tables
        return diffusion._ddim_step(x_t, eps, a_t[i], a_to[i], ts[i], eta=self.eta, constrain=self.constrain, **kw)


class _Dpmpp:
    """The DPM-Solver++(2M) step rule: `vqvs_dpmpp_step`, guided as the DDIM rule is.  It owns the multistep history -- the x0 the
    previous step wrote (clips: shaped like the state; windows: the blended x0 of the long row) and that step's alpha_bar(t).  Every
    entry point builds a rule of its own, so a run starts with none: its first step, whatever `start_step`, is first order."""
    name, draws_noise = "dpmpp", False

    def __init__(self, constrain: bool):
        self.constrain = constrain
        self.flags = _native.DDIM_CONSTRAIN if constrain else 0
        self.x0_prev = self.a_from = None

    def step(self, diffusion, x_t, eps, tables, i, *, cond_fn=None, **noise_keys):
        ts, a_t, a_to, _ = tables  # (noise, seed, clip_offset, step_index and noise_scale belong to drawn noise: there is none)
        x_to, self.x0_prev = diffusion._dpmpp_step(x_t, eps, self.a_from, a_t[i], a_to[i], ts[i], x0_prev=self.x0_prev,
                                                   constrain=self.constrain, cond_fn=cond_fn)
        self.a_from = a_t[i]
        return x_to


class _Clips:
    """The state layout of `ddpm_sample` / `ddim_sample` / `dpmpp_sample`: a batch of clips [B, ..., T], predicted and stepped whole."""

    def __init__(self, diffusion: Diffusion, rule, predictor: Callable, cond_fn: Optional[Callable]):
        self.diffusion, self.rule, self.predictor, self.cond_fn = diffusion, rule, predictor, cond_fn

    def rows(self, x_T) -> int:
        return x_T.shape[0]

    def start(self, x_T, source, keep, alpha, **kw):
        return x_T if source is None else self.diffusion._keep_start(x_T, source, keep, alpha, **kw)

    def predict(self, x_t, tables, i):
        return self.predictor(x_t, tables[0][i])

    def step(self, x_t, eps, nz, tables, i, **kw):
        _native.require_cuda(eps, nz)
        return self.rule.step(self.diffusion, x_t, eps, tables, i, noise=nz, cond_fn=self.cond_fn, step_index=i, **kw)

    def keep(self, x_t, source, keep, alpha, **kw) -> None:
        self.diffusion._keep_(x_t, source, keep, alpha, **kw)


def guidance_mix(outs: torch.Tensor, reps: int, s1: float = 0.0, s2: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`vqvs_guidance_mix` on the predictor's output `outs` [reps * n, ...] of a reps-fold batch (block 0 the fully conditioned
    prediction): base + s1 * (base - block 1) + s2 * (base - block 2), every operation rounded on its own -- bit for bit what those
    tensor expressions give.  Written into `out` [n, ...] (contiguous float32), or -- None -- IN PLACE over block 0 of a contiguous
    float32 `outs` (a copy of anything else); the [n, ...] result is returned."""
    _native.require_cuda(outs, out)
    reps = int(reps)
    if reps < 1 or outs.dim() < 2 or outs.shape[0] < reps or outs.shape[0] % reps or not outs[0].numel():
        raise ValueError(f"outs of shape {tuple(outs.shape)} is not a {reps}-fold batch of rows")
    outs = outs.detach().to(torch.float32).contiguous()
    n = outs.shape[0] // reps
    if out is None:
        out = outs[:n]
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, *outs.shape[1:]):
        raise ValueError(f"out must be contiguous float32 of shape {(n, *outs.shape[1:])}, got {out.dtype} {tuple(out.shape)}")
    with torch.cuda.device(outs.device):
        _native.check(_native.lib().vqvs_guidance_mix(outs.data_ptr(), out.data_ptr(), n, outs[0].numel(), reps, float(s1), float(s2),
                                                      _native._stream_ptr()))
    return out


def randn_clips(n: int, T: int, device, seed: int, clip_offset: int = 0, stream_id: int = 1) -> torch.Tensor:
    """x_T ~ N(0,1) of shape [n,1,T] from the counter-based generator (keyed by global clip index)."""
    out = torch.empty(n, 1, T, device=device, dtype=torch.float32)
    _native.require_cuda(out)
    with torch.cuda.device(out.device):
        _native.check(_native.lib().vqvs_randn(out.data_ptr(), n, T, int(seed), int(clip_offset), int(stream_id), _native._stream_ptr()))
    return out
