#!/usr/bin/env python3
"""
Evaluate a VQ-VAE checkpoint over a data set on MI355X: how well the codebook fits the encoder (vq_loss), how many codes are
alive (used_codes, perplexity), and how much the decoder leverages labels -- how much worse the noise-prediction loss becomes
when the label is randomised (the purpose and the command line of the reference's eval_vqvae.py: `--batch-size`,
`checkpoint_path`, `data_dir`; its body imports classes the reference no longer has, so only those are taken from it).

One pass over the shuffled loader.  Per batch: `VQVAE.losses` with the true labels (encoder, one fused quantise-and-score
kernel, fused noising / squared-error kernels around the HIP decoder), then the decoder half again on the SAME x_t -- same t,
same noise -- with a wrong label per clip, (label + r) % num_labels with r uniform in 1 .. num_labels - 1: never the true one.
After every batch one line:

    {n} samples: cond_q0=... cond_q3=... rand_q0=... rand_q3=... vq_loss=... used_codes=... perplexity=...

cond_q* / rand_q* are the per-quartile-of-t averages with the true / wrong labels (`LossTracker`, window 10^6; rand_* is left
out when the model has fewer than two labels), vq_loss the StandardVQLoss over every clip so far, used_codes and perplexity
those of the accumulated code histogram.  The reference's per-quartile output-std hook is not rebuilt: it measured a module
that no longer exists.

`data_dir`, `--precision`, `--seed`, `--max-samples` and `--dist-backend` are the common parser's and the pass is the shared one
(vq_voice_swap_amd/eval_pass.py): everything random is keyed by the seed and the clip's position in the shuffled pass, so the
result does not depend on the rank count.  Under torchrun (WORLD_SIZE > 1) batches are dealt round-robin, rank 0 merges the
trackers, adds the histograms and the error sums, and prints the one final line.
"""
import os
import sys
from fractions import Fraction

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import LossTracker, StandardVQLoss, VQVAE, code_usage  # noqa: E402
from vq_voice_swap_amd.eval_pass import common_parser, format_line, run_pass  # noqa: E402,F401


def arg_parser():
    return common_parser()


def wrong_labels(labels: torch.Tensor, num_labels: int, seed: int, first: int) -> torch.Tensor:
    """(label + r) % num_labels with r uniform in 1 .. num_labels - 1 from a host generator seeded by (seed, first): in range,
    never the label itself, the same for the same (seed, first)."""
    if num_labels < 2:
        raise ValueError("a wrong label needs at least two labels")
    g = torch.Generator().manual_seed((int(seed) * 0xD1B54A32D192ED03 + 0x9E3779B97F4A7C15 * (int(first) + 1) + 0x5851F42D4C957F2D) % (2 ** 63))
    r = torch.randint(1, num_labels, (len(labels),), generator=g)
    return ((labels.detach().cpu().to(torch.int64) + r) % num_labels).to(labels.device)


class EvalState:
    """What one pass accumulates: the two trackers, the clip count, the summed quantisation error with its element count, and
    the code histogram (int64, on the device the batches run on)."""

    def __init__(self, num_codes: int, device, commitment: float = 0.25):
        self.cond = LossTracker(avg_size=1_000_000, prefix="cond_")
        self.rand = LossTracker(avg_size=1_000_000, prefix="rand_")
        self.loss_fn = StandardVQLoss(commitment)
        self.num_samples = 0
        self.sq_err = Fraction(0)  # EXACT sum of the clips' float64 sums: the same whatever order batches and shards arrive in
        self.numel = 0      # encoder-output elements behind it
        self.hist = torch.zeros(num_codes, dtype=torch.int64, device=device)

    def add_batch(self, model: VQVAE, audio: torch.Tensor, labels, first: int, seed: int) -> None:
        """Score one batch whose first clip is clip `first` of the pass."""
        n = len(audio)
        ts = model.diffusion.draw_ts(n, seed, first)
        out = model.losses(self.loss_fn, audio, labels, ts=ts, seed=seed, clip_offset=first, hist=self.hist)
        self.cond.add(out["ts"], out["mses"])
        if labels is not None and (model.num_labels or 0) > 1:
            wrong = wrong_labels(labels, model.num_labels, seed, first)
            self.rand.add(ts, model.diffusion.denoising_losses(audio, model.predictor, ts, seed=seed, clip_offset=first,
                                                               cond=out["embedded"], labels=wrong))
        self.num_samples += n
        self.sq_err += sum(Fraction(v) for v in out["sq_err"].tolist())
        self.numel += out["embedded"].numel()

    def merge(self, other: "EvalState") -> "EvalState":
        self.cond.merge(other.cond)
        self.rand.merge(other.rand)
        self.num_samples += other.num_samples
        self.sq_err += other.sq_err
        self.numel += other.numel
        self.hist += other.hist.to(self.hist.device)
        return self

    def to_host(self) -> "EvalState":
        self.hist = self.hist.cpu()
        return self

    def log_dict(self):
        log = dict(self.cond.log_dict())
        log.update(self.rand.log_dict())
        log["vq_loss"] = float(self.loss_fn.from_sq_err(float(self.sq_err), self.numel)) if self.numel else 0.0
        log.update(code_usage(self.hist))
        return log


def main(argv=None):
    args = arg_parser().parse_args(argv)

    def build(device, num_labels):
        model = VQVAE.load(args.checkpoint_path).to(device)
        assert model.num_labels == num_labels, f"the model has {model.num_labels} labels, the data {num_labels}"
        model.eval().set_precision(args.precision)
        state = EvalState(model.vq.num_codes, device)
        return state, lambda audio, data_batch, first: state.add_batch(model, audio, data_batch["label"].to(device), first, args.seed)

    run_pass(args, build, no_device="the encoder and the predictor have no CPU path")


if __name__ == "__main__":
    main()
