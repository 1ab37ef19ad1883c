#!/usr/bin/env python3
"""
Noise-prediction MSE of a diffusion model over a data set, averaged per quartile of t, on MI355X.  Counterpart of the
reference's eval_diffusion.py (same positionals and --batch-size, same output line after every batch:
"{n} samples: q0=... q1=..."; reference eval_diffusion.py:14-45): one pass over the shuffled loader, t uniform per clip,
`Diffusion.denoising_losses` (fused noising and squared-error kernels around the HIP UNet), a `LossTracker` of window 10^6.

Differences: `data_dir` is "tones" or a LibriSpeech-layout tree of WAV files; `--precision` (default fp32, the reference's
arithmetic); `--seed` fixes the loader's order, every clip's t and its noise (keyed by the clip's position in that order, so
the result does not depend on the rank count); `--max-samples` ends the pass early.  Under torchrun (WORLD_SIZE > 1) the
batches are dealt round-robin to the ranks, the trackers are merged on rank 0, and rank 0 prints the one final line: the pass
and the flags it shares with the other eval scripts are those of vq_voice_swap_amd/eval_pass.py.
"""
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402,F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import DiffusionModel, LossTracker  # noqa: E402
from vq_voice_swap_amd.eval_pass import common_parser, run_pass  # noqa: E402


def arg_parser():
    return common_parser()


class EvalState:
    """What one pass accumulates: the tracker and the clip count."""

    def __init__(self):
        self.tracker = LossTracker(avg_size=1_000_000)
        self.num_samples = 0

    def add(self, ts, losses) -> None:
        self.tracker.add(ts, losses)
        self.num_samples += len(ts)

    def merge(self, other: "EvalState") -> "EvalState":
        self.tracker.merge(other.tracker)
        self.num_samples += other.num_samples
        return self

    def to_host(self) -> "EvalState":
        return self  # (host values only)

    def log_dict(self):
        return self.tracker.log_dict()


def main(argv=None):
    args = arg_parser().parse_args(argv)

    def build(device, num_labels):
        model = DiffusionModel.load(args.checkpoint_path).to(device).eval().set_precision(args.precision)
        state = EvalState()

        def score(audio, data_batch, first):
            ts = model.diffusion.draw_ts(len(audio), args.seed, first)
            state.add(ts, model.diffusion.denoising_losses(audio, model.predictor, ts, seed=args.seed, clip_offset=first))

        return state, score

    run_pass(args, build, no_device="the predictor has no CPU path")


if __name__ == "__main__":
    main()
