#!/usr/bin/env python3
"""
Evaluate a noised-audio speaker classifier checkpoint over a data set on MI355X: the negative log-likelihood of the label, the
accuracy and the top-k accuracy on `sample_q(audio, ts)`, per quartile of t and overall -- the number the reference only logs
while it trains (`ClassifierTrainLoop.compute_losses`, train_loop.py:551-561, averaged per quartile by its LossTracker), and the
one `stat_generate.py`'s class score and every classifier-guided run rest on.

One pass over the shuffled loader.  Per batch: ts from `Diffusion.draw_ts` (or the fixed `--t`; `--t 0` is the setting
stat_generate.py reads features at), `Diffusion.sample_q_seeded` (noise drawn in the noising kernel, keyed by the seed and the
clip's position in the pass), `Classifier.scores` (the HIP forward, then one fused scoring kernel: NLL, top-1, top-k and
confusion counts from one pass over the logits).  After every batch one line:

    {n} samples: nll_q0=... nll_q3=... acc_q0=... acc_q3=... top5_q0=... top5_q3=... nll=... acc=...

nll_q* / acc_q* / top5_q* are the per-quartile-of-t averages of the clips' NLL, top-1 and top-k hits (`LossTracker`, window
10^6); nll and acc are over every clip so far and EXACT: the float64 clip sums are added as fractions and the hits are integers,
so the line does not depend on the batch size or the rank count.  `--confusion-path` writes the [num_labels, num_labels] matrix
of (label, prediction) counts as .npy.

`data_dir`, `--precision`, `--seed`, `--max-samples` and `--dist-backend` are the common parser's and the pass is the shared one
(vq_voice_swap_amd/eval_pass.py).  Under torchrun (WORLD_SIZE > 1) batches are dealt round-robin, rank 0 merges the states and
prints the one final line.
"""
import os
import sys
from fractions import Fraction

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import Classifier, Diffusion, LossTracker, make_schedule  # noqa: E402
from vq_voice_swap_amd.eval_pass import common_parser, format_line, run_pass  # noqa: E402,F401


def arg_parser():
    p = common_parser()
    p.add_argument("--schedule", default="exp", type=str, help="noise schedule the classifier was trained with")
    p.add_argument("--t", default=None, type=float, help="evaluate every clip at this fixed t in [0, 1] (default: uniform draws)")
    p.add_argument("--topk", default=5, type=int, help="k of the top-k accuracy (clipped to the number of labels)")
    p.add_argument("--confusion-path", default=None, type=str, help="write the (label, prediction) count matrix here as .npy")
    return p


class EvalState:
    """What one pass accumulates: the three trackers, the clip count, the summed NLL with the position count behind it, the hit
    counts, and (optionally) the confusion matrix (int64, on the device the batches run on)."""

    def __init__(self, num_classes: int, device, topk: int = 5, confusion: bool = True):
        self.topk = max(1, min(int(topk), int(num_classes)))
        self.nll = LossTracker(avg_size=1_000_000, prefix="nll_")
        self.acc = LossTracker(avg_size=1_000_000, prefix="acc_")
        self.top = LossTracker(avg_size=1_000_000, prefix=f"top{self.topk}_")
        self.num_samples = 0
        self.nll_sum = Fraction(0)  # EXACT sum of the clips' float64 sums: the same whatever order batches and shards arrive in
        self.positions = 0    # scored positions behind it (one per clip for a classifier)
        self.correct = 0      # positions whose target is the first maximum
        self.topk_correct = 0
        self.confusion = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=device) if confusion else None

    def ts_for(self, diffusion: Diffusion, n: int, first: int, seed: int, t=None) -> torch.Tensor:
        return diffusion.draw_ts(n, seed, first) if t is None else torch.full((n,), float(t), dtype=torch.float32)

    def add_scores(self, ts: torch.Tensor, out) -> None:
        """Fold in one batch's `classification_scores` result."""
        L = int(out["positions"])
        nll, top1, topk = out["nll"].tolist(), out["top1"].tolist(), out["topk"].tolist()
        self.nll.add(ts, [v / L for v in nll])
        self.acc.add(ts, [v / L for v in top1])
        self.top.add(ts, [v / L for v in topk])
        self.num_samples += len(nll)
        self.nll_sum += sum(Fraction(v) for v in nll)
        self.positions += L * len(nll)
        self.correct += sum(top1)
        self.topk_correct += sum(topk)

    def add_batch(self, model, diffusion: Diffusion, audio: torch.Tensor, targets: torch.Tensor, first: int, seed: int, t=None) -> None:
        """Score one batch whose first clip is clip `first` of the pass."""
        ts = self.ts_for(diffusion, len(audio), first, seed, t)
        x_t = diffusion.sample_q_seeded(audio, ts, seed=seed, clip_offset=first)
        self.add_scores(ts, model.scores(x_t, ts.to(audio.device), targets, topk=self.topk, confusion=self.confusion))

    def merge(self, other: "EvalState") -> "EvalState":
        self.nll.merge(other.nll)
        self.acc.merge(other.acc)
        self.top.merge(other.top)
        self.num_samples += other.num_samples
        self.nll_sum += other.nll_sum
        self.positions += other.positions
        self.correct += other.correct
        self.topk_correct += other.topk_correct
        if self.confusion is not None:
            self.confusion += other.confusion.to(self.confusion.device)
        return self

    def to_host(self) -> "EvalState":
        if self.confusion is not None:
            self.confusion = self.confusion.cpu()
        return self

    def log_dict(self):
        log = dict(self.nll.log_dict())
        log.update(self.acc.log_dict())
        log.update(self.top.log_dict())
        log["nll"] = float(self.nll_sum / self.positions) if self.positions else 0.0
        log["acc"] = float(Fraction(self.correct, self.positions)) if self.positions else 0.0
        return log


def main(argv=None):
    args = arg_parser().parse_args(argv)
    if args.t is not None and not 0.0 <= args.t <= 1.0:
        raise SystemExit(f"--t {args.t} is outside [0, 1]")
    diffusion = Diffusion(make_schedule(args.schedule))

    def build(device, num_labels):
        model = Classifier.load(args.checkpoint_path).to(device)
        assert model.num_labels == num_labels, f"the model has {model.num_labels} labels, the data {num_labels}"
        model.eval().set_precision(args.precision)
        state = EvalState(model.num_labels, device, args.topk)
        return state, lambda audio, data_batch, first: state.add_batch(model, diffusion, audio, data_batch["label"].to(device), first, args.seed, args.t)

    merged = run_pass(args, build, no_device="the guidance models have no CPU path")
    if merged is not None and args.confusion_path:
        import numpy as np

        np.save(args.confusion_path, merged.confusion.cpu().numpy())


if __name__ == "__main__":
    main()
