#!/usr/bin/env python3
"""
Evaluate the finished voice conversion of a VQ-VAE checkpoint over a data set on MI355X: every clip is encoded, decoded under a
target label with the chosen sampler, and the result is scored against the source -- how many VQ codes survive the round trip,
and how far the converted spectrum lies from the source's (mel-cepstral distortion and log-mel spectral distance, frame for frame:
the conversion preserves timing, so nothing is aligned).  The numbers answer questions such as "is dpmpp at 25 steps as close to
ddpm at 100 as ddpm at 100 is to itself?"; they are an instrument, not a verdict on any sampler.

One pass over the shuffled loader.  Per batch: `VQVAE.encode`, `VQVAE.decode(codes, target, steps=--sample-steps, sampler=--sampler,
eta=--eta, constrain=True, seed=--seed, clip_offset=first)` -- x_T and every step's noise are keyed by the seed and the clip's
position in the pass --, `VQVAE.code_agreement` and `SpectralDistance` (one fused kernel).  After every batch one line:

    {n} samples: code_match=... mcd=... lsd=... [ref_code_match=... ref_mcd=... ref_lsd=... gap_mcd=... gap_lsd=...] [target_acc=... target_nll=... source_acc=...]

code_match is agreeing codes / codes; mcd and lsd are dB per frame, source against converted (sum of the clips' sums / frames).
`--target other` (default) draws a seeded different label per clip (`wrong_labels` of eval_vqvae.py), `same` reconstructs every clip
under its own label (a codec / vocoder style score), an integer is one fixed label.  `--reference-steps R` decodes the same codes,
labels and x_T a second time with `--reference-sampler` at R steps: ref_* score that run against the source, gap_* the two runs
against each other.  `--classifier PATH` adds a `Classifier` at t = 0 on the converted audio: target_acc / target_nll for the
target label, source_acc how often it still names the source's (left out with `--target same`).  All sums are exact -- integer
counts, and the float64 clip sums added as fractions -- so the line does not depend on the batch size or the rank count.

`data_dir`, `--batch-size`, `--precision`, `--seed`, `--max-samples` and `--dist-backend` are the common parser's and the pass is
the shared one (vq_voice_swap_amd/eval_pass.py).  Under torchrun (WORLD_SIZE > 1) batches are dealt round-robin, rank 0 merges
the states and prints the one final line.
"""
import os
import sys
from fractions import Fraction

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_vqvae import wrong_labels  # noqa: E402
from vq_voice_swap_amd import VQVAE, Classifier, SpectralDistance, randn_clips  # noqa: E402
from vq_voice_swap_amd.eval_pass import common_parser, format_line, run_pass  # noqa: E402,F401

SAMPLERS = ["ddpm", "ddim", "dpmpp"]


def arg_parser():
    p = common_parser()
    p.add_argument("--sampler", default="ddpm", choices=SAMPLERS)
    p.add_argument("--eta", type=float, default=0.0, help="DDIM noise level: 0 deterministic, 1 the DDPM step's variance (--sampler ddim)")
    p.add_argument("--sample-steps", type=int, default=100)
    p.add_argument("--target", default="other", help="'other': a seeded different label per clip; 'same': the clip's own label; N: this label")
    p.add_argument("--reference-steps", type=int, default=None, help="decode a second time at this many steps and score that run and the gap")
    p.add_argument("--reference-sampler", default="ddpm", choices=SAMPLERS)
    p.add_argument("--classifier", default=None, type=str, metavar="PATH", help="a Classifier checkpoint, read at t = 0 on the converted audio")
    return p


def parse_args(argv=None):
    """The command line with everything that can be refused from the flags alone."""
    parser = arg_parser()
    args = parser.parse_args(argv)
    if args.sampler != "ddim" and args.eta:
        parser.error("--eta belongs to --sampler ddim (ddpm has its own variance, dpmpp is deterministic)")
    if args.eta < 0:
        parser.error("--eta must not be negative")
    if args.sample_steps < 1:
        parser.error("--sample-steps must be at least 1")
    if args.reference_steps is not None and args.reference_steps < 1:
        parser.error("--reference-steps must be at least 1")
    if args.target not in ("other", "same"):
        try:
            args.target = int(args.target)
        except ValueError:
            parser.error(f"--target {args.target!r} is neither 'other', 'same' nor a label")
    return args


def check_target(target, num_labels: int) -> None:
    """The refusals that need the label count (known from the data, before the model loads)."""
    if target == "other" and num_labels < 2:
        raise SystemExit(f"--target other needs at least two labels, the data has {num_labels}")
    if isinstance(target, int) and not 0 <= target < num_labels:
        raise SystemExit(f"--target {target} is outside the labels 0..{num_labels - 1}")


def target_labels(labels: torch.Tensor, target, num_labels: int, seed: int, first: int) -> torch.Tensor:
    """The label every clip of a batch is converted to; `first` is the position of the batch's first clip in the pass."""
    if target == "other":
        return wrong_labels(labels, num_labels, seed, first)
    if target == "same":
        return labels
    return torch.full_like(labels, int(target))


def _exact(values) -> Fraction:
    return sum((Fraction(float(v)) for v in values), Fraction(0))


class EvalState:
    """What one pass accumulates: clip, code and frame counts, the agreeing codes (integers) and the distance sums (fractions of
    the clips' float64 sums: the same whatever order batches and shards arrive in); with a reference run the same for it and for
    the gap between the two runs; with a classifier its hits and summed NLL."""

    def __init__(self, reference: bool = False, classifier: bool = False, same: bool = False):
        self.reference, self.classifier, self.same = bool(reference), bool(classifier), bool(same)
        self.num_samples = 0
        self.codes = 0    # code positions behind the *_match counts
        self.frames = 0   # frames behind the distance sums
        self.counts = {"code_match": 0, "ref_code_match": 0, "target_correct": 0, "source_correct": 0}
        self.sums = {k: Fraction(0) for k in ("mcd", "lsd", "ref_mcd", "ref_lsd", "gap_mcd", "gap_lsd", "target_nll")}

    def add_scores(self, codes_per_clip: int, frames_per_clip: int, scores) -> None:
        """Fold in one batch: `scores` maps "code_match" (and "ref_code_match", "target_correct", "source_correct") to one integer
        per clip and "mcd", "lsd" (and the ref_ / gap_ ones, "target_nll") to one float64 sum per clip."""
        n = len(scores["mcd"])
        want = {"code_match", "mcd", "lsd"}
        if self.reference:
            want |= {"ref_code_match", "ref_mcd", "ref_lsd", "gap_mcd", "gap_lsd"}
        if self.classifier:
            want |= {"target_correct", "target_nll"} | (set() if self.same else {"source_correct"})
        if set(scores) != want or any(len(v) != n for v in scores.values()):
            raise ValueError(f"expected {sorted(want)} with {n} entries each, got {sorted(scores)}")
        self.num_samples += n
        self.codes += n * int(codes_per_clip)
        self.frames += n * int(frames_per_clip)
        for key, values in scores.items():
            if key in self.counts:
                self.counts[key] += sum(int(v) for v in values)
            else:
                self.sums[key] += _exact(values)

    def add_batch(self, model: VQVAE, distance: SpectralDistance, audio: torch.Tensor, labels: torch.Tensor, first: int, seed: int,
                  run, classifier=None) -> None:
        """Convert and score one batch whose first clip is clip `first` of the pass; `run` carries target, sampler, eta,
        sample_steps, reference_steps and reference_sampler (the parsed command line)."""
        target = target_labels(labels, run.target, model.num_labels, seed, first)
        codes = model.encode(audio)
        # the draw `decode` would make itself from (seed, clip_offset): made here so that the reference run starts from the same x_T
        x_T = randn_clips(len(audio), codes.shape[-1] * model.encoder.downsample_rate, audio.device, seed, first)

        def decode(sampler, steps):
            return model.decode(codes, target, steps=steps, constrain=True, x_T=x_T, sampler=sampler, eta=run.eta if sampler == "ddim" else 0.0,
                                seed=seed, clip_offset=first)

        def against_source(out, prefix=""):
            d = distance(audio, out)
            return {prefix + "code_match": model.code_agreement(codes, out).tolist(), prefix + "mcd": d["mcd"].tolist(),
                    prefix + "lsd": d["lsd"].tolist()}

        converted = decode(run.sampler, run.sample_steps)
        scores = against_source(converted)
        if self.reference:
            ref = decode(run.reference_sampler, run.reference_steps)
            scores.update(against_source(ref, "ref_"))
            gap = distance(converted, ref)
            scores.update(gap_mcd=gap["mcd"].tolist(), gap_lsd=gap["lsd"].tolist())
        if self.classifier:
            ts = torch.zeros(len(audio), device=audio.device)
            out = classifier.scores(converted, ts, target)
            scores.update(target_correct=out["top1"].tolist(), target_nll=out["nll"].tolist())
            if not self.same:
                scores.update(source_correct=classifier.scores(converted, ts, labels)["top1"].tolist())
        self.add_scores(codes.shape[-1], distance.frames(audio.shape[-1]), scores)

    def merge(self, other: "EvalState") -> "EvalState":
        if (other.reference, other.classifier, other.same) != (self.reference, self.classifier, self.same):
            raise ValueError("cannot merge states of differently configured passes")
        self.num_samples += other.num_samples
        self.codes += other.codes
        self.frames += other.frames
        for key in self.counts:
            self.counts[key] += other.counts[key]
        for key in self.sums:
            self.sums[key] += other.sums[key]
        return self

    def to_host(self) -> "EvalState":
        return self  # (integers and fractions only)

    def log_dict(self):
        per = lambda total, n: float(Fraction(total) / n) if n else 0.0  # noqa: E731
        log = {"code_match": per(self.counts["code_match"], self.codes), "mcd": per(self.sums["mcd"], self.frames),
               "lsd": per(self.sums["lsd"], self.frames)}
        if self.reference:
            log["ref_code_match"] = per(self.counts["ref_code_match"], self.codes)
            for key in ("ref_mcd", "ref_lsd", "gap_mcd", "gap_lsd"):
                log[key] = per(self.sums[key], self.frames)
        if self.classifier:
            log["target_acc"] = per(self.counts["target_correct"], self.num_samples)
            log["target_nll"] = per(self.sums["target_nll"], self.num_samples)
            if not self.same:
                log["source_acc"] = per(self.counts["source_correct"], self.num_samples)
        return log


def main(argv=None):
    args = parse_args(argv)

    def build(device, num_labels):
        model = VQVAE.load(args.checkpoint_path).to(device)
        assert model.num_labels == num_labels, f"the model has {model.num_labels} labels, the data {num_labels}"
        model.eval().set_precision(args.precision)
        classifier = None
        if args.classifier:
            classifier = Classifier.load(args.classifier).to(device)
            assert classifier.num_labels == num_labels, f"the classifier has {classifier.num_labels} labels, the data {num_labels}"
            classifier.eval().set_precision(args.precision)
        distance = SpectralDistance()
        state = EvalState(reference=args.reference_steps is not None, classifier=classifier is not None, same=args.target == "same")
        return state, lambda audio, data_batch, first: state.add_batch(model, distance, audio, data_batch["label"].to(device), first, args.seed,
                                                                        args, classifier)

    run_pass(args, build, no_device="the encoder, the decoder and the distance kernel have no CPU path",
             check_data=lambda num_labels: check_target(args.target, num_labels))


if __name__ == "__main__":
    main()
