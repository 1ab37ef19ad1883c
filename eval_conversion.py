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
                 [f0_shift=... f0_dev=... vuv_err=... voiced=... [ref_f0_shift=... ref_f0_dev=... ref_vuv_err=... gap_f0_dev=... gap_vuv_err=...]]

code_match is agreeing codes / codes; mcd and lsd are dB per frame, source against converted (sum of the clips' sums / frames).
`--target other` (default) draws a seeded different label per clip (`wrong_labels` of eval_vqvae.py), `same` reconstructs every clip
under its own label (a codec / vocoder style score), an integer is one fixed label.  `--reference-steps R` decodes the same codes,
labels and x_T a second time with `--reference-sampler` at R steps: ref_* score that run against the source, gap_* the two runs
against each other.  `--classifier PATH` adds a `Classifier` at t = 0 on the converted audio: target_acc / target_nll for the
target label, source_acc how often it still names the source's (left out with `--target same`).  `--pitch` adds `PitchDistance`
(YIN periods of the 16-bit samples, one fused kernel): f0_shift, the mean over the frames voiced in both clips of the semitones by
which the converted clip is higher than the source; f0_dev, the RMS deviation of that distance around each clip's own mean (the
intonation contour, the register shift removed); vuv_err, frames whose voicing differs / frames; voiced, the source's voiced frames /
frames; with a reference run ref_* for it and gap_f0_dev, gap_vuv_err between the two runs.  All sums are exact -- integer
counts, and the float64 clip sums added as fractions -- so the line does not depend on the batch size or the rank count.

`--guide-label-scale S` / `--guide-vq-scale S` (both off by default) decode -- the reference run too -- with the classifier-free-style
guidance of sample_vqvae_uncond.py (`VQVAE.decode_uncond_guidance`).  With either set the checkpoint is taken to have the
unconditional label at 0 (`enroll_speaker.py --uncond` makes one: one label more than the data has speakers) and `--target` and the
data's labels are speaker numbers WITHOUT that offset, as the classifier counts them.  The line is the usual one: run it at several S
with `--classifier` to see what a scale does to target_acc, target_nll, mcd and code_match.

`--voice SPEC` in place of `--target` converts every clip to a voice spec (vq_voice_swap_amd/speakers.py: a blend "3:0.7,251:0.3", a
vector file "@voice.npy"); a spec that is one label is `--target N`.  A blend or a file is nobody's label, so with `--classifier` only
source_acc is printed for it: target_acc and target_nll need a label to score against.

`data_dir`, `--batch-size`, `--precision`, `--seed`, `--max-samples` and `--dist-backend` are the common parser's and the pass is
the shared one (vq_voice_swap_amd/eval_pass.py).  Under torchrun (WORLD_SIZE > 1) batches are dealt round-robin, rank 0 merges
the states and prints the one final line.
"""
import math
import os
import sys
from fractions import Fraction

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_vqvae import wrong_labels  # noqa: E402
from vq_voice_swap_amd import VQVAE, Classifier, PitchDistance, SpectralDistance, randn_clips  # noqa: E402
from vq_voice_swap_amd.corpus import add_guidance_flags, guided  # noqa: E402
from vq_voice_swap_amd.eval_pass import common_parser, format_line, run_pass  # noqa: E402,F401
from vq_voice_swap_amd.speakers import as_entries, parse_voice, single_label, voice_vectors  # noqa: E402

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
    # the opt-in scores join the parser here: `arg_parser()` stays the flag set the default line is made of
    parser.add_argument("--pitch", action="store_true", help="add F0 scores (YIN on the 16-bit samples): register shift, contour deviation, voicing errors")
    add_guidance_flags(parser)
    parser.add_argument("--voice", type=str, default=None, metavar="SPEC",
                        help="convert every clip to this voice spec instead of --target: a blend `3:0.7,251:0.3`, a vector file `@voice.npy`")
    args = parser.parse_args(argv)
    if args.voice is not None:
        import argparse

        if parser.parse_args(argv, argparse.Namespace(target=None)).target is not None:
            parser.error("--voice takes the place of --target: give one or the other")
        try:
            parse_voice(args.voice)
        except ValueError as e:
            parser.error(str(e))
        if single_label(args.voice) is not None:  # (one label at weight 1 IS --target N, classifier scores included)
            args.target, args.voice = str(single_label(args.voice)), None
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


def check_target(target, num_labels: int, voice=None) -> None:
    """The refusals that need the label count (known from the data, before the model loads)."""
    if voice is not None:
        bad = sorted({l for l, _ in as_entries(voice) if not isinstance(l, str) and not 0 <= l < num_labels})
        if bad:
            raise SystemExit(f"--voice {voice!r}: labels {bad} are outside the labels 0..{num_labels - 1}")
        return
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


def _pitch_scores(out, prefix=""):
    """`PitchDistance`'s per-clip results as the lists `EvalState.add_scores` takes."""
    return {prefix + "f0_n": out["voiced_both"].tolist(), prefix + "f0_s1": out["shift_sum"].tolist(), prefix + "f0_s2": out["shift_sq_sum"].tolist(),
            prefix + "vuv": out["vuv"].tolist(), prefix + "voiced": out["voiced_a"].tolist()}


class EvalState:
    """What one pass accumulates: clip, code and frame counts, the agreeing codes (integers) and the distance sums (fractions of
    the clips' float64 sums: the same whatever order batches and shards arrive in); with a reference run the same for it and for
    the gap between the two runs; with a classifier its hits and summed NLL; with pitch the voicing counts, the summed pitch
    distance and the summed squared deviation around each clip's own mean.  `voice`: the target is a voice spec that is no single
    label, so there is no label to score the classifier against: target_correct / target_nll are left out."""

    def __init__(self, reference: bool = False, classifier: bool = False, same: bool = False, pitch: bool = False, voice: bool = False):
        self.reference, self.classifier, self.same, self.pitch = bool(reference), bool(classifier), bool(same), bool(pitch)
        self.voice = bool(voice)
        self.num_samples = 0
        self.codes = 0    # code positions behind the *_match counts
        self.frames = 0   # frames behind the distance sums
        self.counts = {"code_match": 0, "ref_code_match": 0, "target_correct": 0, "source_correct": 0}
        self.sums = {k: Fraction(0) for k in ("mcd", "lsd", "ref_mcd", "ref_lsd", "gap_mcd", "gap_lsd", "target_nll")}
        if self.pitch:  # per comparison: both-voiced frames, voicing mismatches, source-voiced frames; sum of l, and of the squared
            for prefix in ("", "ref_", "gap_"):  # deviations around each clip's own mean, sum_c (S2_c - S1_c^2 / n_c)
                self.counts.update({prefix + k: 0 for k in ("f0_n", "vuv", "voiced")})
                self.sums.update({prefix + k: Fraction(0) for k in ("f0_s1", "f0_within")})

    def add_scores(self, codes_per_clip: int, frames_per_clip: int, scores) -> None:
        """Fold in one batch: `scores` maps "code_match" (and "ref_code_match", "target_correct", "source_correct") to one integer
        per clip and "mcd", "lsd" (and the ref_ / gap_ ones, "target_nll") to one float64 sum per clip; with pitch also "f0_n", "vuv",
        "voiced" (integers: frames voiced in both, voicing mismatches, frames voiced in the first signal) and "f0_s1", "f0_s2" (the
        float64 sums of l_f and l_f^2), each also with the ref_ and gap_ prefixes when there is a reference run."""
        n = len(scores["mcd"])
        want = {"code_match", "mcd", "lsd"}
        if self.reference:
            want |= {"ref_code_match", "ref_mcd", "ref_lsd", "gap_mcd", "gap_lsd"}
        if self.classifier:
            want |= (set() if self.voice else {"target_correct", "target_nll"}) | (set() if self.same else {"source_correct"})
        prefixes = (("", "ref_", "gap_") if self.reference else ("",)) if self.pitch else ()
        want |= {p + k for p in prefixes for k in ("f0_n", "f0_s1", "f0_s2", "vuv", "voiced")}
        if set(scores) != want or any(len(v) != n for v in scores.values()):
            raise ValueError(f"expected {sorted(want)} with {n} entries each, got {sorted(scores)}")
        if self.pitch:  # a clip's squared deviation around its own shift, exactly; a clip with no frame voiced in both adds nothing
            scores = dict(scores)
            for p in prefixes:
                s2 = scores.pop(p + "f0_s2")
                scores[p + "f0_within"] = [Fraction(float(q)) - Fraction(float(s)) ** 2 / int(c) if int(c) else Fraction(0)
                                           for c, s, q in zip(scores[p + "f0_n"], scores[p + "f0_s1"], s2)]
        self.num_samples += n
        self.codes += n * int(codes_per_clip)
        self.frames += n * int(frames_per_clip)
        for key, values in scores.items():
            if key in self.counts:
                self.counts[key] += sum(int(v) for v in values)
            else:
                self.sums[key] += sum(values, Fraction(0)) if key.endswith("f0_within") else _exact(values)

    def add_batch(self, model: VQVAE, distance: SpectralDistance, audio: torch.Tensor, labels: torch.Tensor, first: int, seed: int,
                  run, classifier=None, pitch=None) -> None:
        """Convert and score one batch whose first clip is clip `first` of the pass; `run` carries target, sampler, eta,
        sample_steps, reference_steps and reference_sampler (the parsed command line); `pitch` is the `PitchDistance` of a state
        built with pitch=True."""
        if self.pitch and pitch is None:
            raise ValueError("a state with pitch=True needs a PitchDistance")
        # under guidance label 0 of the checkpoint is the unconditional one: the speakers, and every label here, are counted without it
        guide = guided(run)
        voice = getattr(run, "voice", None)
        if voice is None:
            target = dict(labels=target_labels(labels, run.target, model.num_labels - 1 if guide else model.num_labels, seed, first))
        else:  # (the spec names speakers without the null label's offset, as --target does)
            target = dict(vectors=voice_vectors(model.predictor, [voice], label_offset=1 if guide else 0).expand(len(audio), -1))
        codes = model.encode(audio)
        # the draw `decode` would make itself from (seed, clip_offset): made here so that the reference run starts from the same x_T
        x_T = randn_clips(len(audio), codes.shape[-1] * model.encoder.downsample_rate, audio.device, seed, first)

        def decode(sampler, steps):
            kw = dict(steps=steps, constrain=True, x_T=x_T, sampler=sampler, eta=run.eta if sampler == "ddim" else 0.0, seed=seed, clip_offset=first)
            if guide:
                return model.decode_uncond_guidance(codes, **target, label_scale=run.guide_label_scale, vq_scale=run.guide_vq_scale, **kw)
            return model.decode(codes, **target, **kw)

        def against_source(out, prefix=""):
            d = distance(audio, out)
            scores = {prefix + "code_match": model.code_agreement(codes, out).tolist(), prefix + "mcd": d["mcd"].tolist(),
                      prefix + "lsd": d["lsd"].tolist()}
            if self.pitch:
                scores.update(_pitch_scores(pitch(audio, out), prefix))
            return scores

        converted = decode(run.sampler, run.sample_steps)
        scores = against_source(converted)
        if self.reference:
            ref = decode(run.reference_sampler, run.reference_steps)
            scores.update(against_source(ref, "ref_"))
            gap = distance(converted, ref)
            scores.update(gap_mcd=gap["mcd"].tolist(), gap_lsd=gap["lsd"].tolist())
            if self.pitch:
                scores.update(_pitch_scores(pitch(converted, ref), "gap_"))
        if self.classifier:
            ts = torch.zeros(len(audio), device=audio.device)
            if not self.voice:
                out = classifier.scores(converted, ts, target["labels"])
                scores.update(target_correct=out["top1"].tolist(), target_nll=out["nll"].tolist())
            if not self.same:
                scores.update(source_correct=classifier.scores(converted, ts, labels)["top1"].tolist())
        self.add_scores(codes.shape[-1], distance.frames(audio.shape[-1]), scores)

    def merge(self, other: "EvalState") -> "EvalState":
        if (other.reference, other.classifier, other.same, other.pitch, other.voice) != (self.reference, self.classifier, self.same, self.pitch, self.voice):
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
            if not self.voice:
                log["target_acc"] = per(self.counts["target_correct"], self.num_samples)
                log["target_nll"] = per(self.sums["target_nll"], self.num_samples)
            if not self.same:
                log["source_acc"] = per(self.counts["source_correct"], self.num_samples)
        if self.pitch:
            def dev(prefix):
                # (S2_c - S1_c^2 / n_c of the clips' ROUNDED sums can fall a rounding below 0 where a clip's l_f are all equal)
                return math.sqrt(max(0.0, per(self.sums[prefix + "f0_within"], self.counts[prefix + "f0_n"])))

            log.update(f0_shift=per(self.sums["f0_s1"], self.counts["f0_n"]), f0_dev=dev(""), vuv_err=per(self.counts["vuv"], self.frames),
                       voiced=per(self.counts["voiced"], self.frames))
            if self.reference:
                log.update(ref_f0_shift=per(self.sums["ref_f0_s1"], self.counts["ref_f0_n"]), ref_f0_dev=dev("ref_"),
                           ref_vuv_err=per(self.counts["ref_vuv"], self.frames), gap_f0_dev=dev("gap_"),
                           gap_vuv_err=per(self.counts["gap_vuv"], self.frames))
        return log


def main(argv=None):
    args = parse_args(argv)

    def build(device, num_labels):
        model = VQVAE.load(args.checkpoint_path).to(device)
        if guided(args):
            assert model.num_labels == num_labels + 1, (f"the model has {model.num_labels} labels, the data {num_labels}: under guidance the "
                                                        "checkpoint holds the unconditional label 0 and then the data's speakers")
        else:
            assert model.num_labels == num_labels, f"the model has {model.num_labels} labels, the data {num_labels}"
        model.eval().set_precision(args.precision)
        classifier = None
        if args.classifier:
            classifier = Classifier.load(args.classifier).to(device)
            assert classifier.num_labels == num_labels, f"the classifier has {classifier.num_labels} labels, the data {num_labels}"
            classifier.eval().set_precision(args.precision)
        distance, pitch = SpectralDistance(), PitchDistance() if args.pitch else None
        state = EvalState(reference=args.reference_steps is not None, classifier=classifier is not None, same=args.target == "same",
                          pitch=args.pitch, voice=args.voice is not None)
        return state, lambda audio, data_batch, first: state.add_batch(model, distance, audio, data_batch["label"].to(device), first, args.seed,
                                                                        args, classifier, pitch)

    run_pass(args, build, no_device="the encoder, the decoder and the distance kernel have no CPU path",
             check_data=lambda num_labels: check_target(args.target, num_labels, args.voice))


if __name__ == "__main__":
    main()
