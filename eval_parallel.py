#!/usr/bin/env python3
"""
Score voice conversions against PARALLEL target recordings on MI355X: the standard objective score of the field, MCD-DTW.

    python eval_parallel.py pairs.tsv data/ --checkpoint model_vqvae.pt --sampler dpmpp --sample-steps 25 --precision fp16 [--pitch]
    python eval_parallel.py pairs.tsv data/ --converted-dir out/ [--pitch]     # score files another run or system wrote; no model
    torchrun --nproc-per-node 8 eval_parallel.py pairs.tsv data/ --checkpoint model_vqvae.pt

`pairs.tsv` holds lines `source<TAB>target<TAB>label`: two recordings of the SAME sentence, read by the source and by the target
speaker (paths relative to `data_dir`; CMU Arctic or VCTK style), and the target speaker's label -- or a voice spec in its place
(vq_voice_swap_amd/speakers.py: a blend "3:0.7,251:0.3", a vector file "@voice.npy" fitted to the target).  The converted source is
compared with the target speaker's own recording, aligned by dynamic time warping under the mel-cepstral cost because the two
readings differ in timing (`AlignedDistance`: `vqvs_mel_cepstra` and `vqvs_dtw_distance`), and the
unconverted source is scored the same way: the number a conversion has to beat.

With `--checkpoint` the sources are converted as `convert_dataset.py` converts them -- packs of at most `--pack-windows` windows
through `VQVAE.encode_long_batch` / `decode_long_batch`, pair i keyed as file id i -- and take the route through a 16-bit file
in memory, so the scores are those of `convert_dataset.py` followed by `--converted-dir`.  With `--converted-dir DIR` the
converted file of a pair is `DIR/<source path>` with the extension .wav.  One line per pack, and at the end rank 0's merged line

    {n} pairs: mcd_dtw=... src_mcd_dtw=... gain=... stretch=... [f0_shift_dtw=... f0_dev_dtw=... vuv_err_dtw=... src_f0_shift_dtw=... src_f0_dev_dtw=... src_vuv_err_dtw=...]

mcd_dtw is sum of path costs / sum of path lengths (dB per aligned frame pair), converted against target; src_mcd_dtw the same for
the source; gain = src_mcd_dtw - mcd_dtw; stretch = sum of path lengths / sum of max(Fa, Fb).  `--pitch` adds the F0 figures of
eval_conversion.py over path cells instead of frames: the mean semitones by which the target is higher than the converted
recording, the RMS deviation around each pair's own mean, and cells voiced in exactly one of the two / cells.  All sums are exact
(integers, and the pairs' float64 sums added as fractions): the merged line does not depend on --pack-windows or the rank count.
The scores are an instrument, not a verdict on any sampler.

Everything wrong with the pairs -- a malformed line, a missing or unreadable file, a label outside the model, a recording shorter
than n_fft / 2 + 1 samples or longer than 2048 frames -- ends the run with the line number before any GPU work: a score over a
silently smaller set is worse than no score.
"""
import argparse
import math
import os
import sys
from fractions import Fraction

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import VQVAE, PitchDistance, SpectralDistance, wav_roundtrip  # noqa: E402
from vq_voice_swap_amd.audio import ChunkReader  # noqa: E402
from vq_voice_swap_amd.corpus import deal_packs, make_packs  # noqa: E402
from vq_voice_swap_amd.dtw import MAX_FRAMES, AlignedDistance  # noqa: E402
from vq_voice_swap_amd.eval_pass import close_ranks, local_device, open_ranks  # noqa: E402
from vq_voice_swap_amd.longform import plan_windows  # noqa: E402
from vq_voice_swap_amd.speakers import parse_voice, voice_vectors  # noqa: E402

SAMPLE_RATE = 16000
SIDES = ("", "src_")  # converted against target, source against target


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    what = p.add_mutually_exclusive_group(required=True)
    what.add_argument("--checkpoint", type=str, default=None, metavar="PATH", help="a VQVAE checkpoint: convert every source to its pair's label")
    what.add_argument("--converted-dir", type=str, default=None, metavar="DIR", help="score DIR/<source path>.wav, written by another run; no model")
    p.add_argument("--sampler", default="ddpm", choices=["ddpm", "ddim", "dpmpp"])
    p.add_argument("--eta", type=float, default=0.0, help="DDIM noise level: 0 deterministic, 1 the DDPM step's variance (--sampler ddim)")
    p.add_argument("--sample-steps", type=int, default=100)
    p.add_argument("--window-seconds", type=float, default=4.0, help="window length (the length the model was trained on)")
    p.add_argument("--overlap-seconds", type=float, default=0.4, help="overlap of neighbouring windows")
    p.add_argument("--window-batch", type=int, default=64, help="windows per forward")
    p.add_argument("--pack-windows", type=int, default=512, help="windows of the recordings converted and scored together")
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--max-pairs", default=None, type=int, help="score the first this many pairs")
    p.add_argument("--pitch", action="store_true", help="add F0 scores over the path's cells (YIN on the 16-bit samples)")
    p.add_argument("pairs", type=str, help="lines `source<TAB>target<TAB>label`, paths relative to data_dir")
    p.add_argument("data_dir", type=str)
    return p


def parse_args(argv=None):
    parser = arg_parser()
    args = parser.parse_args(argv)
    if args.sampler != "ddim" and args.eta:
        parser.error("--eta belongs to --sampler ddim (ddpm has its own variance, dpmpp is deterministic)")
    if args.eta < 0:
        parser.error("--eta must not be negative")
    if args.sample_steps < 1:
        parser.error("--sample-steps must be at least 1")
    if args.pack_windows < 1 or args.window_batch < 1:
        parser.error("--pack-windows and --window-batch must be at least 1")
    if args.max_pairs is not None and args.max_pairs < 1:
        parser.error("--max-pairs must be at least 1")
    return args


def converted_path(converted_dir: str, rel: str) -> str:
    return os.path.join(converted_dir, os.path.splitext(rel)[0] + ".wav")  # (where convert_dataset.py writes it)


def read_wave(path: str) -> np.ndarray:
    """The whole file as float32 [N] at 16 kHz; raises for a file that cannot be read."""
    reader = ChunkReader(path, sample_rate=SAMPLE_RATE)
    try:
        chunks = []
        while (chunk := reader.read(1 << 20)) is not None:
            chunks.append(chunk)
    finally:
        reader.close()
    return np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.float32)


def sample_limits(spectral: SpectralDistance):
    """(fewest, most) samples of a recording: longer than the reflect padding, at most 2048 frames."""
    return spectral.n_fft // 2 + 1, MAX_FRAMES * spectral.hop - 1


def read_pairs(path: str, data_dir: str, *, num_labels=None, converted_dir=None, max_pairs=None, limits=None, length=None):
    """`pairs.tsv` -> [(source, target, label, source samples)].  Blank lines and lines starting with # are skipped.  ValueError with
    `path:line` for a line that is not `source<TAB>target<TAB>label`, a label that is neither a non-negative integer nor a voice spec (kept as text) or lies outside
    0..num_labels-1, a file (source, target or, with `converted_dir`, the converted one) that is missing, cannot be read, or holds
    fewer than limits[0] or more than limits[1] samples.  `length(path)` returns a file's sample count (default: it is read)."""
    limits = sample_limits(SpectralDistance()) if limits is None else limits
    length = (lambda p: read_wave(p).size) if length is None else length
    pairs = []
    with open(path, "rt") as f:
        for number, line in enumerate(f, 1):
            if max_pairs is not None and len(pairs) >= max_pairs:
                break
            line = line.rstrip("\r\n")
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            where = f"{path}:{number}"
            fields = [x.strip() for x in line.split("\t")]
            if len(fields) != 3 or not fields[0] or not fields[1]:
                raise ValueError(f"{where}: expected `source<TAB>target<TAB>label`, got {line!r}")
            source, target, text = fields
            if text.isdigit():
                label, named = int(text), [int(text)]
            else:  # a voice spec in the label's place: kept as text, its labels held to the model's like any other
                try:
                    named = [l for l, _ in parse_voice(text) if not isinstance(l, str)]
                except ValueError as e:
                    raise ValueError(f"{where}: label {text!r} is not a non-negative integer or a voice spec ({e})") from None
                label = text
            for l in named:
                if num_labels is not None and l >= num_labels:
                    raise ValueError(f"{where}: label {l} outside the model's 0..{num_labels - 1}")
            files = [os.path.join(data_dir, source), os.path.join(data_dir, target)]
            if converted_dir is not None:
                files.append(converted_path(converted_dir, source))
            counts = []
            for name in files:
                if not os.path.isfile(name):
                    raise ValueError(f"{where}: no file {name}")
                try:
                    n = int(length(name))
                except Exception as e:
                    raise ValueError(f"{where}: cannot read {name}: {e}") from e
                if not limits[0] <= n <= limits[1]:
                    raise ValueError(f"{where}: {name} holds {n} samples, outside {limits[0]}..{limits[1]} (at most {MAX_FRAMES} frames)")
                counts.append(n)
            pairs.append((source, target, label, counts[0]))
    if not pairs:
        raise ValueError(f"{path}: no pairs")
    return pairs


def _exact(values) -> Fraction:
    return sum((Fraction(float(v)) for v in values), Fraction(0))


class ParallelState:
    """What a run accumulates, per side ("" converted against target, "src_" source against target): path costs (fractions of the
    pairs' float64 sums), path lengths and max(Fa, Fb) (integers); with pitch the cells voiced in both and in exactly one, the
    summed shift and the summed squared deviation around each pair's own mean.  The same whatever order pairs arrive in."""

    def __init__(self, pitch: bool = False):
        self.pitch = bool(pitch)
        self.num_pairs = 0
        self.counts = {s + k: 0 for s in SIDES for k in ("steps", "longer") + (("f0_n", "vuv") if self.pitch else ())}
        self.sums = {s + k: Fraction(0) for s in SIDES for k in ("cost",) + (("f0_s1", "f0_within") if self.pitch else ())}

    def add_scores(self, scores) -> None:
        """`scores` maps, per side, "cost" to one float64 per pair and "steps", "longer" to one integer per pair; with pitch also
        "f0_n", "vuv" (integers) and "f0_s1", "f0_s2" (float64 sums of l and l^2 over the pair's `f0_n` cells)."""
        want = {s + k for s in SIDES for k in ("cost", "steps", "longer") + (("f0_n", "vuv", "f0_s1", "f0_s2") if self.pitch else ())}
        n = len(scores.get("cost", ()))
        if set(scores) != want or any(len(v) != n for v in scores.values()):
            raise ValueError(f"expected {sorted(want)} with {n} entries each, got {sorted(scores)}")
        scores = dict(scores)
        if self.pitch:
            for s in SIDES:  # a pair's squared deviation around its own shift, exactly; a pair with no such cell adds nothing
                s2 = scores.pop(s + "f0_s2")
                scores[s + "f0_within"] = [Fraction(float(q)) - Fraction(float(v)) ** 2 / int(c) if int(c) else Fraction(0)
                                           for c, v, q in zip(scores[s + "f0_n"], scores[s + "f0_s1"], s2)]
        self.num_pairs += n
        for key, values in scores.items():
            if key in self.counts:
                self.counts[key] += sum(int(v) for v in values)
            else:
                self.sums[key] += sum(values, Fraction(0)) if key.endswith("f0_within") else _exact(values)

    def merge(self, other: "ParallelState") -> "ParallelState":
        if other.pitch != self.pitch:
            raise ValueError("cannot merge states of differently configured runs")
        self.num_pairs += other.num_pairs
        for key in self.counts:
            self.counts[key] += other.counts[key]
        for key in self.sums:
            self.sums[key] += other.sums[key]
        return self

    def log_dict(self):
        per = lambda total, n: float(Fraction(total) / n) if n else 0.0  # noqa: E731
        mcd, src = per(self.sums["cost"], self.counts["steps"]), per(self.sums["src_cost"], self.counts["src_steps"])
        log = {"mcd_dtw": mcd, "src_mcd_dtw": src,
               "gain": per(self.sums["src_cost"] * self.counts["steps"] - self.sums["cost"] * self.counts["src_steps"],
                           self.counts["steps"] * self.counts["src_steps"]),
               "stretch": per(self.counts["steps"], self.counts["longer"])}
        if self.pitch:
            for s in SIDES:
                # (S2 - S1^2 / n of a pair's ROUNDED sums can fall a rounding below 0 where its l are all equal)
                log.update({s + "f0_shift_dtw": per(self.sums[s + "f0_s1"], self.counts[s + "f0_n"]),
                            s + "f0_dev_dtw": math.sqrt(max(0.0, per(self.sums[s + "f0_within"], self.counts[s + "f0_n"]))),
                            s + "vuv_err_dtw": per(self.counts[s + "vuv"], self.counts[s + "steps"])})
        return log


def format_line(num_pairs: int, log) -> str:
    return f"{num_pairs} pairs: " + " ".join(f"{key}={value:.06f}" for key, value in log.items())


def pad_batch(waves, device):
    """float32 recordings of different lengths -> ([n, Tmax] on the device, zero-padded; their lengths)."""
    lengths = [int(w.shape[-1]) for w in waves]
    out = torch.zeros(len(waves), max(lengths), dtype=torch.float32, device=device)
    for row, w in enumerate(waves):
        out[row, :lengths[row]] = w.reshape(-1).to(device)
    return out, lengths


def side_scores(out, prefix: str, pitch: bool):
    longer = torch.maximum(out["frames_a"], out["frames_b"])
    scores = {prefix + "cost": out["cost"].tolist(), prefix + "steps": out["steps"].tolist(), prefix + "longer": longer.tolist()}
    if pitch:
        scores.update({prefix + "f0_n": out["both"].tolist(), prefix + "vuv": out["vuv"].tolist(), prefix + "f0_s1": out["shift_sum"].tolist(),
                       prefix + "f0_s2": out["shift_sq_sum"].tolist()})
    return scores


def score_pack(aligned: AlignedDistance, converted, sources, targets, device, pitch: bool):
    """The scores of one pack: lists of float32 recordings (any lengths) -> the dictionary `ParallelState.add_scores` takes."""
    tgt, len_t = pad_batch(targets, device)
    scores = {}
    for prefix, waves in zip(SIDES, (converted, sources)):
        x, len_x = pad_batch(waves, device)
        scores.update(side_scores(aligned(x, len_x, tgt, len_t), prefix, pitch))
    return scores


def convert_run(args, model, device, waves, labels, first: int, window: int, hop: int):
    """Recordings with consecutive ids first, first + 1, ... -> what convert_dataset.py's files hold for them once read back."""
    batch = [torch.from_numpy(w[None, None]).to(device) for w in waves]
    codes, counts = model.encode_long_batch(batch, window, hop, args.window_batch)
    if all(isinstance(l, int) for l in labels):
        target = dict(labels=torch.tensor(labels).long().to(device))
    else:  # voice specs: one vector per recording, made on the device
        target = dict(vectors=voice_vectors(model.predictor, labels))
    outs = model.decode_long_batch(codes, **target, counts=counts, num_samples=[b.shape[-1] for b in batch], window=window, hop=hop,
                                   steps=args.sample_steps, constrain=True, seed=args.seed, clip_offset=first, window_batch=args.window_batch,
                                   sampler=args.sampler, eta=args.eta)
    return [wav_roundtrip(out.reshape(-1), "linear") for out in outs]


def main(argv=None):
    args = parse_args(argv)
    window = round(args.window_seconds * SAMPLE_RATE)
    hop = window - round(args.overlap_seconds * SAMPLE_RATE)
    plan_windows(1, window, hop)  # (the rules on the window flags)
    spectral = SpectralDistance()
    model = None
    try:  # before any GPU work: whatever is wrong with the pairs ends the run here
        if args.checkpoint is not None:
            model = VQVAE.load(args.checkpoint)
        pairs = read_pairs(args.pairs, args.data_dir, num_labels=None if model is None else model.num_labels, converted_dir=args.converted_dir,
                           max_pairs=args.max_pairs, limits=sample_limits(spectral))
    except ValueError as e:
        raise SystemExit(str(e))
    packs = make_packs([plan_windows(n, window, hop)[0] for _, _, _, n in pairs], args.pack_windows)
    rank, world = open_ranks("gloo")  # (only the final state travels between ranks)
    device = local_device("the decoder, the cepstra and the alignment kernel have no CPU path")
    if rank == 0:
        print(f"{len(pairs)} pairs in {len(packs)} packs")
    if model is not None:
        model.to(device)
        model.eval()
        model.set_precision(args.precision)
    aligned = AlignedDistance(spectral, PitchDistance() if args.pitch else None)
    state = ParallelState(pitch=args.pitch)
    for pack in deal_packs(packs, rank, world):
        def load(name):
            try:
                return read_wave(name)
            except Exception as e:
                raise SystemExit(f"cannot read {name}: {e}")

        sources = [load(os.path.join(args.data_dir, pairs[i][0])) for i in pack]
        targets = [torch.from_numpy(load(os.path.join(args.data_dir, pairs[i][1]))) for i in pack]
        if model is not None:
            converted = convert_run(args, model, device, sources, [pairs[i][2] for i in pack], pack[0], window, hop)
        else:
            converted = [torch.from_numpy(load(converted_path(args.converted_dir, pairs[i][0]))) for i in pack]
        state.add_scores(score_pack(aligned, converted, [torch.from_numpy(s) for s in sources], targets, device, args.pitch))
        if world == 1:
            print(f"pack of {len(pack)}: " + format_line(state.num_pairs, state.log_dict()))
    if world > 1:
        import torch.distributed as dist

        gathered = [None] * world if rank == 0 else None
        dist.gather_object(state, gathered, dst=0)
        if rank == 0:
            for other in gathered[1:]:
                state.merge(other)
    if rank == 0:
        print(format_line(state.num_pairs, state.log_dict()))
    close_ranks(world)
    return state if rank == 0 else None


if __name__ == "__main__":
    main()
