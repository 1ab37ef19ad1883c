#!/usr/bin/env python3
"""
Convert every recording of a data set to a target speaker, on MI355X (not in the reference, which converts one clip).

    python convert_dataset.py model_vqvae.pt data/ out/ --label 7 --sampler dpmpp --sample-steps 25 --precision fp16
    torchrun --nproc-per-node 8 convert_dataset.py model_vqvae.pt data/ out/ --label-map targets.tsv

The files of `data_dir` (the walk of the eval scripts: WAV files below top-level directories) are sorted by relative path; a file's
global id is its place in that list.  Files are taken in order into packs of at most `--pack-windows` windows, the packs are dealt
to the ranks, and a pack runs `VQVAE.encode_long_batch` -> `decode_long_batch`: the windows of all its recordings fill the forwards
together and ONE packed step kernel follows, so a corpus of short utterances runs at the rate of full batches.  Each result goes to
`out_dir/<relative path>` (extension .wav) and has its input's length.

A file's output depends on (checkpoint, flags, --seed, its global id) only: not on --pack-windows, --window-batch or the number of
ranks, and with `--whole-file` flags to match it is what `sample_vqvae.py --whole-file` writes for the file with id 0.  So a run that
was interrupted resumes with `--skip-existing` and ends with the files an uninterrupted run would have written.
`--label N` converts everything to speaker N; `--label-map FILE` (lines `top-level-directory<TAB>label`) picks the target by the
file's top-level directory.  An unreadable or empty file is skipped with a warning and counted.

`--guide-label-scale S` / `--guide-vq-scale S` (both off by default) decode with the classifier-free-style guidance of
sample_vqvae_uncond.py (`VQVAE.decode_long_batch_uncond_guidance`).  With either set the checkpoint is taken to have the unconditional
label at 0 (`enroll_speaker.py --uncond` makes one) and `--label` / `--label-map` are speaker numbers WITHOUT that offset; a file's
output is then what `sample_vqvae_uncond.py --whole-file` writes for the file with id 0 under the same scales.

`--voice SPEC` converts everything to a voice given as a spec (vq_voice_swap_amd/speakers.py: "3:0.7,251:0.3" a blend of speakers,
"@voice.npy" a vector file of `enroll_speaker.py --input-file`), and the second column of `--label-map` may be a spec as well.
`--anonymize K` gives every top-level directory a voice that is nobody's: `pseudo_voice(--seed, directory, speakers, K)`, a convex blend
of K speakers that depends on the seed and the directory's name alone; the mapping goes to `out_dir/pseudo_voices.tsv` (a label map this
script reads back).  A file's output then depends on (checkpoint, flags, --seed, its directory's name, its global id) only, and is what
`sample_vqvae.py --whole-file --voice <the spec>` writes for the file with id 0.

`--strength S` and `--keep-pauses DB` (with `--min-pause`, `--pause-guard`, `--no-skip-kept`) are sample_vqvae.py's: the conversion
starts from the noised input, and the pauses of every recording -- runs of 10 ms frames at or below DB dBFS -- come out as they went
in, bit for bit.  Windows that lie in a pause whole are left out of the forwards, which changes no output
bit; the final line then also reports the seconds kept and the windows skipped.
"""
import argparse
import os
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import VQVAE, EncoderPredictor  # noqa: E402
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter  # noqa: E402
from vq_voice_swap_amd.corpus import (add_guidance_flags, add_pause_flags, check_pause_flags, deal_packs, guided, list_files, make_packs,  # noqa: E402
                                      pause_settings, read_label_map, skip_kept, top_directory)
from vq_voice_swap_amd.dataset import build_file_index  # noqa: E402
from vq_voice_swap_amd.eval_pass import close_ranks, local_device, open_ranks  # noqa: E402
from vq_voice_swap_amd.longform import plan_windows  # noqa: E402
from vq_voice_swap_amd.speakers import as_entries, parse_voice, pseudo_voice, voice_vectors  # noqa: E402

SAMPLE_RATE = 16000


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    target = p.add_mutually_exclusive_group(required=True)
    target.add_argument("--label", type=int, default=None, help="the speaker every file is converted to")
    target.add_argument("--label-map", type=str, default=None, metavar="FILE",
                        help="lines `top-level-directory<TAB>label`: the target speaker of the files below each directory")
    p.add_argument("--sampler", default="ddpm", choices=["ddpm", "ddim", "dpmpp"])
    p.add_argument("--eta", type=float, default=0.0, help="DDIM noise level: 0 deterministic, 1 the DDPM step's variance (--sampler ddim)")
    p.add_argument("--sample-steps", type=int, default=100)
    p.add_argument("--window-seconds", type=float, default=4.0, help="window length (the length the model was trained on)")
    p.add_argument("--overlap-seconds", type=float, default=0.4, help="overlap of neighbouring windows")
    p.add_argument("--window-batch", type=int, default=64, help="windows per forward")
    p.add_argument("--pack-windows", type=int, default=512, help="windows of the recordings converted together")
    p.add_argument("--enc-pred-path", type=str, default=None)
    p.add_argument("--enc-pred-scale", type=float, default=1.0)
    p.add_argument("--encoding", type=str, default="linear")
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--max-files", default=None, type=int, help="convert the first this many files of the sorted list")
    p.add_argument("--skip-existing", action="store_true", help="leave a file whose output exists alone: resume an interrupted run")
    p.add_argument("checkpoint_path", type=str)
    p.add_argument("data_dir", type=str)
    p.add_argument("out_dir", type=str)
    return p


def parse_args(argv=None):
    parser = arg_parser()
    add_guidance_flags(parser)  # (they join here: `arg_parser()` stays the flag set of the unguided run, which they leave as it was)
    # the voice targets join the group of --label / --label-map here, for the same reason; a flag that is not given leaves no
    # attribute behind (`voice_of` / `anonymize_of` read them), so the namespace of a run without them is what it was
    target = parser._mutually_exclusive_groups[0]
    target.add_argument("--voice", type=str, default=argparse.SUPPRESS, metavar="SPEC",
                        help="the voice every file is converted to: a label, a blend `3:0.7,251:0.3`, a vector file `@voice.npy`")
    target.add_argument("--anonymize", type=int, default=argparse.SUPPRESS, metavar="K",
                        help="every top-level directory gets a pseudo-voice blended of K speakers, listed in out_dir/pseudo_voices.tsv")
    # ... and --strength and the pause flags, likewise
    parser.add_argument("--strength", type=float, default=argparse.SUPPRESS,
                        help="in (0, 1]: below 1 the conversion starts from the noised input and runs the last ceil(S * steps) steps")
    add_pause_flags(parser)
    args = parser.parse_args(argv)
    if not 0.0 < strength_of(args) <= 1.0:
        parser.error("--strength must lie in (0, 1]")
    check_pause_flags(parser, args)
    if voice_of(args) is not None:
        try:
            parse_voice(args.voice)
        except ValueError as e:
            parser.error(str(e))
    if anonymize_of(args) is not None and not 1 <= args.anonymize <= 8:
        parser.error("--anonymize takes 1..8 speakers per pseudo-voice")
    if args.sampler != "ddim" and args.eta:
        parser.error("--eta belongs to --sampler ddim (ddpm has its own variance, dpmpp is deterministic)")
    if args.eta < 0:
        parser.error("--eta must not be negative")
    if args.pack_windows < 1 or args.window_batch < 1:
        parser.error("--pack-windows and --window-batch must be at least 1")
    if args.max_files is not None and args.max_files < 1:
        parser.error("--max-files must be at least 1")
    return args


def voice_of(args):
    return getattr(args, "voice", None)


def anonymize_of(args):
    return getattr(args, "anonymize", None)


def strength_of(args) -> float:
    return getattr(args, "strength", 1.0)


def keeps_source(args) -> bool:
    """Whether the run hands the recordings themselves to the decoder: --strength below 1 or --keep-pauses."""
    return strength_of(args) < 1.0 or getattr(args, "keep_pauses", None) is not None


def summary(args, totals, seconds: float) -> str:
    """The final line; with --strength or the pause flags it also says what was kept and skipped."""
    line = (f"{int(totals[0])} files written, {int(totals[1])} skipped: {totals[2] / SAMPLE_RATE:.1f} s of audio, {int(totals[3])} windows, "
            f"{int(totals[4])} packs in {seconds:.1f} s")
    if keeps_source(args) or hasattr(args, "no_skip_kept"):
        line += f", kept {totals[5] / SAMPLE_RATE:.1f} s, skipped {int(totals[6])} of {int(totals[3])} windows"
    return line


def out_path(out_dir: str, rel: str) -> str:
    return os.path.join(out_dir, os.path.splitext(rel)[0] + ".wav")


def plan(args, window: int, hop: int):
    """Everything that needs no device: (files, labels by id, packs of ids of ALL ranks).  Raises ValueError for a bad label map.
    A label is an int, or a voice spec as text (--voice, a spec in the label map); under --anonymize it is the file's top-level
    directory for now: `main` turns the directories into pseudo-voices once the checkpoint says how many speakers there are."""
    files = list_files(build_file_index(args.data_dir))
    if args.max_files is not None:
        files = files[:args.max_files]
    if args.label_map is not None:
        mapping = read_label_map(args.label_map, sorted({top_directory(rel) for rel, _ in files}))
        labels = [mapping[top_directory(rel)] for rel, _ in files]
    elif anonymize_of(args) is not None:
        labels = [top_directory(rel) for rel, _ in files]
    elif voice_of(args) is not None:
        labels = [args.voice] * len(files)
    else:
        labels = [args.label] * len(files)
    ids = [i for i, (rel, _) in enumerate(files) if not (args.skip_existing and os.path.exists(out_path(args.out_dir, rel)))]
    windows = [plan_windows(max(1, int(files[i][1] * SAMPLE_RATE)), window, hop)[0] for i in ids]
    return files, labels, make_packs(windows, args.pack_windows, ids)


def read_wave(path: str, encoding: str):
    """The whole file as float32 [N], or None (with a warning) when it cannot be read or holds no sample."""
    try:
        reader = ChunkReader(path, sample_rate=SAMPLE_RATE, encoding=encoding)
        try:
            chunks = []
            while (chunk := reader.read(1 << 20)) is not None:
                chunks.append(chunk)
        finally:
            reader.close()
    except Exception as e:  # (a corpus run goes on past one bad file)
        print(f"warning: skipping {path}: {e}", file=sys.stderr)
        return None
    if not chunks:
        print(f"warning: skipping {path}: no samples", file=sys.stderr)
        return None
    return np.concatenate(chunks)


def convert_pack(args, model, enc_pred, device, files, labels, pack, window: int, hop: int):
    """One pack of consecutive ids -> (files written, files skipped, samples, windows, decode calls, samples kept, windows skipped).
    A file that cannot be read leaves a gap in the ids, so the rest of the pack is decoded as runs of consecutive ids (`make_packs` on
    what was read)."""
    waves = {i: w for i in pack if (w := read_wave(os.path.join(args.data_dir, files[i][0]), args.encoding)) is not None}
    got = sorted(waves)
    written = samples = windows = calls = kept = skipped = 0
    counts = [plan_windows(waves[i].size, window, hop)[0] for i in got]
    for run in make_packs(counts, max(args.pack_windows, max(counts, default=1)), got):
        batch = [torch.from_numpy(waves[i][None, None]).to(device) for i in run]
        codes, run_counts = model.encode_long_batch(batch, window, hop, args.window_batch)
        decode, guide_kw = model.decode_long_batch, {}
        if guided(args):  # (labels are not offset here: the guided decode shifts them past the unconditional label itself)
            decode, guide_kw = model.decode_long_batch_uncond_guidance, dict(label_scale=args.guide_label_scale, vq_scale=args.guide_vq_scale)
        if all(isinstance(labels[i], int) for i in run):
            target = torch.tensor([labels[i] for i in run]).long().to(device)
        else:  # voice specs: one vector per recording, made on the device (specs name speakers without the null label's offset)
            target = None
            guide_kw["vectors"] = voice_vectors(model.predictor, [labels[i] for i in run], label_offset=1 if guided(args) else 0)
        stats = {}
        if keeps_source(args):
            guide_kw.update(sources=batch, strength=strength_of(args), keep_pauses=pause_settings(args, SAMPLE_RATE), skip_kept=skip_kept(args),
                            stats=stats)
        outs = decode(codes, target, counts=run_counts, num_samples=[b.shape[-1] for b in batch], window=window, hop=hop,
                      steps=args.sample_steps, constrain=True, seed=args.seed, clip_offset=run[0], enc_pred=enc_pred,
                      enc_pred_scale=args.enc_pred_scale, window_batch=args.window_batch, sampler=args.sampler, eta=args.eta, **guide_kw)
        for i, out in zip(run, outs):
            path = out_path(args.out_dir, files[i][0])
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            writer = ChunkWriter(path + ".part", sample_rate=SAMPLE_RATE, encoding=args.encoding)
            try:
                writer.write(out.clamp(-1, 1).cpu().numpy().flatten())
            finally:
                writer.close()
            os.replace(path + ".part", path)  # (an interrupted run leaves no half-written output for --skip-existing to trust)
            written += 1
            samples += out.shape[-1]
        windows += sum(run_counts)
        calls += 1
        kept += stats.get("kept_samples", 0)
        skipped += stats.get("skipped_windows", 0)
    return written, len(pack) - len(got), samples, windows, calls, kept, skipped


def main(argv=None):
    args = parse_args(argv)
    window = round(args.window_seconds * SAMPLE_RATE)
    hop = window - round(args.overlap_seconds * SAMPLE_RATE)
    plan_windows(1, window, hop)  # (the rules on the window flags)
    try:
        files, labels, packs = plan(args, window, hop)  # before any GPU work: a bad label map ends the run here
    except ValueError as e:
        raise SystemExit(str(e))
    rank, world = open_ranks("gloo")  # (only the final counts travel between ranks)
    device = local_device("the sampler has no CPU path")
    if rank == 0:
        print(f"{len(files)} files, {sum(len(p) for p in packs)} to convert in {len(packs)} packs; loading model from checkpoint...")
    model = VQVAE.load(args.checkpoint_path)
    speakers = model.num_labels - 1 if guided(args) else model.num_labels  # (guided: label 0 of the checkpoint is the unconditional one)
    if anonymize_of(args) is not None:
        try:
            voices = {d: pseudo_voice(args.seed, d, speakers, args.anonymize) for d in sorted(set(labels))}
        except ValueError as e:
            raise SystemExit(str(e))
        labels = [voices[d] for d in labels]
        if rank == 0:
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, "pseudo_voices.tsv"), "w") as f:
                f.write("".join(f"{d}\t{spec}\n" for d, spec in voices.items()))
    bad = sorted({l for spec in set(labels) for l, _ in as_entries(spec) if not isinstance(l, str) and not 0 <= l < speakers})
    if bad:
        raise SystemExit(f"labels {bad} outside the model's 0..{speakers - 1}" + (" (speakers, the unconditional label not counted)" if guided(args) else ""))
    model.to(device)
    model.eval()
    model.set_precision(args.precision)
    enc_pred = None
    if args.enc_pred_path:
        enc_pred = EncoderPredictor.load(args.enc_pred_path).to(device)
        enc_pred.eval()
        enc_pred.set_precision(args.precision)

    start = time.time()
    totals = np.zeros(7, dtype=np.int64)  # written, skipped, samples, windows, packs, samples kept, windows skipped
    for pack in deal_packs(packs, rank, world):
        done = np.array(convert_pack(args, model, enc_pred, device, files, labels, pack, window, hop), dtype=np.int64)
        totals[:len(done)] += done
    if world > 1:
        import torch.distributed as dist

        gathered = [None] * world if rank == 0 else None
        dist.gather_object(totals, gathered, dst=0)
        if rank == 0:
            totals = np.sum(gathered, axis=0)
    if rank == 0:
        print(summary(args, totals, time.time() - start))
    close_ranks(world)
    return totals


if __name__ == "__main__":
    main()
