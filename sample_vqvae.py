#!/usr/bin/env python3
"""
Encode a clip with a VQ-VAE and decode it as another speaker, on MI355X.  Counterpart of the reference's
sample_vqvae.py (same flags and positionals; reference sample_vqvae.py:76-92): read 4 s of 16 kHz audio,
`encode`, `decode(labels, constrain=True)`, clamp, write WAV; `--check-vq` re-encodes the result.
`--whole-file` (not in the reference) converts the whole input instead: `encode_long` / `decode_long` on overlapping windows.
`--sampler ddim` (with `--eta`, default 0: deterministic) samples with the DDIM step instead of the ancestral DDPM loop; with
`--source-label L` it starts from `VQVAE.invert` of the input under its own codes and label L instead of from a fresh draw.
`--keep START:END` (seconds, repeatable) leaves those ranges of the input as they are and converts the rest around them;
`--strength S` below 1 starts from the noised input instead of from pure noise.  Both work with either sampler and with `--whole-file`.
`--keep-pauses DB` leaves the pauses of the input as they are as well: runs of at least `--min-pause` seconds of 10 ms frames at or
below DB dBFS, less `--pause-guard` seconds at each end that touches speech (vq_voice_swap_amd/pauses.py).  With `--whole-file` the
windows that lie in a kept region whole are left out of the forwards (`--no-skip-kept` runs them; the output is the same).
`--voice SPEC` in place of `--label` names the target as a voice spec (vq_voice_swap_amd/speakers.py): "3:0.7,251:0.3" blends speakers,
"@voice.npy" is a vector fitted to a recording by `enroll_speaker.py --input-file`.  `--voice-at SEC:SPEC` (two or more, with
`--whole-file`) moves the voice along the file: each window takes the voice at its centre, interpolated between the points.
Differences: WAV in/out directly (no ffmpeg); the model is put in eval mode (the reference's train-mode VQ
bookkeeping crashes on current numpy; outputs are identical).  `--enc-pred-path` loads an
EncoderPredictor whose guidance gradient comes from the library's explicit backward schedule (no autograd).
"""
import argparse
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import VQVAE, EncoderPredictor  # noqa: E402
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter, keep_mask, parse_keep_range  # noqa: E402
from vq_voice_swap_amd.corpus import add_pause_flags, check_pause_flags, pause_settings, skip_kept  # noqa: E402
from vq_voice_swap_amd.pauses import pause_mask  # noqa: E402
from vq_voice_swap_amd.speakers import as_entries, morph_vectors, parse_voice, voice_vectors  # noqa: E402


def arg_parser(sampler_flags: bool = False, keep_flags: bool = False):
    """The command line.  `sampler_flags` adds --sampler / --eta / --source-label and `keep_flags` adds --keep / --strength, all of
    which `main` parses (`parse_args`); without them the parser is the one of the DDPM-only script, flag for flag."""
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    if sampler_flags:
        p.add_argument("--sampler", default="ddpm", choices=["ddpm", "ddim", "dpmpp"])
        p.add_argument("--eta", type=float, default=0.0, help="DDIM noise level: 0 deterministic, 1 the DDPM step's variance (--sampler ddim)")
        p.add_argument("--source-label", type=int, default=None,
                       help="with --sampler ddim: start from the DDIM inversion of the input under this label (the speaker it was spoken by)")
    if keep_flags:
        p.add_argument("--keep", action="append", default=[], metavar="START:END",
                       help="seconds of the input to leave as they are (repeatable; an empty side is the start / end of the file)")
        p.add_argument("--strength", type=float, default=1.0,
                       help="in (0, 1]: below 1 the conversion starts from the noised input and runs the last ceil(S * steps) steps")
    p.add_argument("--sample-rate", type=int, default=16000)
    p.add_argument("--sample-steps", type=int, default=100)
    p.add_argument("--seconds", type=int, default=4)
    p.add_argument("--label", type=int, default=None, required=True)
    p.add_argument("--input-file", type=str, default=None, required=True)
    p.add_argument("--encoding", type=str, default="linear")
    p.add_argument("--enc-pred-path", type=str, default=None)
    p.add_argument("--enc-pred-scale", type=float, default=1.0)
    p.add_argument("--no-vq", action="store_true")
    p.add_argument("--check-vq", action="store_true")
    p.add_argument("--seed", default=None, type=int)
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    p.add_argument("--whole-file", action="store_true",
                   help="convert the whole input, not its first --seconds: overlapping windows of one long signal, blended at every step")
    p.add_argument("--window-seconds", type=float, default=None, help="window length with --whole-file (default: --seconds)")
    p.add_argument("--overlap-seconds", type=float, default=0.4, help="overlap of neighbouring windows with --whole-file")
    p.add_argument("--window-batch", type=int, default=64, help="windows per forward with --whole-file")
    p.add_argument("checkpoint_path", type=str)
    p.add_argument("output_file", type=str)
    return p


def add_voice_flags(parser) -> None:
    """--voice / --voice-at beside --label, which stops being required on its own: `check_voice_flags` asks for exactly one target.
    (They join in `parse_args`: `arg_parser()` stays the flag set it was.)"""
    for action in parser._actions:
        if "--label" in action.option_strings:
            action.required = False
    parser.add_argument("--voice", type=str, default=None, metavar="SPEC",
                        help="the target as a voice spec instead of --label: a label, a blend `3:0.7,251:0.3`, a vector file `@voice.npy`")
    parser.add_argument("--voice-at", action="append", default=[], metavar="SEC:SPEC",
                        help="with --whole-file, two or more times: the voice at that second of the file; windows between two points blend them")


def check_voice_flags(parser, args) -> None:
    """Exactly one of --label / --voice / --voice-at; args.voice_at becomes the sorted-as-given [(seconds, spec)]."""
    points = []
    for text in args.voice_at:
        sec, sep, spec = text.partition(":")
        try:
            if not sep:
                raise ValueError(f"--voice-at {text!r}: expected SEC:SPEC")
            parse_voice(spec)
            points.append((float(sec), spec))
        except ValueError as e:
            parser.error(str(e) if "voice" in str(e) else f"--voice-at {text!r}: {sec!r} is not a number of seconds")
    args.voice_at = points
    if (args.label is not None) + (args.voice is not None) + bool(points) != 1:
        parser.error("give exactly one target: --label, --voice or --voice-at")
    if args.voice is not None:
        try:
            parse_voice(args.voice)
        except ValueError as e:
            parser.error(str(e))
    if points:
        if not args.whole_file:
            parser.error("--voice-at moves the voice along a whole file: it needs --whole-file")
        if len(points) < 2:
            parser.error("--voice-at needs at least two points (one voice for the whole file is --voice)")
        if any(b[0] <= a[0] for a, b in zip(points, points[1:])) or points[0][0] < 0:
            parser.error("--voice-at points must be given in order of strictly increasing, non-negative seconds")


def check_voice_labels(args, speakers: int) -> None:
    """The labels that --label / --voice / --voice-at name against the model's speaker count (before any device work)."""
    specs = [args.label] if args.label is not None else [args.voice] if args.voice is not None else [spec for _, spec in args.voice_at]
    bad = sorted({l for spec in specs for l, _ in as_entries(spec) if not isinstance(l, str) and not 0 <= l < speakers})
    if bad:
        raise SystemExit(f"labels {bad} outside the model's speakers 0..{speakers - 1}")


def target_kwargs(args, model, device, label_offset: int = 0, windows=None):
    """The decode keywords that name the target: labels= for --label, vectors= for --voice ([1,E]) and --voice-at (`windows` =
    (n, window, hop): [n,E], one per window).  `label_offset` 1: a checkpoint with the null label in front, for the VECTORS only --
    the guided decode offsets labels itself."""
    if args.voice_at:
        n, window, hop = windows
        return dict(vectors=morph_vectors(model.predictor, args.voice_at, n, window, hop, args.sample_rate, label_offset))
    if args.voice is not None:
        return dict(vectors=voice_vectors(model.predictor, [args.voice], label_offset))
    return dict(labels=torch.tensor([args.label]).long().to(device))


def parse_args(argv=None):
    parser = arg_parser(sampler_flags=True, keep_flags=True)
    add_voice_flags(parser)
    add_pause_flags(parser)  # (--keep-pauses / --min-pause / --pause-guard / --no-skip-kept join here, as the voice flags do)
    args = parser.parse_args(argv)
    check_voice_flags(parser, args)
    check_pause_flags(parser, args)
    if args.sampler != "ddim" and args.eta:
        parser.error("--eta belongs to --sampler ddim (ddpm has its own variance, dpmpp is deterministic)")
    if args.eta < 0:
        parser.error("--eta must not be negative")
    try:
        args.keep = [parse_keep_range(text) for text in args.keep]
    except ValueError as e:
        parser.error(str(e))
    if not 0.0 < args.strength <= 1.0:
        parser.error("--strength must lie in (0, 1]")
    if args.source_label is not None and (args.keep or args.strength < 1 or hasattr(args, "keep_pauses")):
        parser.error("--source-label starts from the inverted input: it cannot be combined with --keep, --keep-pauses or --strength")
    if args.source_label is not None:
        if args.sampler != "ddim":
            parser.error("--source-label needs --sampler ddim (the inversion is the DDIM step run backwards)")
        if args.whole_file:
            parser.error("--source-label is not available with --whole-file")
        if args.no_vq:
            parser.error("--source-label is not available with --no-vq")
    return args


def source_kwargs(args, wave: torch.Tensor):
    """decode's source / keep / strength keywords for the input `wave` [1,1,N]: nothing unless --keep, --keep-pauses or --strength
    asks.  With --whole-file the pauses are `decode_long`'s to find (keep_pauses= / skip_kept=, on the padded row); a clip's are found
    here -- a pack of one recording of one window, without overlap -- and OR-ed into the mask."""
    pauses = pause_settings(args, args.sample_rate)
    if not args.keep and args.strength == 1.0 and pauses is None:
        return {}
    kw = dict(source=wave, strength=args.strength)
    if args.keep:
        mask = keep_mask(args.keep, wave.shape[-1], args.sample_rate)
        print(f"keeping {mask.mean():.1%} of the input ({int(mask.sum())} of {mask.size} samples)")
        kw["keep"] = torch.from_numpy(mask[None, None]).to(wave.device)
    if pauses is not None and args.whole_file:
        kw.update(keep_pauses=pauses, skip_kept=skip_kept(args))
    elif pauses is not None:
        found = pause_mask(wave, [1], wave.shape[-1], wave.shape[-1], **pauses)
        print(f"keeping {float(found.float().mean()):.1%} of the input as pauses")
        kw["keep"] = found if "keep" not in kw else torch.bitwise_or(kw["keep"].to(torch.uint8), found)
    return kw


def main(argv=None):
    args = parse_args(argv)
    print("loading model from checkpoint...")
    model = VQVAE.load(args.checkpoint_path)
    check_voice_labels(args, model.num_labels)
    assert args.source_label is None or 0 <= args.source_label < model.num_labels
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: the sampler has no CPU path")
    device = torch.device("cuda")
    model.to(device)
    model.eval()
    model.set_precision(args.precision)
    enc_pred = None
    if args.enc_pred_path:  # reference sample_vqvae.py:24-28
        print("loading encoder predictor")
        enc_pred = EncoderPredictor.load(args.enc_pred_path).to(device)
        enc_pred.eval()
        enc_pred.set_precision(args.precision)

    if args.whole_file:
        return convert_whole_file(args, model, enc_pred, device)

    print(f"loading waveform from {args.input_file}...")
    reader = ChunkReader(args.input_file, sample_rate=args.sample_rate, encoding=args.encoding)
    try:
        chunk = reader.read(args.seconds * args.sample_rate)
    finally:
        reader.close()
    rate = model.downsample_rate  # 256 behind a UNet encoder, lcm(256, 320) = 1280 behind the MFCC encoder (4 s = 64000 fits both)
    usable = (len(chunk) // rate) * rate
    in_seq = torch.from_numpy(chunk[None, None, :usable]).to(device)

    print("encoding audio sequence...")
    encoded = model.encoder(in_seq) if args.no_vq else model.encode(in_seq)

    print("decoding audio samples...")
    x_T = None
    if args.source_label is not None:
        print("inverting the input to its latent...")
        x_T = model.invert(in_seq, torch.tensor([args.source_label]).long().to(device), steps=args.sample_steps, codes=encoded)
    sample = model.decode(encoded, **target_kwargs(args, model, device), steps=args.sample_steps, progress=True, constrain=True, seed=args.seed,
                          enc_pred=enc_pred, enc_pred_scale=args.enc_pred_scale, x_T=x_T, sampler=args.sampler, eta=args.eta,
                          **source_kwargs(args, in_seq))

    if args.check_vq:
        assert not args.no_vq
        count = (encoded == model.encode(sample)).float().mean()
        print(f"fraction of consistent VQ codes: {count}")

    print(f"saving result to {args.output_file}...")
    writer = ChunkWriter(args.output_file, sample_rate=args.sample_rate, encoding=args.encoding)
    try:
        writer.write(sample.clamp(-1, 1).cpu().numpy().flatten())
    finally:
        writer.close()


def convert_whole_file(args, model, enc_pred, device):
    """--whole-file: every sample of the input, through `encode_long` / `decode_long`; the output has the input's length."""
    if args.no_vq:
        raise SystemExit("--no-vq is not available with --whole-file")
    window = round((args.seconds if args.window_seconds is None else args.window_seconds) * args.sample_rate)
    hop = window - round(args.overlap_seconds * args.sample_rate)
    print(f"loading waveform from {args.input_file}...")
    reader = ChunkReader(args.input_file, sample_rate=args.sample_rate, encoding=args.encoding)
    try:
        chunks = []
        while (chunk := reader.read(1 << 20)) is not None:
            chunks.append(chunk)
    finally:
        reader.close()
    if not chunks:
        raise SystemExit(f"{args.input_file} holds no samples")
    wave = torch.from_numpy(np.concatenate(chunks)[None, None]).to(device)
    num_samples = wave.shape[-1]

    print(f"encoding {num_samples} samples in windows of {window} every {hop}...")
    encoded = model.encode_long(wave, window, hop, args.window_batch)

    print(f"decoding {encoded.shape[0]} windows...")
    target = target_kwargs(args, model, device, windows=(encoded.shape[0], window, hop))
    sample = model.decode_long(encoded, **target, num_samples=num_samples, window=window, hop=hop, steps=args.sample_steps, progress=True,
                               constrain=True, seed=args.seed, enc_pred=enc_pred, enc_pred_scale=args.enc_pred_scale,
                               window_batch=args.window_batch, sampler=args.sampler, eta=args.eta, **source_kwargs(args, wave))

    if args.check_vq:
        count = (encoded == model.encode_long(sample, window, hop, args.window_batch)).float().mean()
        print(f"fraction of consistent VQ codes: {count}")

    print(f"saving result to {args.output_file}...")
    writer = ChunkWriter(args.output_file, sample_rate=args.sample_rate, encoding=args.encoding)
    try:
        writer.write(sample.clamp(-1, 1).cpu().numpy().flatten())
    finally:
        writer.close()


if __name__ == "__main__":
    main()
