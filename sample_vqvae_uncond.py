#!/usr/bin/env python3
"""
Encode a clip with a VQ-VAE and decode it with unconditional ("classifier-free"-style) guidance towards the VQ codes and / or
the speaker label, on MI355X.  Counterpart of the reference's sample_vqvae_uncond.py (same flags and positionals; reference
sample_vqvae_uncond.py:14-92): the model is one fine-tuned by train_vqvae_uncond.py -- or a class-conditional checkpoint whose null
label `enroll_speaker.py --uncond` learned --, whose label 0 is the unconditional label (hence `--label + 1 < num_labels`).
Differences: WAV in / out directly (no ffmpeg); `--schedule` is parsed, not eval()ed;
eval mode; `--seed`, `--precision`, `--sampler {ddpm,ddim,dpmpp}` and `--eta` are new; any combination of the two guidance scales works (the reference's always-tripled
batch only lines up when both are non-zero, vq_vae.py:188-203).  `--whole-file`, `--window-seconds`, `--overlap-seconds`,
`--window-batch`, `--keep` and `--strength` are sample_vqvae.py's, with its meanings and defaults: the whole input through
`encode_long` / `decode_long_uncond_guidance`, regions of the input left as they are, a start from the noised input.  `--schedule`
works with all of them (every sampling loop takes it).  `--voice SPEC` and `--voice-at SEC:SPEC` are sample_vqvae.py's too; their
specs name speakers as `--label` does here, without the null label's offset.  `--keep-pauses`, `--min-pause`, `--pause-guard` and
`--no-skip-kept` are sample_vqvae.py's as well.
"""
import argparse
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sample_vqvae import add_voice_flags, check_voice_flags, check_voice_labels, source_kwargs, target_kwargs  # noqa: E402
from vq_voice_swap_amd import VQVAE  # noqa: E402
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter, parse_keep_range, parse_time_schedule  # noqa: E402
from vq_voice_swap_amd.corpus import add_pause_flags, check_pause_flags  # noqa: E402


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--sample-rate", type=int, default=16000)
    p.add_argument("--sample-steps", type=int, default=100)
    p.add_argument("--seconds", type=int, default=4)
    p.add_argument("--label", type=int, default=None, required=True)
    p.add_argument("--input-file", type=str, default=None, required=True)
    p.add_argument("--encoding", type=str, default="linear")
    p.add_argument("--schedule", default="lambda t: t", type=str)
    p.add_argument("--guide-label-scale", type=float, default=1.0)
    p.add_argument("--guide-vq-scale", type=float, default=0.0)
    p.add_argument("--no-vq", action="store_true")
    p.add_argument("--check-vq", action="store_true")
    p.add_argument("--seed", default=None, type=int)
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    p.add_argument("--sampler", default="ddpm", choices=["ddpm", "ddim", "dpmpp"])
    p.add_argument("--eta", type=float, default=0.0, help="DDIM noise level: 0 deterministic, 1 the DDPM step's variance (--sampler ddim)")
    p.add_argument("--whole-file", action="store_true",
                   help="convert the whole input, not its first --seconds: overlapping windows of one long signal, blended at every step")
    p.add_argument("--window-seconds", type=float, default=None, help="window length with --whole-file (default: --seconds)")
    p.add_argument("--overlap-seconds", type=float, default=0.4, help="overlap of neighbouring windows with --whole-file")
    p.add_argument("--window-batch", type=int, default=64, help="windows per forward with --whole-file")
    p.add_argument("--keep", action="append", default=[], metavar="START:END",
                   help="seconds of the input to leave as they are (repeatable; an empty side is the start / end of the file)")
    p.add_argument("--strength", type=float, default=1.0,
                   help="in (0, 1]: below 1 the conversion starts from the noised input and runs the last ceil(S * steps) steps")
    p.add_argument("checkpoint_path", type=str)
    p.add_argument("output_file", type=str)
    return p


def parse_args(argv=None):
    parser = arg_parser()
    add_voice_flags(parser)
    add_pause_flags(parser)  # (sample_vqvae.py's --keep-pauses / --min-pause / --pause-guard / --no-skip-kept)
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
    if args.window_batch < 1:
        parser.error("--window-batch must be at least 1")
    if args.whole_file and args.no_vq:
        parser.error("--no-vq is not available with --whole-file (the windows are decoded from their codes)")
    return args


def write_wave(args, sample: torch.Tensor) -> None:
    print(f"saving result to {args.output_file}...")
    writer = ChunkWriter(args.output_file, sample_rate=args.sample_rate, encoding=args.encoding)
    try:
        writer.write(sample.clamp(-1, 1).cpu().numpy().flatten())
    finally:
        writer.close()


def main(argv=None):
    args = parse_args(argv)
    schedule = parse_time_schedule(args.schedule)
    print("loading model from checkpoint...")
    model = VQVAE.load(args.checkpoint_path)
    check_voice_labels(args, model.num_labels - 1)  # (label 0 of the checkpoint is the unconditional one)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: the sampler has no CPU path")
    device = torch.device("cuda")
    model.to(device)
    model.eval()
    model.set_precision(args.precision)

    if args.whole_file:
        return convert_whole_file(args, model, schedule, device)

    print(f"loading waveform from {args.input_file}...")
    reader = ChunkReader(args.input_file, sample_rate=args.sample_rate, encoding=args.encoding)
    try:
        chunk = reader.read(args.seconds * args.sample_rate)
    finally:
        reader.close()
    rate = model.downsample_rate
    in_seq = torch.from_numpy(chunk[None, None, : (len(chunk) // rate) * rate]).to(device)

    print("encoding audio sequence...")
    encoded = model.encoder(in_seq) if args.no_vq else model.encode(in_seq)

    print("decoding audio samples...")
    sample = model.decode_uncond_guidance(encoded, **target_kwargs(args, model, device, label_offset=1), steps=args.sample_steps, progress=True, constrain=True,
                                          label_scale=args.guide_label_scale, vq_scale=args.guide_vq_scale, schedule=schedule,
                                          seed=args.seed, sampler=args.sampler, eta=args.eta, **source_kwargs(args, in_seq))

    if args.check_vq:
        assert not args.no_vq
        count = (encoded == model.encode(sample)).float().mean()
        print(f"fraction of consistent VQ codes: {count}")

    write_wave(args, sample)


def convert_whole_file(args, model, schedule, device):
    """--whole-file: every sample of the input, through `encode_long` / `decode_long_uncond_guidance`; the output has the input's
    length (sample_vqvae.py's `convert_whole_file` under guidance)."""
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
    target = target_kwargs(args, model, device, label_offset=1, windows=(encoded.shape[0], window, hop))
    sample = model.decode_long_uncond_guidance(encoded, **target, label_scale=args.guide_label_scale, vq_scale=args.guide_vq_scale,
                                               num_samples=num_samples, window=window, hop=hop, steps=args.sample_steps, progress=True,
                                               constrain=True, seed=args.seed, window_batch=args.window_batch, sampler=args.sampler,
                                               eta=args.eta, schedule=schedule, **source_kwargs(args, wave))

    if args.check_vq:
        count = (encoded == model.encode_long(sample, window, hop, args.window_batch)).float().mean()
        print(f"fraction of consistent VQ codes: {count}")

    write_wave(args, sample)


if __name__ == "__main__":
    main()
