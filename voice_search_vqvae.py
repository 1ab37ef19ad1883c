#!/usr/bin/env python3
"""
Find the speaker label under which a VQ-VAE reconstructs a clip best, on MI355X.  Counterpart of the reference's
voice_search_vqvae.py (same flags, positionals and printed table; reference voice_search_vqvae.py:17-65): read the clip, encode
it once, score it under every label at `--num-timesteps` values of t with the same noise, sort the labels by mean loss.
The num_labels x num_timesteps conditional forwards run through `speaker_search_losses`: the clip and the noise are never
copied per row (the noise is drawn inside the kernels from `--seed`).

Differences: WAV input directly (no ffmpeg); `--precision` sets the decoder's mode (default fp32; the encoder always runs in
fp32); `--seed` fixes the noise.
"""
import argparse
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import VQVAE, speaker_search_losses  # noqa: E402
from vq_voice_swap_amd.audio import ChunkReader  # noqa: E402


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--sample-rate", type=int, default=16000)
    p.add_argument("--seconds", type=int, default=4)
    p.add_argument("--encoding", type=str, default="linear")
    p.add_argument("--num-timesteps", type=int, default=16)
    p.add_argument("--num-seeds", type=int, default=1)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--top-k", type=int, default=20)
    p.add_argument("--input-file", type=str, default=None, required=True)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    p.add_argument("checkpoint_path", type=str)
    return p


def search_grid(num_labels, num_timesteps, device):
    """(labels, ts) of every pair, label-major: each label at linspace(0, 1, num_timesteps)."""
    labels = torch.arange(num_labels, device=device).repeat_interleave(num_timesteps)
    ts = torch.linspace(0.0, 1.0, steps=num_timesteps, dtype=torch.float32, device=device).repeat(num_labels)
    return labels, ts


def main(argv=None):
    args = arg_parser().parse_args(argv)
    print("loading model from checkpoint...")
    model = VQVAE.load(args.checkpoint_path)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: the model has no CPU path")
    device = torch.device("cuda")
    model.to(device)
    model.eval()
    model.set_precision(args.precision)

    print(f"loading waveform from {args.input_file}...")
    reader = ChunkReader(args.input_file, sample_rate=args.sample_rate, encoding=args.encoding)
    try:
        chunk = reader.read(args.seconds * args.sample_rate)
    finally:
        reader.close()
    if chunk is None:
        raise SystemExit(f"{args.input_file}: no audio samples")
    rate = model.downsample_rate
    usable = (len(chunk) // rate) * rate
    if usable == 0:
        raise SystemExit(f"{args.input_file}: {len(chunk)} samples are fewer than the model's downsample rate {rate}")
    in_seq = torch.from_numpy(chunk[None, None, :usable]).to(device)

    print("encoding audio sequence...")
    encoded = model.vq.embed(model.encode(in_seq)).detach()

    print("evaluating all losses...")
    labels, ts = search_grid(model.num_labels, args.num_timesteps, device)
    losses = speaker_search_losses(model, in_seq, encoded, labels, ts, args.batch_size, args.num_seeds, args.seed)
    losses = losses.reshape([-1, args.num_timesteps]).mean(-1).cpu().numpy().tolist()

    print(f"top {min(args.top_k, len(losses))} sorted losses")
    print("-------")
    for label, loss in sorted(enumerate(losses), key=lambda x: x[1])[: args.top_k]:
        print(f"{label}\t\t{loss:.6f}")


if __name__ == "__main__":
    main()
