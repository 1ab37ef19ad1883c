#!/usr/bin/env python3
"""
Noise-prediction MSE of a diffusion model over a data set, averaged per quartile of t, on MI355X.  Counterpart of the
reference's eval_diffusion.py (same positionals and --batch-size, same output line after every batch:
"{n} samples: q0=... q1=..."; reference eval_diffusion.py:14-45): one pass over the shuffled loader, t uniform per clip,
`Diffusion.denoising_losses` (fused noising and squared-error kernels around the HIP UNet), a `LossTracker` of window 10^6.

Differences: `data_dir` is "tones" or a LibriSpeech-layout tree of WAV files; `--precision` (default fp32, the reference's
arithmetic); `--seed` fixes the loader's order, every clip's t and its noise (keyed by the clip's position in that order, so
the result does not depend on the rank count); `--max-samples` ends the pass early.  Under torchrun (WORLD_SIZE > 1) the
batches are dealt round-robin to the ranks, the trackers are merged on rank 0, and rank 0 prints the one final line.
"""
import argparse
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import DiffusionModel, LossTracker, create_data_loader  # noqa: E402


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--batch-size", type=int, default=4)
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--max-samples", default=None, type=int, help="stop after this many clips (default: one pass over the data)")
    p.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend when WORLD_SIZE > 1")
    p.add_argument("checkpoint_path", type=str)
    p.add_argument("data_dir", type=str)
    return p


def format_line(num_samples, tracker):
    msg = " ".join(f"{key}={value:.06f}" for key, value in tracker.log_dict().items())
    return f"{num_samples} samples: {msg}"


def main(argv=None):
    args = arg_parser().parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = 0
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group(args.dist_backend)
        rank = dist.get_rank()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: the predictor has no CPU path")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    torch.cuda.set_device(device)

    data_loader, _ = create_data_loader(directory=args.data_dir, batch_size=args.batch_size, seed=args.seed, rank=rank, world=world)
    if rank == 0:
        print("loading model from checkpoint...")
    model = DiffusionModel.load(args.checkpoint_path).to(device)
    model.eval()
    model.set_precision(args.precision)

    tracker = LossTracker(avg_size=1_000_000)
    num_samples = 0
    for i, data_batch in enumerate(data_loader):
        first = (rank + i * world) * args.batch_size  # position of the batch's first clip in the shuffled pass
        if args.max_samples is not None and first + args.batch_size > args.max_samples:
            break
        audio_seq = data_batch["samples"][:, None].to(device)
        ts = model.diffusion.draw_ts(len(audio_seq), args.seed, first)
        losses = model.diffusion.denoising_losses(audio_seq, model.predictor, ts, seed=args.seed, clip_offset=first)
        tracker.add(ts, losses)
        num_samples += len(ts)
        if world == 1:
            print(format_line(num_samples, tracker))
    if world > 1:
        import torch.distributed as dist

        gathered = [None] * world if rank == 0 else None
        dist.gather_object((num_samples, tracker), gathered, dst=0)
        if rank == 0:
            total, merged = 0, LossTracker(avg_size=1_000_000)
            for n, t in gathered:
                total += n
                merged.merge(t)
            print(format_line(total, merged))
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
