"""
The one sharded evaluation pass behind the eval_*.py scripts (host logic only): the common command line, the rank and device
plumbing, the loop that deals the batches of a seeded, shuffled loader round-robin to the ranks, and the merge on rank 0.

A script supplies `build(device, num_labels) -> (state, score)`: its models live in that closure.  `score(audio, data_batch, first)`
folds one batch into `state`; `first` is the position of the batch's first clip in the shuffled pass, the key of everything random,
so the printed line does not depend on the batch size or the rank count.  A state has `num_samples`, `log_dict()`, `merge(other)`
and `to_host()` (whatever lives on the device moves to the host, so that the state can be sent to rank 0).
"""
import argparse
import os

import torch

from .dataset import create_data_loader


def common_parser():
    """The flags and positionals every evaluation script has; a script adds its own."""
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--batch-size", type=int, default=4)
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--max-samples", default=None, type=int, help="stop after this many clips (default: one pass over the data)")
    p.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend when WORLD_SIZE > 1")
    p.add_argument("checkpoint_path", type=str)
    p.add_argument("data_dir", type=str)
    return p


def format_line(num_samples, log):
    msg = " ".join(f"{key}={value}" if isinstance(value, int) else f"{key}={value:.06f}" for key, value in log.items())
    return f"{num_samples} samples: {msg}"


def open_ranks(backend):
    """(rank, world) of this process; under torchrun (WORLD_SIZE > 1) the process group is opened first."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return 0, 1
    import torch.distributed as dist

    dist.init_process_group(backend)
    return dist.get_rank(), world


def close_ranks(world):
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()


def local_device(what):
    """This rank's device, selected; `what` says which part of the script has no CPU path."""
    if not torch.cuda.is_available():
        raise SystemExit(f"no ROCm device visible: {what}")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    torch.cuda.set_device(device)
    return device


def score_batches(data_loader, state, score, device, *, batch_size, max_samples, rank, world):
    """This rank's batches of the pass, each scored once; a single rank prints a line per batch."""
    for i, data_batch in enumerate(data_loader):
        first = (rank + i * world) * batch_size  # position of the batch's first clip in the shuffled pass
        if max_samples is not None and first + batch_size > max_samples:
            break
        score(data_batch["samples"][:, None].to(device), data_batch, first)
        if world == 1:
            print(format_line(state.num_samples, state.log_dict()))


def merge_ranks(state, rank, world):
    """The whole pass's state on rank 0 (the other ranks' states merged into its own in rank order; it prints the one line), None
    elsewhere."""
    if world > 1:
        import torch.distributed as dist

        gathered = [None] * world if rank == 0 else None
        dist.gather_object(state.to_host(), gathered, dst=0)
        if rank == 0:
            for other in gathered[1:]:
                state.merge(other)
            print(format_line(state.num_samples, state.log_dict()))
    return state if rank == 0 else None


def run_pass(args, build, *, no_device, check_data=None):
    """One pass of a script over `args.data_dir`.  `check_data(num_labels)` may refuse the command line once the data is known,
    before a device is required; `no_device` is the script's wording for a machine without one."""
    rank, world = open_ranks(args.dist_backend)
    data_loader, num_labels = create_data_loader(directory=args.data_dir, batch_size=args.batch_size, seed=args.seed, rank=rank, world=world)
    if check_data is not None:
        check_data(num_labels)
    device = local_device(no_device)
    if rank == 0:
        print("loading model from checkpoint...")
    state, score = build(device, num_labels)
    score_batches(data_loader, state, score, device, batch_size=args.batch_size, max_samples=args.max_samples, rank=rank, world=world)
    merged = merge_ranks(state, rank, world)
    close_ranks(world)
    return merged
