#!/usr/bin/env python3
"""
Evaluate a VQ-VAE checkpoint over a data set on MI355X: how well the codebook fits the encoder (vq_loss), how many codes are
alive (used_codes, perplexity), and how much the decoder leverages labels -- how much worse the noise-prediction loss becomes
when the label is randomised (the purpose and the command line of the reference's eval_vqvae.py: `--batch-size`,
`checkpoint_path`, `data_dir`; its body imports classes the reference no longer has, so only those are taken from it).

One pass over the shuffled loader.  Per batch: `VQVAE.losses` with the true labels (encoder, one fused quantise-and-score
kernel, fused noising / squared-error kernels around the HIP decoder), then the decoder half again on the SAME x_t -- same t,
same noise -- with a wrong label per clip, (label + r) % num_labels with r uniform in 1 .. num_labels - 1: never the true one.
After every batch one line:

    {n} samples: cond_q0=... cond_q3=... rand_q0=... rand_q3=... vq_loss=... used_codes=... perplexity=...

cond_q* / rand_q* are the per-quartile-of-t averages with the true / wrong labels (`LossTracker`, window 10^6; rand_* is left
out when the model has fewer than two labels), vq_loss the StandardVQLoss over every clip so far, used_codes and perplexity
those of the accumulated code histogram.  The reference's per-quartile output-std hook is not rebuilt: it measured a module
that no longer exists.

`data_dir`, `--precision`, `--seed`, `--max-samples` and `--dist-backend` are those of eval_diffusion.py: everything random is
keyed by the seed and the clip's position in the shuffled pass, so the result does not depend on the rank count.  Under
torchrun (WORLD_SIZE > 1) batches are dealt round-robin, rank 0 merges the trackers, adds the histograms and the error sums,
and prints the one final line.
"""
import argparse
import os
import sys
from fractions import Fraction

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import LossTracker, StandardVQLoss, VQVAE, code_usage, create_data_loader  # noqa: E402


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


def wrong_labels(labels: torch.Tensor, num_labels: int, seed: int, first: int) -> torch.Tensor:
    """(label + r) % num_labels with r uniform in 1 .. num_labels - 1 from a host generator seeded by (seed, first): in range,
    never the label itself, the same for the same (seed, first)."""
    if num_labels < 2:
        raise ValueError("a wrong label needs at least two labels")
    g = torch.Generator().manual_seed((int(seed) * 0xD1B54A32D192ED03 + 0x9E3779B97F4A7C15 * (int(first) + 1) + 0x5851F42D4C957F2D) % (2 ** 63))
    r = torch.randint(1, num_labels, (len(labels),), generator=g)
    return ((labels.detach().cpu().to(torch.int64) + r) % num_labels).to(labels.device)


class EvalState:
    """What one pass accumulates: the two trackers, the clip count, the summed quantisation error with its element count, and
    the code histogram (int64, on the device the batches run on)."""

    def __init__(self, num_codes: int, device, commitment: float = 0.25):
        self.cond = LossTracker(avg_size=1_000_000, prefix="cond_")
        self.rand = LossTracker(avg_size=1_000_000, prefix="rand_")
        self.loss_fn = StandardVQLoss(commitment)
        self.num_samples = 0
        self.sq_err = Fraction(0)  # EXACT sum of the clips' float64 sums: the same whatever order batches and shards arrive in
        self.numel = 0      # encoder-output elements behind it
        self.hist = torch.zeros(num_codes, dtype=torch.int64, device=device)

    def add_batch(self, model: VQVAE, audio: torch.Tensor, labels, first: int, seed: int) -> None:
        """Score one batch whose first clip is clip `first` of the pass."""
        n = len(audio)
        ts = model.diffusion.draw_ts(n, seed, first)
        out = model.losses(self.loss_fn, audio, labels, ts=ts, seed=seed, clip_offset=first, hist=self.hist)
        self.cond.add(out["ts"], out["mses"])
        if labels is not None and (model.num_labels or 0) > 1:
            wrong = wrong_labels(labels, model.num_labels, seed, first)
            self.rand.add(ts, model.diffusion.denoising_losses(audio, model.predictor, ts, seed=seed, clip_offset=first,
                                                               cond=out["embedded"], labels=wrong))
        self.num_samples += n
        self.sq_err += sum(Fraction(v) for v in out["sq_err"].tolist())
        self.numel += out["embedded"].numel()

    def merge(self, other: "EvalState") -> "EvalState":
        self.cond.merge(other.cond)
        self.rand.merge(other.rand)
        self.num_samples += other.num_samples
        self.sq_err += other.sq_err
        self.numel += other.numel
        self.hist += other.hist.to(self.hist.device)
        return self

    def to_host(self) -> "EvalState":
        self.hist = self.hist.cpu()
        return self

    def log_dict(self):
        log = dict(self.cond.log_dict())
        log.update(self.rand.log_dict())
        log["vq_loss"] = float(self.loss_fn.from_sq_err(float(self.sq_err), self.numel)) if self.numel else 0.0
        log.update(code_usage(self.hist))
        return log


def format_line(num_samples, log):
    msg = " ".join(f"{key}={value}" if isinstance(value, int) else f"{key}={value:.06f}" for key, value in log.items())
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
        raise SystemExit("no ROCm device visible: the encoder and the predictor have no CPU path")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    torch.cuda.set_device(device)

    data_loader, num_labels = create_data_loader(directory=args.data_dir, batch_size=args.batch_size, seed=args.seed, rank=rank, world=world)
    if rank == 0:
        print("loading model from checkpoint...")
    model = VQVAE.load(args.checkpoint_path).to(device)
    assert model.num_labels == num_labels, f"the model has {model.num_labels} labels, the data {num_labels}"
    model.eval()
    model.set_precision(args.precision)

    state = EvalState(model.vq.num_codes, device)
    for i, data_batch in enumerate(data_loader):
        first = (rank + i * world) * args.batch_size  # position of the batch's first clip in the shuffled pass
        if args.max_samples is not None and first + args.batch_size > args.max_samples:
            break
        audio_seq = data_batch["samples"][:, None].to(device)
        labels = data_batch["label"].to(device)
        state.add_batch(model, audio_seq, labels, first, args.seed)
        if world == 1:
            print(format_line(state.num_samples, state.log_dict()))
    if world > 1:
        import torch.distributed as dist

        gathered = [None] * world if rank == 0 else None
        dist.gather_object(state.to_host(), gathered, dst=0)
        if rank == 0:
            merged = gathered[0]
            for other in gathered[1:]:
                merged.merge(other)
            print(format_line(merged.num_samples, merged.log_dict()))
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
