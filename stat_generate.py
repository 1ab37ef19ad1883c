#!/usr/bin/env python3
"""
Feature statistics of a folder of samples under a speaker classifier: the counterpart of the reference's stat_generate.py
(same flags and npz keys).  Every clip goes through the classifier's stem at t = 0 (`Classifier.features`, one HIP forward
that also returns the softmax probabilities); the feature mean and covariance are accumulated on the device
(`FeatureStats`, f64 MFMA moments) instead of stacking every feature vector on the host.  Prints the class score.

Differences: `--data-dir` (the LibriSpeech loader) is refused; files are read whole in sorted order and batched by equal
length (a length must be a multiple of the classifier's downsample rate); `--precision` is new (default fp32, the
reference's arithmetic).  Under torchrun (WORLD_SIZE > 1) each rank takes a contiguous shard of the sorted file list,
the statistics are merged across ranks and rank 0 writes the npz.
"""
import argparse
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import Classifier, FeatureStats  # noqa: E402
from vq_voice_swap_amd.audio import ChunkReader  # noqa: E402
from vq_voice_swap_amd.eval_pass import close_ranks, local_device, open_ranks  # noqa: E402
from vq_voice_swap_amd.sampler import shard_range  # noqa: E402


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--checkpoint-path", default="model_classifier.pt", type=str)
    p.add_argument("--batch-size", default=4, type=int)
    p.add_argument("--num-samples", default=None, type=int)
    p.add_argument("--sample-dir", default=None, type=str)
    p.add_argument("--data-dir", default=None, type=str)
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16", "bf16"])
    p.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend when WORLD_SIZE > 1")
    p.add_argument("output_path", type=str)
    return p


def parse_args(argv=None):
    parser = arg_parser()
    args = parser.parse_args(argv)
    if args.data_dir is not None:
        parser.error("--data-dir is not supported: the LibriSpeech loader is not part of this package; write the clips to a folder "
                     "of WAV files and pass --sample-dir")
    if args.sample_dir is None:
        parser.error("--sample-dir is required")
    if args.batch_size < 1:
        parser.error("--batch-size must be at least 1")
    return args


def list_samples(sample_dir, num_samples=None):
    files = sorted(os.path.join(sample_dir, x) for x in os.listdir(sample_dir) if not x.startswith(".") and x.endswith(".wav"))
    return files[:num_samples] if num_samples else files


def read_clip(path):
    r = ChunkReader(path, sample_rate=16000)
    parts = []
    while True:
        chunk = r.read(1 << 20)
        if chunk is None:
            break
        parts.append(chunk)
    r.close()
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


def batches_of_equal_length(files, batch_size, rate):
    """Consecutive files of one length, at most batch_size of them, as [n, 1, T] float32 host tensors."""
    batch, length = [], None
    for path in files:
        x = read_clip(path)
        if x.size == 0 or x.size % rate:
            raise SystemExit(f"{path}: {x.size} samples is not a positive multiple of the classifier's downsample rate {rate}")
        if batch and (x.size != length or len(batch) == batch_size):
            yield torch.from_numpy(np.stack(batch))[:, None]
            batch = []
        batch.append(x)
        length = x.size
    if batch:
        yield torch.from_numpy(np.stack(batch))[:, None]


def main(argv=None):
    args = parse_args(argv)
    rank, world = open_ranks(args.dist_backend)
    device = local_device("the classifier has no CPU path")
    classifier = Classifier.load(args.checkpoint_path).to(device).eval().set_precision(args.precision)

    files = list_samples(args.sample_dir, args.num_samples)
    begin, end = shard_range(len(files), rank, world)
    stats = FeatureStats(classifier.feature_dim, device)
    for batch in batches_of_equal_length(files[begin:end], args.batch_size, classifier.downsample_rate):
        feat, probs = classifier.features(batch.to(device), return_probs=True)
        stats.update(feat)
        stats.add_probs(probs)
    if world > 1:
        stats.all_reduce()
    if rank == 0:
        if stats.n < 2:
            raise SystemExit(f"{stats.n} clip(s) in {args.sample_dir}: a covariance needs at least two")
        print(f"classifier score: {stats.class_score()}")
        stats.save(args.output_path)
    close_ranks(world)


if __name__ == "__main__":
    main()
