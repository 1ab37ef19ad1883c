#!/usr/bin/env python3
"""
Enrol new speakers into a trained speaker `Classifier` on MI355X: learn one row and one bias of its head, `out.1`, per speaker and
leave every other parameter -- the stem, the attention pool, the old rows -- as the checkpoint has it.  The counterpart of
enroll_speaker.py for the other model that knows the label set: `data_dir` holds one sub-directory per NEW speaker (the same ones,
in the same sorted order, that enroll_speaker.py was given), `--pretrained-path` the trained classifier.  The loss is the one the
reference trains the classifier on (`ClassifierTrainLoop.compute_losses`, train_loop.py:551-561): the NLL of the label on audio
noised to a random t, with its `--curriculum-start` / `--curriculum-steps` (`sample_timesteps`: ts ** power).

Per step: noise the batch, `vqvs_classifier_features` (the stem's forward), `vqvs_head_xent_grad`, `vqvs_head_adamw` -- the gradient
is closed-form in the new rows, so there is no backward schedule, no autograd and no torch optimiser (vq_voice_swap_amd/enroll.py).
Speaker k of `data_dir` becomes label `old_count + k`.  A line `step N: loss=... acc=... q0=... q1=... q2=... q3=...` is printed per
step (NLL quartiles of t, `LossTracker`).

With new speakers alone every clip's target is a new label, and with ONE new speaker nothing in the loss bounds its row: the NLL falls
for ever as the row grows.  `--replay-dir DIR` names the old speakers' data set (its sorted sub-directories are labels 0 .. K - 1; it
may hold fewer speakers than the checkpoint, never more): every step's batch is then `--batch-size` new clips followed by
`--replay-batch` replay clips, whose targets are old labels and which therefore only push the new logits down.

At every save: `step N: holdout_nll=... holdout_acc=... (n clips)` on the `--holdout N` new clips kept out of training, at fixed
(t, noise), and with a replay set `replay_new_mass=...`, the mean probability the grown head gives to ANY new label on the replay clips
held out by the same rule.  `<output-dir>/model.pt` loads with `Classifier.load` (eval_conversion.py --classifier, sample_diffusion.py
--classifier-path, stat_generate.py); `<output-dir>/enroll.pt` holds the rows, the AdamW moments and the step count: a run that finds
it resumes at the next batch of the pass it stopped in.
"""
import argparse
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from enroll_speaker import epoch_batches, load_clips, local_device, model_labels, split_holdout  # noqa: E402
from vq_voice_swap_amd import Classifier, Diffusion, LossTracker, atomic_save, create_data_loader  # noqa: E402
from vq_voice_swap_amd.enroll import ClassifierEnroller  # noqa: E402


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--weight-decay", default=0.0, type=float)
    p.add_argument("--batch-size", default=8, type=int)
    p.add_argument("--output-dir", default="ckpt_classifier_added", type=str)
    p.add_argument("--pretrained-path", default=None, type=str, required=True)
    p.add_argument("--save-interval", default=1000, type=int)
    p.add_argument("--encoding", default="linear", type=str)
    p.add_argument("--schedule", default="exp", type=str)
    p.add_argument("--curriculum-start", default=30.0, type=float)
    p.add_argument("--curriculum-steps", default=0, type=int)
    p.add_argument("--steps", default=1000, type=int, help="optimiser steps of this run")
    p.add_argument("--init", default="zeros", type=str, help="zeros | mean | the index of an existing speaker to start from")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--holdout", default=0, type=int, metavar="N", help="keep N clips out of training and log their NLL and accuracy at every save")
    p.add_argument("--seconds", default=4.0, type=float, help="clip length")
    p.add_argument("--precision", default="fp32", type=str, help="precision mode of the stem's forward")
    p.add_argument("--replay-dir", default=None, type=str, metavar="DIR", help="the old speakers' data set: sub-directories in sorted order are labels 0 .. K-1")
    p.add_argument("--replay-batch", default=None, type=int, metavar="R", help="replay clips behind the new ones in every batch (default: --batch-size)")
    p.add_argument("data_dir", type=str)
    return p


def parse_init(text: str):
    return text if text in ("zeros", "mean") else int(text)


def curriculum_power(step: int, start: float, steps: int) -> float:
    """The exponent of `sample_timesteps` (train_loop.py:563-569) at `step` optimiser steps already taken: ts ** power with power
    going linearly from `start` to 1 over the first `steps` steps, 1 from there on."""
    if step < steps:
        frac = step / steps
        return start * (1 - frac) + frac
    return 1.0


def batch_ts(n: int, seed: int, clip_offset: int, power: float) -> torch.Tensor:
    """The times of a training batch: `Diffusion.draw_ts` of (seed, clip_offset), raised to the curriculum's power."""
    ts = Diffusion.draw_ts(n, seed, clip_offset)
    return ts if power == 1.0 else ts ** power


def compose_batch(new_audio, new_loader_labels, old_count: int, replay_audio=None, replay_labels=None):
    """(audio, labels of the grown model) of one step: the new clips first, their loader labels offset by `old_count`; behind them the
    replay clips under their own labels, 0 .. old_count - 1."""
    labels = model_labels(new_loader_labels, old_count)
    if replay_audio is None:
        return new_audio, labels
    if replay_audio.shape[1:] != new_audio.shape[1:]:
        raise ValueError(f"replay clips of shape {tuple(replay_audio.shape[1:])}, new clips of shape {tuple(new_audio.shape[1:])}")
    return torch.cat([new_audio, replay_audio], dim=0), torch.cat([labels, replay_labels.to(torch.int64)])


def holdout_scores(enroller: ClassifierEnroller, clips: torch.Tensor, labels: torch.Tensor, batch_size: int, seed: int):
    """(mean NLL, accuracy, mean new-label mass) of held-out clips at t = (i + 1/2) / N and the noise of (seed, clip i): the same
    numbers at every call."""
    n = len(clips)
    ts = (torch.arange(n, dtype=torch.float32) + 0.5) / n
    nll = hits = mass = 0.0
    for i in range(0, n, batch_size):
        out = enroller.losses(clips[i:i + batch_size], labels[i:i + batch_size], ts=ts[i:i + batch_size], seed=seed, clip_offset=i)
        nll += float(out["nll"].double().sum().item())
        hits += float(out["top1"].double().sum().item())
        mass += float(out["new_mass"].double().sum().item())
    return nll / n, hits / n, mass / n


def save(enroller: ClassifierEnroller, output_dir: str) -> None:
    atomic_save(enroller.checkpoint(), os.path.join(output_dir, "model.pt"))
    atomic_save(enroller.state_dict(), os.path.join(output_dir, "enroll.pt"))


def main(argv=None):
    args = arg_parser().parse_args(argv)
    if args.steps < 0 or args.save_interval < 1 or args.holdout < 0 or args.curriculum_steps < 0:
        raise SystemExit("--steps, --holdout and --curriculum-steps must not be negative, --save-interval must be positive")
    if "tones" in (args.data_dir, args.replay_dir) and args.seconds != 4.0:
        raise SystemExit("the synthetic set 'tones' has clips of 4 s: --seconds does not apply to it")
    replay_batch = args.batch_size if args.replay_batch is None else args.replay_batch
    if args.replay_dir is not None and replay_batch < 1:
        raise SystemExit("--replay-batch must be positive")

    def open_set(directory, batch_size):
        kw = {} if directory == "tones" else dict(window_duration=args.seconds)
        loader, count = create_data_loader(directory=directory, batch_size=batch_size, encoding=args.encoding, **kw)
        return loader.dataset, count  # (the clips are read by index below: the held-out ones are left out of every pass)

    def split(dataset, batch_size, what):
        try:
            held_idx, train_idx = split_holdout(len(dataset), args.holdout, args.seed)
        except ValueError as e:
            raise SystemExit(str(e))
        if len(train_idx) // batch_size == 0:
            raise SystemExit(f"{what}: {len(train_idx)} training clips are fewer than one batch of {batch_size}")
        return held_idx, train_idx

    dataset, num_new = open_set(args.data_dir, args.batch_size)
    held_idx, train_idx = split(dataset, args.batch_size, args.data_dir)
    per_epoch = len(train_idx) // args.batch_size
    print(f"loading from pretrained model: {args.pretrained_path} ...")
    model = Classifier.load(args.pretrained_path)
    device = local_device()
    model.to(device).eval().set_precision(args.precision)
    old_count = model.num_labels
    print(f"{old_count} speakers in the checkpoint, {num_new} new: labels {old_count} .. {old_count + num_new - 1}")
    replay = None
    if args.replay_dir is not None:
        replay, replay_speakers = open_set(args.replay_dir, replay_batch)
        if replay_speakers > old_count:
            raise SystemExit(f"{args.replay_dir}: {replay_speakers} speakers, the checkpoint has {old_count} labels")
        replay_held_idx, replay_train_idx = split(replay, replay_batch, args.replay_dir)
        replay_per_epoch = len(replay_train_idx) // replay_batch
    elif num_new == 1:
        print("warning: one new speaker and no --replay-dir: every target is the new label, nothing in the loss bounds its row", file=sys.stderr)
    enroller = ClassifierEnroller(model, num_new, schedule_name=args.schedule, lr=args.lr, weight_decay=args.weight_decay,
                                  init=parse_init(args.init), seed=args.seed)
    os.makedirs(args.output_dir, exist_ok=True)
    resume = os.path.join(args.output_dir, "enroll.pt")
    if os.path.exists(resume):
        print(f"resuming from {resume} ...")
        enroller.load_state_dict(torch.load(resume, map_location="cpu"))

    held = replay_held = None
    if held_idx:
        held, labels = load_clips(dataset, held_idx, device)
        held_labels = model_labels(labels, old_count).to(device)
        if replay is not None:
            replay_held, replay_held_labels = load_clips(replay, replay_held_idx, device)
            replay_held_labels = replay_held_labels.to(device)
    per_step = args.batch_size + (replay_batch if replay is not None else 0)
    tracker = LossTracker()
    last = enroller.steps + args.steps
    while enroller.steps < last:
        # step s (counted over all runs into this output directory) takes batch s % per_epoch of pass s // per_epoch of the new clips, and
        # of the replay clips by their own count: a resumed run goes on where the last one stopped
        epoch, at = divmod(enroller.steps, per_epoch)
        for batch in epoch_batches(train_idx, args.batch_size, args.seed, epoch)[at:]:
            audio, labels = load_clips(dataset, batch, device)
            replay_audio = replay_labels = None
            if replay is not None:
                r_epoch, r_at = divmod(enroller.steps, replay_per_epoch)
                replay_audio, replay_labels = load_clips(replay, epoch_batches(replay_train_idx, replay_batch, args.seed + 1, r_epoch)[r_at], device)
            audio, labels = compose_batch(audio, labels, old_count, replay_audio, replay_labels)
            offset = enroller.steps * per_step
            ts = batch_ts(len(audio), args.seed, offset, curriculum_power(enroller.steps, args.curriculum_start, args.curriculum_steps))
            out = enroller.step(audio, labels.to(device), ts=ts, seed=args.seed, clip_offset=offset)
            tracker.add(out["ts"], out["nlls"])
            quartiles = " ".join(f"{k}={v:.6f}" for k, v in tracker.log_dict().items())
            print(f"step {enroller.steps}: loss={out['loss'].item():.6f} acc={out['acc'].item():.4f} {quartiles}")
            if enroller.steps % args.save_interval == 0 or enroller.steps == last:
                save(enroller, args.output_dir)
                if held is not None:
                    nll, acc, _ = holdout_scores(enroller, held, held_labels, args.batch_size, args.seed + 1)
                    line = f"step {enroller.steps}: holdout_nll={nll:.6f} holdout_acc={acc:.4f}"
                    if replay_held is not None:
                        line += f" replay_new_mass={holdout_scores(enroller, replay_held, replay_held_labels, replay_batch, args.seed + 2)[2]:.6e}"
                    print(line + f" ({len(held)} clips)")
            if enroller.steps == last:
                break
    if args.steps == 0:
        save(enroller, args.output_dir)
    model.check_status()
    print(f"wrote {os.path.join(args.output_dir, 'model.pt')}: {old_count + num_new} speakers")


if __name__ == "__main__":
    main()
