#!/usr/bin/env python3
"""
Enrol new speakers into a trained class-conditional VQ-VAE on MI355X: learn one `class_embed` row per speaker and leave every other
parameter as the checkpoint has it.  Counterpart of the reference's train_vqvae_add.py (`VQVAEAddClassesTrainLoop`,
train_loop.py:438-485): `data_dir` holds one sub-directory per NEW speaker, `--pretrained-path` the trained VQ-VAE; the flags that
loop has keep their names and defaults (`--lr`, `--weight-decay`, `--batch-size`, `--save-interval`, `--encoding`, `--output-dir`).

Per step: encode and quantise the batch, noise it, `vqvs_unet_embed_grad` (the predictor's forward schedule and an explicit backward
schedule down to the conditioning vector), `vqvs_embed_adamw` -- no autograd, no torch optimiser (vq_voice_swap_amd/enroll.py).
Speaker k of `data_dir` (sorted order) becomes label `old_count + k` of the written checkpoint, as the reference offsets its labels
(train_loop.py:450); a line `step N: loss=... q0=... q1=... q2=... q3=...` is printed per step (loss quartiles of t, `LossTracker`).

Not in the reference: `--steps` (it trains until interrupted), `--init` (normal | mean | the index of an existing speaker, say the
closest one voice_search_vqvae.py names), `--seed` (batch order, t, noise and the normal init), `--holdout N` (N clips are kept out of
training -- chosen by index from `--seed`, left out of every pass and of a resumed run -- and their mean loss at fixed (t, noise) is
printed at every save), `--seconds` (clip length; `data_dir` may also be the synthetic set "tones", whose clips are 4 s).  `<output-dir>/model.pt` is a
checkpoint that `sample_vqvae.py --label <old_count + k>` loads as it is; `<output-dir>/enroll.pt` holds the rows, the AdamW moments
and the step count; a run that finds it resumes from there: the same held-out clips, the next batch of the pass it stopped in.

`--uncond` learns the UNCONDITIONAL ("null") label instead (`NullLabelEnroller`): `data_dir` is any tree of recordings of the speakers
the model already knows, its directory labels are ignored, and every clip trains one row that is written in FRONT of the table -- label
0 of the written checkpoint, old speaker k its label k + 1, the layout of the reference's train_vqvae_uncond.py, which
sample_vqvae_uncond.py and the `--guide-label-scale` of convert_dataset.py / eval_conversion.py expect.  The output directory is then
ckpt_vqvae_uncond unless `--output-dir` names one; `--init mean` is the start to prefer (the centre of the known speakers); a run never
resumes the enroll.pt of the other kind.

`--input-file ref.wav` (repeatable) `--vector-out voice.npy`, in place of `data_dir`: a voice from a recording.  The recordings are cut
into `--seconds` clips (the last partial clip is dropped), ONE row is learned from them with the same `SpeakerEnroller`, and the row is
written as a voice file (vq_voice_swap_amd/speakers.py: the .npy vector bit for bit, a side-car .json) that `sample_vqvae.py --voice
@voice.npy` and the other scripts' voice specs read; no checkpoint is written and nothing resumes.  In the directory mode
`--vectors-out DIR` writes such a file per new speaker (named after its directory) beside the checkpoint.
"""
import argparse
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd import VQVAE, LossTracker, atomic_save, create_data_loader  # noqa: E402
from vq_voice_swap_amd.enroll import NullLabelEnroller, SpeakerEnroller  # noqa: E402
from vq_voice_swap_amd.speakers import save_voice  # noqa: E402

SAMPLE_RATE = 16000

UNCOND_OUTPUT_DIR = "ckpt_vqvae_uncond"


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--weight-decay", default=0.0, type=float)
    p.add_argument("--batch-size", default=8, type=int)
    p.add_argument("--output-dir", default="ckpt_vqvae_added", type=str)
    p.add_argument("--pretrained-path", default=None, type=str, required=True)
    p.add_argument("--save-interval", default=1000, type=int)
    p.add_argument("--encoding", default="linear", type=str)
    p.add_argument("--steps", default=1000, type=int, help="optimiser steps of this run")
    p.add_argument("--init", default="normal", type=str, help="normal | mean | the index of an existing speaker to start from")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--holdout", default=0, type=int, metavar="N", help="keep N clips out of training and log their mean loss at every save")
    p.add_argument("--seconds", default=4.0, type=float, help="clip length")
    p.add_argument("data_dir", type=str)
    return p


def parse_args(argv=None):
    """The arguments; under `--uncond` an `--output-dir` that was not given is UNCOND_OUTPUT_DIR (the flag's own default stays)."""
    parser = arg_parser()
    # the null-label mode joins the parser here: `arg_parser()` stays the flag set of the reference's train_vqvae_add.py and this script's own
    parser.add_argument("--uncond", action="store_true",
                        help=f"learn the unconditional label (row 0, old speakers one up) from recordings of the known speakers; writes to "
                             f"{UNCOND_OUTPUT_DIR} unless --output-dir is given")
    # ... and so does the voice-file mode: recordings in place of data_dir, which stops being required on its own
    for action in parser._actions:
        if action.dest == "data_dir":
            action.nargs, action.default = "?", None
    parser.add_argument("--input-file", action="append", default=[], metavar="WAV",
                        help="in place of data_dir (repeatable): learn ONE row from these recordings and write it to --vector-out")
    parser.add_argument("--vector-out", default=None, type=str, metavar="NPY", help="the voice file of the --input-file mode")
    parser.add_argument("--vectors-out", default=None, type=str, metavar="DIR",
                        help="directory mode: also write one voice file per new speaker, DIR/<speaker directory>.npy")
    args = parser.parse_args(argv)
    given = parser.parse_args(argv, argparse.Namespace(output_dir=None)).output_dir is not None
    if args.uncond and not given:
        args.output_dir = UNCOND_OUTPUT_DIR
    if args.input_file:
        if args.data_dir is not None:
            parser.error("--input-file takes the place of data_dir: give one or the other")
        if args.vector_out is None or not args.vector_out.endswith(".npy"):
            parser.error("--input-file needs --vector-out FILE.npy")
        if args.uncond or args.vectors_out is not None:
            parser.error("--input-file learns one speaker's row: --uncond and --vectors-out belong to the directory mode")
    else:
        if args.data_dir is None:
            parser.error("data_dir (or --input-file) is required")
        if args.vector_out is not None:
            parser.error("--vector-out belongs to --input-file (the directory mode has --vectors-out DIR)")
        if args.vectors_out is not None and args.uncond:
            parser.error("--vectors-out writes the new speakers' rows: --uncond learns none")
    return args


def parse_init(text: str):
    return text if text in ("normal", "mean") else int(text)


def model_labels(loader_labels: torch.Tensor, old_count: int) -> torch.Tensor:
    """Labels of the loader (speaker k of data_dir) -> labels of the grown model: k + old_count (reference train_loop.py:450)."""
    return loader_labels.to(torch.int64) + int(old_count)


def local_device():
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: the encoder and the predictor have no CPU path")
    return torch.device("cuda")


def split_holdout(n: int, holdout: int, seed: int):
    """(held, train): dataset indices.  The held-out clips are the first `holdout` entries of a permutation of 0 .. n - 1 seeded by
    `seed` alone, so they are the same clips in every pass and in a resumed run; no training batch ever holds one."""
    if holdout > n:
        raise ValueError(f"--holdout {holdout}: the data set has {n} clips")
    order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) * 2654435761 % (2 ** 63) + 1)).tolist()
    return sorted(order[:holdout]), sorted(order[holdout:])


def epoch_batches(train, batch_size: int, seed: int, epoch: int):
    """The index batches of pass `epoch` over the training clips: a permutation seeded by (seed, epoch), the incomplete last batch
    dropped, as the loader does."""
    g = torch.Generator().manual_seed((int(seed) + 0x9E3779B97F4A7C15 * (int(epoch) + 1)) % (2 ** 63))
    order = [train[i] for i in torch.randperm(len(train), generator=g).tolist()]
    return [order[i:i + batch_size] for i in range(0, len(order) - batch_size + 1, batch_size)]


def load_clips(dataset, indices, device):
    """(audio [n, 1, T] on the device, loader labels [n]) of the clips `indices`."""
    items = [dataset[i] for i in indices]
    audio = torch.stack([torch.as_tensor(it["samples"]) for it in items])[:, None].to(device)
    return audio, torch.tensor([int(it["label"]) for it in items], dtype=torch.int64)


def holdout_loss(enroller: SpeakerEnroller, clips: torch.Tensor, rows: torch.Tensor, batch_size: int, seed: int) -> float:
    """Mean loss of the held-out clips at t = (i + 1/2) / N and the noise of (seed, clip i): the same numbers at every call."""
    n = len(clips)
    ts = (torch.arange(n, dtype=torch.float32) + 0.5) / n
    total = 0.0
    for i in range(0, n, batch_size):
        mses = enroller.losses(clips[i:i + batch_size], rows[i:i + batch_size], ts=ts[i:i + batch_size], seed=seed, clip_offset=i)[0]
        total += float(mses.double().sum().item())
    return total / n


def save(enroller: SpeakerEnroller, output_dir: str) -> None:
    atomic_save(enroller.checkpoint(), os.path.join(output_dir, "model.pt"))
    atomic_save(enroller.state_dict(), os.path.join(output_dir, "enroll.pt"))


def cut_clips(waves, clip: int) -> torch.Tensor:
    """Recordings (float32 [N_r] arrays) -> [n, 1, clip]: each cut into whole clips from its start, the last partial clip dropped."""
    clips = [torch.from_numpy(w[i:i + clip].copy()) for w in waves for i in range(0, len(w) - clip + 1, clip)]
    if not clips:
        raise ValueError(f"the recordings hold fewer than one clip of {clip} samples")
    return torch.stack(clips)[:, None]


def voice_meta(args, model, enroller, holdout=None) -> dict:
    meta = dict(base_channels=int(model.predictor.base_channels), steps=int(enroller.steps), pretrained_path=args.pretrained_path)
    if holdout is not None:
        meta["holdout_loss"] = float(holdout)
    return meta


def enroll_files(args) -> None:
    """--input-file: one row from the clips of the recordings, written as a voice file.  Step s takes batch s % per_epoch of pass
    s // per_epoch of `epoch_batches` over the clips (the held-out ones left out), keyed as the directory mode keys its steps."""
    from vq_voice_swap_amd.audio import ChunkReader

    waves = []
    for path in args.input_file:
        reader = ChunkReader(path, sample_rate=SAMPLE_RATE, encoding=args.encoding)
        try:
            chunks = []
            while (chunk := reader.read(1 << 20)) is not None:
                chunks.append(chunk)
        finally:
            reader.close()
        if chunks:
            import numpy as np

            waves.append(np.concatenate(chunks))
    try:
        clips = cut_clips(waves, round(args.seconds * SAMPLE_RATE))
        held_idx, train_idx = split_holdout(len(clips), args.holdout, args.seed)
    except ValueError as e:
        raise SystemExit(str(e))
    if not train_idx:
        raise SystemExit(f"--holdout {args.holdout} leaves no clip to train on ({len(clips)} clips)")
    batch_size = min(args.batch_size, len(train_idx))
    per_epoch = len(train_idx) // batch_size
    print(f"loading from pretrained model: {args.pretrained_path} ...")
    model = VQVAE.load(args.pretrained_path)
    if model.num_labels is None:
        raise SystemExit("the pretrained model is not class-conditional: a voice is a vector in the place of its class_embed rows")
    device = local_device()
    model.to(device).eval()
    clips = clips.to(device)
    print(f"{len(clips)} clips of {args.seconds} s from {len(waves)} recordings: learning one row in batches of {batch_size}")
    enroller = SpeakerEnroller(model, 1, lr=args.lr, weight_decay=args.weight_decay, init=parse_init(args.init), seed=args.seed)
    tracker = LossTracker()
    while enroller.steps < args.steps:
        epoch, at = divmod(enroller.steps, per_epoch)
        for batch in epoch_batches(train_idx, batch_size, args.seed, epoch)[at:]:
            out = enroller.step(clips[batch], torch.zeros(len(batch), dtype=torch.int64, device=device), seed=args.seed,
                                clip_offset=enroller.steps * batch_size)
            tracker.add(out["ts"], out["mses"])
            quartiles = " ".join(f"{k}={v:.6f}" for k, v in tracker.log_dict().items())
            print(f"step {enroller.steps}: loss={out['loss'].item():.6f} {quartiles}")
            if enroller.steps == args.steps:
                break
    held = None
    if held_idx:
        held = holdout_loss(enroller, clips[held_idx], torch.zeros(len(held_idx), dtype=torch.int64, device=device), batch_size, args.seed + 1)
        print(f"step {enroller.steps}: holdout={held:.6f} ({len(held_idx)} clips)")
    model.predictor.check_status()
    os.makedirs(os.path.dirname(args.vector_out) or ".", exist_ok=True)
    save_voice(args.vector_out, enroller.rows[0], voice_meta(args, model, enroller, held))
    print(f"wrote {args.vector_out}: a voice of {enroller.rows.shape[1]} entries")


def main(argv=None):
    args = parse_args(argv)
    if args.steps < 0 or args.save_interval < 1 or args.holdout < 0:
        raise SystemExit("--steps and --holdout must not be negative, --save-interval must be positive")
    if args.input_file:
        return enroll_files(args)
    if args.data_dir == "tones" and args.seconds != 4.0:
        raise SystemExit("the synthetic set 'tones' has clips of 4 s: --seconds does not apply to it")
    loader_kw = {} if args.data_dir == "tones" else dict(window_duration=args.seconds)
    loader, num_new = create_data_loader(directory=args.data_dir, batch_size=args.batch_size, encoding=args.encoding, **loader_kw)
    dataset = loader.dataset  # (the clips are read by index below: the held-out ones are left out of every pass)
    try:
        held_idx, train_idx = split_holdout(len(dataset), args.holdout, args.seed)
    except ValueError as e:
        raise SystemExit(str(e))
    per_epoch = len(train_idx) // args.batch_size
    if per_epoch == 0:
        raise SystemExit(f"{args.data_dir}: {len(train_idx)} training clips are fewer than one batch of {args.batch_size}")
    print(f"loading from pretrained model: {args.pretrained_path} ...")
    model = VQVAE.load(args.pretrained_path)
    if model.num_labels is None:
        raise SystemExit("the pretrained model is not class-conditional: there is no class_embed table to grow")
    device = local_device()
    model.to(device).eval()
    old_count = model.num_labels
    if args.uncond:
        print(f"{old_count} speakers in the checkpoint: learning the unconditional label 0, speakers become labels 1 .. {old_count}")
        enroller = NullLabelEnroller(model, lr=args.lr, weight_decay=args.weight_decay, init=parse_init(args.init), seed=args.seed)
    else:
        print(f"{old_count} speakers in the checkpoint, {num_new} new: labels {old_count} .. {old_count + num_new - 1}")
        enroller = SpeakerEnroller(model, num_new, lr=args.lr, weight_decay=args.weight_decay, init=parse_init(args.init), seed=args.seed)
    os.makedirs(args.output_dir, exist_ok=True)
    resume = os.path.join(args.output_dir, "enroll.pt")
    if os.path.exists(resume):
        print(f"resuming from {resume} ...")
        try:
            enroller.load_state_dict(torch.load(resume, map_location="cpu"))
        except ValueError as e:
            raise SystemExit(f"{resume}: {e}")

    def rows_of(loader_labels):
        if args.uncond:  # (directory labels are ignored: every clip trains the one row)
            return torch.zeros_like(loader_labels, dtype=torch.int64).to(device)
        return (model_labels(loader_labels, old_count) - enroller.first_label).to(device)

    held, held_rows = None, None
    if held_idx:
        held, labels = load_clips(dataset, held_idx, device)
        held_rows = rows_of(labels)
    tracker = LossTracker()
    last = enroller.steps + args.steps
    while enroller.steps < last:
        # step s (counted over all runs into this output directory) takes batch s % per_epoch of pass s // per_epoch: a resumed run goes on
        # where the last one stopped
        epoch, at = divmod(enroller.steps, per_epoch)
        for batch in epoch_batches(train_idx, args.batch_size, args.seed, epoch)[at:]:
            audio, labels = load_clips(dataset, batch, device)
            out = enroller.step(audio, rows_of(labels), seed=args.seed, clip_offset=enroller.steps * args.batch_size)
            tracker.add(out["ts"], out["mses"])
            quartiles = " ".join(f"{k}={v:.6f}" for k, v in tracker.log_dict().items())
            print(f"step {enroller.steps}: loss={out['loss'].item():.6f} {quartiles}")
            if enroller.steps % args.save_interval == 0 or enroller.steps == last:
                save(enroller, args.output_dir)
                if held is not None:
                    print(f"step {enroller.steps}: holdout={holdout_loss(enroller, held, held_rows, args.batch_size, args.seed + 1):.6f} ({len(held)} clips)")
            if enroller.steps == last:
                break
    if args.steps == 0:
        save(enroller, args.output_dir)
    model.predictor.check_status()
    if args.vectors_out is not None:
        os.makedirs(args.vectors_out, exist_ok=True)
        names = [str(s) for s in dataset.speaker_ids]
        last_held = holdout_loss(enroller, held, held_rows, args.batch_size, args.seed + 1) if held is not None else None
        for k in range(num_new):
            save_voice(os.path.join(args.vectors_out, f"{names[k]}.npy"), enroller.rows[k], voice_meta(args, model, enroller, last_held))
        print(f"wrote {num_new} voice files to {args.vectors_out}")
    if args.uncond:
        print(f"wrote {os.path.join(args.output_dir, 'model.pt')}: the unconditional label and {old_count} speakers")
    else:
        print(f"wrote {os.path.join(args.output_dir, 'model.pt')}: {old_count + num_new} speakers")


if __name__ == "__main__":
    main()
