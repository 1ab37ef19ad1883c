"""
Converting a whole data set (convert_dataset.py): the host-side bookkeeping, no device and no model.

The files of a LibriSpeech-layout tree (`dataset.build_file_index`) are sorted by relative path, and a file's GLOBAL ID is its place in
that list.  The id keys everything random about the file's conversion, so its output does not depend on how the files are grouped
into packs, on the window batch or on the number of ranks.  A pack is a run of CONSECUTIVE ids -- `decode_long_batch` keys recording r
of a pack as clip_offset + r -- of at most a budget of windows; packs are dealt to the ranks round-robin.
"""
import os
from typing import Dict, List, Optional, Sequence, Tuple


def list_files(index: dict) -> List[Tuple[str, float]]:
    """(relative path, seconds) of every file of a `build_file_index` tree, sorted by relative path: position = global id."""
    out: List[Tuple[str, float]] = []

    def walk(node: dict, prefix: str) -> None:
        for name, item in node.items():
            rel = os.path.join(prefix, name) if prefix else name
            if isinstance(item, dict):
                walk(item, rel)
            else:
                out.append((rel, float(item)))

    walk(index, "")
    return sorted(out)


def add_guidance_flags(parser) -> None:
    """`--guide-label-scale` / `--guide-vq-scale` of convert_dataset.py and eval_conversion.py, both off by default."""
    parser.add_argument("--guide-label-scale", type=float, default=0.0, metavar="S",
                        help="classifier-free-style guidance towards the target label (sample_vqvae_uncond.py); needs a checkpoint whose label 0 "
                             "is the unconditional one (enroll_speaker.py --uncond); labels are then speaker numbers without that offset")
    parser.add_argument("--guide-vq-scale", type=float, default=0.0, metavar="S",
                        help="the same towards the VQ codes; meaningful only for a model fine-tuned with dropped codes")


def guided(args) -> bool:
    """Whether a parsed command line asks for label / code guidance: the checkpoint then has the unconditional label at 0 and every
    label on the command line is a speaker number without that offset.  (The flags absent: a namespace of the unguided parser.)"""
    return bool(getattr(args, "guide_label_scale", 0.0)) or bool(getattr(args, "guide_vq_scale", 0.0))


PAUSE_FRAME_SECONDS = 0.01  # the detector's frame on the command line: 10 ms


def add_pause_flags(parser) -> None:
    """`--keep-pauses` / `--min-pause` / `--pause-guard` / `--no-skip-kept` of convert_dataset.py and the sample_vqvae scripts.  A flag
    that is not given leaves no attribute behind (`pause_settings` and `skip_kept` read them), so the namespace of a run without
    them is what it was."""
    import argparse

    parser.add_argument("--keep-pauses", type=float, default=argparse.SUPPRESS, metavar="DB",
                        help="leave the pauses of the input as they are: runs of 10 ms frames at or below this level in dBFS (e.g. -50)")
    parser.add_argument("--min-pause", type=float, default=argparse.SUPPRESS, metavar="SECONDS", help="the shortest pause that is kept (default 0.3)")
    parser.add_argument("--pause-guard", type=float, default=argparse.SUPPRESS, metavar="SECONDS",
                        help="converted anyway at each end of a pause that touches speech (default 0.05)")
    parser.add_argument("--no-skip-kept", action="store_true", default=argparse.SUPPRESS,
                        help="run the predictor on windows that are kept whole as well (the output is the same bit for bit)")


def check_pause_flags(parser, args) -> None:
    """The pause flags of a parsed command line: the level, the two lengths, and -- the detector is defined on linear samples -- no
    --keep-pauses with --encoding ulaw."""
    import math

    db = getattr(args, "keep_pauses", None)
    if db is None:
        if hasattr(args, "min_pause") or hasattr(args, "pause_guard"):
            parser.error("--min-pause and --pause-guard belong to --keep-pauses")
        return
    if not math.isfinite(db) or db > 0:
        parser.error("--keep-pauses takes a level in dBFS, at or below 0")
    if getattr(args, "encoding", "linear") == "ulaw":
        parser.error("--keep-pauses is defined on linear samples: it cannot be combined with --encoding ulaw")
    if not 0 < getattr(args, "min_pause", 0.3) <= 3600 or not 0 <= getattr(args, "pause_guard", 0.05) <= 3600:
        parser.error("--min-pause must be positive and --pause-guard not negative (seconds, an hour at the most)")


def pause_settings(args, sample_rate: int) -> Optional[dict]:
    """The detector's settings (`pauses.pause_mask`'s keywords) of a parsed command line, or None without --keep-pauses."""
    db = getattr(args, "keep_pauses", None)
    if db is None:
        return None
    frame = round(PAUSE_FRAME_SECONDS * sample_rate)
    if frame < 4 or frame % 4:
        raise SystemExit(f"--keep-pauses: a 10 ms frame at {sample_rate} Hz is {frame} samples, not a multiple of 4")
    return dict(threshold_db=float(db), frame=frame, min_pause_frames=max(1, round(getattr(args, "min_pause", 0.3) / PAUSE_FRAME_SECONDS)),
                guard_frames=round(getattr(args, "pause_guard", 0.05) / PAUSE_FRAME_SECONDS))


def skip_kept(args) -> bool:
    return not getattr(args, "no_skip_kept", False)


def top_directory(rel_path: str) -> str:
    return rel_path.replace("\\", "/").split("/", 1)[0]


def read_label_map(path: str, directories: Optional[Sequence[str]] = None) -> Dict[str, int]:
    """`--label-map FILE`: lines `top-level-directory<TAB>label` (blank lines and lines starting with # are skipped) -> {directory:
    label}.  ValueError for a line without exactly one tab, an empty directory, a label that is neither a non-negative integer nor a voice spec
    (speakers.parse_voice; kept as text), a directory named twice, and -- with `directories`, the top-level directories of the data -- a directory the file does not map."""
    mapping: Dict[str, int] = {}
    with open(path, "rt") as f:
        for number, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            fields = line.split("\t")
            if len(fields) != 2 or not fields[0].strip():
                raise ValueError(f"{path}:{number}: expected `directory<TAB>label`, got {line!r}")
            name, text = fields[0].strip(), fields[1].strip()
            if not text.isdigit():  # (not a label: a voice spec -- a blend, a vector file -- kept as text for speakers.voice_vectors)
                from .speakers import parse_voice

                try:
                    parse_voice(text)
                except ValueError as e:
                    raise ValueError(f"{path}:{number}: label {text!r} is not a non-negative integer or a voice spec ({e})") from None
            if name in mapping:
                raise ValueError(f"{path}:{number}: directory {name!r} is mapped twice")
            mapping[name] = int(text) if text.isdigit() else text
    if directories is not None:
        missing = sorted(set(directories) - set(mapping))
        if missing:
            raise ValueError(f"{path} maps no label to {missing}")
    return mapping


def make_packs(windows: Sequence[int], budget: int, ids: Optional[Sequence[int]] = None) -> List[List[int]]:
    """Files of `windows[i]` windows each, with global ids `ids` (default 0, 1, ...; ascending) -> packs of ids, in order.  A pack is
    a run of consecutive ids whose windows add up to at most `budget`; a file with more windows than that is a pack of its own, and
    a gap in the ids (a file left out) ends a pack."""
    if budget < 1:
        raise ValueError(f"a pack holds at least 1 window, got a budget of {budget}")
    ids = list(range(len(windows))) if ids is None else [int(i) for i in ids]
    if len(ids) != len(windows) or any(b <= a for a, b in zip(ids, ids[1:])):
        raise ValueError("ids must be ascending, one per file")
    packs: List[List[int]] = []
    used = 0
    for i, n in zip(ids, windows):
        if int(n) < 1:
            raise ValueError(f"file {i} has {n} windows: at least 1")
        if packs and used + int(n) <= budget and packs[-1][-1] + 1 == i:
            packs[-1].append(i)
            used += int(n)
        else:
            packs.append([i])
            used = int(n)
    return packs


def deal_packs(packs: Sequence[List[int]], rank: int, world: int) -> List[List[int]]:
    """The packs of rank `rank` of `world`: every world-th one."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside 0..{world - 1}")
    return [list(p) for p in packs[rank::world]]
