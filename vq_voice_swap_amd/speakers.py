"""
Speaker vectors as inputs: the predictor's conditioning is emb = time_mlp(t) + v, so any v is a voice.  This
module turns voice SPECS into such vectors on the device, for `UNetPredictor.forward(vectors=)` and everything above it.

A spec is text:
    "7"                   the label 7 (row 7 of class_embed)
    "3:0.7,251:0.3"       a blend: 0.7 * row 3 + 0.3 * row 251 -- weights as given, never renormalised, at most 8 entries
    "@voice.npy"          a vector file (`save_voice`; `enroll_speaker.py --input-file ... --vector-out`), also as an entry of a blend:
                          "@a.npy:0.5,7:0.5"
`parse_voice` reads one; `voice_vectors` makes the [n, E] vectors of a list of specs with ONE `vqvs_speaker_mix` call, whose arithmetic
is fixed (fp32 products and sums in entry order, each rounded on its own), so a voice is reproducible from its spec; `morph_vectors`
makes one vector per window of a long file from (seconds, spec) points; `pseudo_voice` derives a voice that is nobody's from a seed and
a key with hashlib alone, for corpus anonymisation.
"""

from __future__ import annotations

import hashlib
import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

MAX_ENTRIES = 8  # entries of one spec
MAX_SLOTS = 16   # J of vqvs_speaker_mix: two specs between the points of a morph

Entry = Tuple[Union[int, str], float]  # (label or vector-file path, weight)


def parse_voice(text: str) -> List[Entry]:
    """Spec text -> [(source, weight)]: source an int label or the path of a vector file (the text behind "@"), weight a float (1.0
    where the entry gives none).  Anything malformed is a ValueError that names the text."""
    def bad(why: str):
        return ValueError(f"voice spec {text!r}: {why}")

    if not isinstance(text, str) or not text.strip():
        raise bad("empty")
    entries: List[Entry] = []
    for part in text.split(","):
        part = part.strip()
        if not part:
            raise bad("an empty entry")
        src, sep, wtext = part.partition(":") if not part.startswith("@") else part.rpartition(":")
        if part.startswith("@") and not sep:
            src, wtext = part, ""
        weight = 1.0
        if sep:
            try:
                weight = float(wtext)
            except ValueError:
                raise bad(f"weight {wtext!r} of entry {part!r} is not a number") from None
            if not math.isfinite(weight):
                raise bad(f"weight {wtext!r} of entry {part!r} is not finite")
        src = src.strip()
        if src.startswith("@"):
            if len(src) == 1:
                raise bad(f"entry {part!r} names no file")
            entries.append((src[1:], weight))
            continue
        if not src.isdigit():
            raise bad(f"entry {part!r} is neither a label (a non-negative integer) nor @file")
        entries.append((int(src), weight))
    if len(entries) > MAX_ENTRIES:
        raise bad(f"{len(entries)} entries, at most {MAX_ENTRIES}")
    return entries


def as_entries(spec) -> List[Entry]:
    """A spec as text, as a bare label or already parsed -> entries."""
    if isinstance(spec, str):
        return parse_voice(spec)
    if isinstance(spec, (int, np.integer)):
        return parse_voice(str(int(spec)))
    return [(s if isinstance(s, str) else int(s), float(w)) for s, w in spec]


def single_label(spec) -> Optional[int]:
    """The label of a spec that is exactly one label at weight 1 (what a classifier can score against), else None."""
    entries = as_entries(spec)
    if len(entries) == 1 and not isinstance(entries[0][0], str) and entries[0][1] == 1.0:
        return int(entries[0][0])
    return None


def format_voice(entries: Sequence[Entry]) -> str:
    """Entries -> spec text that `parse_voice` reads back to the same labels and the same float32 weights."""
    return ",".join(f"{'@' + s if isinstance(s, str) else int(s)}:{float(np.float32(w))!r}" for s, w in entries)


def mix_tables(entry_lists: Sequence[Sequence[Entry]], num_labels: int, label_offset: int = 0):
    """(idx [n, J] int32, w [n, J] float32, files) of `vqvs_speaker_mix` for n entry lists over a table of `num_labels` rows with the
    vector files as rows num_labels, num_labels + 1, ... behind it (`files`, in order of first use).  Labels are shifted by
    `label_offset` (1: a checkpoint with the null label in front); unused slots are -1 / 0."""
    if not len(entry_lists):
        raise ValueError("no voice specs")
    J = max(len(e) for e in entry_lists)
    if not 1 <= J <= MAX_SLOTS:
        raise ValueError(f"a voice of {J} entries: the mix takes 1..{MAX_SLOTS}")
    idx = np.full((len(entry_lists), J), -1, dtype=np.int32)
    w = np.zeros((len(entry_lists), J), dtype=np.float32)
    files: Dict[str, int] = {}
    for b, entries in enumerate(entry_lists):
        for j, (src, weight) in enumerate(entries):
            if isinstance(src, str):
                row = num_labels + files.setdefault(src, len(files))
            else:
                row = int(src) + int(label_offset)
                if not int(label_offset) <= row < num_labels:
                    raise IndexError(f"voice label {src}: the model has labels 0..{num_labels - int(label_offset) - 1}")
            idx[b, j] = row
            w[b, j] = np.float32(weight)
    return idx, w, list(files)


def speaker_mix(table, idx, w, out=None):
    """`vqvs_speaker_mix`: table [K, E] f32, idx [B, J] int32 (negative: slot unused), w [B, J] f32 on the device ->
    out [B, E] = sum over the used slots, in slot order, of w * table[idx].  IndexError for an index >= K."""
    import torch

    from . import _native

    _native.require_cuda(table, idx, w, out)
    if table.dim() != 2 or idx.dim() != 2 or idx.shape != w.shape:
        raise ValueError(f"expected table [K, E] and idx, w [B, J], got {tuple(table.shape)}, {tuple(idx.shape)}, {tuple(w.shape)}")
    if table.dtype != torch.float32 or w.dtype != torch.float32 or idx.dtype != torch.int32:
        raise ValueError(f"expected a float32 table and weights and int32 indices, got {table.dtype}, {w.dtype}, {idx.dtype}")
    if table.stride(1) != 1 or table.stride(0) != table.shape[1]:
        table = table.contiguous()
    idx, w = idx.contiguous(), w.contiguous()
    K, E = table.shape
    B, J = idx.shape
    if idx.numel() and int(idx.max().item()) >= K:
        raise IndexError(f"speaker mix: index {int(idx.max().item())} out of range for a table of {K} rows")
    if out is None:
        out = torch.empty(B, E, device=table.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, E) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 [{B}, {E}] tensor")
    with torch.cuda.device(table.device):
        _native.check(_native.lib().vqvs_speaker_mix(table.data_ptr(), K, E, idx.data_ptr(), w.data_ptr(), J, out.data_ptr(), B,
                                                     _native._stream_ptr()))
    return out


def _mix_entries(predictor, entry_lists, label_offset: int):
    import torch

    if getattr(predictor, "num_labels", None) is None:
        raise ValueError("voices need a class-conditional predictor (num_labels)")
    table = predictor.class_embed.weight.detach().to(torch.float32)
    K, E = table.shape
    idx, w, files = mix_tables(entry_lists, K, label_offset)
    rows = []
    for path in files:
        vec, _ = load_voice(path)
        if vec.shape != (E,):
            raise ValueError(f"voice file {path!r} holds {vec.shape[0]} entries: this model's vectors have 4 * base_channels = {E}")
        rows.append(torch.from_numpy(vec))
    if rows:
        table = torch.cat([table, torch.stack(rows).to(table.device)])
    return speaker_mix(table, torch.from_numpy(idx).to(table.device), torch.from_numpy(w).to(table.device))


def voice_vectors(predictor, specs, label_offset: int = 0):
    """[n, E] conditioning vectors of n specs (text, bare labels or parsed entries) over `predictor.class_embed`, by one
    `vqvs_speaker_mix`; vector files become extra rows behind the table.  `label_offset` 1 serves checkpoints with the null label in
    front: specs name speakers without the offset."""
    return _mix_entries(predictor, [as_entries(s) for s in specs], label_offset)


def morph_entries(points, n: int, window: int, hop: int, sample_rate: int) -> List[List[Entry]]:
    """The entries of each of `n` windows under the morph `points` [(seconds, spec)], sorted by time: window b has the voice at its
    centre (b * hop + window / 2) / sample_rate -- the first point's before it, the last point's after it, and between two points A, B
    at fraction u A's entries with weights float32((1 - u) * w) followed by B's with float32(u * w)."""
    pts = [(float(t), as_entries(s)) for t, s in points]
    if not pts:
        raise ValueError("a morph needs at least one (seconds, spec) point")
    if any(b[0] <= a[0] for a, b in zip(pts, pts[1:])):
        raise ValueError(f"morph points must be sorted by strictly increasing time, got {[t for t, _ in pts]}")
    out = []
    for b in range(int(n)):
        c = (b * hop + window / 2) / sample_rate
        if c <= pts[0][0]:
            out.append(list(pts[0][1]))
        elif c >= pts[-1][0]:
            out.append(list(pts[-1][1]))
        else:
            i = max(k for k in range(len(pts) - 1) if pts[k][0] <= c)
            (ta, A), (tb, B) = pts[i], pts[i + 1]
            u = (c - ta) / (tb - ta)
            out.append([(s, float(np.float32((1.0 - u) * w))) for s, w in A] + [(s, float(np.float32(u * w))) for s, w in B])
    return out


def morph_vectors(predictor, points, n: int, window: int, hop: int, sample_rate: int, label_offset: int = 0):
    """[n, E]: one vector per window of a long file whose voice moves through `points` (`morph_entries`), one mix call for all windows;
    `VQVAE.decode_long(vectors=)` cross-fades the windows as it does any others."""
    return _mix_entries(predictor, morph_entries(points, n, window, hop, sample_rate), label_offset)


def _digest(seed, key, what: str, i: int) -> bytes:
    return hashlib.sha256(f"{seed}\0{key}\0{what}\0{i}".encode("utf-8")).digest()


def pseudo_voice(seed, key, num_labels: int, k: int, exclude=()) -> str:
    """A pseudo-speaker: the spec of `k` distinct labels with convex weights, a function of (seed, key) alone -- built from sha256, so
    it does not depend on any library's generators.  Labels: the k of 0..num_labels-1 outside `exclude` with the smallest
    sha256(f"{seed}\\0{key}\\0label\\0{l}"), in that order.  Weights: g_j / sum g with g_j = -log(u_j), u_j = (x_j + 0.5) / 2^53 for x_j
    the top 53 bits of the first 8 bytes (big-endian) of sha256(f"{seed}\\0{key}\\0w\\0{j}"), computed in float64 and rounded to
    float32 once."""
    exclude = {int(e) for e in exclude}
    pool = [l for l in range(int(num_labels)) if l not in exclude]
    if not 1 <= int(k) <= min(len(pool), MAX_ENTRIES):
        raise ValueError(f"pseudo_voice: k={k} outside 1..{min(len(pool), MAX_ENTRIES)} ({len(pool)} labels to draw from, {MAX_ENTRIES} entries per spec)")
    labels = sorted(pool, key=lambda l: _digest(seed, key, "label", l))[:int(k)]
    g = [-math.log(((int.from_bytes(_digest(seed, key, "w", j)[:8], "big") >> 11) + 0.5) / 2.0 ** 53) for j in range(int(k))]
    total = sum(g)
    return format_voice([(l, gj / total) for l, gj in zip(labels, g)])


def save_voice(path: str, vector, meta: Optional[dict] = None) -> None:
    """A voice file: `path` (.npy) holds the [E] float32 vector bit for bit, the side-car .json beside it what it was fitted on
    (the checkpoint's base_channels, the steps, the holdout loss if there was one)."""
    if not str(path).endswith(".npy"):
        raise ValueError(f"voice file {path!r}: the name must end in .npy")
    vec = vector.detach().cpu().numpy() if hasattr(vector, "detach") else np.asarray(vector)
    if vec.ndim != 1 or vec.dtype != np.float32:
        raise ValueError(f"a voice is one float32 vector [E], got {vec.dtype} {vec.shape}")
    np.save(path, np.ascontiguousarray(vec))
    with open(os.path.splitext(path)[0] + ".json", "w") as f:
        json.dump(dict(meta or {}, entries=int(vec.shape[0])), f, indent=1, sort_keys=True)
        f.write("\n")


def load_voice(path: str):
    """(vector [E] float32 ndarray, meta dict -- empty without a side-car) of a voice file."""
    vec = np.load(path, allow_pickle=False)
    if vec.ndim != 1 or vec.dtype != np.float32:
        raise ValueError(f"voice file {path!r}: expected one float32 vector [E], got {vec.dtype} {vec.shape}")
    side = os.path.splitext(path)[0] + ".json"
    meta = {}
    if os.path.exists(side):
        with open(side) as f:
            meta = json.load(f)
    return vec, meta
