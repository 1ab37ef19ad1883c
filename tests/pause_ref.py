"""The pause detector and the kept-window test of the library (include/vqvs.h "Pauses"), restated in int64 numpy in the RUN form of
the definition, and the packed keep region as a loop over recordings calling tests/keep_ref.py: the references that
tests/test_pauses.py checks against themselves and tests/test_pauses_gpu.py compares the kernels with.  It does not import the
library.

Per recording row of L samples: q = clamp(rint(x * 32768), -32768, 32767), NaN -> 0; frame f covers [f frame, min((f + 1) frame, L))
with c_f samples; the frame is quiet iff sum q^2 <= thr * c_f; a pause is a maximal run of quiet frames at least min_frames long, and
its kept part is the run less guard_frames at each end that touches a loud frame."""
import numpy as np

import keep_ref


def quantise(x):
    """float32 samples -> int64, the sample rule of vqvs_pitch_distance: x * 32768 is exact in float32, rint rounds ties to even."""
    p = np.asarray(x, dtype=np.float32) * np.float32(32768.0)
    q = np.clip(np.rint(p.astype(np.float64)), -32768.0, 32767.0)
    return np.where(np.isnan(p), 0.0, q).astype(np.int64)


def quiet_frames(x, frame, thr):
    """The quiet flag of every frame of one row (bool [F])."""
    q = quantise(x)
    L = q.shape[0]
    F = -(-L // frame)
    flags = np.zeros(F, bool)
    for f in range(F):
        seg = q[f * frame:min((f + 1) * frame, L)]
        flags[f] = int((seg * seg).sum()) <= int(thr) * seg.shape[0]
    return flags


def kept_frames_runs(quiet, min_frames, guard):
    """RUN form: (kept flag per frame, number of pauses)."""
    F = len(quiet)
    kept = np.zeros(F, bool)
    pauses, f = 0, 0
    while f < F:
        if not quiet[f]:
            f += 1
            continue
        g = f
        while g < F and quiet[g]:
            g += 1  # the run is [f, g)
        if g - f >= min_frames:
            pauses += 1
            lo = f + (guard if f > 0 else 0)    # an end that touches a loud frame is trimmed; the row's own ends are not
            hi = g - (guard if g < F else 0)
            kept[lo:max(lo, hi)] = True
        f = g
    return kept, pauses


def kept_frames_scan(quiet, min_frames, guard):
    """SCAN form: left(f) the last loud frame <= f or -1, right(f) the first loud frame >= f or F."""
    F = len(quiet)
    left, right = np.empty(F, np.int64), np.empty(F, np.int64)
    last = -1
    for f in range(F):
        if not quiet[f]:
            last = f
        left[f] = last
    nxt = F
    for f in range(F - 1, -1, -1):
        if not quiet[f]:
            nxt = f
        right[f] = nxt
    f = np.arange(F)
    return np.asarray(quiet, bool) & (right - left - 1 >= min_frames) & ((left < 0) | (f - left > guard)) & ((right >= F) | (right - f > guard))


def pause_mask_row(x, frame, thr, min_frames, guard):
    """One row -> (uint8 mask [L], kept samples, pauses)."""
    L = len(x)
    kept, pauses = kept_frames_runs(quiet_frames(x, frame, thr), min_frames, guard)
    mask = np.repeat(kept, frame)[:L].astype(np.uint8)
    return mask, int(mask.sum()), pauses


def pack_offsets(counts, W, H):
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    V = W - H
    offs = [int(first[r]) * H + r * V for r in range(len(counts))]
    lens = [int(c) * H + V for c in counts]
    return first, offs, lens


def pause_mask(x, counts, W, H, frame, thr, min_frames, guard):
    """The rows of a pack end to end -> (uint8 mask in the same layout, int64 [R, 2] of kept samples and pauses)."""
    _, offs, lens = pack_offsets(counts, W, H)
    out = np.zeros(len(x), np.uint8)
    stats = np.zeros((len(counts), 2), np.int64)
    for r, (o, n) in enumerate(zip(offs, lens)):
        out[o:o + n], stats[r, 0], stats[r, 1] = pause_mask_row(x[o:o + n], frame, thr, min_frames, guard)
    return out, stats


def windows_kept(keep, counts, W, H):
    """uint8 [N]: 1 for a window whose W mask bytes are all non-zero."""
    first, offs, _ = pack_offsets(counts, W, H)
    out = np.zeros(int(first[-1]), np.uint8)
    for r, c in enumerate(counts):
        for b in range(int(c)):
            out[int(first[r]) + b] = np.all(np.asarray(keep)[offs[r] + b * H:offs[r] + b * H + W] != 0)
    return out


def keep_region_packed(x, windows, x0, keep, noise, alpha, counts, W, H, noise_scale=1.0, seed=0, clip=0, index=0):
    """The packed keep region: `keep_ref.keep_region_windows` on every recording's own slices at clip + r.  x, x0, keep, noise in
    pack layout, windows [N, W] or None -> (x, windows, magnitude)."""
    first, offs, lens = pack_offsets(counts, W, H)
    out, mag = np.asarray(x, dtype=np.float64).copy(), np.zeros(len(x))
    win = None if windows is None else np.asarray(windows, dtype=np.float64).copy()
    for r, (o, n) in enumerate(zip(offs, lens)):
        sl, ws = slice(o, o + n), slice(int(first[r]), int(first[r + 1]))
        out[sl], w, mag[sl] = keep_ref.keep_region_windows(out[sl], None if win is None else win[ws], x0[sl], None if keep is None else keep[sl],
                                                           None if noise is None else noise[sl], alpha, int(counts[r]), W, H,
                                                           noise_scale=noise_scale, seed=seed, clip=clip + r, index=index)
        if win is not None:
            win[ws] = w
    return out, win, mag
