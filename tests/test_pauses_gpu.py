"""Pauses on the device: `vqvs_keep_region_windows_packed` against the per-recording `vqvs_keep_region_windows` call, `vqvs_pause_mask`
and `vqvs_windows_kept` against the int64 numpy definition (tests/pause_ref.py), `decode_long_batch(sources=, keeps=, keep_pauses=)`
against `decode_long` on each recording alone, skipping on against skipping off, and `convert_dataset.py --keep-pauses` end to end.
Every comparison is bitwise: the packed keep IS the single call on each recording's slices, the detector is integer arithmetic, and a
skipped window cannot reach the result.

The window loops run on the tiny VQ-VAE of tests/test_keep_gpu.py.  Its downsample rate is 256 and `decode_long` takes windows and
hops that are multiples of it, so the loops use the smallest geometry with a partial overlap, window 768 and hop 512 (256 / 192 is
refused by `check_rate`)."""
import os
import sys

import numpy as np
import pytest
import torch

import pause_ref
from test_keep_gpu import ALPHAS, CLIP, INDEX, SEED, bits, call_windows, det_model, read_s16, window_masks
from vq_voice_swap_amd import VQVAE, EncoderPredictor, _native, pauses
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter
from vq_voice_swap_amd.longform import gather_windows, plan_pack

from util import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(16, 16), (16, 12), (32, 16)]
COUNTS = [(1,), (2, 1), (1, 3, 1), (4,)]
KEEP_ALPHAS = [1.0, 0.5, 2.0 ** -20, 0.0]
assert set(KEEP_ALPHAS) <= set(ALPHAS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def first_of(counts, dev):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)


# ---------------------------------------------------------------- 1. the packed keep region
def pack_masks(counts, W, H):
    """name -> uint8 [total] or None: the masks of tests/test_keep_gpu.py on every recording's own row, and `seam`, which keeps exactly
    the last quad of recording r and the first of r + 1."""
    _, offs, lens = pause_ref.pack_offsets(counts, W, H)
    per = [window_masks(c, W, H) for c in counts]
    masks = {k: (None if per[0][k] is None else np.concatenate([p[k] for p in per])) for k in per[0]}
    seam = np.zeros(offs[-1] + lens[-1], np.uint8)
    for o in offs[1:]:
        seam[o - 4:o + 4] = 1
    seam[:4] = seam[-4:] = 1
    masks["seam"] = seam
    return masks


def call_packed(x, windows, x0, keep, noise, alpha, counts, W, H, seed=SEED, clip=CLIP, index=INDEX):
    """`vqvs_keep_region_windows_packed` on copies of x [total] and windows [N, W] (or None), each in front of a NaN guard."""
    total, N = x.numel(), sum(counts)
    guard = torch.full((64,), float("nan"), device=x.device)
    xb = torch.cat([x, guard])
    wb = None if windows is None else torch.cat([windows.reshape(-1), guard])
    first = first_of(counts, x.device)
    _native.check(_native.lib().vqvs_keep_region_windows_packed(xb.data_ptr(), _native._ptr(wb), x0.data_ptr(), _native._ptr(keep), _native._ptr(noise),
                                                                alpha.data_ptr(), first.data_ptr(), len(counts), W, H, 1.0, seed, clip, index,
                                                                _native._stream_ptr()))
    assert torch.isnan(xb[total:]).all() and (wb is None or torch.isnan(wb[N * W:]).all()), "the kernel wrote past the end of an output"
    return xb[:total], None if wb is None else wb[:N * W].view(N, W)


@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("W,H", GEOMETRIES)
def test_packed_keep_is_the_single_call_on_every_recording(dev, W, H, counts):
    first, offs, lens = pause_ref.pack_offsets(counts, W, H)
    total, N = offs[-1] + lens[-1], sum(counts)
    x0, noise = (seeded((total,), 91 + k).to(dev) for k in range(2))
    x = torch.full((total,), float("nan"), device=dev)  # a sample outside the mask keeps its NaN: it is not written
    windows = torch.full((N, W), float("nan"), device=dev)
    cases = 0
    for alpha in KEEP_ALPHAS:
        a = torch.tensor([alpha], dtype=torch.float32, device=dev)
        for name, m in pack_masks(counts, W, H).items():
            keep = None if m is None else torch.from_numpy(m).to(dev)
            for nz in (noise, None):  # supplied and drawn
                what = f"(W, H)=({W}, {H}) counts={counts} alpha={alpha} mask={name} noise={'supplied' if nz is not None else 'drawn'}"
                got, win = call_packed(x, windows, x0, keep, nz, a, counts, W, H)
                alone, _ = call_packed(x, None, x0, keep, nz, a, counts, W, H)  # the optional output changes nothing
                assert torch.equal(bits(alone), bits(got)), what
                for r, (o, n) in enumerate(zip(offs, lens)):
                    sl, ws = slice(o, o + n), slice(int(first[r]), int(first[r + 1]))
                    want, want_win = call_windows(x[sl], windows[ws], x0[sl], None if keep is None else keep[sl], None if nz is None else nz[sl], a,
                                                  counts[r], W, H, clip=CLIP + r)
                    assert torch.equal(bits(got[sl]), bits(want)), (what, r)
                    assert torch.equal(bits(win[ws]), bits(want_win)), (what, r)
                kept = torch.ones(total, dtype=torch.bool, device=dev) if keep is None else keep != 0
                assert torch.isnan(got[~kept]).all() and not torch.isnan(got[kept]).any(), what
                if alpha == 1.0:
                    assert torch.equal(bits(got)[kept], bits(x0)[kept]), what
                cases += 1
    assert cases == len(KEEP_ALPHAS) * 8 * 2
    # against the float64 reference, supplied noise, within the bound of tests/test_keep_gpu.py (two roundings of the magnitude)
    m = pack_masks(counts, W, H)["half"]
    a = torch.tensor([0.5], dtype=torch.float32, device=dev)
    start = seeded((total,), 93).to(dev)
    got, win = call_packed(start, gather_pack(start, counts, W, H), x0, torch.from_numpy(m).to(dev), noise, a, counts, W, H)
    want, want_win, mag = pause_ref.keep_region_packed(start.cpu().numpy(), gather_pack(start, counts, W, H).cpu().numpy(), x0.cpu().numpy(), m,
                                                       noise.cpu().numpy(), 0.5, counts, W, H)
    assert (np.abs(got.cpu().double().numpy() - want) <= 2 * 2.0 ** -24 * mag + 1e-300)[m != 0].all()
    assert torch.equal(bits(got)[torch.from_numpy(m == 0)], bits(start)[torch.from_numpy(m == 0)])
    assert torch.equal(bits(win), bits(gather_pack(got, counts, W, H)))  # every window copy is the long state's value


def gather_pack(x, counts, W, H):
    _, offs, lens = pause_ref.pack_offsets(counts, W, H)
    return torch.cat([gather_windows(x[o:o + n], W, H).view(-1, W) for o, n in zip(offs, lens)])


# ---------------------------------------------------------------- 2. the detector
FRAME, THR = 8, 4
DW, DH = 404, 300  # rows of 300 n + 104 samples: 50.5, 88, 125.5 and 163 frames of 8 -- a partial tail frame at odd n
SETTINGS = [(5, 2), (5, 3), (1, 0), (3, 1), (12, 1)]  # (min_frames, guard_frames); (5, 3): a pause of 5 or 6 frames has no kept part


def lsb(v):
    return np.float32(v / 32768.0)


def design_row(L, seed):
    """One row with, in frames of 8 (min_frames 5): a quiet run at the row's start [0, 6); a run of exactly min_frames [9, 14); a run
    of min_frames - 1 [17, 21); a run [24, 36) whose frame 30 has E = thr * c exactly, ended by frame 36 with E = thr * c + 1; a quiet run
    to the row's end (through a partial tail frame when L % 8); seeded quiet / loud frames between frame 40 and that run.  Loud frames
    hold values off the 16-bit grid and beyond +-1; quiet ones ties at +-0.5, a NaN and small values."""
    rng = np.random.default_rng(seed)
    F = -(-L // FRAME)
    quiet = np.zeros(F, bool)
    for a, b in ((0, 6), (9, 14), (17, 21), (24, 36), (F - 7, F)):
        quiet[a:b] = True
    if F - 7 > 41:
        quiet[40:F - 8] = rng.random(F - 48) < 0.7
    x = np.zeros(F * FRAME, np.float32)
    for f in range(F):
        seg = x[f * FRAME:(f + 1) * FRAME]
        if quiet[f]:
            seg[:] = rng.choice([lsb(0), lsb(1), lsb(-1), lsb(0.5), lsb(-0.5), lsb(0.4), lsb(1.49)], FRAME)  # |q| <= 1: E <= 8
            if f % 3 == 0:
                seg[rng.integers(FRAME)] = np.nan
        else:
            seg[:] = rng.choice([lsb(100.3), lsb(-77.5), np.float32(2.0), np.float32(-3.0), np.float32(0.25), np.float32(np.inf), lsb(3.5)], FRAME)
    x[30 * FRAME:31 * FRAME] = [lsb(v) for v in (4, 4, 0, 0, 0.5, -0.5, 0, 0)]   # E = 32 = thr * 8: quiet
    x[36 * FRAME:37 * FRAME] = [lsb(v) for v in (4, -4, 1, 0, 0.5, 0, 0, 0)]     # E = 33: loud
    x = x[:L]
    want = quiet.copy()
    want[36] = False
    assert np.array_equal(pause_ref.quiet_frames(x, FRAME, THR), want), "the design is not what the reference sees"
    return x


def design_pack(counts, seed=0):
    _, offs, lens = pause_ref.pack_offsets(counts, DW, DH)
    return np.concatenate([design_row(n, seed + 10 * r + n) for r, n in enumerate(lens)])


def call_pause_mask(x, counts, W, H, frame, thr, min_frames, guard, with_counts=True):
    """`vqvs_pause_mask` with guard bytes behind the mask and the counts, both pre-filled with a value the kernel never writes."""
    dev, total, R = x.device, x.numel(), len(counts)
    keep = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device=dev)
    stats = torch.full((2 * R + 8,), -7, dtype=torch.int64, device=dev) if with_counts else None
    first = first_of(counts, dev)
    _native.check(_native.lib().vqvs_pause_mask(x.data_ptr(), keep.data_ptr(), _native._ptr(stats), first.data_ptr(), R, W, H, frame, thr, min_frames,
                                                guard, _native._stream_ptr()))
    assert (keep[total:] == 0xAB).all() and (stats is None or (stats[2 * R:] == -7).all()), "the kernel wrote past the end of an output"
    return keep[:total], None if stats is None else stats[:2 * R].view(R, 2)


@pytest.mark.parametrize("counts", COUNTS)
def test_pause_mask_is_the_definition(dev, counts):
    x_np = design_pack(counts)
    x = torch.from_numpy(x_np).to(dev)
    trimmed = False
    for min_frames, guard in SETTINGS:
        got, stats = call_pause_mask(x, counts, DW, DH, FRAME, THR, min_frames, guard)
        want, want_stats = pause_ref.pause_mask(x_np, counts, DW, DH, FRAME, THR, min_frames, guard)
        assert np.array_equal(got.cpu().numpy(), want), (counts, min_frames, guard)
        assert np.array_equal(stats.cpu().numpy(), want_stats), (counts, min_frames, guard)
        assert torch.equal(got, call_pause_mask(x, counts, DW, DH, FRAME, THR, min_frames, guard, with_counts=False)[0])
        assert set(np.unique(want)) == {0, 1}, "a degenerate design: the mask must hold both values"
        quiet = np.concatenate([np.repeat(pause_ref.quiet_frames(x_np[o:o + n], FRAME, THR), FRAME)[:n]
                                for o, n in zip(*pause_ref.pack_offsets(counts, DW, DH)[1:])])
        trimmed |= guard > 0 and bool((quiet & (want == 0)).any()) and bool(want_stats[:, 1].min() > 0)
        # the wrapper, at the level that gives this integer threshold
        if (min_frames, guard) == (5, 2):
            m, s = pauses.pause_mask(x.view(1, 1, -1), counts, DW, DH, threshold_db=-84.0, frame=FRAME, min_pause_frames=5, guard_frames=2,
                                     return_counts=True)
            assert pauses.threshold_energy(-84.0) == THR and torch.equal(m.view(-1), got) and torch.equal(s, stats)
    assert trimmed, "no run was trimmed"
    # a recording's mask alone is its mask inside the pack, and an unaligned input takes the one-sample path to the same mask
    _, offs, lens = pause_ref.pack_offsets(counts, DW, DH)
    whole, _ = call_pause_mask(x, counts, DW, DH, FRAME, THR, 5, 2)
    for r, (o, n) in enumerate(zip(offs, lens)):
        alone, _ = call_pause_mask(x[o:o + n].clone(), (counts[r],), DW, DH, FRAME, THR, 5, 2)
        assert torch.equal(alone, whole[o:o + n]), r
    shifted = torch.cat([torch.zeros(1, device=dev), x])[1:]
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(call_pause_mask(shifted, counts, DW, DH, FRAME, THR, 5, 2)[0], whole)


def test_pause_mask_carries_across_chunks(dev):
    """One row of 5001 frames -- 20 chunks of 256 -- with pauses that span chunks, chunks without a loud frame and chunks without a
    quiet one: left(f) and right(f) come from chunks away."""
    n = 133
    L = n * DH + (DW - DH)
    F = -(-L // FRAME)
    assert (L, F) == (40004, 5001)
    rng = np.random.default_rng(5)
    quiet = rng.random(F) < 0.7
    for a, b, v in ((299, 300, False), (300, 1500, True), (1500, 1800, False), (3999, 4000, False), (2000, 2500, True), (2500, 2501, False), (2501, 2700, True), (3000, 3300, False),
                    (4000, F, True), (0, 1, True)):
        quiet[a:b] = v
    x_np = np.where(np.repeat(quiet, FRAME), lsb(1), lsb(100)).astype(np.float32)[:L]
    x = torch.from_numpy(x_np).to(dev)
    for min_frames, guard in ((600, 100), (450, 0), (2, 1), (1 << 20, 0), (1, 1 << 20)):
        got, stats = call_pause_mask(x, (n,), DW, DH, FRAME, THR, min_frames, guard)
        want, want_stats = pause_ref.pause_mask(x_np, (n,), DW, DH, FRAME, THR, min_frames, guard)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), want_stats), (min_frames, guard)
    want, want_stats = pause_ref.pause_mask(x_np, (n,), DW, DH, FRAME, THR, 600, 100)
    assert set(np.unique(want)) == {0, 1} and want_stats[0, 1] == 2 and want_stats[0, 0] == (1200 - 200 + 1001 - 100) * FRAME - 4
    # the same row between two others: its mask does not depend on its place
    counts = (2, n, 1)
    _, offs, lens = pause_ref.pack_offsets(counts, DW, DH)
    pack = np.concatenate([design_row(lens[0], 1), x_np, design_row(lens[2], 2)])
    got, _ = call_pause_mask(torch.from_numpy(pack).to(dev), counts, DW, DH, FRAME, THR, 600, 100)
    assert np.array_equal(got.cpu().numpy()[offs[1]:offs[1] + L], want)
    assert np.array_equal(got.cpu().numpy(), pause_ref.pause_mask(pack, counts, DW, DH, FRAME, THR, 600, 100)[0])


def test_pause_mask_other_frames(dev):
    """The frame sizes that take another lane grouping in the energy pass (1, 2, 32 and 64 lanes per frame, several passes per frame),
    on random rows around the threshold."""
    counts, W, H = (1, 3, 1), 2052, 1500
    _, offs, lens = pause_ref.pack_offsets(counts, W, H)
    total = offs[-1] + lens[-1]
    rng = np.random.default_rng(9)
    for frame, thr in ((4, 9), (12, 9), (160, 9), (256, 9), (1000, 9), (4096, 9)):
        level = np.repeat(rng.choice([1.0, 2.9, 3.1, 40.0], -(-total // frame) + 1), frame)[:total]
        x_np = (level * rng.choice([-1.0, 1.0], total) / 32768.0).astype(np.float32)
        got, stats = call_pause_mask(torch.from_numpy(x_np).to(dev), counts, W, H, frame, thr, 2, 1)
        want, want_stats = pause_ref.pause_mask(x_np, counts, W, H, frame, thr, 2, 1)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), want_stats), frame


# ---------------------------------------------------------------- 3. the kept windows
@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("W,H", GEOMETRIES + [(DW, DH)])
def test_windows_kept(dev, W, H, counts):
    _, offs, lens = pause_ref.pack_offsets(counts, W, H)
    total, N = offs[-1] + lens[-1], sum(counts)
    masks = {"ones": np.full(total, 255, np.uint8), "zeros": np.zeros(total, np.uint8)}
    if (W, H) == (DW, DH):
        x_np = design_pack(counts)
        for min_frames, guard in SETTINGS:
            masks[f"pauses{min_frames}.{guard}"] = pause_ref.pause_mask(x_np, counts, W, H, FRAME, THR, min_frames, guard)[0]
        for b in range(N):  # all but one sample of one window
            m = np.ones(total, np.uint8)
            r = int(np.searchsorted(np.cumsum(counts), b, side="right"))
            m[b * H + r * (W - H) + (7 * b) % W] = 0
            masks[f"hole{b}"] = m
    else:
        masks.update({k: v for k, v in pack_masks(counts, W, H).items() if v is not None})
    first = first_of(counts, dev)
    some = set()
    for name, m in masks.items():
        out = torch.full((N + 64,), 0xAB, dtype=torch.uint8, device=dev)
        keep = torch.from_numpy(m).to(dev)
        _native.check(_native.lib().vqvs_windows_kept(keep.data_ptr(), out.data_ptr(), first.data_ptr(), len(counts), W, H, _native._stream_ptr()))
        assert (out[N:] == 0xAB).all(), "the kernel wrote past the end of its output"
        want = pause_ref.windows_kept(m, counts, W, H)
        assert np.array_equal(out[:N].cpu().numpy(), want), name
        assert torch.equal(pauses.windows_kept(keep.view(1, 1, -1), counts, W, H), out[:N]) and torch.equal(pauses.windows_kept(keep.bool(), counts, W, H), out[:N])
        some |= set(want.tolist())
    assert some == {0, 1}


# ---------------------------------------------------------------- 4. the window loops
LW, LH, STEPS = 768, 512, 4
NUM_SAMPLES = [1700, 1200, 700]  # 3, 2 and 1 windows of 768 every 512
DETECTOR = dict(threshold_db=-60.0, frame=16, min_pause_frames=4, guard_frames=1)


@pytest.fixture(scope="module")
def vqvae(dev):
    return det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=3), dev)


@pytest.fixture(scope="module")
def recordings(dev):
    """Tone bursts with gaps: recording 0 is silent up to sample 800 (its window 0 lies in the pause whole), recording 1 from sample
    400 on (its window 1, with the padding behind it), recording 2 has a gap too short to hold a window."""
    waves = []
    for r, n in enumerate(NUM_SAMPLES):
        w = (0.3 * np.sin(np.arange(n) * (0.05 + 0.01 * r))).astype(np.float32)
        a, b = ((0, 800), (400, n), (300, 500))[r]
        w[a:b] = 0.0
        waves.append(torch.from_numpy(w[None, None]).to(dev))
    keeps = [torch.zeros(1, 1, NUM_SAMPLES[0], dtype=torch.bool, device=dev), None, None]
    keeps[0][..., 1000:1100] = True  # a range the user keeps, beside the pauses
    return waves, keeps


def expected_masks(recordings):
    """Per recording the un-padded mask the run keeps, from the numpy definition; and the pack's skipped windows."""
    waves, keeps = recordings
    counts, offsets, total = plan_pack(NUM_SAMPLES, LW, LH)
    assert counts == [3, 2, 1]
    thr = pauses.threshold_energy(DETECTOR["threshold_db"])
    masks, whole = [], []
    for r, (w, c) in enumerate(zip(waves, counts)):
        row = np.zeros((c - 1) * LH + LW, np.float32)
        row[:NUM_SAMPLES[r]] = w.cpu().numpy().reshape(-1)
        m = pause_ref.pause_mask_row(row, DETECTOR["frame"], thr, DETECTOR["min_pause_frames"], DETECTOR["guard_frames"])[0]
        if keeps[r] is not None:
            m[:NUM_SAMPLES[r]] |= keeps[r].cpu().numpy().reshape(-1).astype(np.uint8)
        whole += pause_ref.windows_kept(m, (c,), LW, LH).tolist()
        masks.append(torch.from_numpy(m[:NUM_SAMPLES[r]] != 0).to(w.device).view(1, 1, -1))
    return masks, whole


class Counting:
    """Counts the rows the decoder's predictor is run on."""

    def __init__(self, model):
        self.model, self.rows, self.calls = model, 0, 0

    def __enter__(self):
        self.forward = self.model.predictor.forward

        def counting(xs, *a, **kw):
            self.rows += xs.shape[0]
            self.calls += 1
            return self.forward(xs, *a, **kw)

        self.model.predictor.forward = counting
        return self

    def __exit__(self, *exc):
        del self.model.predictor.forward


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
def test_pack_with_pauses_is_each_recording_alone(dev, vqvae, recordings, sampler):
    waves, keeps = recordings
    codes, counts = vqvae.encode_long_batch(waves, LW, LH)
    masks, whole = expected_masks(recordings)
    assert whole == [1, 0, 0, 0, 1, 0], "the design must skip some windows and run others"
    label = torch.tensor([1, 2, 0], device=dev)
    kw = dict(window=LW, hop=LH, steps=STEPS, constrain=True, seed=9, sampler=sampler, keep_pauses=DETECTOR)
    if sampler == "ddim":
        kw["eta"] = 0.5
    first = np.concatenate([[0], np.cumsum(counts)])
    for strength in (1.0, 0.5):
        alone = [vqvae.decode_long(codes[first[r]:first[r + 1]], label[r:r + 1], num_samples=NUM_SAMPLES[r], clip_offset=5 + r, source=waves[r],
                                   keep=keeps[r], strength=strength, **kw) for r in range(3)]
        for wb in ((1, 2, 64) if strength == 1.0 else (2,)):
            stats = {}
            with Counting(vqvae) as seen:
                got = vqvae.decode_long_batch(codes, label, counts=counts, num_samples=NUM_SAMPLES, clip_offset=5, sources=waves, keeps=keeps,
                                              strength=strength, window_batch=wb, stats=stats, **kw)
            run_steps = STEPS if strength == 1.0 else 2
            assert seen.rows == run_steps * whole.count(0), (sampler, wb, seen.rows)  # exactly the active windows were predicted
            assert stats == dict(kept_samples=sum(int(m.sum()) for m in masks), windows=6, skipped_windows=2)
            for r in range(3):
                assert got[r].shape == (1, 1, NUM_SAMPLES[r])
                assert torch.equal(bits(got[r]), bits(alone[r])), (sampler, strength, wb, r)
                assert torch.equal(bits(got[r])[masks[r]], bits(waves[r])[masks[r]]), (sampler, strength, wb, r)  # kept samples ARE the source
                assert masks[r].any() and not masks[r].all() and not torch.equal(got[r][~masks[r]], waves[r][~masks[r]])
        with Counting(vqvae) as seen:
            full = vqvae.decode_long_batch(codes, label, counts=counts, num_samples=NUM_SAMPLES, clip_offset=5, sources=waves, keeps=keeps,
                                           strength=strength, window_batch=2, skip_kept=False, **kw)
        assert seen.rows == (STEPS if strength == 1.0 else 2) * 6
        for r in range(3):  # skipping changes no bit
            assert torch.equal(bits(full[r]), bits(got[r])), (sampler, strength, r)
    plain = vqvae.decode_long_batch(codes, label, counts=counts, num_samples=NUM_SAMPLES, clip_offset=5, **{k: v for k, v in kw.items() if k != "keep_pauses"})
    assert not torch.equal(plain[1][masks[1]], waves[1][masks[1]])  # without the flags the pauses are re-synthesised


@pytest.mark.parametrize("mode", ["guidance", "enc_pred"])
def test_skipping_under_guidance_and_a_cond_fn(dev, vqvae, recordings, mode):
    waves, keeps = recordings
    codes, counts = vqvae.encode_long_batch(waves, LW, LH)
    masks, whole = expected_masks(recordings)
    label = torch.tensor([1], device=dev)
    kw = dict(counts=counts, num_samples=NUM_SAMPLES, window=LW, hop=LH, steps=STEPS, constrain=True, seed=9, clip_offset=5, sampler="ddim",
              sources=waves, keeps=keeps, keep_pauses=DETECTOR, window_batch=2)
    reps = 1
    if mode == "guidance":
        decode, reps = vqvae.decode_long_batch_uncond_guidance, 2
        kw.update(label_scale=2.0, vq_scale=0.0)
    else:
        ep = EncoderPredictor(base_channels=32, downsample_rate=256, num_latents=vqvae.dictionary_size, bottleneck_dim=64)
        decode = vqvae.decode_long_batch
        kw.update(enc_pred=det_model(ep, dev), enc_pred_scale=0.5)
    with Counting(vqvae) as seen:
        got = decode(codes, label, **kw)
    assert seen.rows == STEPS * reps * whole.count(0)
    with Counting(vqvae) as seen:
        full = decode(codes, label, skip_kept=False, **kw)
    assert seen.rows == STEPS * reps * len(whole)
    for r in range(3):
        assert torch.equal(bits(got[r]), bits(full[r])), (mode, r)
        assert torch.equal(bits(got[r])[masks[r]], bits(waves[r])[masks[r]]), (mode, r)
    first = np.concatenate([[0], np.cumsum(counts)])
    one = {k: v for k, v in kw.items() if k not in ("counts", "num_samples", "sources", "keeps", "clip_offset")}
    single = vqvae.decode_long_uncond_guidance if mode == "guidance" else vqvae.decode_long
    for r in (0, 1):
        alone = single(codes[first[r]:first[r + 1]], label, num_samples=NUM_SAMPLES[r], clip_offset=5 + r, source=waves[r], keep=keeps[r], **one)
        assert torch.equal(bits(alone), bits(got[r])), (mode, r)


# ---------------------------------------------------------------- 5. the scripts
def tone_bursts(n, i):
    w = (0.3 * np.sin(np.arange(n) * (0.05 + 0.01 * i))).astype(np.float32)
    for a, b in (((1400, 5600),), ((0, 2300),), ((900, 1300), (2500, 4000)))[i]:
        w[a:b] = 0.0
    return w


def test_convert_dataset_keeps_pauses(dev, vqvae, tmp_path, capsys):
    """`convert_dataset.py --keep-pauses -40 --strength 0.7` writes per file the bytes of `sample_vqvae.py --whole-file` with the same
    flags (the file with id 0 of a run: each file also alone in a directory), the pause samples of the output are what `ChunkWriter`
    writes for the source itself, and the final line reports the windows skipped."""
    sys.path.insert(0, ROOT)
    import convert_dataset
    import sample_vqvae

    ck = str(tmp_path / "v.pt")
    vqvae.save(ck)
    files = (("s1/a.wav", 8000), ("s1/b.wav", 4000), ("s2/a.wav", 6000))
    flags = ["--window-seconds", "0.128", "--overlap-seconds", "0.032", "--sample-steps", "4", "--seed", "9", "--keep-pauses", "-40", "--strength", "0.7",
             "--min-pause", "0.05", "--pause-guard", "0.01"]
    settings = dict(frame=160, thr=pauses.threshold_energy(-40), min_frames=5, guard=1)
    for i, (rel, n) in enumerate(files):
        for root in (tmp_path / "data", tmp_path / f"only{i}"):
            os.makedirs(root / os.path.dirname(rel), exist_ok=True)
            w = ChunkWriter(str(root / rel), 16000)
            w.write(tone_bursts(n, i))
            w.close()
    capsys.readouterr()
    totals = convert_dataset.main([ck, str(tmp_path / "data"), str(tmp_path / "out"), "--label", "2", "--pack-windows", "64", *flags])
    line = [l for l in capsys.readouterr().out.splitlines() if "files written" in l][-1]
    counts = plan_pack([n for _, n in files], 2048, 1536)[0]
    skipped_total = kept_total = 0
    for i, (rel, n) in enumerate(files):
        r = ChunkReader(str(tmp_path / "data" / rel), 16000)
        samples = r.read(n)
        r.close()
        row = np.zeros((counts[i] - 1) * 1536 + 2048, np.float32)
        row[:n] = samples
        mask = pause_ref.pause_mask_row(row, **settings)[0]
        skipped_total += int(pause_ref.windows_kept(mask, (counts[i],), 2048, 1536).sum())
        mask = mask[:n] != 0
        kept_total += int(mask.sum())
        assert mask.any() and not mask.all()
        echo = str(tmp_path / "echo.wav")
        w = ChunkWriter(echo, 16000)
        w.write(samples)
        w.close()
        out = read_s16(str(tmp_path / "out" / rel))
        assert out.shape == (n,) and np.array_equal(out[mask], read_s16(echo)[mask]), rel  # the pauses are the source's own samples
        assert (out[~mask] != read_s16(echo)[~mask]).mean() > 0.5, rel
        # the file alone in its directory has id 0: what sample_vqvae.py --whole-file writes with the same flags
        convert_dataset.main([ck, str(tmp_path / f"only{i}"), str(tmp_path / f"out{i}"), "--label", "2", *flags])
        one = str(tmp_path / f"one{i}.wav")
        sample_vqvae.main(["--label", "2", "--input-file", str(tmp_path / f"only{i}" / rel), "--whole-file", *flags, ck, one])
        with open(one, "rb") as a, open(tmp_path / f"out{i}" / rel, "rb") as b:
            assert a.read() == b.read(), rel
        if i == 0:
            with open(one, "rb") as a, open(tmp_path / "out" / rel, "rb") as b:
                assert a.read() == b.read()
    assert skipped_total >= 1 and [int(t) for t in totals] == [3, 0, 18000, sum(counts), 1, kept_total, skipped_total]
    assert line.endswith(f", kept {kept_total / 16000:.1f} s, skipped {skipped_total} of {sum(counts)} windows"), line


def test_sample_vqvae_clip_keeps_pauses(dev, vqvae, tmp_path):
    """Without --whole-file a clip is a pack of one recording of one window without overlap: its pauses, OR-ed with --keep, come out as
    the source's own samples on the writer's grid."""
    sys.path.insert(0, ROOT)
    import sample_vqvae

    ck, src, dst, echo = (str(tmp_path / name) for name in ("v.pt", "in.wav", "out.wav", "echo.wav"))
    vqvae.save(ck)
    N = 16000
    wave = (0.3 * np.sin(np.arange(N) * 0.05)).astype(np.float32)
    wave[4000:9000] = 0.0
    w = ChunkWriter(src, 16000)
    w.write(wave)
    w.close()
    r = ChunkReader(src, 16000)
    samples = r.read(N)
    r.close()
    usable = N // 256 * 256  # a single clip is cut to a multiple of the model's rate
    w = ChunkWriter(echo, 16000)
    w.write(samples[:usable])
    w.close()
    sample_vqvae.main(["--label", "2", "--input-file", src, "--sample-steps", "3", "--seed", "9", "--seconds", "1", "--keep-pauses", "-40",
                       "--min-pause", "0.05", "--pause-guard", "0.01", "--keep", "0.9:0.95", ck, dst])
    mask = pause_ref.pause_mask_row(samples[:usable], 160, pauses.threshold_energy(-40), 5, 1)[0] != 0
    assert mask[4160:8800].all() and not mask[:4160].any() and not mask[8800:].any()
    mask[14400:15200] = True
    out, want = read_s16(dst), read_s16(echo)
    assert out.shape == want.shape == (usable,) and np.array_equal(out[mask], want[mask])
    assert (out[~mask] != want[~mask]).mean() > 0.5
