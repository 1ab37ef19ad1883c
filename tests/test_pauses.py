"""Pauses, host side: exports, declarations and argument checks of `vqvs_keep_region_windows_packed`, `vqvs_pause_mask` and
`vqvs_windows_kept`; the dB threshold; the run form of the detector's definition against its scan form (tests/pause_ref.py); the
scripts' flags and final line; the `skip=` / `pack_...=` keywords of the window loops on CPU tensors (none of this needs a device)."""
import contextlib
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import pause_ref
import vq_voice_swap_amd
from vq_voice_swap_amd import _native, longform, pauses, plan_pack
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEEP_ARGS = ["float* d_x", "float* d_windows", "const float* d_x0", "const uint8_t* d_keep", "const float* d_noise", "const float* d_alpha",
             "const int32_t* d_first", "int R", "int W", "int H", "float noise_scale", "uint64_t seed", "uint64_t clip", "uint32_t index",
             "void* stream"]
MASK_ARGS = ["const float* d_x", "uint8_t* d_keep", "int64_t* d_counts", "const int32_t* d_first", "int R", "int W", "int H", "int frame",
             "int64_t thr", "int min_frames", "int guard_frames", "void* stream"]
KEPT_ARGS = ["const uint8_t* d_keep", "uint8_t* d_out", "const int32_t* d_first", "int R", "int W", "int H", "void* stream"]
METHODS = ["ddpm_sample_windows", "ddim_sample_windows", "dpmpp_sample_windows"]


# ---------------------------------------------------------------- 1. exports, declarations, refusals
def test_symbols_are_exported_and_declared(lib_built):
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    for name, want in (("vqvs_keep_region_windows_packed", KEEP_ARGS), ("vqvs_pause_mask", MASK_ARGS), ("vqvs_windows_kept", KEPT_ARGS)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl, f"include/vqvs.h does not declare {name}"
        assert [a.strip() for a in " ".join(decl.group(1).split()).split(",")] == want
        assert len(getattr(lib_built, name).argtypes) == len(want)
    for name in ("pause_mask", "threshold_energy", "windows_kept"):
        assert name in vq_voice_swap_amd.__all__ and getattr(vq_voice_swap_amd, name) is getattr(pauses, name)


def host_buffers(count, floats=256):
    bufs = [(C.c_float * floats)() for _ in range(count)]
    return bufs, [C.cast(b, C.c_void_p) for b in bufs]


def refused(L, rc, *words):
    """VQVS_ERR_ARG, and the message names every one of `words`."""
    msg = L.vqvs_last_error() or b""
    return rc == -1 and all(w.encode() in msg for w in words)


def inside(p, nbytes):
    return C.c_void_p(p.value + nbytes)


GEOMETRY = [(dict(R=0), "R="), (dict(R=-1), "R="), (dict(R=65536), "R="), (dict(first=None), "first"),
            (dict(W=18, H=12), "W="), (dict(W=16, H=10), "H="), (dict(W=0, H=0), "W="), (dict(W=16, H=0), "H="), (dict(W=-16, H=-12), "W="),
            (dict(W=12, H=16), "overlap"), (dict(W=28, H=12), "overlap")]


def test_packed_keep_refuses_bad_arguments_without_a_device(lib_built):
    """Every refusal of include/vqvs.h: VQVS_ERR_ARG with host-only pointers, which a call that reached the device would fault on."""
    L = lib_built
    hold, (x, win, x0, keep, noise, alpha, first) = host_buffers(7)
    ok = dict(x=x, win=win, x0=x0, keep=keep, noise=noise, alpha=alpha, first=first, R=3, W=16, H=12, scale=1.0)  # R * W = 48 samples at the least

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_keep_region_windows_packed(a["x"], a["win"], a["x0"], a["keep"], a["noise"], a["alpha"], a["first"], a["R"], a["W"], a["H"],
                                                 a["scale"], 1, 2, 3, None)

    cases = [(dict(x=None), "d_x "), (dict(x0=None), "d_x0"), (dict(alpha=None), "d_alpha"),
             (dict(scale=float("nan")), "noise_scale"), (dict(scale=float("inf")), "noise_scale"),
             (dict(x0=x), "d_x0"), (dict(keep=x), "d_keep"), (dict(noise=x), "d_noise"), (dict(noise=inside(x, 4 * 47)), "d_noise"),
             (dict(keep=inside(x, 4 * 48 - 1)), "d_keep"),  # the mask is R * W BYTES at the least: its first byte is the last of x
             (dict(win=x), "d_windows"), (dict(win=x0), "d_windows"), (dict(win=keep), "d_windows"), (dict(win=noise), "d_windows"),
             (dict(win=alpha), "d_windows"), (dict(win=inside(x, 4 * 47)), "d_windows"), (dict(x=inside(win, 4 * 47)), "d_windows"),
             (dict(first=x), "d_first"), (dict(first=inside(x, 4 * 47)), "d_first"), (dict(win=first), "d_first"),
             (dict(win=None, keep=None, noise=None, x0=None), "d_x0")] + GEOMETRY
    for bad, word in cases:
        assert refused(L, call(**bad), word), (bad, L.vqvs_last_error())
    assert refused(L, call(win=x), "overlap") and refused(L, call(x=None), "non-NULL")


def test_pause_mask_refuses_bad_arguments_without_a_device(lib_built):
    L = lib_built
    hold, (x, keep, counts, first) = host_buffers(4)
    ok = dict(x=x, keep=keep, counts=counts, first=first, R=3, W=16, H=12, frame=8, thr=4, min_frames=3, guard=1)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_pause_mask(a["x"], a["keep"], a["counts"], a["first"], a["R"], a["W"], a["H"], a["frame"], a["thr"], a["min_frames"],
                                 a["guard"], None)

    cases = [(dict(x=None), "d_x "), (dict(keep=None), "d_keep"), (dict(counts=None, keep=None), "d_keep"),
             (dict(frame=0), "frame="), (dict(frame=2), "frame="), (dict(frame=10), "frame="), (dict(frame=4100), "frame="), (dict(frame=-8), "frame="),
             (dict(thr=-1), "thr="), (dict(thr=(1 << 30) + 1), "thr="), (dict(thr=1 << 40), "thr="),
             (dict(min_frames=0), "min_frames="), (dict(min_frames=(1 << 20) + 1), "min_frames="), (dict(min_frames=-3), "min_frames="),
             (dict(guard=-1), "guard_frames="), (dict(guard=(1 << 20) + 1), "guard_frames="),
             (dict(keep=x), "d_keep"), (dict(keep=inside(x, 4 * 48 - 1)), "d_keep"), (dict(keep=first), "d_keep"), (dict(keep=inside(first, 15)), "d_keep"),
             (dict(counts=x), "d_counts"), (dict(counts=first), "d_counts"), (dict(counts=keep), "d_counts"),
             (dict(counts=inside(keep, 47)), "d_counts")] + GEOMETRY  # the mask is R * W BYTES: its last byte is the first of the counts
    for bad, word in cases:
        assert refused(L, call(**bad), word), (bad, L.vqvs_last_error())
    assert refused(L, call(keep=x), "overlap")
    # the limits themselves pass the checks that come before the device: the next refusal is another argument's
    assert refused(L, call(frame=4096, thr=1 << 30, min_frames=1 << 20, guard=1 << 20, keep=None), "d_keep")
    assert refused(L, call(frame=4, thr=0, min_frames=1, guard=0, keep=None), "d_keep")


def test_windows_kept_refuses_bad_arguments_without_a_device(lib_built):
    L = lib_built
    hold, (keep, out, first) = host_buffers(3)
    ok = dict(keep=keep, out=out, first=first, R=3, W=16, H=12)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_windows_kept(a["keep"], a["out"], a["first"], a["R"], a["W"], a["H"], None)

    cases = [(dict(keep=None), "d_keep"), (dict(out=None), "d_out"), (dict(out=keep), "d_out"), (dict(out=inside(keep, 47)), "d_out"),
             (dict(out=first), "d_out"), (dict(out=inside(first, 15)), "d_out")] + GEOMETRY
    for bad, word in cases:
        assert refused(L, call(**bad), word), (bad, L.vqvs_last_error())


# ---------------------------------------------------------------- 2. the threshold and the definition
def test_threshold_energy():
    assert [pauses.threshold_energy(db) for db in (-40, -50, -60)] == [107374, 10737, 1073]
    assert pauses.threshold_energy(0) == 1 << 30 and pauses.threshold_energy(-1000) == 0
    for bad in (0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            pauses.threshold_energy(bad)


def test_run_form_equals_scan_form():
    rng = np.random.default_rng(20)
    seen_trim = seen_short = 0
    for case in range(2000):
        F = int(rng.integers(1, 60))
        quiet = rng.random(F) < rng.choice([0.3, 0.6, 0.9])
        min_frames, guard = int(rng.integers(1, 8)), int(rng.integers(0, 5))
        runs, pauses_found = pause_ref.kept_frames_runs(quiet, min_frames, guard)
        assert np.array_equal(runs, pause_ref.kept_frames_scan(quiet, min_frames, guard)), (case, quiet, min_frames, guard)
        assert not runs[~quiet].any()
        seen_trim += bool((quiet & ~runs).any() and runs.any())
        seen_short += pauses_found > 0 and not runs.any()
    assert seen_trim > 100 and seen_short > 10  # trimmed pauses, and pauses no longer than their guards, both occur
    # by hand: min 3, guard 1
    q = np.array([1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1], bool)
    kept, found = pause_ref.kept_frames_runs(q, 3, 1)
    assert found == 3 and kept.astype(int).tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1]


def test_reference_quantiser_and_frames():
    x = np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, float("nan"), 2.0, -2.0, float("inf"), 0.99999, 1 / 32768], np.float32)
    assert pause_ref.quantise(x).tolist() == [0, 2, 2, 0, 0, 32767, -32768, 32767, 32767, 1]  # ties to even, NaN -> 0, saturation
    row = np.zeros(20, np.float32)
    row[0:8] = 2 / 32768          # E = 32 = thr * c: quiet
    row[8:16] = 2 / 32768
    row[15] = np.float32(np.sqrt(5.0)) / 32768  # rint -> 2: still quiet ...
    row[16:20] = [2 / 32768, 2 / 32768, 2 / 32768, 3 / 32768]  # the partial tail frame, c = 4: E = 21 = thr * c + 5: loud
    assert pause_ref.quiet_frames(row, 8, 4).tolist() == [True, True, False]
    row[7] = 3 / 32768            # E = 37 = thr * c + 5
    assert pause_ref.quiet_frames(row, 8, 4).tolist() == [False, True, False]
    # a pack of 2 + 1 windows of 16 every 12: windows 0..15 and 12..27 of recording 0, 28..43 of recording 1
    keep = np.ones(44, np.uint8)
    assert pause_ref.windows_kept(keep, (2, 1), 16, 12).tolist() == [1, 1, 1]
    keep[27] = 0  # the last sample of recording 0 is not in recording 1's window
    assert pause_ref.windows_kept(keep, (2, 1), 16, 12).tolist() == [1, 0, 1]
    keep[27], keep[28] = 255, 0
    assert pause_ref.windows_kept(keep, (2, 1), 16, 12).tolist() == [1, 1, 0]
    keep[12] = 0  # an overlap sample: both windows that cover it
    assert pause_ref.windows_kept(keep, (2, 1), 16, 12).tolist() == [0, 0, 0]


# ---------------------------------------------------------------- 3. the scripts' flags and final line
def test_convert_dataset_pause_flags(capsys):
    sys.path.insert(0, ROOT)
    import convert_dataset
    from vq_voice_swap_amd.corpus import pause_settings, skip_kept

    base = ["m.pt", "data", "out", "--label", "7"]
    plain = convert_dataset.parse_args(base)
    assert not any(hasattr(plain, k) for k in ("strength", "keep_pauses", "min_pause", "pause_guard", "no_skip_kept"))
    assert pause_settings(plain, 16000) is None and skip_kept(plain) and not convert_dataset.keeps_source(plain)
    a = convert_dataset.parse_args(base + ["--keep-pauses", "-50", "--strength", "0.6"])
    assert (a.keep_pauses, a.strength) == (-50.0, 0.6) and convert_dataset.keeps_source(a) and skip_kept(a)
    assert pause_settings(a, 16000) == dict(threshold_db=-50.0, frame=160, min_pause_frames=30, guard_frames=5)
    a = convert_dataset.parse_args(base + ["--keep-pauses", "-40", "--min-pause", "0.5", "--pause-guard", "0", "--no-skip-kept"])
    assert pause_settings(a, 16000) == dict(threshold_db=-40.0, frame=160, min_pause_frames=50, guard_frames=0) and not skip_kept(a)
    for bad in (["--keep-pauses", "-50", "--encoding", "ulaw"], ["--keep-pauses", "3"], ["--keep-pauses", "nan"], ["--min-pause", "0.5"],
                ["--pause-guard", "0.1"], ["--keep-pauses", "-50", "--min-pause", "0"], ["--keep-pauses", "-50", "--pause-guard", "-1"],
                ["--strength", "0"], ["--strength", "1.5"], ["--keep-pauses", "loud"]):
        with pytest.raises(SystemExit):
            convert_dataset.parse_args(base + bad)
    capsys.readouterr()
    assert convert_dataset.parse_args(base + ["--strength", "0.5", "--encoding", "ulaw"]).strength == 0.5  # (ulaw refuses the detector alone)
    # the final line: unchanged without the flags, byte for byte; with them it says what was kept and skipped
    totals = np.array([4, 1, 160000, 11, 2, 48000, 3], np.int64)
    old = "4 files written, 1 skipped: 10.0 s of audio, 11 windows, 2 packs in 1.5 s"
    assert convert_dataset.summary(plain, totals, 1.5) == old
    assert convert_dataset.summary(a, totals, 1.5) == old + ", kept 3.0 s, skipped 3 of 11 windows"
    assert convert_dataset.summary(convert_dataset.parse_args(base + ["--strength", "0.5"]), totals, 1.5).endswith("skipped 3 of 11 windows")


def test_sample_scripts_pause_flags():
    sys.path.insert(0, ROOT)
    import sample_vqvae
    import sample_vqvae_uncond
    from vq_voice_swap_amd.corpus import pause_settings, skip_kept

    for script, base in ((sample_vqvae, ["--label", "1", "--input-file", "in.wav", "ck.pt", "out.wav"]),
                         (sample_vqvae_uncond, ["--label", "1", "--input-file", "in.wav", "ck.pt", "out.wav"])):
        plain = script.parse_args(base)
        assert not hasattr(plain, "keep_pauses") and pause_settings(plain, 16000) is None
        for extra in ([], ["--whole-file"]):
            a = script.parse_args(base + extra + ["--keep-pauses", "-45", "--min-pause", "0.2", "--pause-guard", "0.03", "--keep", "1:2"])
            assert pause_settings(a, 16000) == dict(threshold_db=-45.0, frame=160, min_pause_frames=20, guard_frames=3) and skip_kept(a)
            assert a.keep == [(1.0, 2.0)]
        for bad in (["--keep-pauses", "-45", "--encoding", "ulaw"], ["--min-pause", "0.2"], ["--keep-pauses", "1"]):
            with pytest.raises(SystemExit):
                script.parse_args(base + bad)
    with pytest.raises(SystemExit):
        sample_vqvae.parse_args(["--sampler", "ddim", "--source-label", "0", "--keep-pauses", "-45", "--label", "1", "--input-file", "in.wav", "c", "o"])


# ---------------------------------------------------------------- 4. the keywords of the window loops, on CPU tensors
def never(*a, **kw):
    raise AssertionError("the run must be refused before the predictor is called")


@pytest.mark.parametrize("method", METHODS)
def test_skip_is_refused_unless_every_skipped_window_is_kept_whole(method):
    sample = getattr(Diffusion(make_schedule("exp")), method)
    W, H, counts = 16, 12, (2, 1)
    _, offsets, total = plan_pack([28, 16], W, H)
    assert (offsets, total) == ([0, 28], 44)
    x = torch.zeros(1, 1, total)
    keep = torch.zeros(1, 1, total, dtype=torch.uint8)
    keep[..., 12:44] = 1  # windows 1 (12..27) and 2 (28..43) whole; window 0 only in its overlap with window 1
    pack = dict(window=W, hop=H, counts=counts, pack_source=x)
    for skip in ([1, 0, 0], [1, 1, 1], [0, 1, 1, 0], [0, 1]):
        with pytest.raises(ValueError, match="skip"):
            sample(x, never, 4, pack_keep=keep, skip=torch.tensor(skip, dtype=torch.uint8), **pack)
    cut = keep.clone()
    cut[..., 27] = 0  # one sample short
    for bad in (dict(pack_keep=cut), dict(pack_keep=None), dict(pack_keep=keep.bool()[..., :-4])):
        with pytest.raises(ValueError, match="skip"):
            sample(x, never, 4, skip=torch.tensor([False, True, True]), **dict(pack, **bad))
    with pytest.raises(ValueError, match="skip"):
        sample(x, never, 4, pack_keep=keep, skip=torch.tensor([0.0, 1.0, 1.0]), **pack)
    # one recording: the same rule on source= / keep=
    Np = 2 * H + W
    x1, keep1 = torch.zeros(1, 1, Np), torch.zeros(1, 1, Np, dtype=torch.bool)
    keep1[..., 12:28] = True
    for skip, mask in (([1, 0, 0], keep1), ([0, 1, 0], None), ([0, 0, 1], keep1)):
        with pytest.raises(ValueError, match="skip"):
            sample(x1, never, 4, window=W, hop=H, source=x1, keep=mask, skip=torch.tensor(skip, dtype=torch.bool))
    # a valid list passes the checks and the run gets as far as the device check (CPU tensors are refused there)
    with pytest.raises(_native.NativeError):
        sample(x, never, 4, pack_keep=keep, skip=torch.tensor([0, 1, 1], dtype=torch.uint8), **pack)
    with pytest.raises(_native.NativeError):
        sample(x1, never, 4, window=W, hop=H, source=x1, keep=keep1, skip=torch.tensor([False, True, False]))


@pytest.mark.parametrize("method", METHODS)
def test_old_and_new_keywords_keep_to_their_layouts(method):
    sample = getattr(Diffusion(make_schedule("exp")), method)
    W, H, counts = 16, 12, (2, 1)
    _, _, total = plan_pack([28, 16], W, H)
    x, ones = torch.zeros(1, 1, total), torch.ones(1, 1, total, dtype=torch.bool)
    for bad in (dict(source=x), dict(source=x, keep=ones), dict(keep=ones), dict(source=x, start_step=1), dict(start_step=1)):
        with pytest.raises(ValueError, match="pack_source"):  # the message names the keywords a pack takes
            sample(x, never, 4, window=W, hop=H, counts=counts, **bad)
    x1 = torch.zeros(1, 1, 2 * H + W)
    for bad in (dict(pack_source=x1), dict(pack_keep=torch.ones_like(x1, dtype=torch.bool)), dict(pack_start_step=1)):
        with pytest.raises(ValueError, match="counts"):
            sample(x1, never, 4, window=W, hop=H, **bad)
    # the pack's keywords go through the checks of source / keep / start_step
    for bad in (dict(pack_keep=ones), dict(pack_start_step=2), dict(pack_source=x, pack_start_step=4), dict(pack_source=x[..., :-4]),
                dict(pack_source=x, pack_keep=ones.float())):
        with pytest.raises(ValueError):
            sample(x, never, 4, window=W, hop=H, counts=counts, **bad)


@pytest.mark.parametrize("method", METHODS)
def test_new_keywords_reach_the_layout(method, monkeypatch):
    """`pack_source` / `pack_keep` / `pack_start_step` / `skip` arrive at a stubbed `_Windows` and at `Diffusion._sample` as the source,
    mask and first step of the run."""
    d = Diffusion(make_schedule("exp"))
    W, H, counts = 16, 12, (2, 1)
    _, _, total = plan_pack([28, 16], W, H)
    x = torch.zeros(1, 1, total)
    keep = torch.zeros(1, 1, total, dtype=torch.uint8)
    keep[..., 12:44] = 1
    seen = {}

    class Stub:
        def __init__(self, *args, skip=None, counts=None):
            seen.update(counts=counts, skip=skip, window=args[3], hop=args[4])

    monkeypatch.setattr(longform, "_Windows", Stub)
    monkeypatch.setattr(d, "_sample", lambda what, layout, x_T, steps, **kw: seen.update(what=what, layout=layout, **kw))
    getattr(d, method)(x, never, 4, window=W, hop=H, counts=counts, pack_source=x, pack_keep=keep, pack_start_step=2,
                       skip=torch.tensor([0, 1, 1], dtype=torch.uint8), seed=3)
    assert seen["what"] == method and isinstance(seen["layout"], Stub) and seen["counts"] == counts and (seen["window"], seen["hop"]) == (W, H)
    assert seen["source"] is x and seen["keep"] is keep and seen["start_step"] == 2 and seen["seed"] == 3
    assert seen["skip"].dtype == torch.bool and seen["skip"].tolist() == [False, True, True]


def test_predict_walks_the_active_windows(monkeypatch):
    """`_Windows.predict` under a skip list, on CPU tensors: slices of `window_batch` ACTIVE windows, gathered, with `first=idx[0]` and
    `rows=idx` for the predictor and cond_fn, eps and grad scattered back and the skipped rows zero; without a skip list `first=` alone."""
    monkeypatch.setattr(_native, "require_cuda", lambda *tensors: None)
    monkeypatch.setattr(_native, "_stream_ptr", lambda: 0)
    n, W, H = 6, 8, 4
    calls = []

    def predictor(xw, ts, **kw):
        calls.append(("pred", xw.clone(), dict(kw)))
        return xw + 1

    def cond_fn(xw, ts, **kw):
        calls.append(("cond", xw.clone(), dict(kw)))
        return xw * 2

    rule = type("Rule", (), dict(name="ddim", flags=0))()
    windows = torch.arange(n * W, dtype=torch.float32).view(n, 1, W)
    tables = [torch.zeros(3, 2)] * 4
    for skip, want in ((torch.tensor([True, False, False, True, False, True]), [[1, 2], [4]]), (None, None)):
        del calls[:]
        layout = longform._Windows(rule, predictor, cond_fn, W, H, 2, longform._ddim_fill, None, skip=skip)
        layout.n, layout.mb = n, 2
        layout.plan_skip(torch.device("cpu"))
        layout.gather = lambda x, *a, **kw: (x, windows.clone())
        layout.start(torch.zeros(1, 1, (n - 1) * H + W), None, None, None)
        layout.predict(None, tables, 1)
        preds, conds = [c for c in calls if c[0] == "pred"], [c for c in calls if c[0] == "cond"]
        if want is None:
            assert [c[2] for c in preds] == [dict(first=0), dict(first=2), dict(first=4)] == [c[2] for c in conds]
            assert torch.equal(layout.eps, windows + 1) and torch.equal(layout.grad, windows * 2)
            continue
        assert [(c[2]["first"], c[2]["rows"].tolist()) for c in preds] == [(w[0], w) for w in want] == [(c[2]["first"], c[2]["rows"].tolist()) for c in conds]
        for c, w in zip(preds, want):
            assert torch.equal(c[1], windows[w])
        active = [i for w in want for i in w]
        assert torch.equal(layout.eps[active], windows[active] + 1) and torch.equal(layout.grad[active], windows[active] * 2)
        rest = [i for i in range(n) if i not in active]
        assert not layout.eps[rest].any() and not layout.grad[rest].any()
        first_rows = [c[2]["rows"] for c in preds]
        del calls[:]
        layout.predict(None, tables, 2)  # the same index tensors at every step: a callee may key a cache by them
        assert all(a is b for a, b in zip(first_rows, [c[2]["rows"] for c in calls if c[0] == "pred"]))
