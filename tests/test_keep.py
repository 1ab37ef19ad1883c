"""Keeping regions of a recording, host side: exports, declarations and argument checks of `vqvs_keep_region` /
`vqvs_keep_region_windows`; the `--keep` range parser and the `--strength` table; `decode_long`'s padding of source and mask; the
keyword combinations the samplers refuse; the float64 reference tests/keep_ref.py against itself (none of this needs a device)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import keep_ref
import philox_ref
import vq_voice_swap_amd
from vq_voice_swap_amd import _native, plan_windows
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SINGLE_ARGS = ["float* d_x", "const float* d_x0", "const uint8_t* d_keep", "const float* d_noise", "const float* d_alpha", "int B", "int T",
               "float noise_scale", "uint64_t seed", "uint64_t clip_offset", "uint32_t index", "void* stream"]
WINDOWS_ARGS = ["float* d_x", "float* d_windows", "const float* d_x0", "const uint8_t* d_keep", "const float* d_noise", "const float* d_alpha",
                "int n", "int W", "int H", "float noise_scale", "uint64_t seed", "uint64_t clip", "uint32_t index", "void* stream"]


# ---------------------------------------------------------------- 1. exports, declarations, refusals
def test_symbols_are_exported_and_declared(lib_built):
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    for name, want in (("vqvs_keep_region", SINGLE_ARGS), ("vqvs_keep_region_windows", WINDOWS_ARGS)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl, f"include/vqvs.h does not declare {name}"
        assert [a.strip() for a in " ".join(decl.group(1).split()).split(",")] == want
        assert len(getattr(lib_built, name).argtypes) == len(want)
    philox = open(os.path.join(ROOT, "vq_voice_swap_amd", "csrc", "philox.hpp")).read()
    assert re.search(r"PHILOX_STREAM_KEEP = 3u", philox)
    assert _native.STREAM_KEEP == keep_ref.STREAM_KEEP == 3
    assert (_native.STREAM_STEP, _native.STREAM_XT, _native.STREAM_LOSS) == (philox_ref.STREAM_STEP, philox_ref.STREAM_XT, philox_ref.STREAM_LOSS)
    assert callable(vq_voice_swap_amd.Diffusion.keep_region)


def host_buffers(count, floats=256):
    bufs = [(C.c_float * floats)() for _ in range(count)]
    return bufs, [C.cast(b, C.c_void_p) for b in bufs]


def refused(L, rc, *words):
    """VQVS_ERR_ARG, and the message names every one of `words`."""
    msg = L.vqvs_last_error() or b""
    return rc == -1 and all(w.encode() in msg for w in words)


def test_single_form_refuses_bad_arguments_without_a_device(lib_built):
    """Every refusal of include/vqvs.h: VQVS_ERR_ARG with host-only pointers, which a call that reached the device would fault on;
    the message names the argument."""
    L = lib_built
    hold, (x, x0, keep, noise, alpha) = host_buffers(5)
    ok = dict(x=x, x0=x0, keep=keep, noise=noise, alpha=alpha, B=2, T=16, scale=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_keep_region(a["x"], a["x0"], a["keep"], a["noise"], a["alpha"], a["B"], a["T"], a["scale"], 1, 2, 3, None)

    def inside(p, nbytes):
        return C.c_void_p(p.value + nbytes)

    cases = [(dict(x=None), "d_x "), (dict(x0=None), "d_x0"), (dict(alpha=None), "d_alpha"),
             (dict(B=0), "B="), (dict(B=-1), "B="), (dict(B=65536), "B="), (dict(T=0), "T="), (dict(T=-4), "T="), (dict(T=(1 << 30) + 1), "T="),
             (dict(scale=float("nan")), "noise_scale"), (dict(scale=float("inf")), "noise_scale"), (dict(scale=-float("inf")), "noise_scale"),
             (dict(x0=x), "d_x0"), (dict(keep=x), "d_keep"), (dict(noise=x), "d_noise"),
             (dict(x0=inside(x, 16)), "d_x0"),             # partial overlaps, from either side
             (dict(x=inside(x0, 4 * 31)), "d_x0"),         # the last sample of x0 is the first of x
             (dict(keep=inside(x, 4 * 32 - 1)), "d_keep"),  # the mask is B * T BYTES: its first byte is the last of x
             (dict(noise=inside(x, 100)), "d_noise"),
             (dict(keep=None, noise=None, x=None), "d_x ")]  # the optional arguments do not switch the checks off
    for bad, word in cases:
        assert refused(L, call(**bad), word), (bad, L.vqvs_last_error())
    assert refused(L, call(x0=x), "overlap")


def test_windows_form_refuses_bad_arguments_without_a_device(lib_built):
    """The rules above and every limit of `vqvs_ddpm_step_windows` on (n, W, H) (tests/test_longform.py)."""
    L = lib_built
    hold, (x, win, x0, keep, noise, alpha) = host_buffers(6)
    ok = dict(x=x, win=win, x0=x0, keep=keep, noise=noise, alpha=alpha, n=3, W=16, H=12, scale=1.0)  # Np = 40, n * W = 48

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_keep_region_windows(a["x"], a["win"], a["x0"], a["keep"], a["noise"], a["alpha"], a["n"], a["W"], a["H"], a["scale"],
                                          1, 2, 3, None)

    def inside(p, nbytes):
        return C.c_void_p(p.value + nbytes)

    cases = [(dict(x=None), "d_x "), (dict(x0=None), "d_x0"), (dict(alpha=None), "d_alpha"),
             (dict(n=0), "n="), (dict(n=-1), "n="), (dict(n=65536), "65535"),
             (dict(W=18, H=12), "W="), (dict(W=16, H=10), "H="), (dict(W=0, H=0), "W="), (dict(W=16, H=0), "H="), (dict(W=-16, H=-12), "W="),
             (dict(W=16, H=-4), "H="), (dict(W=12, H=16), "overlap"), (dict(W=28, H=12), "overlap"),
             (dict(n=65535, W=65536, H=32768), "2^31"), (dict(n=40000, W=1 << 20, H=1 << 19), "2^31"),
             (dict(scale=float("nan")), "noise_scale"), (dict(scale=float("inf")), "noise_scale"),
             (dict(x0=x), "d_x0"), (dict(keep=x), "d_keep"), (dict(noise=x), "d_noise"), (dict(noise=inside(x, 4 * 39)), "d_noise"),
             (dict(win=x), "d_windows"), (dict(win=x0), "d_windows"), (dict(win=keep), "d_windows"), (dict(win=noise), "d_windows"),
             (dict(win=alpha), "d_windows"), (dict(win=inside(x, 4 * 39)), "d_windows"),
             (dict(x=inside(win, 4 * 47)), "d_windows"),  # the windows hold n * W = 48 samples, more than the state's 40
             (dict(win=None, keep=None, noise=None, x0=None), "d_x0")]
    for bad, word in cases:
        assert refused(L, call(**bad), word), (bad, L.vqvs_last_error())
    assert refused(L, call(win=x), "overlap")
    assert refused(L, call(x=None), "non-NULL")


# ---------------------------------------------------------------- 2. --keep and --strength
def test_keep_ranges_parse():
    from vq_voice_swap_amd.audio import keep_mask, keep_sample_ranges, parse_keep_range

    assert parse_keep_range("1.5:2") == (1.5, 2.0)
    assert parse_keep_range(":0.5") == (None, 0.5)
    assert parse_keep_range("3:") == (3.0, None)
    assert parse_keep_range(" 0 : 1e-1 ") == (0.0, 0.1)
    for bad in ("2:1.5", "1:1", "-1:2", "1:-2", ":-0.5", "1", "1:2:3", "a:b", "", "nan:1", "0:inf"):
        with pytest.raises(ValueError):
            parse_keep_range(bad)
    rate, N = 16000, 64000
    assert keep_sample_ranges([(1.5, 2.0)], N, rate) == [(24000, 32000)]
    assert keep_sample_ranges([(None, 0.5)], N, rate) == [(0, 8000)]
    assert keep_sample_ranges([(3.0, None)], N, rate) == [(48000, 64000)]
    # overlapping and touching ranges merge, in any order; disjoint ones stay apart
    assert keep_sample_ranges([(2.0, 3.0), (0.5, 1.0), (2.5, 3.5), (1.0, 1.25)], N, rate) == [(8000, 20000), (32000, 56000)]
    # indices are round(seconds * rate) -- not a floor, not a ceiling
    for sec in (0.00004, 0.00007, 1.23456789, 0.1 + 0.2, 2.99997):
        assert keep_sample_ranges([(sec, None)], N, rate) == [(round(sec * rate), N)], sec
        assert keep_sample_ranges([(None, sec)], N, rate) == ([(0, round(sec * rate))] if round(sec * rate) else []), sec
    # a file shorter than END, or than START: clipped, and an empty range is dropped
    assert keep_sample_ranges([(3.0, 10.0)], N, rate) == [(48000, 64000)]
    assert keep_sample_ranges([(5.0, 10.0)], N, rate) == []
    mask = keep_mask([(0.5, 0.75), (3.9, 12.0)], N, rate)
    assert mask.dtype == bool and mask.shape == (N,)
    want = np.zeros(N, dtype=bool)
    want[8000:12000] = True
    want[62400:] = True
    assert np.array_equal(mask, want)
    assert not keep_mask([], N, rate).any() and keep_mask([(None, None)], N, rate).all()


def test_sample_vqvae_flags():
    sys.path.insert(0, ROOT)
    import sample_vqvae

    base = ["--label", "1", "--input-file", "in.wav", "ck.pt", "out.wav"]
    args = sample_vqvae.parse_args(base)
    assert args.keep == [] and args.strength == 1.0
    args = sample_vqvae.parse_args(["--keep", "1.5:2", "--keep", ":0.5", "--strength", "0.5", "--whole-file", "--sampler", "ddim"] + base)
    assert args.keep == [(1.5, 2.0), (None, 0.5)] and args.strength == 0.5
    for bad in (["--keep", "2:1"], ["--keep", "-1:2"], ["--strength", "0"], ["--strength", "1.5"], ["--strength", "-0.1"],
                ["--sampler", "ddim", "--source-label", "0", "--keep", "0:1"]):
        with pytest.raises(SystemExit):
            sample_vqvae.parse_args(bad + base)


def test_strength_table():
    from vq_voice_swap_amd.diffusion import strength_to_start_step

    want = {(1, 1): 0, (2, 1): 0, (10, 1): 0, (50, 1): 0,
            (1, 0.5): 0, (2, 0.5): 1, (10, 0.5): 5, (50, 0.5): 25,
            (1, 0.01): 0, (2, 0.01): 1, (10, 0.01): 9, (50, 0.01): 49}
    for (steps, strength), start in want.items():
        got = strength_to_start_step(strength, steps)
        assert got == start and 0 <= got <= steps - 1, (steps, strength, got)
    for bad in (0, -0.5, 1.0001, 2, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            strength_to_start_step(bad, 10)


def test_decode_long_padding_agrees_with_plan_windows():
    from vq_voice_swap_amd.longform import pad_source_keep

    for N, W, H in ((5000, 2048, 1536), (2048, 2048, 1536), (100, 2048, 1536), (7000, 1024, 1024)):
        n, padded = plan_windows(N, W, H)
        source = torch.arange(1, N + 1, dtype=torch.float32).view(1, 1, N)
        for keep in (torch.ones(1, 1, N, dtype=torch.bool), torch.ones(1, 1, N, dtype=torch.uint8), None):
            s, k = pad_source_keep(source, keep, N, padded)
            assert s.shape == (1, 1, padded) == (1, 1, (n - 1) * H + W)
            assert torch.equal(s[..., :N], source) and not s[..., N:].any()  # zeros: what encode_long pads the encoder's input with
            if keep is None:
                assert k is None
            else:
                assert k.shape == (1, 1, padded) and k.dtype == torch.uint8
                assert k[..., :N].all() and not k[..., N:].any()  # the padding is never kept
        for bad in (dict(source=source[..., :-1]), dict(keep=torch.ones(1, 1, N + 1, dtype=torch.bool)), dict(keep=torch.ones(1, 1, N))):
            kw = dict(dict(source=source, keep=None), **bad)
            with pytest.raises(ValueError):
                pad_source_keep(kw["source"], kw["keep"], N, padded)


# ---------------------------------------------------------------- 3. refused keyword combinations
def test_samplers_refuse_bad_keyword_combinations():
    """ValueError before anything touches a device (the tensors here are CPU tensors, which the loops refuse only afterwards)."""
    d = Diffusion(make_schedule("exp"))
    W, H, n = 16, 12, 3
    Np = (n - 1) * H + W

    def predictor(x, ts, **kw):
        raise AssertionError("the predictor must not be reached")

    single = dict(x=torch.zeros(2, 1, 64), calls=[lambda x, **kw: d.ddpm_sample(x, predictor, 4, **kw),
                                                  lambda x, **kw: d.ddim_sample(x, predictor, 4, **kw)])
    long = dict(x=torch.zeros(1, 1, Np), calls=[lambda x, **kw: d.ddpm_sample_windows(x, predictor, 4, window=W, hop=H, **kw),
                                                lambda x, **kw: d.ddim_sample_windows(x, predictor, 4, window=W, hop=H, **kw)])
    for group in (single, long):
        x = group["x"]
        src, keep = torch.zeros_like(x), torch.zeros_like(x, dtype=torch.bool)
        bad = [dict(keep=keep),                                    # a mask without a source
               dict(start_step=2),                                 # a late start without a source
               dict(source=src, start_step=4), dict(source=src, start_step=-1), dict(source=src, start_step=100),
               dict(source=src, start_step=1.5),
               dict(source=src[..., :-4], keep=keep), dict(source=src, keep=keep[..., :-4]), dict(source=src.squeeze(1)),
               dict(source=src, keep=keep.squeeze(1)), dict(source=src, keep=keep.float())]
        for call in group["calls"]:
            for kw in bad:
                with pytest.raises(ValueError):
                    call(x, **kw)
            with pytest.raises(_native.NativeError):  # a well-formed call gets as far as the device check
                call(x, source=src, keep=keep, start_step=3)
    with pytest.raises(ValueError):
        d.keep_region(torch.zeros(2, 1, 64), torch.zeros(2, 1, 60), 0.5, seed=0, index=0)
    with pytest.raises(ValueError):
        d.keep_region(torch.zeros(2, 1, 64), torch.zeros(2, 1, 64), 0.5, torch.zeros(2, 1, 60, dtype=torch.bool), seed=0, index=0)


def test_decode_refuses_bad_keyword_combinations(lib_built):
    from vq_voice_swap_amd import VQVAE
    from vq_voice_swap_amd.longform import decode_long

    model = VQVAE(base_channels=32, pred_name="unet", num_labels=3)
    codes = torch.zeros(1, 8, dtype=torch.int64)
    wave, mask = torch.zeros(1, 1, 2048), torch.zeros(1, 1, 2048, dtype=torch.bool)
    for kw in (dict(keep=mask), dict(strength=0.5), dict(source=wave, strength=0.0), dict(source=wave, strength=1.5),
               dict(source=wave, strength=-1.0)):
        with pytest.raises(ValueError):
            model.decode(codes, steps=4, **kw)
        with pytest.raises(ValueError):
            model.decode_long(codes, num_samples=2048, window=2048, hop=1536, steps=4, **kw)
        with pytest.raises(ValueError):
            decode_long(model, codes, num_samples=2048, window=2048, hop=1536, steps=4, **kw)


# ---------------------------------------------------------------- 4. the reference against itself
def ref_inputs(B, T, seed=0):
    rng = np.random.default_rng(seed)
    f = lambda: rng.standard_normal((B, T)).astype(np.float32)  # noqa: E731
    return f(), f(), f()


def test_reference_self_checks():
    B, T = 3, 37
    x, x0, noise = ref_inputs(B, T)
    keep = np.random.default_rng(1).integers(0, 2, (B, T)).astype(np.uint8)
    # alpha = 1: the source exactly, nothing drawn (a noise of NaN is never touched)
    for nz in (noise, None, np.full((B, T), np.nan)):
        out, _ = keep_ref.keep_region(x, x0, None, nz, [1.0] * B)
        assert np.array_equal(out, x0.astype(np.float64))
    out, _ = keep_ref.keep_region(x, x0, keep, noise, [1.0] * B)
    assert np.array_equal(out, np.where(keep != 0, x0, x).astype(np.float64))
    # an all-zero mask is the identity, whatever alpha
    for alpha in (1.0, 0.5, 0.0):
        out, _ = keep_ref.keep_region(x, x0, np.zeros((B, T), np.uint8), noise, [alpha] * B)
        assert np.array_equal(out, x.astype(np.float64))
    # alpha = 0: the noise; noise_scale = 0: ca x0; per-row alphas
    out, _ = keep_ref.keep_region(x, x0, None, noise, [0.0] * B)
    assert np.array_equal(out, noise.astype(np.float64))
    out, mag = keep_ref.keep_region(x, x0, None, noise, [0.25, 0.5, 1.0], noise_scale=0.0)
    ca = np.array([keep_ref.coefficients(a)[0] for a in (0.25, 0.5, 1.0)], dtype=np.float64)[:, None]
    assert np.array_equal(out, ca * x0) and np.array_equal(mag, np.abs(ca * x0))
    assert keep_ref.coefficients(0.25) == (np.float32(0.5), np.float32(np.sqrt(0.75)))
    # drawn noise: stream 3 of the generator at (seed, clip_offset + row, index)
    out, _ = keep_ref.keep_region(x, x0, None, None, [0.0] * B, seed=5, clip_offset=7, index=2)
    assert np.array_equal(out, philox_ref.randn(B, T, 5, 7, keep_ref.STREAM_KEEP, step=2))
    assert not np.array_equal(out, philox_ref.randn(B, T, 5, 7, philox_ref.STREAM_STEP, step=2))


@pytest.mark.parametrize("given", [True, False])
def test_reference_windows_form(given):
    # n = 1 is the single form
    W = 16
    x, x0, noise = ref_inputs(1, W, seed=2)
    keep = np.array([[1, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1]], dtype=np.uint8)
    nz = noise if given else None
    want, want_mag = keep_ref.keep_region(x, x0, keep, nz, [0.3], seed=5, clip_offset=9, index=4)
    got, win, mag = keep_ref.keep_region_windows(x[0], x.copy(), x0[0], keep[0], None if nz is None else nz[0], 0.3, 1, W, W, seed=5, clip=9, index=4)
    assert np.array_equal(got, want[0]) and np.array_equal(win, want) and np.array_equal(mag, want_mag[0])
    # n = 3 with an overlap: the long state is one row of Np samples, and every window copy of a kept sample follows it
    n, W, H = 3, 16, 12
    Np = (n - 1) * H + W
    x, x0, noise = ref_inputs(1, Np, seed=3)
    keep = (np.random.default_rng(4).random((1, Np)) < 0.6).astype(np.uint8)
    nz = noise if given else None
    windows = np.stack([x[0, b * H:b * H + W] for b in range(n)])
    want, _ = keep_ref.keep_region(x, x0, keep, nz, [0.3], seed=5, clip_offset=9, index=4)
    got, win, _ = keep_ref.keep_region_windows(x[0], windows, x0[0], keep[0], None if nz is None else nz[0], 0.3, n, W, H, seed=5, clip=9, index=4)
    assert np.array_equal(got, want[0])
    assert np.array_equal(win, np.stack([got[b * H:b * H + W] for b in range(n)]))
