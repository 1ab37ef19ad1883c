"""Keeping regions of a recording on the device: `vqvs_keep_region` / `vqvs_keep_region_windows` against the float64 reference
tests/keep_ref.py with supplied and with drawn noise, the four sampling loops with `source` / `keep` / `start_step` against loops
written here from the single-step entry points, and `sample_vqvae.py --keep / --strength` end to end.

Bound per kept sample with supplied noise: |got - ref| <= 2 * 2^-24 * (|ca x0| + |cn z|) -- one rounding for the product cn * z and
one for the fmaf; ca and cn are the reference's own float32 values.  With drawn noise the device's normal differs from the float64
reference's by at most NORMAL_ABS = 1.2e-5 (derived in tests/test_rng_gpu.py), which enters through cn: the bound grows by
cn * NORMAL_ABS.  Everything else -- samples outside the mask, alpha = 1, the windows form against the single form, the samplers
against the hand-written loops -- is compared bit for bit.

A run prints the largest fraction of each bound; on an MI355X it was 0.86 with supplied noise and 0.19 with drawn noise."""
import os
import sys

import numpy as np
import pytest
import torch

import keep_ref
from vq_voice_swap_amd import VQVAE, DiffusionModel, _native
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule
from vq_voice_swap_amd.longform import gather_windows

from util import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 4), (3, 1001), (2, 4099), (2, 1028)]  # (the last: whole aligned quads -- the 16-byte path -- in more than one block)
WINDOW_SHAPES = [(1, 16, 16), (3, 16, 12), (4, 32, 16), (3, 16, 16)]
ALPHAS = [1.0, 0.9990234375, 0.5, 2.0 ** -20, 0.0]
NORMAL_ABS = 1.2e-5  # |device normal - reference normal| (tests/test_rng_gpu.py)
EPS = 2.0 ** -24
SEED, CLIP, INDEX = (1 << 32) + 7, (1 << 32) + 5, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def single_masks(B, T):
    """name -> uint8 [B, T] or None.  Edges off the quad grid (and different in every row), the first and the last sample alone, all
    ones, all zeros, a random half, and no mask at all."""
    edges = np.zeros((B, T), np.uint8)
    for b in range(B):
        lo = 1 + b
        edges[b, lo:max(lo + 1, T - 2 - b)] = 1
    ends = np.zeros((B, T), np.uint8)
    ends[:, 0] = ends[:, -1] = 1
    half = (np.random.default_rng(B * 7919 + T).random((B, T)) < 0.5).astype(np.uint8)
    return {"edges": edges, "ends": ends, "ones": np.full((B, T), 255, np.uint8), "zeros": np.zeros((B, T), np.uint8), "half": half, "null": None}


def window_masks(n, W, H):
    """The same for one long row of Np samples, plus an edge pair INSIDE the first overlap [H, W) (or, without one, across the first
    window boundary)."""
    Np = (n - 1) * H + W
    masks = {k: (None if v is None else v[0]) for k, v in single_masks(1, Np).items()}
    inner = np.zeros(Np, np.uint8)
    if n > 1 and W > H:
        inner[H + 1:W - 1] = 1
    elif n > 1:
        inner[H - 1:H + 2] = 1
    else:
        inner[1:W - 1] = 1
    masks["overlap"] = inner
    return masks


def call_single(x, x0, keep, noise, alpha, noise_scale=1.0, seed=SEED, clip_offset=CLIP, index=INDEX):
    """`vqvs_keep_region` on a copy of x [B, T] that has a NaN row behind its last row; returns the B rows."""
    B, T = x.shape
    buf = torch.cat([x, torch.full((1, T), float("nan"), device=x.device)]).contiguous()
    _native.check(_native.lib().vqvs_keep_region(buf.data_ptr(), x0.data_ptr(), _native._ptr(keep), _native._ptr(noise), alpha.data_ptr(), B, T,
                                                 noise_scale, seed, clip_offset, index, _native._stream_ptr()))
    assert torch.isnan(buf[B]).all(), "the kernel wrote past the last row"
    return buf[:B]


def call_windows(x, windows, x0, keep, noise, alpha, n, W, H, noise_scale=1.0, seed=SEED, clip=CLIP, index=INDEX):
    """`vqvs_keep_region_windows` on copies of x [Np] and windows [n, W] (or None), each in front of a NaN guard."""
    Np = (n - 1) * H + W
    guard = torch.full((64,), float("nan"), device=x.device)
    xb = torch.cat([x, guard])
    wb = None if windows is None else torch.cat([windows.reshape(-1), guard])
    _native.check(_native.lib().vqvs_keep_region_windows(xb.data_ptr(), _native._ptr(wb), x0.data_ptr(), _native._ptr(keep), _native._ptr(noise),
                                                         alpha.data_ptr(), n, W, H, noise_scale, seed, clip, index, _native._stream_ptr()))
    assert torch.isnan(xb[Np:]).all() and (wb is None or torch.isnan(wb[n * W:]).all()), "the kernel wrote past the end of an output"
    return xb[:Np], None if wb is None else wb[:n * W].view(n, W)


def check_against_ref(got, x, x0, keep_np, want, mag, cn_extra, what):
    """Kept samples within the bound, the others bit for bit the input; returns the largest fraction of the bound."""
    kept = np.ones(want.shape, bool) if keep_np is None else keep_np != 0
    assert torch.equal(bits(got)[torch.from_numpy(~kept)], bits(x)[torch.from_numpy(~kept)]), f"{what}: a sample outside the mask changed"
    err = np.abs(got.cpu().double().numpy() - want)[kept]
    bound = (2 * EPS * mag + cn_extra)[kept]
    assert (err <= bound).all(), (what, float((err - bound).max()))
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---------------------------------------------------------------- 1. supplied noise
@pytest.mark.parametrize("B,T", SHAPES)
def test_single_form_vs_reference_supplied_noise(dev, B, T):
    x, x0, noise = (seeded((B, T), 11 + k).to(dev) for k in range(3))
    worst = 0.0
    for alpha in ALPHAS:
        a = torch.tensor([alpha] * B, dtype=torch.float32, device=dev)
        for name, m in single_masks(B, T).items():
            keep = None if m is None else torch.from_numpy(m).to(dev)
            got = call_single(x, x0, keep, noise, a)
            want, mag = keep_ref.keep_region(x.cpu().numpy(), x0.cpu().numpy(), m, noise.cpu().numpy(), [alpha] * B)
            worst = max(worst, check_against_ref(got, x, x0, m, want, mag, 0.0, f"B={B} T={T} alpha={alpha} mask={name}"))
            if alpha == 1.0:  # the source itself, bit for bit, with a noise that must not be read
                kept = torch.ones(B, T, dtype=torch.bool) if m is None else torch.from_numpy(m != 0)
                assert torch.equal(bits(got)[kept], bits(x0)[kept]), name
                poisoned = call_single(x, x0, keep, torch.full_like(noise, float("nan")), a)
                assert torch.equal(bits(poisoned), bits(got)), name
    print(f"[margin] keep_region B={B} T={T} supplied noise: {worst:.3f} of the bound")
    # per-row alphas; noise_scale 0 reads no noise either and leaves ca * x0
    alphas = [ALPHAS[(b + 1) % len(ALPHAS)] for b in range(B)]
    a = torch.tensor(alphas, dtype=torch.float32, device=dev)
    want, mag = keep_ref.keep_region(x.cpu().numpy(), x0.cpu().numpy(), None, noise.cpu().numpy(), alphas)
    check_against_ref(call_single(x, x0, None, noise, a), x, x0, None, want, mag, 0.0, "per-row alphas")
    got = call_single(x, x0, None, torch.full_like(noise, float("nan")), a, noise_scale=0.0)
    ca = torch.tensor([keep_ref.coefficients(v)[0] for v in alphas], device=dev).view(B, 1)
    assert torch.equal(bits(got), bits(ca * x0))
    # unaligned base pointers take the one-sample path: the same values
    if T % 4 == 0 and T > 4:
        shifted = [torch.cat([torch.zeros(1, device=dev), t.reshape(-1)])[1:].view(B, T) for t in (x, x0, noise)]
        assert shifted[0].data_ptr() % 16 == 4
        a5 = torch.tensor([0.5] * B, dtype=torch.float32, device=dev)
        m = torch.from_numpy(single_masks(B, T)["edges"]).to(dev)
        got = call_single(x, shifted[1], m, shifted[2], a5)
        assert torch.equal(bits(got), bits(call_single(x, x0, m, noise, a5)))


@pytest.mark.parametrize("n,W,H", WINDOW_SHAPES)
def test_windows_form_vs_reference_supplied_noise(dev, n, W, H):
    Np = (n - 1) * H + W
    x, x0, noise = (seeded((Np,), 21 + k).to(dev) for k in range(3))
    windows = gather_windows(x, W, H).view(n, W)
    worst = 0.0
    for alpha in ALPHAS:
        a = torch.tensor([alpha], dtype=torch.float32, device=dev)
        for name, m in window_masks(n, W, H).items():
            keep = None if m is None else torch.from_numpy(m).to(dev)
            got, win = call_windows(x, windows, x0, keep, noise, a, n, W, H)
            want, want_win, mag = keep_ref.keep_region_windows(x.cpu().numpy(), windows.cpu().numpy(), x0.cpu().numpy(), m, noise.cpu().numpy(),
                                                               alpha, n, W, H)
            what = f"(n, W, H)=({n}, {W}, {H}) alpha={alpha} mask={name}"
            worst = max(worst, check_against_ref(got, x, x0, m, want, mag, 0.0, what))
            # every window copy -- both copies of an overlap sample -- is the long state's value, kept or not
            assert torch.equal(bits(win), bits(gather_windows(got, W, H).view(n, W))), what
            assert np.array_equal(want_win, np.stack([want[b * H:b * H + W] for b in range(n)]))
            alone, _ = call_windows(x, None, x0, keep, noise, a, n, W, H)  # the optional output changes nothing
            assert torch.equal(bits(alone), bits(got)), what
            if alpha == 1.0:
                kept = torch.ones(Np, dtype=torch.bool) if m is None else torch.from_numpy(m != 0)
                assert torch.equal(bits(got)[kept], bits(x0)[kept]), what
            if n == 1:  # one window is the single form, bit for bit
                single = call_single(x.view(1, W), x0.view(1, W), None if keep is None else keep.view(1, W), noise.view(1, W), a)
                assert torch.equal(bits(got), bits(single.view(-1))), what
    print(f"[margin] keep_region_windows (n, W, H)=({n}, {W}, {H}) supplied noise: {worst:.3f} of the bound")


# ---------------------------------------------------------------- 2. drawn noise
@pytest.mark.parametrize("B,T", SHAPES)
def test_single_form_drawn_noise(dev, B, T):
    x, x0 = (seeded((B, T), 31 + k).to(dev) for k in range(2))
    masks = single_masks(B, T)
    worst = 0.0
    for alpha in ALPHAS:
        a = torch.tensor([alpha] * B, dtype=torch.float32, device=dev)
        cn = float(keep_ref.coefficients(alpha)[1])
        for name in ("edges", "half", "null"):
            m = masks[name]
            keep = None if m is None else torch.from_numpy(m).to(dev)
            got = call_single(x, x0, keep, None, a)
            want, mag = keep_ref.keep_region(x.cpu().numpy(), x0.cpu().numpy(), m, None, [alpha] * B, seed=SEED, clip_offset=CLIP, index=INDEX)
            worst = max(worst, check_against_ref(got, x, x0, m, want, mag, cn * NORMAL_ABS, f"drawn B={B} T={T} alpha={alpha} mask={name}"))
    print(f"[margin] keep_region B={B} T={T} drawn noise: {worst:.3f} of the bound")
    # alpha = 0 leaves the draw itself: another one for another index, not the step stream's, and a clip's own wherever it is addressed
    zero = torch.zeros(B, dtype=torch.float32, device=dev)
    draw = call_single(x, x0, None, None, zero)
    assert torch.equal(bits(draw), bits(call_single(x, x0, None, None, zero)))
    assert not torch.equal(draw, call_single(x, x0, None, None, zero, index=INDEX + 1))
    assert not torch.equal(draw, call_single(x, x0, None, None, zero, seed=SEED + 1))
    step_stream = torch.empty(B, T, device=dev)  # vqvs_randn draws any stream at step 0: stream 0 there is the step noise of step 0
    _native.check(_native.lib().vqvs_randn(step_stream.data_ptr(), B, T, SEED, CLIP, _native.STREAM_STEP, _native._stream_ptr()))
    at_zero = call_single(x, x0, None, None, zero, index=0)
    assert not torch.equal(at_zero, step_stream)
    if T >= 8:
        assert float((at_zero - step_stream).abs().max()) > 0.1
    for b in range(B):  # row b of a batch at CLIP is row 0 of a batch at CLIP + b
        alone = call_single(x[b:b + 1], x0[b:b + 1], None, None, zero[:1], clip_offset=CLIP + b)
        assert torch.equal(bits(alone), bits(draw[b:b + 1])), b


@pytest.mark.parametrize("n,W,H", WINDOW_SHAPES)
def test_windows_form_drawn_noise(dev, n, W, H):
    Np = (n - 1) * H + W
    x, x0 = (seeded((Np,), 41 + k).to(dev) for k in range(2))
    windows = gather_windows(x, W, H).view(n, W)
    worst = 0.0
    for alpha in ALPHAS:
        a = torch.tensor([alpha], dtype=torch.float32, device=dev)
        cn = float(keep_ref.coefficients(alpha)[1])
        for name, m in window_masks(n, W, H).items():
            keep = None if m is None else torch.from_numpy(m).to(dev)
            got, win = call_windows(x, windows, x0, keep, None, a, n, W, H)
            want, _, mag = keep_ref.keep_region_windows(x.cpu().numpy(), None, x0.cpu().numpy(), m, None, alpha, n, W, H, seed=SEED, clip=CLIP,
                                                        index=INDEX)
            what = f"drawn (n, W, H)=({n}, {W}, {H}) alpha={alpha} mask={name}"
            worst = max(worst, check_against_ref(got, x, x0, m, want, mag, cn * NORMAL_ABS, what))
            # one row of Np samples at clip_offset = clip, bit for bit; and both copies of every overlap sample are the long state's
            row = call_single(x.view(1, Np), x0.view(1, Np), None if keep is None else keep.view(1, Np), None, a)
            assert torch.equal(bits(got), bits(row.view(-1))), what
            assert torch.equal(bits(win), bits(gather_windows(got, W, H).view(n, W))), what
    print(f"[margin] keep_region_windows (n, W, H)=({n}, {W}, {H}) drawn noise: {worst:.3f} of the bound")


def test_python_wrapper(dev):
    d = Diffusion(make_schedule("exp"))
    B, T = 3, 1001
    x, x0 = seeded((B, 1, T), 51).to(dev), seeded((B, 1, T), 52).to(dev)
    m = torch.from_numpy(single_masks(B, T)["edges"]).view(B, 1, T).to(dev)
    a = torch.tensor([0.5, 0.25, 1.0], device=dev)
    before = x.clone()
    got = d.keep_region(x, x0, a, m, seed=SEED, clip_offset=CLIP, index=INDEX)
    assert torch.equal(x, before) and got.shape == x.shape and got.data_ptr() != x.data_ptr()  # a new tensor
    assert torch.equal(bits(got.view(B, T)), bits(call_single(x.view(B, T), x0.view(B, T), m.view(B, T), None, a)))
    assert torch.equal(got, d.keep_region(x, x0, a, m.bool(), seed=SEED, clip_offset=CLIP, index=INDEX))  # bool or uint8
    nz = seeded((B, 1, T), 53).to(dev)
    got = d.keep_region(x, x0, 0.5, noise=nz, noise_scale=0.5, seed=0, index=0)  # one alpha for every row, every sample
    want = call_single(x.view(B, T), x0.view(B, T), None, nz.view(B, T), torch.full((B,), 0.5, device=dev), noise_scale=0.5)
    assert torch.equal(bits(got.view(B, T)), bits(want))


# ---------------------------------------------------------------- 3. the samplers
def det_model(m, dev):
    det_init_(m.state_dict().items())
    m.eval()
    m.to(dev)
    m.set_precision("fp32")
    return m


@pytest.fixture(scope="module")
def unet(dev):
    return det_model(DiffusionModel("unet", 32), dev)


def ddpm_step(x, eps, a_t, a_prev, constrain, last, step, clip_offset=CLIP):
    B, T = x.shape[0], x.shape[-1]
    out = torch.empty_like(x)
    _native.check(_native.lib().vqvs_ddpm_step(x.data_ptr(), eps.data_ptr(), None, a_t.data_ptr(), a_prev.data_ptr(), out.data_ptr(), B, T,
                                               _native.DDPM_CONSTRAIN if constrain else 0, 0.0 if last else 1.0, SEED, clip_offset, step,
                                               _native._stream_ptr()))
    return out


def ddim_step(x, eps, a_t, a_to, eta, constrain, last, step, clip_offset=CLIP):
    B, T = x.shape[0], x.shape[-1]
    out = torch.empty_like(x)
    _native.check(_native.lib().vqvs_ddim_step(x.data_ptr(), eps.data_ptr(), None, None, a_t.data_ptr(), a_to.data_ptr(), out.data_ptr(), B, T,
                                               _native.DDIM_CONSTRAIN if constrain else 0, eta, 0.0 if last else 1.0, SEED, clip_offset, step,
                                               _native._stream_ptr()))
    return out


def hand_loop(d, sampler, x_T, predictor, steps, source, keep, start_step, eta=0.5, constrain=True):
    """The loop of section 2 of the issue from the single-step entry points and `Diffusion.keep_region`."""
    ts_all, a_t_all, a_to_all, _ = d.step_tables(steps, x_T.shape[0], None, x_T.device)
    kw = dict(seed=SEED, clip_offset=CLIP)
    if start_step > 0:
        x = d.keep_region(torch.full_like(x_T, float("nan")), source, a_t_all[start_step], None, index=start_step, **kw)
    else:
        x = d.keep_region(x_T, source, a_t_all[0], keep, index=0, **kw)
    for i in range(start_step, steps):
        eps = predictor(x, ts_all[i]).contiguous()
        last = i + 1 == steps
        if sampler == "ddpm":
            x = ddpm_step(x, eps, a_t_all[i], a_to_all[i], constrain, last, i)
        else:
            x = ddim_step(x, eps, a_t_all[i], a_to_all[i], eta, constrain, last, i)
        x = d.keep_region(x, source, a_to_all[i], keep, index=i + 1, **kw)
    return x


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_single_clip_samplers(dev, unet, sampler):
    B, T, steps = 2, 1024, 3
    d = unet.diffusion
    x_T, source = seeded((B, 1, T), 61).to(dev), (0.3 * seeded((B, 1, T), 62)).to(dev)
    keep = torch.zeros(B, 1, T, dtype=torch.bool, device=dev)
    keep[0, 0, 101:517] = True
    keep[1, 0, :3] = True
    keep[1, 0, 700:] = True
    kw = dict(constrain=True, seed=SEED, clip_offset=CLIP)
    if sampler == "ddim":
        kw["eta"] = 0.5
    sample = d.ddpm_sample if sampler == "ddpm" else d.ddim_sample
    plain = sample(x_T, unet.predictor, steps, **kw)
    # the defaults, spelled out, change nothing; nor does an all-zero mask, nor a source without a mask
    assert torch.equal(bits(plain), bits(sample(x_T, unet.predictor, steps, source=None, keep=None, start_step=0, **kw)))
    assert torch.equal(bits(plain), bits(sample(x_T, unet.predictor, steps, source=source, keep=torch.zeros_like(keep), **kw)))
    assert torch.equal(bits(plain), bits(sample(x_T, unet.predictor, steps, source=source, **kw)))
    # source and keep: the hand-written loop, bit for bit; the kept samples are the source's
    for mask in (keep, keep.to(torch.uint8)):
        got = sample(x_T, unet.predictor, steps, source=source, keep=mask, **kw)
        assert torch.equal(bits(got), bits(hand_loop(d, sampler, x_T, unet.predictor, steps, source, keep, 0)))
    assert torch.equal(bits(got)[keep], bits(source)[keep])
    assert not torch.equal(got[~keep], plain[~keep]) and not torch.equal(got[~keep], source[~keep])
    # a late start: from the noised source, x_T unused
    late = sample(x_T, unet.predictor, steps, source=source, keep=keep, start_step=2, **kw)
    assert torch.equal(bits(late), bits(hand_loop(d, sampler, x_T, unet.predictor, steps, source, keep, 2)))
    assert torch.equal(bits(late), bits(sample(torch.zeros_like(x_T), unet.predictor, steps, source=source, keep=keep, start_step=2, **kw)))
    assert torch.equal(bits(late)[keep], bits(source)[keep]) and not torch.equal(late, got)
    nomask = sample(x_T, unet.predictor, steps, source=source, start_step=2, **kw)
    assert torch.equal(bits(nomask), bits(hand_loop(d, sampler, x_T, unet.predictor, steps, source, torch.zeros_like(keep), 2)))


def analytic_predictor(w, ts, first=0):
    m = w.shape[0]
    return 0.5 * torch.sin(3 * w) + 0.1 * (first + torch.arange(m, device=w.device, dtype=torch.float32)).view(m, 1, 1)


def hand_loop_windows(d, sampler, x_T, steps, source, keep, start_step, n, W, H, eta=0.5):
    """The same for one long state: `vqvs_ddpm_step_windows` / `vqvs_ddim_step_windows`, then `Diffusion.keep_region` on the long row
    (the windows form draws what one row of Np samples draws) and the windows gathered again."""
    L = _native.lib()
    ts_all, a_t_all, a_to_all, _ = d.step_tables(steps, n, None, x_T.device)
    kw = dict(seed=SEED, clip_offset=CLIP)
    if start_step > 0:
        x = d.keep_region(torch.full_like(x_T, float("nan")), source, a_t_all[start_step, :1], None, index=start_step, **kw)
    else:
        x = d.keep_region(x_T, source, a_t_all[0, :1], keep, index=0, **kw)
    for i in range(start_step, steps):
        windows = gather_windows(x, W, H)
        eps = analytic_predictor(windows, ts_all[i]).contiguous()
        out = torch.empty_like(x)
        scale = 0.0 if i + 1 == steps else 1.0
        if sampler == "ddpm":
            _native.check(L.vqvs_ddpm_step_windows(x.data_ptr(), eps.data_ptr(), None, a_t_all[i].data_ptr(), a_to_all[i].data_ptr(), out.data_ptr(),
                                                   None, n, W, H, _native.DDPM_CONSTRAIN, scale, SEED, CLIP, i, _native._stream_ptr()))
        else:
            _native.check(L.vqvs_ddim_step_windows(x.data_ptr(), eps.data_ptr(), None, None, a_t_all[i].data_ptr(), a_to_all[i].data_ptr(),
                                                   out.data_ptr(), None, n, W, H, _native.DDIM_CONSTRAIN, eta, scale, SEED, CLIP, i,
                                                   _native._stream_ptr()))
        x = d.keep_region(out, source, a_to_all[i, :1], keep, index=i + 1, **kw)
    return x


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_windows_samplers(dev, sampler):
    n, W, H, steps = 3, 2048, 1536, 3
    Np = (n - 1) * H + W
    d = Diffusion(make_schedule("exp"))
    x_T, source = seeded((1, 1, Np), 71).to(dev), (0.3 * seeded((1, 1, Np), 72)).to(dev)
    keep = torch.zeros(1, 1, Np, dtype=torch.bool, device=dev)
    keep[..., :5] = True
    keep[..., 1000:1801] = True  # ends inside the first overlap [1536, 2048)
    keep[..., 3073:] = True      # from the second overlap's second sample to the end
    kw = dict(window=W, hop=H, constrain=True, seed=SEED, clip_offset=CLIP)
    if sampler == "ddim":
        kw["eta"] = 0.5
    sample = d.ddpm_sample_windows if sampler == "ddpm" else d.ddim_sample_windows
    plain = sample(x_T, analytic_predictor, steps, **kw)
    assert torch.equal(bits(plain), bits(sample(x_T, analytic_predictor, steps, source=None, keep=None, start_step=0, **kw)))
    assert torch.equal(bits(plain), bits(sample(x_T, analytic_predictor, steps, source=source, keep=torch.zeros_like(keep), **kw)))
    seen = []

    def recording(w, ts, first):
        seen.append(w.clone())
        return analytic_predictor(w, ts, first)

    got = sample(x_T, recording, steps, source=source, keep=keep, **kw)
    assert torch.equal(bits(got), bits(hand_loop_windows(d, sampler, x_T, steps, source, keep, 0, n, W, H)))
    assert torch.equal(bits(got)[keep], bits(source)[keep]) and not torch.equal(got[~keep], plain[~keep])
    for w in seen:  # the windows the predictor saw agree on the samples they share, kept or not
        assert torch.equal(w[:-1, 0, H:], w[1:, 0, :W - H])
    assert torch.equal(bits(got), bits(sample(x_T, analytic_predictor, steps, source=source, keep=keep, window_batch=1, **kw)))
    late = sample(x_T, analytic_predictor, steps, source=source, keep=keep, start_step=2, **kw)
    assert torch.equal(bits(late), bits(hand_loop_windows(d, sampler, x_T, steps, source, keep, 2, n, W, H)))
    assert torch.equal(bits(late)[keep], bits(source)[keep]) and not torch.equal(late, got)


# ---------------------------------------------------------------- 4. VQVAE and the script
@pytest.fixture(scope="module")
def vqvae(dev):
    return det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=3), dev)


def test_vqvae_decode_and_decode_long(dev, vqvae):
    N, W, H, steps = 5000, 2048, 1536, 3
    wave = (0.3 * seeded((1, 1, N), 81)).clamp(-1, 1).to(dev)
    label = torch.tensor([1], device=dev)
    keep = torch.zeros(1, 1, N, dtype=torch.bool, device=dev)
    keep[..., 1700:3100] = True
    codes = vqvae.encode_long(wave, W, H)
    kw = dict(num_samples=N, window=W, hop=H, steps=steps, constrain=True, seed=9, clip_offset=5)
    plain = vqvae.decode_long(codes, label, **kw)
    got = vqvae.decode_long(codes, label, source=wave, keep=keep, **kw)
    assert got.shape == (1, 1, N) and torch.equal(bits(got)[keep], bits(wave)[keep]) and not torch.equal(got[~keep], plain[~keep])
    assert torch.equal(plain, vqvae.decode_long(codes, label, source=wave, strength=1.0, **kw))
    soft = vqvae.decode_long(codes, label, source=wave, keep=keep, strength=0.5, sampler="ddim", **kw)
    assert torch.equal(bits(soft)[keep], bits(wave)[keep]) and not torch.equal(soft, got)
    # one window: decode_long is decode, with the new keywords too
    one, m1 = wave[..., :W].contiguous(), keep[..., :W].contiguous()
    c1 = vqvae.encode(one)
    for extra in (dict(keep=m1), dict(keep=m1, strength=0.5), dict(strength=0.5, sampler="ddim", eta=0.5)):
        a = vqvae.decode(c1, label, steps=steps, constrain=True, seed=9, clip_offset=5, source=one, **extra)
        b = vqvae.decode_long(c1, label, **dict(kw, num_samples=W), source=one, **extra)
        assert torch.equal(bits(a), bits(b)), extra
        if "keep" in extra:
            assert torch.equal(bits(a)[m1], bits(one)[m1])


def read_s16(path):
    import wave

    with wave.open(path, "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


@pytest.mark.parametrize("whole_file", [False, True])
def test_sample_vqvae_keep_and_strength(dev, vqvae, tmp_path, whole_file):
    """The kept range of the written WAV is the input on the writer's s16 grid -- the input's samples as ChunkReader hands them
    to the model, s16 / 2^15, written by ChunkWriter's own quantisation (* (2^15 - 1), truncated) -- and the rest is not."""
    sys.path.insert(0, ROOT)
    import sample_vqvae

    ck, src, echo = (str(tmp_path / name) for name in ("v.pt", "in.wav", "echo.wav"))
    vqvae.save(ck)
    rate = 16000
    N = 8000 if whole_file else rate  # 0.5 s in windows of 0.128 s; or the first --seconds 1
    w = ChunkWriter(src, rate)
    w.write(0.3 * np.sin(np.arange(N) * 0.05).astype(np.float32))
    w.close()
    r = ChunkReader(src, rate)
    samples = r.read(N)
    r.close()
    w = ChunkWriter(echo, rate)
    w.write(samples)
    w.close()
    want = read_s16(echo)
    a, b = round(0.1 * rate), round(0.25 * rate)
    common = ["--label", "2", "--input-file", src, "--sample-steps", "3", "--seed", "9"]
    common += ["--whole-file", "--window-seconds", "0.128", "--overlap-seconds", "0.032", "--window-batch", "2"] if whole_file else ["--seconds", "1"]
    outs = {}
    usable = N if whole_file else N // 256 * 256  # a single clip is cut to a multiple of the model's rate
    want = want[:usable]
    for name, flags in (("keep", ["--keep", "0.1:0.2", "--keep", "0.15:0.25"]), ("strength", ["--strength", "0.5"]),
                        ("both", ["--keep", "0.1:0.25", "--strength", "0.5", "--sampler", "ddim", "--eta", "0.5"]), ("plain", [])):
        dst = str(tmp_path / f"{name}.wav")
        sample_vqvae.main(common + flags + [ck, dst])
        outs[name] = read_s16(dst)
        assert outs[name].shape == want.shape
    for name in ("keep", "both"):
        assert np.array_equal(outs[name][a:b], want[a:b]), name
        rest = np.concatenate([outs[name][:a] != want[:a], outs[name][b:] != want[b:]])
        assert rest.mean() > 0.5, (name, rest.mean())
    assert not np.array_equal(outs["strength"], outs["plain"]) and not np.array_equal(outs["strength"][a:b], want[a:b])
    assert not np.array_equal(outs["keep"], outs["plain"])
