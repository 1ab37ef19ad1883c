"""Long-form conversion on the device: `vqvs_ddpm_step_windows` against `vqvs_ddpm_step` (bit for bit where the two coincide), against
the numpy oracle tests/longform_ref.py and against the reference generator tests/philox_ref.py; `Diffusion.ddpm_sample_windows` step
by step against the oracle; `VQVAE.encode_long` / `decode_long` and `sample_vqvae.py --whole-file` end to end.

No run on an MI355X has been recorded yet: no figure is quoted here and profiles/longform_margins.jsonl does not exist.  A run with
VQVS_LONGFORM_MARGINS=profiles/longform_margins.jsonl appends the measured maxima next to their bounds."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

import longform_ref
import philox_ref
from oracle import ref_cpu
from vq_voice_swap_amd import VQVAE, _native, plan_windows
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

from util import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, W, H): one window; three sum chunks with a ragged last one and V < H; W / 4 no multiple of the 256-thread block; V == H
SHAPES = [(1, 4352, 4352), (3, 9216, 6144), (4, 4352, 2304), (2, 512, 256)]
STEP_REL = {"exp": 2e-6, "cos": 4e-6}  # the project's gates for this arithmetic (test_ddpm_previous_vs_golden, ..._cos_schedule_...)
NORMAL_ABS = 1.2e-5  # |device normal - reference normal| (tests/test_rng_gpu.py)
SEED, CLIP = (1 << 32) + 7, (1 << 32) + 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(name, value, bound):
    rec = {"test": name, "max_abs_err": float(value), "bound": float(bound), "fraction_of_bound": float(value / bound)}
    print(f"[margin] {name}: max abs err {value:.3e} (bound {bound:.3e})")
    path = os.environ.get("VQVS_LONGFORM_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def scalar(v, dev):
    return torch.tensor([float(v)], dtype=torch.float32, device=dev)


def windows_call(x, eps, noise, a_t, a_prev, n, W, H, flags, noise_scale=1.0, seed=SEED, clip=CLIP, step=3, want_windows=True):
    """(x_prev [Np], windows [n, W] or None) of one call; both outputs lie in front of a NaN guard that the call must leave alone."""
    Np = (n - 1) * H + W
    assert x.numel() == Np and eps.numel() == n * W and (noise is None or noise.numel() == Np)
    out = torch.full((Np + 64,), float("nan"), device=x.device)
    win = torch.full((n * W + 64,), float("nan"), device=x.device) if want_windows else None
    _native.check(_native.lib().vqvs_ddpm_step_windows(x.data_ptr(), eps.data_ptr(), _native._ptr(noise), a_t.data_ptr(), a_prev.data_ptr(),
                                                       out.data_ptr(), _native._ptr(win), n, W, H, flags, noise_scale, seed, clip, step,
                                                       _native._stream_ptr()))
    for buf, size in ((out, Np), (win, n * W)):
        if buf is not None:
            assert torch.isnan(buf[size:]).all(), "the kernel wrote past the end of an output"
            assert torch.isfinite(buf[:size]).all(), "the kernel left elements unwritten (or wrote non-finite values)"
    return out[:Np], None if win is None else win[:n * W].view(n, W)


def step_call(x, eps, noise, a_t, a_prev, flags, noise_scale, seed, clip, step):
    """`vqvs_ddpm_step` on ONE row."""
    T = x.numel()
    out = torch.empty(T, device=x.device)
    _native.check(_native.lib().vqvs_ddpm_step(x.data_ptr(), eps.data_ptr(), _native._ptr(noise), a_t.data_ptr(), a_prev.data_ptr(),
                                               out.data_ptr(), 1, T, flags, noise_scale, seed, clip, step, _native._stream_ptr()))
    return out


def inputs(n, W, H, dev, seed=11):
    Np = (n - 1) * H + W
    return seeded((Np,), seed).to(dev), seeded((n, W), seed + 1).to(dev), seeded((Np,), seed + 2).to(dev)


# ---------------------------------------------------------------- 1. bit identity with vqvs_ddpm_step
def test_one_window_is_the_single_clip_step_bit_for_bit(dev):
    n, W, H = SHAPES[0]
    x, eps, noise = inputs(n, W, H, dev)
    a_t, a_prev = scalar(0.3, dev), scalar(0.37, dev)
    for flags, given, scale in itertools.product(range(4), (False, True), (0.0, 1.0)):
        nz = noise if given else None
        got, win = windows_call(x, eps, nz, a_t, a_prev, n, W, H, flags, scale)
        want = step_call(x, eps, nz, a_t, a_prev, flags, scale, SEED, CLIP, 3)
        assert torch.equal(got, want), (flags, given, scale, (got - want).abs().max().item())
        assert torch.equal(win[0], want)


def test_no_overlap_without_constrain_is_one_long_row_bit_for_bit(dev):
    n, W = 3, 4352
    x, eps, noise = inputs(n, W, W, dev)
    a_t, a_prev = scalar(0.3, dev), scalar(0.37, dev)
    for flags, given in itertools.product((0, _native.DDPM_SIGMA_LARGE), (False, True)):
        nz = noise if given else None
        got, win = windows_call(x, eps, nz, a_t, a_prev, n, W, W, flags)
        want = step_call(x, eps.view(-1), nz, a_t, a_prev, flags, 1.0, SEED, CLIP, 3)
        assert torch.equal(got, want), (flags, given)
        assert torch.equal(win.view(-1), want)


# ---------------------------------------------------------------- 2. arithmetic against the numpy oracle
@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("n,W,H", SHAPES)
def test_step_vs_numpy_oracle(dev, schedule, n, W, H):
    """max |got - want| <= 2e-6 * max(1, max |want|) (4e-6 under the cos schedule) with explicit noise, every flag combination."""
    x, eps, noise = inputs(n, W, H, dev, seed=21)
    xn, en, nn = x.cpu().numpy(), eps.cpu().numpy(), noise.cpu().numpy()
    worst = 0.0
    for t, step in ((0.6, 0.02), (0.3, 0.02)):
        ts = torch.tensor([t], dtype=torch.float32)
        a_t, a_prev = ref_cpu.schedule_alpha(schedule, ts), ref_cpu.schedule_alpha(schedule, ts - step)
        for flags in range(4):
            kw = dict(sigma_large=bool(flags & 1), constrain=bool(flags & 2))
            want, want_win = longform_ref.step_windows(xn, en, nn, a_t.item(), a_prev.item(), n, W, H, **kw)
            got, win = windows_call(x, eps, noise, a_t.to(dev), a_prev.to(dev), n, W, H, flags)
            err = np.abs(got.cpu().numpy() - want).max()
            bound = STEP_REL[schedule] * max(1.0, np.abs(want).max())
            print(f"step windows {schedule} (n, W, H)=({n}, {W}, {H}) t={t} {kw}: max abs err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (t, kw, err, bound)
            assert np.abs(win.cpu().numpy() - want_win).max() <= bound
            worst = max(worst, err / bound)
    record(f"2 step vs numpy oracle {schedule} (n, W, H)=({n}, {W}, {H}) (largest fraction of the gate)", worst, 1.0)


# ---------------------------------------------------------------- 3. generated noise
@pytest.mark.parametrize("n,W,H", [(3, 9216, 6144), (2, 512, 256)])
def test_generated_noise_is_one_row_of_the_step_stream(dev, n, W, H):
    """x = 0, eps = 0, no flags: the kernel returns sigma z.  Divided by sigma (float64, alphas whose coefficient arithmetic is exact
    up to the last division and the square root) it is z of ONE row of Np values of (seed, clip, step, stream 0), whatever the
    windows are, within the tolerance of tests/test_rng_gpu.py::test_step_word_vs_reference: 1.2e-5 + 3 * 2^-24 |z|."""
    Np = (n - 1) * H + W
    zero = torch.zeros(Np, device=dev)
    a_t, a_prev = scalar(0.25, dev), scalar(0.5, dev)
    sig = np.sqrt((1 - 0.25 / 0.5) * (1 - 0.5) / (1 - 0.25))
    worst = 0.0
    for s in (0, 7):
        got, win = windows_call(zero, torch.zeros(n, W, device=dev), None, a_t, a_prev, n, W, H, 0, step=s)
        want = philox_ref.randn(1, Np, SEED, CLIP, philox_ref.STREAM_STEP, step=s)[0]
        excess = np.abs(got.cpu().double().numpy() / sig - want) - 3 * 2.0 ** -24 * np.abs(want)
        assert excess.max() <= NORMAL_ABS, (s, excess.max())
        worst = max(worst, excess.max())
        # ... and the windows that share a sample share its draw
        assert torch.equal(win, got.unfold(0, W, H))
    record(f"3 generated noise vs reference (n, W, H)=({n}, {W}, {H}) (less 3 * 2^-24 |z|)", worst, NORMAL_ABS)
    # with real inputs and every flag: what the same call gives when handed the reference's draws, within the step's own gate plus
    # the generator's tolerance (sigma <= 1); and twice the same
    x, eps, _ = inputs(n, W, H, dev, seed=31)
    given = torch.from_numpy(philox_ref.randn(1, Np, SEED, CLIP, philox_ref.STREAM_STEP, step=7)[0].astype(np.float32)).to(dev)
    a_t, a_prev = scalar(0.3, dev), scalar(0.37, dev)
    for flags in range(4):
        got, _ = windows_call(x, eps, None, a_t, a_prev, n, W, H, flags, step=7)
        ref, _ = windows_call(x, eps, given, a_t, a_prev, n, W, H, flags, step=7)
        again, _ = windows_call(x, eps, None, a_t, a_prev, n, W, H, flags, step=7)
        assert (got - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item()) + NORMAL_ABS, flags
        assert torch.equal(got, again)


# ---------------------------------------------------------------- 4. the window output
@pytest.mark.parametrize("n,W,H", SHAPES)
def test_window_output_is_the_long_state_gathered(dev, n, W, H):
    x, eps, noise = inputs(n, W, H, dev, seed=41)
    a_t, a_prev = scalar(0.3, dev), scalar(0.37, dev)
    for flags, nz in ((0, noise), (3, None), (2, noise)):
        got, win = windows_call(x, eps, nz, a_t, a_prev, n, W, H, flags)
        assert torch.equal(win, got.unfold(0, W, H)), flags
        alone, _ = windows_call(x, eps, nz, a_t, a_prev, n, W, H, flags, want_windows=False)  # the optional output changes nothing
        assert torch.equal(alone, got)


# ---------------------------------------------------------------- 5. ddpm_sample_windows
def analytic_predictor(rec):
    def predictor(w, ts, first):
        m = w.shape[0]
        eps = 0.5 * torch.sin(3 * w) + 0.1 * (first + torch.arange(m, device=w.device, dtype=torch.float32)).view(m, 1, 1)
        rec.append((first, w.clone(), ts.clone(), eps.clone()))
        return eps

    return predictor


def analytic_cond_fn(mean, ts_prev, first):
    m = mean.shape[0]
    index = first + torch.arange(m, device=mean.device, dtype=torch.float32)  # the window's own index, however the batch is sliced
    return torch.tanh(mean) * (ts_prev + 0.1 * index).view(m, 1, 1)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("constrain", [False, True])
def test_ddpm_sample_windows_step_by_step_vs_oracle(dev, guided, constrain):
    """Every step on its own: the oracle applied to the windows the predictor was handed and to what it returned, against the
    windows it was handed next (or the result), under the gate of test 2.  Errors are not compounded through 1 / sqrt(alpha_bar(1))."""
    n, W, H, steps = 3, 2048, 1536, 4
    Np = (n - 1) * H + W
    d = Diffusion(make_schedule("exp"))
    x_T = seeded((1, 1, Np), 51).to(dev)
    noises = [seeded((1, 1, Np), 60 + i).to(dev) for i in range(steps)]
    cond_fn = analytic_cond_fn if guided else None
    runs = {}
    for wb in (3, 1):
        rec = []
        out = d.ddpm_sample_windows(x_T, analytic_predictor(rec), steps, window=W, hop=H, window_batch=wb, constrain=constrain, cond_fn=cond_fn,
                                    noise=noises)
        assert out.shape == (1, 1, Np)
        assert [r[0] for r in rec] == [b for _ in range(steps) for b in range(0, n, wb)]
        runs[wb] = (out, rec)
    assert torch.equal(runs[1][0], runs[3][0])  # slices of one window or of three: the same sample
    out, rec = runs[3]
    worst = 0.0
    for i in range(steps):
        _, w_in, ts, eps = rec[i]
        t = (steps - i) / steps
        assert torch.equal(ts.cpu(), torch.tensor([t] * n, dtype=torch.float32))
        w_np = w_in.cpu().numpy().reshape(n, W)
        x = np.concatenate([w_np[0]] + [w_np[b, W - H:] for b in range(1, n)])
        assert np.array_equal(longform_ref.window_view(x, n, W, H), w_np)  # the windows agree on the samples they share
        tt = torch.tensor([t], dtype=torch.float32)
        tp = tt - torch.full_like(tt, 1 / steps)
        a_t, a_prev = ref_cpu.schedule_alpha("exp", tt).item(), ref_cpu.schedule_alpha("exp", tp).item()
        e = eps.cpu().numpy().reshape(n, W)
        if guided:
            grad = lambda mean: analytic_cond_fn(torch.from_numpy(mean).view(n, 1, W), tp.expand(n), 0).numpy().reshape(n, W)  # noqa: E731
            e = longform_ref.guided_eps(w_np, e, grad, a_t, a_prev)
        last = i + 1 == steps
        want, _ = longform_ref.step_windows(x, e, None if last else noises[i].cpu().numpy(), a_t, a_prev, n, W, H, constrain=constrain)
        got = (out if last else torch.cat([rec[i + 1][1][0, 0]] + [rec[i + 1][1][b, 0, W - H:] for b in range(1, n)])).cpu().numpy().reshape(-1)
        err, bound = np.abs(got - want).max(), STEP_REL["exp"] * max(1.0, np.abs(want).max())
        print(f"ddpm_sample_windows guided={guided} constrain={constrain} step {i}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (i, err, bound)
        worst = max(worst, err / bound)
    record(f"5 ddpm_sample_windows guided={guided} constrain={constrain}, each of {steps} steps vs oracle (largest fraction of the gate)", worst, 1.0)


# ---------------------------------------------------------------- 6. end to end
def det_model(m):
    det_init_(m.state_dict().items())
    m.eval()
    return m


@pytest.fixture(scope="module")
def vqvae(dev):
    model = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=3)).to(dev)
    model.set_precision("fp32")
    return model


def test_encode_decode_long(dev, vqvae):
    N, W, H, steps = 5000, 2048, 1536, 4
    n, padded = plan_windows(N, W, H)
    assert (n, padded) == (3, 5120)
    wave = (0.3 * seeded((1, 1, N), 71)).clamp(-1, 1).to(dev)
    label = torch.tensor([1], device=dev)
    codes = vqvae.encode_long(wave, W, H, window_batch=3)
    assert codes.shape == (n, W // 256) and codes.dtype == torch.int64
    assert torch.equal(codes, vqvae.encode_long(wave, W, H, window_batch=1))
    assert torch.equal(codes[0:1], vqvae.encode(wave[..., :W]))
    kw = dict(num_samples=N, window=W, hop=H, steps=steps, constrain=True, seed=9, clip_offset=5)
    out = vqvae.decode_long(codes, label, window_batch=3, **kw)
    assert out.shape == (1, 1, N) and bool(torch.isfinite(out).all())
    # the library's claim that a clip does not depend on its batch, here for windows
    assert torch.equal(out, vqvae.decode_long(codes, label, window_batch=1, **kw))
    assert torch.equal(out, vqvae.decode_long(codes, label.expand(n), window_batch=2, **kw))  # one label, or one per window
    for bad in (dict(window=W + 4), dict(hop=H + 4), dict(num_samples=2 * N)):  # off the model's rate; more windows than codes
        with pytest.raises(ValueError):
            vqvae.decode_long(codes, label, **dict(kw, **bad))


def test_one_window_decode_long_is_decode(dev, vqvae):
    W, H = 2048, 1536
    wave = (0.3 * seeded((1, 1, W), 72)).clamp(-1, 1).to(dev)
    label = torch.tensor([2], device=dev)
    codes = vqvae.encode_long(wave, W, H)
    assert torch.equal(codes, vqvae.encode(wave))
    got = vqvae.decode_long(codes, label, num_samples=W, window=W, hop=H, steps=4, constrain=True, seed=9, clip_offset=5)
    want = vqvae.decode(codes, label, steps=4, constrain=True, seed=9, clip_offset=5)
    assert torch.equal(got, want)


def test_sample_vqvae_whole_file(dev, vqvae, tmp_path):
    sys.path.insert(0, ROOT)
    import sample_vqvae

    ck, src, dst = (str(tmp_path / name) for name in ("v.pt", "in.wav", "out.wav"))
    vqvae.save(ck)
    N = 8000  # 0.5 s
    w = ChunkWriter(src, 16000)
    w.write(0.3 * np.sin(np.arange(N) * 0.05).astype(np.float32))
    w.close()
    sample_vqvae.main(["--label", "2", "--input-file", src, "--sample-steps", "3", "--seed", "9", "--check-vq", "--whole-file",
                       "--window-seconds", "0.128", "--overlap-seconds", "0.032", "--window-batch", "2", ck, dst])
    r = ChunkReader(dst, 16000)
    got = r.read(N + 1000)
    r.close()
    assert got.shape == (N,) and np.isfinite(got).all()
