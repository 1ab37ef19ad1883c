"""The DDIM sampler on the device: `vqvs_ddim_step` and `vqvs_ddim_step_windows` against the float64 oracle tests/ddim_ref.py under
its bound C * 2^-24 * M (the roundings are counted in that file's docstring), against each other bit for bit where they coincide, and
against the reference generator tests/philox_ref.py; `Diffusion.ddim_sample` step by step, plain and guided; `VQVAE.decode` /
`decode_long` / `invert` and the scripts end to end.  fp32 mode throughout.

No run on an MI355X has been recorded yet: no figure is quoted here and profiles/ddim_margins.jsonl does not exist.  A run with
VQVS_DDIM_MARGINS=profiles/ddim_margins.jsonl appends the largest fraction of the bound each test found."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddim_ref
import philox_ref
from test_longform_gpu import SHAPES as WINDOW_SHAPES
from vq_voice_swap_amd import Classifier, DiffusionModel, VQVAE, _native, plan_windows
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

from util import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, CLIP, STEP = (1 << 32) + 7, (1 << 32) + 5, 3
CONSTRAIN, INVERT = _native.DDIM_CONSTRAIN, _native.DDIM_INVERT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(name, fraction):
    print(f"[margin] {name}: largest fraction of the bound {fraction:.3f}")
    path = os.environ.get("VQVS_DDIM_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": name, "fraction_of_bound": float(fraction)}) + "\n")


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def guarded(size, dev):
    return torch.full((size + 64,), float("nan"), device=dev)


def unguard(buf, size):
    assert torch.isnan(buf[size:]).all(), "the kernel wrote past the end of an output"
    assert torch.isfinite(buf[:size]).all(), "the kernel left elements unwritten (or wrote non-finite values)"
    return buf[:size]


def step_call(x, eps, grad, noise, a_t, a_to, flags, eta, noise_scale=1.0, seed=SEED, clip=CLIP, step=STEP):
    """`vqvs_ddim_step` on [B, T] device tensors; the output lies in front of a NaN guard that the call must leave alone."""
    B, T = x.shape
    out = guarded(B * T, x.device)
    _native.check(_native.lib().vqvs_ddim_step(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(noise), a_t.data_ptr(),
                                               a_to.data_ptr(), out.data_ptr(), B, T, flags, eta, noise_scale, seed, clip, step,
                                               _native._stream_ptr()))
    return unguard(out, B * T).view(B, T)


def windows_call(x, eps, grad, noise, a_t, a_to, n, W, H, flags, eta, noise_scale=1.0, seed=SEED, clip=CLIP, step=STEP, want_windows=True):
    Np = (n - 1) * H + W
    assert x.numel() == Np and eps.numel() == n * W and (noise is None or noise.numel() == Np) and (grad is None or grad.numel() == n * W)
    out = guarded(Np, x.device)
    win = guarded(n * W, x.device) if want_windows else None
    _native.check(_native.lib().vqvs_ddim_step_windows(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(noise), a_t.data_ptr(),
                                                       a_to.data_ptr(), out.data_ptr(), _native._ptr(win), n, W, H, flags, eta, noise_scale,
                                                       seed, clip, step, _native._stream_ptr()))
    return unguard(out, Np), None if win is None else unguard(win, n * W).view(n, W)


def fraction(got, want, bound):
    """max |got - want| / bound over the elements (a zero bound admits a zero error only)."""
    err = np.abs(got.detach().cpu().double().numpy().reshape(want.shape) - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


# ---------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("B,T", ddim_ref.SHAPES)
def test_kernel_vs_oracle(dev, schedule, B, T):
    """|got - want| <= 13 * 2^-24 * M per element (ddim_ref: C_STEP), plus sig * (1.2e-5 + 3 * 2^-24 |z|) with generated noise; flags
    {0, CONSTRAIN} x eta {0, 0.5, 1} x grad {NULL, given} x noise {given, generated}, rows at the three (t, step) pairs in turn."""
    xs = ddim_ref.case_inputs(B, T)
    x, eps, grad, noise = (to_dev(a, dev) for a in xs)
    z = philox_ref.randn(B, T, SEED, CLIP, philox_ref.STREAM_STEP, step=STEP)
    worst = 0.0
    for first in range(3):
        a_t, a_to = ddim_ref.alphas(schedule, B, first)
        for flags, eta, guided, generated in itertools.product((0, CONSTRAIN), ddim_ref.ETAS, (False, True), (False, True)):
            want, M, sig = ddim_ref.step(xs[0], xs[1], a_t, a_to, grad=xs[2] if guided else None, noise=z if generated else xs[3], eta=eta,
                                         constrain=bool(flags))
            got = step_call(x, eps, grad if guided else None, None if generated else noise, to_dev(a_t, dev), to_dev(a_to, dev), flags, eta)
            frac = fraction(got, want, ddim_ref.bound(M, sig=sig, z=z if generated else None))
            print(f"ddim step {schedule} (B, T)=({B}, {T}) first={first} flags={flags} eta={eta} guided={guided} generated={generated}: "
                  f"{frac:.3f} of the bound")
            assert frac <= 1.0, (first, flags, eta, guided, generated, frac)
            worst = max(worst, frac)
    record(f"1 ddim step vs oracle {schedule} (B, T)=({B}, {T})", worst)


# ---------------------------------------------------------------- 2. INVERT
@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("B,T", ddim_ref.SHAPES)
def test_invert_vs_oracle_and_round_trip(dev, schedule, B, T):
    """The INVERT step under the bound of test 1; then the eta = 0 step back with the same eps returns x within the sum of the two
    steps' bounds (the second taken at the state the device produced)."""
    xs = ddim_ref.case_inputs(B, T, seed=201)
    x, eps = to_dev(xs[0], dev), to_dev(xs[1], dev)
    worst = [0.0, 0.0]
    for first in range(3):
        a_hi_t, a_lo_t = ddim_ref.alphas(schedule, B, first)  # alpha_bar(t) < alpha_bar(t - step)
        want, M1, _ = ddim_ref.step(xs[0], xs[1], a_lo_t, a_hi_t, invert=True)
        up = step_call(x, eps, None, None, to_dev(a_lo_t, dev), to_dev(a_hi_t, dev), INVERT, 0.0)
        frac = fraction(up, want, ddim_ref.bound(M1))
        print(f"ddim invert {schedule} (B, T)=({B}, {T}) first={first}: {frac:.3f} of the bound")
        assert frac <= 1.0, (first, frac)
        back = step_call(up, eps, None, None, to_dev(a_hi_t, dev), to_dev(a_lo_t, dev), 0, 0.0)
        _, M2, _ = ddim_ref.step(up.cpu().numpy(), xs[1], a_hi_t, a_lo_t)
        trip = fraction(back, xs[0].astype(np.float64), ddim_ref.bound(M1) + ddim_ref.bound(M2))
        print(f"ddim invert then step {schedule} (B, T)=({B}, {T}) first={first}: {trip:.3f} of the two bounds' sum")
        assert trip <= 1.0, (first, trip)
        worst = [max(worst[0], frac), max(worst[1], trip)]
    record(f"2 ddim invert vs oracle {schedule} (B, T)=({B}, {T})", worst[0])
    record(f"2 ddim invert then step, sum of the two bounds {schedule} (B, T)=({B}, {T})", worst[1])


# ---------------------------------------------------------------- 3. eta = 0 is deterministic
def test_eta_zero_draws_and_reads_nothing(dev):
    B, T = 3, 4099
    x, eps, grad, _ = (to_dev(a, dev) for a in ddim_ref.case_inputs(B, T, seed=301))
    a_t, a_to = (to_dev(a, dev) for a in ddim_ref.alphas("exp", B, 0))
    poison = torch.full((B, T), float("nan"), device=dev)
    for flags, g in itertools.product((0, CONSTRAIN), (None, grad)):
        one = step_call(x, eps, g, None, a_t, a_to, flags, 0.0, seed=1, clip=0, step=0)
        assert torch.equal(one, step_call(x, eps, g, None, a_t, a_to, flags, 0.0, seed=SEED, clip=CLIP, step=9))
        assert torch.equal(one, step_call(x, eps, g, poison, a_t, a_to, flags, 0.0))  # (a NaN read would reach the output)
    up = step_call(x, eps, None, poison, a_to, a_t, INVERT, 0.0)  # INVERT, and noise_scale = 0 at eta = 1: the same
    assert torch.equal(up, step_call(x, eps, None, None, a_to, a_t, INVERT, 0.0, seed=5))
    assert torch.isfinite(step_call(x, eps, None, poison, a_t, a_to, 0, 1.0, noise_scale=0.0)).all()
    assert not torch.equal(step_call(x, eps, None, None, a_t, a_to, 0, 1.0, seed=1), step_call(x, eps, None, None, a_t, a_to, 0, 1.0, seed=2))


# ---------------------------------------------------------------- 4. the noise stream
def test_generated_noise_is_the_ddpm_step_stream(dev):
    """x = 0, eps = 0, eta = 1: the kernel returns sig z.  Divided by sig (float64, from the float32 alphas) it is philox_ref's row of
    (seed, clip_offset + b, step_index, stream 0) -- the words `vqvs_ddpm_step` draws -- within 1.2e-5 + 3 * 2^-24 |z|."""
    B, T = 3, 1001
    zero = torch.zeros(B, T, device=dev)
    a_t, a_to = np.full(B, 0.25, dtype=np.float32), np.full(B, 0.5, dtype=np.float32)
    sig = ddim_ref.coef(a_t, a_to, 1.0)["sig"][0]
    assert abs(sig - np.sqrt((1 - 0.5) / (1 - 0.25) * (1 - 0.25 / 0.5))) < 1e-15
    d_a_t, d_a_to = to_dev(a_t, dev), to_dev(a_to, dev)  # (held in names: a temporary's memory is handed to the next allocation)
    worst = 0.0
    for step in (0, 7):
        got = step_call(zero, zero, None, None, d_a_t, d_a_to, 0, 1.0, step=step)
        want = philox_ref.randn(B, T, SEED, CLIP, philox_ref.STREAM_STEP, step=step)
        excess = np.abs(got.cpu().double().numpy() / sig - want) - 3 * ddim_ref.U * np.abs(want)
        assert excess.max() <= ddim_ref.NORMAL_ABS, (step, excess.max())
        worst = max(worst, excess.max() / ddim_ref.NORMAL_ABS)
        ddpm = torch.empty(B, T, device=dev)  # ... and `vqvs_ddpm_step` at the same counters: sigma z with its own float32 sigma
        _native.check(_native.lib().vqvs_ddpm_step(zero.data_ptr(), zero.data_ptr(), None, d_a_t.data_ptr(), d_a_to.data_ptr(),
                                                   ddpm.data_ptr(), B, T, 0, 1.0, SEED, CLIP, step, _native._stream_ptr()))
        assert (got - ddpm).abs().max().item() <= 5 * ddim_ref.U * sig * np.abs(want).max()  # (the two sigmas' roundings and the products')
    record("4 generated noise vs reference generator (less 3 * 2^-24 |z|, over 1.2e-5)", worst)


# ---------------------------------------------------------------- 5. windows
def window_inputs(n, W, H, dev, seed=11):
    Np = (n - 1) * H + W
    host = [seeded((Np,), seed).numpy(), seeded((n, W), seed + 1).numpy(), (0.5 * seeded((n, W), seed + 2)).numpy(), seeded((Np,), seed + 3).numpy()]
    return host, [to_dev(a, dev) for a in host]


def scalar(v, dev):
    return torch.tensor([float(v)], dtype=torch.float32, device=dev)


def test_one_window_is_the_single_clip_step_bit_for_bit(dev):
    n, W, H = WINDOW_SHAPES[0]
    _, (x, eps, grad, noise) = window_inputs(n, W, H, dev)
    a_t, a_to = scalar(0.3, dev), scalar(0.37, dev)
    for flags, eta, given, guided in itertools.product((0, CONSTRAIN), ddim_ref.ETAS, (False, True), (False, True)):
        nz, g = noise if given else None, grad if guided else None
        got, win = windows_call(x, eps, g, nz, a_t, a_to, n, W, H, flags, eta)
        want = step_call(x.view(1, W), eps, g, None if nz is None else nz.view(1, W), a_t, a_to, flags, eta)
        assert torch.equal(got, want[0]), (flags, eta, given, guided, (got - want[0]).abs().max().item())
        assert torch.equal(win[0], want[0])
    up, _ = windows_call(x, eps, None, None, a_to, a_t, n, W, H, INVERT, 0.0)
    assert torch.equal(up, step_call(x.view(1, W), eps, None, None, a_to, a_t, INVERT, 0.0)[0])


def test_no_overlap_without_constrain_is_one_long_row_bit_for_bit(dev):
    n, W = 3, 4352
    _, (x, eps, grad, noise) = window_inputs(n, W, W, dev)
    a_t, a_to = scalar(0.3, dev), scalar(0.37, dev)
    for eta, given, guided in itertools.product((0.0, 0.5), (False, True), (False, True)):
        nz, g = noise if given else None, grad if guided else None
        got, win = windows_call(x, eps, g, nz, a_t, a_to, n, W, W, 0, eta)
        want = step_call(x.view(1, -1), eps.view(1, -1), None if g is None else g.view(1, -1), None if nz is None else nz.view(1, -1), a_t, a_to,
                         0, eta)[0]
        assert torch.equal(got, want), (eta, given, guided)
        assert torch.equal(win.view(-1), want)


@pytest.mark.parametrize("schedule", ["exp", "cos"])
@pytest.mark.parametrize("n,W,H", WINDOW_SHAPES)
def test_windows_vs_oracle(dev, schedule, n, W, H):
    """The general case under the bound of test 1, with C = 16 where two windows meet (ddim_ref: C_BLEND): flags {0, CONSTRAIN} x eta
    {0, 0.5, 1} x grad {NULL, [n, W]}, explicit noise, the three (t, step) pairs; the window output is the state gathered."""
    host, (x, eps, grad, noise) = window_inputs(n, W, H, dev, seed=21)
    worst = 0.0
    for first in range(3):
        a_t, a_to = ddim_ref.alphas(schedule, 1, first)
        for flags, eta, guided in itertools.product((0, CONSTRAIN), ddim_ref.ETAS, (False, True)):
            want, want_win, M, Cn, _ = ddim_ref.step_windows(host[0], host[1], a_t, a_to, n, W, H, grad=host[2] if guided else None,
                                                            noise=host[3], eta=eta, constrain=bool(flags))
            got, win = windows_call(x, eps, grad if guided else None, noise, to_dev(a_t, dev), to_dev(a_to, dev), n, W, H, flags, eta)
            frac = fraction(got, want, ddim_ref.bound(M, Cn))
            print(f"ddim windows {schedule} (n, W, H)=({n}, {W}, {H}) first={first} flags={flags} eta={eta} guided={guided}: {frac:.3f} of the bound")
            assert frac <= 1.0, (first, flags, eta, guided, frac)
            assert torch.equal(win, got.unfold(0, W, H))
            assert fraction(win, want_win, ddim_ref.window_view(ddim_ref.bound(M, Cn), n, W, H)) <= 1.0
            worst = max(worst, frac)
    alone, _ = windows_call(x, eps, grad, noise, to_dev(a_t, dev), to_dev(a_to, dev), n, W, H, CONSTRAIN, 1.0, want_windows=False)
    assert torch.equal(alone, got)  # the optional output changes nothing
    record(f"5 ddim windows vs oracle {schedule} (n, W, H)=({n}, {W}, {H})", worst)


# ---------------------------------------------------------------- 6. / 7. ddim_sample step by step
def det_model(m, dev):
    det_init_(m.state_dict().items())
    m.eval()
    m.to(dev)
    m.set_precision("fp32")
    return m


@pytest.fixture(scope="module")
def unet(dev):
    return det_model(DiffusionModel("unet", 32), dev)


def run_recorded(d, x_T, predictor, steps, cond_fn=None, **kw):
    rec, grads = [], []

    def pred(x, ts):
        e = predictor(x, ts)
        rec.append((x.clone(), ts.clone(), e.clone()))
        return e

    guide = None
    if cond_fn is not None:
        def guide(x, ts):
            g = cond_fn(x, ts)
            grads.append((x.clone(), ts.clone(), g.clone()))
            return g

        guide.native_modules = getattr(cond_fn, "native_modules", ())
    return d.ddim_sample(x_T, pred, steps, cond_fn=guide, **kw), rec, grads


def check_steps(d, out, rec, grads, steps, eta, constrain, noises, name):
    """Each step on its own: the oracle applied to what the predictor (and the cond_fn) saw and returned, against what they saw next."""
    B, T = out.shape[0], out.shape[-1]
    _, a_t_all, a_to_all, _ = d.step_tables(steps, B, None, torch.device("cpu"))
    worst = 0.0
    for i in range(steps):
        x, ts, eps = rec[i]
        assert torch.equal(ts.cpu(), torch.full((B,), (steps - i) / steps, dtype=torch.float32))
        g = None
        if grads:
            assert torch.equal(grads[i][0], x) and torch.equal(grads[i][1], ts)  # the gradient is taken AT (x_t, t)
            g = grads[i][2].cpu().numpy().reshape(B, T)
        last = i + 1 == steps
        nz = None if last or not eta else noises[i].cpu().numpy().reshape(B, T)
        want, M, _ = ddim_ref.step(x.cpu().numpy().reshape(B, T), eps.cpu().numpy().reshape(B, T), a_t_all[i].numpy(), a_to_all[i].numpy(), grad=g,
                                   noise=nz, eta=eta, constrain=constrain)
        got = out if last else rec[i + 1][0]
        frac = fraction(got, want, ddim_ref.bound(M))
        print(f"{name} step {i}: {frac:.3f} of the bound")
        assert frac <= 1.0, (name, i, frac)
        worst = max(worst, frac)
    assert float(a_to_all[-1][0]) == 1.0  # the last step lands on x0 itself
    record(f"{name}, each of {steps} steps vs oracle", worst)


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("constrain", [False, True])
def test_ddim_sample_step_by_step_vs_oracle(dev, unet, eta, constrain):
    B, T, steps = 2, 1024, 4
    d = unet.diffusion
    x_T = seeded((B, 1, T), 51).to(dev)
    noises = [seeded((B, 1, T), 60 + i).to(dev) for i in range(steps)]
    out, rec, _ = run_recorded(d, x_T, unet.predictor, steps, eta=eta, constrain=constrain, noise=noises)
    assert out.shape == (B, 1, T) and len(rec) == steps
    check_steps(d, out, rec, [], steps, eta, constrain, noises, f"6 ddim_sample eta={eta} constrain={constrain}")
    # sharding invariance with generated noise: the rows as one batch, and as two calls with clip_offset
    kw = dict(eta=eta, constrain=constrain, seed=SEED)
    both = d.ddim_sample(x_T, unet.predictor, steps, clip_offset=CLIP, **kw)
    for b in range(B):
        assert torch.equal(both[b:b + 1], d.ddim_sample(x_T[b:b + 1], unet.predictor, steps, clip_offset=CLIP + b, **kw)), b
    if eta == 0:
        assert torch.equal(both, out) and torch.equal(both, d.ddim_sample(x_T, unet.predictor, steps, **dict(kw, seed=1)))
    else:
        assert not torch.equal(both, d.ddim_sample(x_T, unet.predictor, steps, clip_offset=CLIP, **dict(kw, seed=SEED + 1)))


@pytest.mark.parametrize("constrain", [False, True])
def test_guided_ddim_sample_step_by_step_vs_oracle(dev, unet, constrain):
    B, T, steps, eta = 2, 1024, 4, 0.5
    clf = det_model(Classifier(num_labels=3, base_channels=32), dev)
    d = unet.diffusion
    x_T = seeded((B, 1, T), 52).to(dev)
    noises = [seeded((B, 1, T), 70 + i).to(dev) for i in range(steps)]
    cond_fn = clf.guidance_fn(torch.tensor([2, 0], device=dev), 3.0)
    out, rec, grads = run_recorded(d, x_T, unet.predictor, steps, cond_fn=cond_fn, eta=eta, constrain=constrain, noise=noises)
    assert len(grads) == steps and all(float(g[2].abs().max()) > 0 for g in grads)
    check_steps(d, out, rec, grads, steps, eta, constrain, noises, f"7 guided ddim_sample constrain={constrain}")
    plain, _, _ = run_recorded(d, x_T, unet.predictor, steps, eta=eta, constrain=constrain, noise=noises)
    assert not torch.equal(plain, out)


def test_ddim_sample_windows_step_by_step_vs_oracle(dev):
    """`ddim_sample_windows` with an analytic predictor and cond_fn: every step against the oracle's windows form, slices of one window
    or of three giving the same sample."""
    n, W, H, steps, eta = 3, 2048, 1536, 3, 0.5
    Np = (n - 1) * H + W
    d = Diffusion(make_schedule("exp"))
    x_T = seeded((1, 1, Np), 53).to(dev)
    noises = [seeded((1, 1, Np), 80 + i).to(dev) for i in range(steps)]

    def index(m, first, like):
        return (first + torch.arange(m, device=like.device, dtype=torch.float32)).view(m, 1, 1)

    def cond_fn(w, ts, first):
        return torch.tanh(w) * (ts.view(-1, 1, 1) + 0.1 * index(w.shape[0], first, w))

    runs = {}
    for wb in (3, 1):
        rec = []

        def predictor(w, ts, first):
            e = 0.5 * torch.sin(3 * w) + 0.1 * index(w.shape[0], first, w)
            rec.append((first, w.clone(), ts.clone(), e.clone()))
            return e

        runs[wb] = (d.ddim_sample_windows(x_T, predictor, steps, window=W, hop=H, window_batch=wb, eta=eta, constrain=True, cond_fn=cond_fn,
                                          noise=noises), rec)
    assert torch.equal(runs[1][0], runs[3][0])
    out, rec = runs[3]
    _, a_t_all, a_to_all, _ = d.step_tables(steps, 1, None, torch.device("cpu"))
    worst = 0.0
    for i in range(steps):
        _, w_in, ts, eps = rec[i]
        w_np = w_in.cpu().numpy().reshape(n, W)
        x = np.concatenate([w_np[0]] + [w_np[b, W - H:] for b in range(1, n)])
        assert np.array_equal(ddim_ref.window_view(x, n, W, H), w_np)  # the windows agree on the samples they share
        g = cond_fn(w_in, ts, 0).cpu().numpy().reshape(n, W)
        last = i + 1 == steps
        want, _, M, Cn, _ = ddim_ref.step_windows(x, eps.cpu().numpy(), a_t_all[i].numpy(), a_to_all[i].numpy(), n, W, H, grad=g,
                                                  noise=None if last else noises[i].cpu().numpy(), eta=eta, constrain=True)
        got = out.view(-1) if last else torch.cat([rec[i + 1][1][0, 0]] + [rec[i + 1][1][b, 0, W - H:] for b in range(1, n)])
        frac = fraction(got, want, ddim_ref.bound(M, Cn))
        print(f"ddim_sample_windows step {i}: {frac:.3f} of the bound")
        assert frac <= 1.0, (i, frac)
        worst = max(worst, frac)
    record(f"5 ddim_sample_windows guided, constrained, each of {steps} steps vs oracle", worst)


# ---------------------------------------------------------------- 8. end to end
@pytest.fixture(scope="module")
def vqvae(dev):
    return det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=3), dev)


def test_vqvae_decode_invert_and_decode_long(dev, vqvae):
    W, H, steps = 2048, 1536, 4
    wave = (0.3 * seeded((1, 1, W), 72)).clamp(-1, 1).to(dev)
    codes = vqvae.encode(wave)
    src, dst = torch.tensor([0], device=dev), torch.tensor([2], device=dev)
    kw = dict(steps=steps, constrain=True, sampler="ddim")
    out = vqvae.decode(codes, dst, seed=9, **kw)
    assert out.shape == (1, 1, W) and bool(torch.isfinite(out).all())
    x_T = torch.randn(1, 1, W, generator=torch.Generator().manual_seed(3)).to(dev)
    fixed = vqvae.decode(codes, dst, x_T=x_T, seed=1, **kw)
    assert torch.equal(fixed, vqvae.decode(codes, dst, x_T=x_T, seed=2, **kw))  # eta = 0: x_T alone decides
    assert not torch.equal(fixed, vqvae.decode(codes, dst, x_T=x_T, seed=2, eta=0.5, **kw))
    assert not torch.equal(fixed, vqvae.decode(codes, dst, x_T=x_T, seed=1, steps=steps, constrain=True))  # the DDPM sampler is another one
    with pytest.raises(ValueError):
        vqvae.decode(codes, dst, steps=steps, eta=0.5)  # eta belongs to the DDIM sampler
    with pytest.raises(ValueError):
        vqvae.decode(codes, dst, steps=steps, sampler="heun")
    latent = vqvae.invert(wave, src, steps=steps)
    assert latent.shape == (1, 1, W) and bool(torch.isfinite(latent).all()) and not torch.equal(latent, wave)
    assert torch.equal(latent, vqvae.invert(wave, src, steps=steps, codes=codes))
    swapped = vqvae.decode(codes, dst, x_T=latent, **kw)
    assert swapped.shape == (1, 1, W) and bool(torch.isfinite(swapped).all())
    assert torch.equal(swapped, vqvae.decode(codes, dst, x_T=latent, seed=5, **kw))
    guided = vqvae.decode_uncond_guidance(codes, src, steps=steps, vq_scale=1.5, x_T=x_T, sampler="ddim")
    assert guided.shape == (1, 1, W) and bool(torch.isfinite(guided).all())
    # two windows
    N = 3000
    n, padded = plan_windows(N, W, H)
    assert (n, padded) == (2, 3584)
    long_wave = (0.3 * seeded((1, 1, N), 73)).clamp(-1, 1).to(dev)
    long_codes = vqvae.encode_long(long_wave, W, H)
    lkw = dict(num_samples=N, window=W, hop=H, steps=steps, constrain=True, clip_offset=5, sampler="ddim")
    long_out = vqvae.decode_long(long_codes, dst, seed=9, window_batch=2, **lkw)
    assert long_out.shape == (1, 1, N) and bool(torch.isfinite(long_out).all())
    assert torch.equal(long_out, vqvae.decode_long(long_codes, dst, seed=9, window_batch=1, **lkw))
    assert not torch.equal(long_out, vqvae.decode_long(long_codes, dst, seed=9, **dict(lkw, sampler="ddpm")))
    # one window: decode_long is decode, as for the DDPM sampler
    assert torch.equal(vqvae.decode_long(codes, dst, seed=9, **dict(lkw, num_samples=W)), vqvae.decode(codes, dst, seed=9, clip_offset=5, **kw))


DRIVER = """
import json, sys
sys.path.insert(0, sys.argv[1])
import sample_diffusion, sample_vqvae
for script, argv in json.loads(sys.argv[2]):
    {"sample_diffusion": sample_diffusion, "sample_vqvae": sample_vqvae}[script].main(argv)
"""


def test_scripts_in_a_fresh_process(dev, vqvae, tmp_path):
    """sample_diffusion.py and sample_vqvae.py with the new flags, in ONE fresh child process; `--sampler ddpm` and no flag at all write
    byte-identical files."""
    m = DiffusionModel("unet", 32, num_labels=4)
    det_init_(m.state_dict().items())
    ck, ckv, src = (str(tmp_path / name) for name in ("d.pt", "v.pt", "in.wav"))
    m.save(ck)
    vqvae.save(ckv)
    w = ChunkWriter(src, 16000)
    w.write(0.3 * np.sin(np.arange(64000) * 0.05).astype(np.float32))
    w.close()
    out = {k: str(tmp_path / f"{k}.wav") for k in ("ddim", "ddim_again", "ddpm", "plain", "swap", "whole")}
    common = ["--checkpoint-path", ck, "--sample-steps", "3", "--constrain", "--seed", "5", "--target-class", "1"]
    vq = ["--label", "2", "--input-file", src, "--sample-steps", "3", "--seed", "9"]
    jobs = [("sample_diffusion", common + ["--sampler", "ddim", "--sample-path", out["ddim"]]),
            ("sample_diffusion", common + ["--sampler", "ddim", "--eta", "0", "--sample-path", out["ddim_again"]]),
            ("sample_diffusion", common + ["--sampler", "ddpm", "--sample-path", out["ddpm"]]),
            ("sample_diffusion", common + ["--sample-path", out["plain"]]),
            ("sample_vqvae", vq + ["--sampler", "ddim", "--source-label", "0", ckv, out["swap"]]),
            ("sample_vqvae", vq + ["--sampler", "ddim", "--eta", "0.5", "--whole-file", "--window-seconds", "2.56", "--overlap-seconds", "0.32",
                              ckv, out["whole"]])]
    r = subprocess.run([sys.executable, "-c", DRIVER, ROOT, json.dumps(jobs)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    data = {k: open(p, "rb").read() for k, p in out.items()}
    assert data["ddpm"] == data["plain"] and data["ddim"] == data["ddim_again"] and data["ddim"] != data["ddpm"]
    for k, p in out.items():
        rd = ChunkReader(p, 16000)
        a = rd.read(64000 + 1000)
        rd.close()
        assert a.shape == (64000,) and np.isfinite(a).all() and np.abs(a).max() <= 1.0, k
