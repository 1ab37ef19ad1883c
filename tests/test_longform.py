"""Long-form conversion, host side: the export, declaration and argument checks of `vqvs_ddpm_step_windows`, `plan_windows`, the
numpy oracle tests/longform_ref.py against the reference-pinned `oracle.ref_cpu.ddpm_previous` and against itself, and the new
flags of sample_vqvae.py (none of this needs a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import longform_ref
import vq_voice_swap_amd
from oracle import ref_cpu
from vq_voice_swap_amd import _native, plan_windows

from util import flags_of, seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_declared(lib_built):
    assert "vqvs_ddpm_step_windows" in _native.EXPORTS and hasattr(lib_built, "vqvs_ddpm_step_windows")
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    decl = re.search(r"int vqvs_ddpm_step_windows\(([^;]*)\);", header)
    assert decl, "include/vqvs.h does not declare vqvs_ddpm_step_windows"
    args = [a.strip() for a in " ".join(decl.group(1).split()).split(",")]
    assert args == ["const float* d_x", "const float* d_eps", "const float* d_noise", "const float* d_alpha_t", "const float* d_alpha_prev",
                    "float* d_x_prev", "float* d_windows", "int n", "int W", "int H", "uint32_t flags", "float noise_scale", "uint64_t seed",
                    "uint64_t clip", "uint32_t step_index", "void* stream"]
    assert len(lib_built.vqvs_ddpm_step_windows.argtypes) == len(args)
    assert "plan_windows" in vq_voice_swap_amd.__all__
    assert callable(vq_voice_swap_amd.Diffusion.ddpm_sample_windows) and callable(vq_voice_swap_amd.VQVAE.encode_long)
    assert callable(vq_voice_swap_amd.VQVAE.decode_long)


def test_entry_point_refuses_bad_arguments_without_a_device(lib_built):
    """Every limit of include/vqvs.h: VQVS_ERR_ARG with host-only pointers, which a call that reached the device would fault on."""
    L = lib_built
    bufs = [(C.c_float * 64)() for _ in range(6)]
    x, eps, noise, a_t, a_prev, out = (C.cast(b, C.c_void_p) for b in bufs)
    ok = dict(x=x, eps=eps, noise=noise, a_t=a_t, a_prev=a_prev, out=out, win=None, n=3, W=16, H=12)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_ddpm_step_windows(a["x"], a["eps"], a["noise"], a["a_t"], a["a_prev"], a["out"], a["win"], a["n"], a["W"], a["H"], 3, 1.0,
                                        1, 2, 3, None)

    inside = C.c_void_p(x.value + 16)  # an output that starts inside the input state
    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_prev=None), dict(out=None),
                dict(n=0), dict(n=-1), dict(n=65536),
                dict(W=18, H=12), dict(W=16, H=10), dict(W=0, H=0), dict(W=16, H=0), dict(W=-16, H=-12), dict(W=16, H=-4),
                dict(W=12, H=16),            # V < 0
                dict(W=28, H=12),            # V > H: three windows would cover a sample
                dict(n=65535, W=65536, H=32768),        # Np = 2^31
                dict(n=40000, W=1 << 20, H=1 << 19),    # Np past 2^31: the product is not formed in 32 bits
                dict(out=x), dict(out=inside),
                dict(noise=None, x=None), dict(win=out, n=0)):   # the optional arguments do not switch the checks off
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(n=65536) == -1 and b"65535" in L.vqvs_last_error()
    assert call(W=28, H=12) == -1 and b"overlap" in L.vqvs_last_error()
    assert call(out=x) == -1 and b"overlap x" in L.vqvs_last_error()
    assert call(x=None) == -1 and b"non-NULL" in L.vqvs_last_error()


def test_plan_windows():
    assert plan_windows(5000, 2048, 1536) == (3, 5120)
    for N in (1, 100, 2047, 2048):
        assert plan_windows(N, 2048, 1536) == (1, 2048)
    assert plan_windows(2049, 2048, 1536) == (2, 3584)              # N = W + 1: one more window
    assert plan_windows(3584, 2048, 1536) == (2, 3584) and plan_windows(3585, 2048, 1536) == (3, 5120)
    assert plan_windows(4096, 2048, 2048) == (2, 4096) and plan_windows(4097, 2048, 2048) == (3, 6144)  # hop = window: no overlap
    assert plan_windows(1000, 512, 256) == (3, 1024)                # overlap = hop
    for N, W, H in ((5000, 2048, 1536), (64001, 64000, 57600), (12345, 512, 256), (777, 256, 256)):
        n, padded = plan_windows(N, W, H)
        assert padded == (n - 1) * H + W >= N and (n == 1 or padded - H < N)  # the windows cover N, and the last one is needed
    for N, W, H in ((0, 2048, 1536), (-5, 2048, 1536), (5000, 2050, 1536), (5000, 2048, 1538), (5000, 0, 0), (5000, 2048, 0),
                    (5000, -2048, -1536), (5000, 1536, 2048), (5000, 2048, 1020), (5000, 2048, 512),
                    (2 ** 31, 64000, 57600), (65536 * 256, 256, 256), (2 ** 31 - 100, 1 << 20, 1 << 20)):
        with pytest.raises(ValueError):
            plan_windows(N, W, H)


MODES = (("plain", {}), ("sigma_large", dict(sigma_large=True)), ("constrain", dict(constrain=True)))


@pytest.mark.parametrize("schedule", ["exp", "cos"])
def test_oracle_at_one_window_is_the_reference_step(schedule):
    """At n = 1 the numpy oracle is `ref_cpu.ddpm_previous` up to the float32 rounding of two operation orders (the oracle's is the
    kernel's: reciprocal square roots as 1 / sqrt, c2 = betas / sqrt(1 - a_t) formed first).  Bound: 2e-6 * max(1, max |want|).  The
    longest chain (constrain) has about 16 float32 roundings of 2^-24 = 6e-8 each on quantities no larger than max |want| times the
    factors sqrt(a_t) / sqrt(1 - a_t) and c1 c2, which are below 1.3 at these t: 16 * 6e-8 * 1.3 = 1.3e-6 if every rounding had the
    same sign, and the two sides share most of them.  It is also the project's gate for this arithmetic (test_ddpm_previous_vs_golden)."""
    W = 4352
    x, eps, noise = seeded((1, 1, W), 1), seeded((1, 1, W), 2), seeded((1, 1, W), 3)
    for t, step in ((0.6, 0.02), (0.3, 0.02)):
        ts = torch.tensor([t], dtype=torch.float32)
        a_t = ref_cpu.schedule_alpha(schedule, ts).item()
        a_prev = ref_cpu.schedule_alpha(schedule, ts - step).item()
        for mode, kw in MODES:
            want = ref_cpu.ddpm_previous(schedule, x, ts, step, eps, noise, **kw).reshape(-1).numpy()
            got, win = longform_ref.step_windows(x.numpy(), eps.numpy(), noise.numpy(), a_t, a_prev, 1, W, W, **kw)
            err, bound = np.abs(got - want).max(), 2e-6 * max(1.0, np.abs(want).max())
            print(f"oracle vs ref_cpu {schedule} t={t} {mode}: max abs err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (schedule, t, mode, err, bound)
            assert np.array_equal(win, got[None])


@pytest.mark.parametrize("flags", [dict(), dict(constrain=True), dict(sigma_large=True, constrain=True)])
def test_oracle_without_overlap_is_independent_steps(flags):
    n, W = 3, 4352
    x, eps, noise = (seeded((n * W,), s).numpy() for s in (4, 5, 6))
    got, win = longform_ref.step_windows(x, eps, noise, 0.3, 0.35, n, W, W, **flags)
    for b in range(n):
        sl = slice(b * W, (b + 1) * W)
        one, _ = longform_ref.step_windows(x[sl], eps[sl], noise[sl], 0.3, 0.35, 1, W, W, **flags)
        assert np.array_equal(got[sl], one) and np.array_equal(win[b], one)


@pytest.mark.parametrize("constrain", [False, True])
def test_oracle_blend_runs_from_the_left_window_to_the_right(constrain):
    """Inside an overlap the step is the left window's own step at u -> 0 and the right window's at u -> V - 1: with w = (u + 1/2) / V
    the other side's share is 1 / (2 V) of the two predictions' difference, and the weights rise linearly in between."""
    n, W, H = 2, 2048, 1024
    V, Np = longform_ref.geometry(n, W, H)
    x, noise = seeded((Np,), 7, 0.5).numpy(), seeded((Np,), 8).numpy()
    eps = seeded((n, W), 9).numpy()  # two unrelated predictions of the overlap (a constant offset would leave with the window's mean)
    a_t, a_prev = 0.9, 0.95  # (x0 = 1.05 x - 0.33 eps: few samples reach the clamp, where the two windows' predictions would meet)
    got, win = longform_ref.step_windows(x, eps, noise, a_t, a_prev, n, W, H, constrain=constrain)
    k = longform_ref.step_coef(a_t, a_prev, False)
    eb = longform_ref.window_eps(k, longform_ref.window_view(x, n, W, H), eps, constrain)
    alone = [k["c1"] * (x[b * H:b * H + W] - k["c2"] * eb[b]) + k["sig"] * noise[b * H:b * H + W] for b in range(n)]
    left, right, mid = alone[0][H:], alone[1][:V], got[H:H + V]
    gap = np.abs(left - right)
    scale = float(k["c1"] * k["c2"])
    # the inputs make the windows disagree, at the two ends too: the comparisons below would pass trivially otherwise
    assert gap.mean() > 0.5 * scale and min(gap[0], gap[V - 1]) > 0.1 * scale
    for u, near, far in ((0, left, right), (V - 1, right, left)):
        assert abs(mid[u] - near[u]) <= gap[u] / (2 * V) * 1.001 + 1e-6 and abs(mid[u] - far[u]) >= gap[u] * (1 - 1 / V)
    w = (np.arange(V) + 0.5) / V
    assert np.abs(mid - ((1 - w) * left + w * right)).max() <= 4e-6 * max(1.0, np.abs(got).max())
    # outside the overlap each window stands alone, and both rows of the window output carry the blended samples
    assert np.array_equal(got[:H], alone[0][:H]) and np.array_equal(got[W:], alone[1][V:])
    assert np.array_equal(win[0], got[:W]) and np.array_equal(win[1], got[H:])


def test_script_flags():
    import sample_vqvae

    old = ["--sample-rate", "--sample-steps", "--seconds", "--label", "--input-file", "--encoding", "--enc-pred-path", "--enc-pred-scale",
           "--no-vq", "--check-vq", "--seed", "--precision", "checkpoint_path", "output_file"]
    assert flags_of(sample_vqvae.arg_parser()) == sorted(old + ["--whole-file", "--window-seconds", "--overlap-seconds", "--window-batch"])
    a = sample_vqvae.arg_parser().parse_args(["--label", "2", "--input-file", "in.wav", "ck.pt", "out.wav"])
    assert (a.sample_rate, a.sample_steps, a.seconds, a.label, a.input_file, a.encoding, a.enc_pred_path, a.enc_pred_scale, a.no_vq,
            a.check_vq, a.seed, a.precision, a.checkpoint_path, a.output_file) == \
        (16000, 100, 4, 2, "in.wav", "linear", None, 1.0, False, False, None, "fp32", "ck.pt", "out.wav")
    assert (a.whole_file, a.window_seconds, a.overlap_seconds, a.window_batch) == (False, None, 0.4, 64)
    assert round(a.overlap_seconds * a.sample_rate) == 6400 and 6400 % 256 == 0 and 6400 % 1280 == 0
    a = sample_vqvae.arg_parser().parse_args(["--whole-file", "--window-seconds", "2.56", "--overlap-seconds", "0.32", "--window-batch", "8",
                                              "--label", "0", "--input-file", "in.wav", "ck.pt", "out.wav"])
    assert (a.whole_file, a.window_seconds, a.overlap_seconds, a.window_batch) == (True, 2.56, 0.32, 8)
