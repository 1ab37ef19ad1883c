"""F0 scoring on the device: `vqvs_pitch_distance` against the reference of tests/pitch_ref.py over six input families x three
pairings x three configurations x seven lengths (both sides of the kernel's 4-frame workgroup seam among them), its exact
properties, the `PitchDistance` wrapper, and `eval_conversion.py --pitch` as a child process on one rank and on two.

The gates.  `period_a` and `period_b` are BITWISE the reference's for every frame of every case: the definition is exact integers,
one IEEE division and a fixed sequence of float64 operations, so no frame may differ.  `counts` are equal as integers.  `sums`, per
clip: |got - ref| <= (n + 20) 2^-53 sum|term|, n the clip's frames voiced in both signals, the terms l_f and l_f^2: n covers the
n - 1 sequential additions, 20 the roundings inside a term -- the device's log2 taken as within 2 ulp and the host's within 1 (an
assumption: no accuracy table of the device math library is at hand here to check it against), the division hi / lo, the factor
12 and the squaring, each doubled for l_f^2.  The reference alone is the yardstick; where a clip's b is its a both sums are
exactly +0.0.  The fraction of the bound used is recorded per case (profiles/pitch_margins.jsonl is a run's record).

Measured on MI355X: no frame of the 378 cases differs from the reference; of the 756 sum records (the clip nearest its bound per
case and sum) the worst uses 0.106 of its bound, and 85 differ from the `math.fsum` reference at all."""
import itertools
import re

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import PitchDistance, SpectralDistance, _native, create_data_loader

import pitch_ref as pr
from test_conversion_eval_gpu import BASE, FLOAT, vqvae32
from util import record_margin, run_script, sample_lines

pytestmark = pytest.mark.gpu

SENTINEL = -(1 << 40)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def pitch_call(a, b, cfg, *, period_a=True, period_b=True, counts=True, sums=True, threshold=pr.THRESHOLD):
    """The C entry point on [B, T] device tensors; float outputs start as NaN and counts as a sentinel: an unwritten one shows."""
    B, T = a.shape
    F = T // cfg[1] + 1
    nan = lambda *shape: torch.full(shape, float("nan"), device=a.device, dtype=torch.float64)  # noqa: E731
    out = {"period_a": nan(B, F) if period_a else None, "period_b": nan(B, F) if period_b else None,
           "counts": torch.full((B, 4), SENTINEL, device=a.device, dtype=torch.int64) if counts else None, "sums": nan(B, 2) if sums else None}
    _native.check(_native.lib().vqvs_pitch_distance(a.data_ptr(), _native._ptr(b), _native._ptr(out["period_a"]), _native._ptr(out["period_b"]),
                                                    _native._ptr(out["counts"]), _native._ptr(out["sums"]), B, T, cfg[0], cfg[1], cfg[2], cfg[3],
                                                    threshold, _native._stream_ptr()))
    return out


def bits(t):
    return t.cpu().contiguous().view(torch.int64).numpy() if torch.is_tensor(t) else np.ascontiguousarray(t).view(np.int64)


def same_bits(x, y):
    return all((x[k] is None and y[k] is None) or np.array_equal(bits(x[k]), bits(y[k])) for k in x)


# ---------------------------------------------------------------- the kernel against the reference
@pytest.mark.parametrize("length_index", range(7))
@pytest.mark.parametrize("cfg", pr.CONFIGS)
def test_kernel_vs_reference(dev, cfg, length_index):
    T = pr.lengths(cfg)[length_index]
    failures = []
    for family, pairing in itertools.product(pr.FAMILIES, pr.PAIRINGS):
        c = pr.case(family, T, cfg, pairing)
        a = c.a.to(dev).contiguous()
        b = a if pairing == "same" else c.b.to(dev).contiguous()
        got = pitch_call(a, b, cfg)
        for name, want in (("period_a", c.period_a), ("period_b", c.period_b)):
            g = got[name].cpu().numpy()
            differ = int((bits(g) != bits(want)).sum())
            if differ:
                failures.append((family, pairing, name, f"{differ} of {want.size} frames differ",
                                 float(np.abs(g - want).max())))
        if not np.array_equal(got["counts"].cpu().numpy(), c.counts):
            failures.append((family, pairing, "counts", got["counts"].tolist(), c.counts.tolist()))
        s = got["sums"].cpu().numpy()
        bound = (c.n[:, None] + pr.SUM_FACTOR) * 2.0 ** -53 * c.abs
        err = np.abs(s - c.sums)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        for k, out in enumerate(("shift_sum", "shift_sq_sum")):
            clip = int(np.argmax(ratio[:, k]))
            record_margin("pitch_margins.jsonl", {
                "test": f"window={cfg[0]} hop={cfg[1]} tau={cfg[2]}..{cfg[3]} T={T} {family} {pairing} {out} (clip nearest its bound)",
                "frames": c.frames, "clip": clip, "voiced_both": int(c.n[clip]), "E_gpu": float(err[clip, k]), "bound": float(bound[clip, k]),
                "fraction_of_bound": float(ratio[clip, k])})
        if not (np.isfinite(s).all() and (err <= bound).all()):
            failures.append((family, pairing, "sums", s.tolist(), c.sums.tolist(), bound.tolist()))
        if pairing == "same" and (bits(s) != 0).any():
            failures.append((family, pairing, "sums of b = a are not +0.0", s.tolist()))
    assert not failures, (cfg, T, failures)


# ---------------------------------------------------------------- exact properties
SUBSET = [(pr.CONFIGS[0], 1119), (pr.CONFIGS[0], 1280), (pr.CONFIGS[0], 4000), (pr.CONFIGS[1], 128), (pr.CONFIGS[1], 800), (pr.CONFIGS[2], 2048)]


@pytest.mark.parametrize("cfg,T", SUBSET)
def test_exact_properties(dev, cfg, T):
    for family in ("voiced", "tone_silence_square"):
        c = pr.case(family, T, cfg, "perturb" if family == "voiced" else "roll")
        a, b = c.a.to(dev).contiguous(), c.b.to(dev).contiguous()
        first = pitch_call(a, b, cfg)
        assert not any(torch.isnan(first[k]).any() for k in ("period_a", "period_b", "sums")) and (first["counts"] >= 0).all()
        # b = a, as the same buffer and as an equal copy: sums (0, 0) without a sign bit, no voicing mismatch
        for other in (a, a.clone()):
            zero = pitch_call(a, other, cfg)
            assert (bits(zero["sums"]) == 0).all(), (cfg, T, family)
            assert (zero["counts"][:, 3] == 0).all() and torch.equal(zero["counts"][:, 2], zero["counts"][:, 0])
            assert torch.equal(zero["counts"][:, 1], zero["counts"][:, 0]) and np.array_equal(bits(zero["period_a"]), bits(zero["period_b"]))
        # (b, a): the first sum negated bitwise (where it is not 0), the second equal, the counts swapped
        back = pitch_call(b, a, cfg)
        s, r = first["sums"].cpu(), back["sums"].cpu()
        nonzero = s[:, 0] != 0
        assert np.array_equal(bits(-s[nonzero, 0]), bits(r[nonzero, 0])) and (bits(r[~nonzero, 0]) == 0).all()
        assert np.array_equal(bits(s[:, 1]), bits(r[:, 1]))
        assert torch.equal(back["counts"], first["counts"][:, [1, 0, 2, 3]])
        assert np.array_equal(bits(back["period_a"]), bits(first["period_b"])) and np.array_equal(bits(back["period_b"]), bits(first["period_a"]))
        assert same_bits(pitch_call(a, b, cfg), first)   # run to run
        # the last clip alone, at row 0 of the batch, and where it was
        last = a.shape[0] - 1
        alone = pitch_call(a[last:].contiguous(), b[last:].contiguous(), cfg)
        front = pitch_call(torch.cat([a[last:], a[:last]]).contiguous(), torch.cat([b[last:], b[:last]]).contiguous(), cfg)
        for res in (alone, front):
            assert all(np.array_equal(bits(res[k][0]), bits(first[k][last])) for k in first), (cfg, T, family)
        # each NULL-output combination leaves the other outputs bitwise what they were
        names = ("period_a", "period_b", "counts", "sums")
        for keep in itertools.product((False, True), repeat=4):
            if not any(keep):
                continue
            part = pitch_call(a, b, cfg, **dict(zip(names, keep)))
            for name, kept in zip(names, keep):
                assert (part[name] is None) == (not kept)
                assert not kept or np.array_equal(bits(part[name]), bits(first[name])), (cfg, T, family, keep, name)
        # the same samples 1, 2 and 3 floats off a 16-byte boundary (the staging takes 16-byte loads where the address allows)
        for off in (1, 2, 3):
            moved = [torch.cat([x.new_zeros(off), x.flatten()])[off:].view_as(x) for x in (a, b)]
            assert all(m.data_ptr() % 16 == 4 * off and m.is_contiguous() for m in moved)
            assert same_bits(pitch_call(moved[0], moved[1], cfg), first), (cfg, T, family, off)
        only_a = pitch_call(a, None, cfg, period_b=False, counts=False, sums=False)   # b = NULL: the same period_a
        assert np.array_equal(bits(only_a["period_a"]), bits(first["period_a"]))


def test_last_clip_of_a_batch_beyond_2_to_31_samples(dev):
    """33 clips of 2^26 samples: the last clip starts at element 2^31 of the input, and its results are bitwise those of the clip
    alone (a 32-bit element offset would read another place); the silent clips in front of it are unvoiced in every frame."""
    cfg, B, T = pr.CONFIGS[0], 33, 1 << 26
    F = T // cfg[1] + 1
    t = torch.arange(T, device=dev, dtype=torch.float64) / T
    phase = 2 * np.pi * torch.cumsum(110.0 * 3.0 ** t, 0) / pr.SAMPLE_RATE   # a 110 -> 330 Hz glide, three partials
    clip = (0.5 * (torch.sin(phase) + torch.sin(2 * phase) / 2 + torch.sin(3 * phase) / 3) / (1 + 1 / 2 + 1 / 3)).float()
    del t, phase
    a = torch.zeros(B, T, device=dev)
    a[B - 1] = clip
    assert a.numel() > 1 << 31
    got = pitch_call(a, a, cfg, period_b=False)
    alone = pitch_call(a[B - 1:], a[B - 1:], cfg, period_b=False)
    assert got["period_a"].shape == (B, F) and not torch.isnan(got["period_a"]).any()
    for k in ("period_a", "counts", "sums"):
        assert np.array_equal(bits(got[k][B - 1]), bits(alone[k][0])), k
    assert alone["counts"][0, 0] > 0.95 * F and alone["counts"][0, 3] == 0 and (bits(alone["sums"]) == 0).all()
    assert not got["period_a"][:B - 1].any() and not got["counts"][:B - 1].any() and (bits(got["sums"]) == 0).all()


# ---------------------------------------------------------------- wrapper
def test_wrapper_returns_what_the_raw_call_returns(dev):
    cfg, T = pr.CONFIGS[0], 4000
    c = pr.case("voiced", T, cfg, "roll")
    a, b = c.a.to(dev), c.b.to(dev)
    d = PitchDistance()
    assert (d.window, d.hop, d.tau_min, d.tau_max, d.threshold) == cfg + (pr.THRESHOLD,)
    raw = pitch_call(a, b, cfg)
    keys = {"voiced_a", "voiced_b", "voiced_both", "vuv", "shift_sum", "shift_sq_sum", "frames"}

    def check(out):
        assert set(out) == keys and out["frames"] == T // 160 + 1 == c.frames
        for i, k in enumerate(("voiced_a", "voiced_b", "voiced_both", "vuv")):
            assert out[k].dtype == torch.int64 and out[k].shape == (4,) and torch.equal(out[k], raw["counts"][:, i])
        for i, k in enumerate(("shift_sum", "shift_sq_sum")):
            assert out[k].dtype == torch.float64 and np.array_equal(bits(out[k]), bits(raw["sums"][:, i]))

    check(d(a, b))
    check(d(a[:, None], b[:, None]))
    wide = torch.stack([a, b], dim=2)  # [4, T, 2]: a non-contiguous view is taken as what it shows
    check(d(wide[:, :, 0], wide[:, :, 1]))
    for x in (a, a[:, None], wide[:, :, 0]):
        tr = d.track(x)
        assert set(tr) == {"period", "f0"} and tr["period"].shape == (4, c.frames) and tr["f0"].dtype == torch.float64
        assert np.array_equal(bits(tr["period"]), bits(raw["period_a"])) and np.array_equal(bits(tr["period"]), bits(c.period_a))
        voiced = tr["period"] > 0
        assert torch.equal(tr["f0"][voiced], 16000 / tr["period"][voiced]) and (tr["f0"][~voiced] == 0).all()
    small = PitchDistance(window=64, hop=16, fmin=400.0, fmax=4000.0)
    assert (small.tau_min, small.tau_max) == pr.CONFIGS[1][2:]
    assert np.array_equal(bits(small.track(a)["period"]), bits(pitch_call(a, b, pr.CONFIGS[1])["period_a"]))
    for x, y in ((a, b.cpu()), (a.cpu(), b), (a.cpu(), b.cpu())):  # no CPU path, for either argument
        with pytest.raises(_native.NativeError):
            d(x, y)
    with pytest.raises(_native.NativeError):
        d.track(a.cpu())


# ---------------------------------------------------------------- the script
SIGNED = r"-?\d+\.\d{6}"
LINE = re.compile(rf"^(\d+) samples: code_match=({FLOAT}) mcd=({FLOAT}) lsd=({FLOAT})"
                  rf"(?: ref_code_match=({FLOAT}) ref_mcd=({FLOAT}) ref_lsd=({FLOAT}) gap_mcd=({FLOAT}) gap_lsd=({FLOAT}))?"
                  rf" f0_shift=({SIGNED}) f0_dev=({FLOAT}) vuv_err=({FLOAT}) voiced=({FLOAT})"
                  rf"(?: ref_f0_shift=({SIGNED}) ref_f0_dev=({FLOAT}) ref_vuv_err=({FLOAT}) gap_f0_dev=({FLOAT}) gap_vuv_err=({FLOAT}))?$")


def in_process(model, argv, dev):
    import eval_conversion

    run = eval_conversion.parse_args(argv)
    assert run.pitch
    loader, _ = create_data_loader("tones", batch_size=2, seed=1)
    state = eval_conversion.EvalState(reference=run.reference_steps is not None, same=run.target == "same", pitch=True)
    distance, pitch = SpectralDistance(), PitchDistance()
    for i, batch in zip(range(2), loader):
        state.add_batch(model, distance, batch["samples"][:, None].to(dev), batch["label"].to(dev), 2 * i, 1, run, pitch=pitch)
    return state, eval_conversion.format_line(state.num_samples, state.log_dict())


def test_eval_conversion_script_with_pitch(tmp_path, dev):
    from test_conversion_eval_gpu import LINE as PLAIN, in_process as plain_in_process

    model = vqvae32()
    ckpt = tmp_path / "vqvae32.pt"
    model.save(str(ckpt))
    args = [str(ckpt)] + BASE + ["--pitch"]
    lines = sample_lines(run_script("eval_conversion.py", args))
    assert len(lines) == 2
    for n, ln in zip((2, 4), lines):
        m = LINE.match(ln)
        assert m and int(m.group(1)) == n and m.group(5) is None and m.group(14) is None, ln
        for group in (12, 13):  # vuv_err * frames and voiced * frames are counts
            count = float(m.group(group)) * n * 401
            assert abs(count - round(count)) <= 1e-6 * n * 401 and 0 <= round(count) <= n * 401, ln
    state, line = in_process(model.to(dev).set_precision("fp32"), args, dev)
    assert lines[-1] == line and (state.num_samples, state.frames) == (4, 4 * 401)
    assert state.counts["voiced"] > 0   # the data set is tones
    assert sample_lines(run_script("eval_conversion.py", args, ranks=2)) == lines[-1:]  # one merged line, the one a single rank ends with
    # without the flag: today's line (the script itself runs so in test_conversion_eval_gpu.py), the prefix of the new one
    _, plain = plain_in_process(model, args[:-1], dev)
    assert PLAIN.match(plain) and lines[-1].startswith(plain + " f0_shift=")


def test_eval_conversion_script_with_pitch_and_reference(tmp_path, dev):
    model = vqvae32()
    ckpt = tmp_path / "vqvae32.pt"
    model.save(str(ckpt))
    # the reference run repeats the first one: same sampler, steps, codes, labels and x_T
    args = [str(ckpt)] + BASE + ["--pitch", "--target", "same", "--reference-steps", "2", "--reference-sampler", "ddpm"]
    lines = sample_lines(run_script("eval_conversion.py", args))
    assert len(lines) == 2
    for n, ln in zip((2, 4), lines):
        m = LINE.match(ln)
        assert m and int(m.group(1)) == n and m.group(5) is not None, ln
        assert (m.group(14), m.group(15), m.group(16)) == (m.group(10), m.group(11), m.group(12))  # ref_* are the unprefixed values
        assert (m.group(17), m.group(18)) == ("0.000000", "0.000000")                              # gap_f0_dev, gap_vuv_err
    state, line = in_process(model.to(dev).set_precision("fp32"), args, dev)
    assert lines[-1] == line and state.sums["gap_f0_s1"] == 0 and state.counts["gap_vuv"] == 0
