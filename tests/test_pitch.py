"""F0 scoring, host side: the export and every argument refusal of `vqvs_pitch_distance` and of `PitchDistance`, the reference's
analytic checks and exactness conditions (tests/pitch_ref.py), the mutants the device test's gates must reject, and
eval_conversion.py's state, line and flag with `--pitch` (none of this needs a device)."""
import ctypes as C
import itertools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import vq_voice_swap_amd
from vq_voice_swap_amd import PitchDistance, _native

import pitch_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["const float* a", "const float* b", "double* period_a", "double* period_b", "long long* counts", "double* sums", "int B", "int T",
        "int window", "int hop", "int tau_min", "int tau_max", "double threshold", "void* stream"]


def test_symbol_is_exported_and_declared(lib_built):
    assert "vqvs_pitch_distance" in _native.EXPORTS and hasattr(lib_built, "vqvs_pitch_distance")
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    decl = re.search(r"int vqvs_pitch_distance\(([^;]*)\);", header)
    assert decl, "include/vqvs.h does not declare vqvs_pitch_distance"
    assert [a.strip() for a in " ".join(decl.group(1).split()).split(",")] == ARGS
    assert len(lib_built.vqvs_pitch_distance.argtypes) == len(ARGS)
    assert "PitchDistance" in vq_voice_swap_amd.__all__ and vq_voice_swap_amd.PitchDistance is PitchDistance
    from vq_voice_swap.pitch import PitchDistance as shim  # the import-path shim

    assert shim is PitchDistance


def test_entry_point_refuses_bad_arguments_without_a_device(lib_built):
    """Every refusal of include/vqvs.h with host-only pointers: a call that reached the device would fault on them, so VQVS_ERR_ARG
    proves it did not.  (The accepted argument set itself is never sent: it is what the device tests send.)"""
    L = lib_built
    sizes = dict(a=2 * 64 * 4, b=2 * 64 * 4, period_a=2 * 9 * 8, period_b=2 * 9 * 8, counts=2 * 32, sums=2 * 16)
    keep = {k: (C.c_char * n)() for k, n in sizes.items()}
    ptr = {k: C.cast(v, C.c_void_p) for k, v in keep.items()}
    ok = dict(ptr, B=2, T=64, window=16, hop=8, tau_min=2, tau_max=8, threshold=0.15)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_pitch_distance(a["a"], a["b"], a["period_a"], a["period_b"], a["counts"], a["sums"], a["B"], a["T"], a["window"], a["hop"],
                                     a["tau_min"], a["tau_max"], a["threshold"], None)

    inside = lambda name, off=8: C.c_void_p(ptr[name].value + off)  # noqa: E731
    none = dict(period_a=None, period_b=None, counts=None, sums=None)
    bad = [dict(a=None), dict(none),
           # b = NULL: only period_a may, and must, be asked for
           dict(b=None), dict(none, b=None), dict(none, b=None, period_a=ptr["period_a"], period_b=ptr["period_b"]),
           dict(none, b=None, period_a=ptr["period_a"], counts=ptr["counts"]), dict(none, b=None, period_a=ptr["period_a"], sums=ptr["sums"]),
           dict(B=0), dict(B=-1), dict(B=65536),
           dict(T=0), dict(T=-64), dict(T=(1 << 30) + 1),
           dict(window=15), dict(window=0), dict(window=-16), dict(window=2049),
           dict(hop=0), dict(hop=-8), dict(hop=17),
           dict(tau_min=1), dict(tau_min=0), dict(tau_min=-2), dict(tau_min=8), dict(tau_min=9),
           dict(tau_max=2), dict(tau_max=1024), dict(tau_max=0), dict(tau_max=-8),
           dict(window=2048, tau_max=513), dict(window=1026, tau_max=1023),   # window * tau_max > 2^20
           dict(threshold=0.0), dict(threshold=-0.1), dict(threshold=1.0000001), dict(threshold=float("inf")), dict(threshold=float("nan")),
           # an output inside an input or another output
           dict(period_a=inside("a")), dict(period_b=inside("b")), dict(counts=inside("a")), dict(sums=inside("b", 2 * 64 * 4 - 8)),
           dict(period_b=ptr["period_a"]), dict(counts=inside("period_a")), dict(sums=inside("counts")), dict(sums=inside("period_b", 0)),
           # outputs may be NULL: everything else is still checked
           dict(none, sums=ptr["sums"], B=0), dict(none, period_a=ptr["period_a"], b=None, T=0), dict(period_b=None, a=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.vqvs_last_error(), kw
    for kw, text in ((dict(B=65536), b"65535"), (dict(T=(1 << 30) + 1), b"2^30"), (dict(window=2049), b"window=2049"), (dict(hop=17), b"hop=17"),
                     (dict(tau_min=1), b"tau_min=1"), (dict(tau_max=1024), b"tau_max=1024"), (dict(window=2048, tau_max=513), b"2^20"),
                     (dict(threshold=0.0), b"threshold"), (dict(threshold=float("nan")), b"threshold=nan"), (dict(none), b"nothing to compute"),
                     (dict(a=None), b"non-NULL"), (dict(b=None), b"b is NULL"), (dict(none, b=None), b"period_a must be given"),
                     (dict(period_b=ptr["period_a"]), b"overlap")):
        assert call(**kw) == -1 and text in L.vqvs_last_error(), (kw, L.vqvs_last_error())


def test_wrapper_checks_raise_before_a_device():
    d = PitchDistance()
    assert (d.sample_rate, d.window, d.hop, d.tau_min, d.tau_max, d.threshold) == (16000, 400, 160, 32, 266, 0.15)
    assert (d.window, d.hop, d.tau_min, d.tau_max) == pr.CONFIGS[0] and d.frames(64000) == 401 and d.frames(1119) == 7 and d.frames(1) == 1
    e = PitchDistance(sample_rate=22050, fmin=70.0, fmax=441.0)
    assert (e.tau_min, e.tau_max) == (50, 315)   # ceil and floor
    x = torch.zeros(2, 1, 800)
    for a, b in ((x, torch.zeros(2, 1, 801)), (x, torch.zeros(3, 1, 800)), (x[:, 0], x),       # shapes differ
                 (x.double(), x.double()), (x, x.half()), (x.int(), x.int()),                 # dtypes
                 (torch.zeros(800), torch.zeros(800)), (torch.zeros(2, 2, 800), torch.zeros(2, 2, 800)),  # ranks
                 (torch.zeros(0, 1, 800), torch.zeros(0, 1, 800)), (torch.zeros(2, 1, 0), torch.zeros(2, 1, 0)), (x, x.numpy())):
        with pytest.raises(ValueError):
            d(a, b)
    for t in (x.double(), torch.zeros(800), torch.zeros(2, 2, 800), torch.zeros(2, 0), x.numpy()):
        with pytest.raises(ValueError):
            d.track(t)
    for a, b in ((x, x), (x[:, 0], x[:, 0])):  # nothing left to object to but the device: there is no CPU path
        with pytest.raises(_native.NativeError):
            d(a, b)
        with pytest.raises(_native.NativeError):
            d.track(a)
    for kw in (dict(window=15), dict(window=2049), dict(hop=0), dict(hop=401), dict(fmin=15.0), dict(fmax=16001.0), dict(fmin=500.0), dict(fmin=600.0),
               dict(fmin=0.0), dict(fmin=-60.0), dict(fmax=float("inf")), dict(fmin=float("nan")), dict(sample_rate=0), dict(window=2048, fmin=30.0),
               dict(threshold=0.0), dict(threshold=1.5), dict(threshold=float("nan")), dict(fmin=490.0, fmax=500.0)):
        with pytest.raises(ValueError):
            PitchDistance(**kw)


# ---------------------------------------------------------------- the reference
def test_reference_quantisation_and_framing():
    x = np.array([0.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 1.0, -1.0, 1.2, -1.2, np.nan, np.inf, -np.inf,
                  3.4e38, 1e-45], dtype=np.float32)
    assert pr.quantise(x).tolist() == [0, 0, 2, 2, 0, -2, 32767, -32768, 32767, -32768, 0, 32767, -32768, 32767, 0]   # half to even
    assert pr.quantise(x, "truncate").tolist()[:6] == [0, 0, 1, 2, 0, -1] and pr.quantise(x, "clamp_32768")[6] == 32768
    # d against a plain double loop, frame placement included: frame f reads q[f hop - S // 2 ...), zeros outside the clip
    cfg = (16, 8, 2, 9)
    q = np.random.default_rng(0).integers(-32768, 32768, (2, 50))
    d = pr.difference(q, cfg)
    assert d.shape == (2, 50 // 8 + 1, 10) and d.dtype == np.int64 and (d[..., 0] == 0).all()
    S = 16 + 9
    at = lambda b, n: int(q[b, n]) if 0 <= n < 50 else 0  # noqa: E731
    for b, f, tau in itertools.product(range(2), range(7), range(1, 10)):
        s = f * 8 - S // 2
        assert d[b, f, tau] == sum((at(b, s + j) - at(b, s + j + tau)) ** 2 for j in range(16))


def test_reference_analytic_periods():
    """The 440 Hz tone and the 100 Hz square of mfcc_ref.make_batch within 0.1 % of the true period; noise, silence, the 1e-3
    noise and the full-scale levels unvoiced in every frame; a non-finite sample costs no frame its voicing."""
    cfg, T = pr.CONFIGS[0], 9600
    tone, silence, square = pr.tracked("tone_silence_square", T, cfg, False)
    for track, true in ((tone, 16000 / 440), (square, 160.0)):
        voiced = track[track > 0]
        assert voiced.size >= 0.9 * track.size and abs(np.median(voiced) - true) <= 1e-3 * true, (true, np.median(voiced))
    assert not silence.any() and not pr.tracked("noise", T, cfg, False).any() and not pr.tracked("fullscale", T, cfg, False).any()
    loud, quiet, tone2 = pr.tracked("loud_quiet_tone", T, cfg, False)
    assert not loud.any() and not quiet.any() and np.array_equal(tone2, tone)
    bad, clean = pr.tracked("nonfinite", T, cfg, False)
    assert ((bad > 0) == (clean > 0)).all() and abs(np.median(bad[bad > 0]) - 16000 / 220) <= 1e-3 * 16000 / 220
    assert 0 < (bad != clean).sum() <= 12   # the frames that hold one of the three samples


def test_reference_three_semitone_glide():
    """A five-harmonic glide from 110 to 330 Hz against the same glide 3 semitones higher: the mean distance within 0.05 semitone
    of 3, the deviation around it below 0.1, and antisymmetry bitwise."""
    cfg, T = pr.CONFIGS[0], 16000
    a, b = (pr.track(pr.glide(T, 110.0, 330.0, st).astype(np.float32)[None], cfg) for st in (0.0, 3.0))
    ab, ba = pr.compare(a, b), pr.compare(b, a)
    n = int(ab["n"][0])
    assert n >= 0.95 * a.size and ab["counts"][0, 3] == 0
    s1, s2 = ab["sums"][0]
    assert abs(s1 / n - 3.0) <= 0.05 and math.sqrt(s2 / n - (s1 / n) ** 2) < 0.1, (s1 / n, math.sqrt(s2 / n - (s1 / n) ** 2))
    assert ba["sums"][0, 0] == -s1 and ba["sums"][0, 1] == s2 and (ba["counts"][0] == ab["counts"][0][[1, 0, 2, 3]]).all()
    same = pr.compare(a, a)
    assert same["sums"].view(np.int64).tolist() == [[0, 0]] and same["counts"][0, 3] == 0 and same["n"][0] == ab["counts"][0, 0]


# (the second configuration searches 400 .. 4000 Hz: of all the clips only the 440 Hz tone has its period there)
MUTANT_CASES = [(pr.CONFIGS[0], 4000, "voiced"), (pr.CONFIGS[0], 1280, "voiced"), (pr.CONFIGS[1], 800, "tone_silence_square"), (pr.CONFIGS[2], 4000, "voiced")]


@pytest.mark.parametrize("cfg", pr.CONFIGS)
def test_shared_cases_hold_the_exactness_conditions(cfg):
    """Every case of the device test builds (the reference asserts d, d tau and c below 2^53 as it goes); the periods are 0 or lie
    in [tau_min - 1, tau_max + 1]; b = a gives sums of exactly +0.0; the tones are voiced, the noises are not, and the clamp binds in the voiced family."""
    voiced_frames = {}
    for T, family, pairing in itertools.product(pr.lengths(cfg), pr.FAMILIES, pr.PAIRINGS):
        c = pr.case(family, T, cfg, pairing)
        assert c.frames == T // cfg[1] + 1 and c.period_a.shape == c.period_b.shape == (c.a.shape[0], c.frames)
        for p in (c.period_a, c.period_b):
            assert p.dtype == np.float64 and (((p >= cfg[2] - 1) & (p <= cfg[3])) | (p == 0)).all()
        assert c.counts.dtype == np.int64 and (c.counts[:, 2] <= np.minimum(c.counts[:, 0], c.counts[:, 1])).all()
        assert (c.counts[:, 0] + c.counts[:, 1] - 2 * c.counts[:, 2] == c.counts[:, 3]).all()
        if pairing == "same":
            assert (c.sums.view(np.int64) == 0).all() and (c.counts[:, 3] == 0).all()
        voiced_frames[family] = voiced_frames.get(family, 0) + int(c.counts[:, 0].sum())
    # (the second configuration searches 400 .. 4000 Hz: of all the clips only the 440 Hz tone has its period there)
    assert voiced_frames["tone_silence_square"] > 0 and (voiced_frames["voiced"] > 0) == (cfg != pr.CONFIGS[1])
    assert voiced_frames["noise"] == 0 and voiced_frames["fullscale"] == 0
    assert (np.abs(pr.make_family("voiced", 4000).numpy()[3]) > 1.0).any()


def test_every_mutant_is_visible_to_the_gates():
    """On shared cases of every configuration: each tracking mutant changes at least one per-frame period (the device test compares
    them bitwise) -- all seven on the voiced family at the default configuration --, and each comparison mutant moves a sum beyond
    the device test's bound with a factor of 100 to spare wherever a clip has a frame voiced in both signals."""
    seen = {m: 0 for m in pr.MUTANTS}
    for cfg, T, family in MUTANT_CASES:
        c = pr.case(family, T, cfg, "perturb")
        assert (c.n > 0).any(), (cfg, T, family)
        changed = {}
        for m in pr.TRACKING_MUTANTS:
            pa, pb, _ = c.mutant(m)
            changed[m] = ((pa != c.period_a).sum(1) + (pb != c.period_b).sum(1)).tolist()
            seen[m] += sum(changed[m]) > 0
        print(f"{cfg} T={T} {family}: frames changed per clip {changed}")
        bound = (c.n[:, None] + pr.SUM_FACTOR) * 2.0 ** -53 * c.abs
        for m in pr.COMPARE_MUTANTS:
            _, _, got = c.mutant(m)
            assert (got["counts"] == c.counts).all()
            moved = np.abs(got["sums"] - c.sums) > 100 * bound
            assert moved[c.n > 0].any(axis=1).all(), (m, got["sums"], c.sums)
            assert m != "sign_flipped" or not moved[:, 1].any()   # the squares do not see the sign
            seen[m] += 1
        if (cfg, T, family) == MUTANT_CASES[0]:   # every tracking mutant is visible on the default configuration
            assert all(sum(v) > 0 for v in changed.values()), changed
            assert sum(changed["clamp_32768"][:3]) == 0 and changed["clamp_32768"][3] > 0   # only the clipped voice reaches the clamp
    assert all(n > 0 for n in seen.values()), seen


# ---------------------------------------------------------------- eval_conversion.py --pitch
PITCH_KEYS = ("f0_n", "f0_s1", "f0_s2", "vuv", "voiced")


def pitch_scores(g, n, reference, frames=401, unvoiced_clip=None):
    """Random per-clip results (test_conversion_eval.batch_scores with the pitch keys); clip `unvoiced_clip` has n_c = 0."""
    from test_conversion_eval import batch_scores

    s = batch_scores(g, n, reference, False, False)
    for p in ("", "ref_", "gap_") if reference else ("",):
        cnt = g.integers(1, frames + 1, n)
        if unvoiced_clip is not None:
            cnt[unvoiced_clip] = 0
        mean, spread = g.normal(0.0, 3.0, n), g.random(n)
        s[p + "f0_n"] = cnt.tolist()
        s[p + "f0_s1"] = np.where(cnt > 0, cnt * mean, 0.0).tolist()
        s[p + "f0_s2"] = np.where(cnt > 0, cnt * (mean ** 2 + spread ** 2), 0.0).tolist()
        s[p + "vuv"], s[p + "voiced"] = g.integers(0, frames + 1, n).tolist(), g.integers(0, frames + 1, n).tolist()
    return s


SIGNED = r"-?\d+\.\d{6}"
TAIL = re.compile(rf" f0_shift=({SIGNED}) f0_dev=(\d+\.\d{{6}}) vuv_err=(\d\.\d{{6}}) voiced=(\d\.\d{{6}})"
                  rf"( ref_f0_shift={SIGNED} ref_f0_dev=\d+\.\d{{6}} ref_vuv_err=\d\.\d{{6}} gap_f0_dev=\d+\.\d{{6}} gap_vuv_err=\d\.\d{{6}})?$")


def test_parse_args_accepts_pitch():
    import eval_conversion

    assert eval_conversion.parse_args(["vqvae.pt", "tones"]).pitch is False
    assert eval_conversion.parse_args(["--pitch", "vqvae.pt", "tones"]).pitch is True
    a = eval_conversion.parse_args(["vqvae.pt", "tones", "--pitch", "--reference-steps", "100", "--sampler", "dpmpp", "--sample-steps", "25"])
    assert (a.pitch, a.reference_steps, a.sampler, a.sample_steps) == (True, 100, "dpmpp", 25)


def test_state_with_pitch_line_and_key_sets():
    import eval_conversion
    from test_conversion_eval import LINE as PLAIN, batch_scores

    g = np.random.default_rng(11)
    st = eval_conversion.EvalState(pitch=True)
    empty = st.log_dict()
    assert list(empty) == ["code_match", "mcd", "lsd", "f0_shift", "f0_dev", "vuv_err", "voiced"] and not any(empty.values())
    assert eval_conversion.format_line(0, empty).endswith(" f0_shift=0.000000 f0_dev=0.000000 vuv_err=0.000000 voiced=0.000000")
    # two clips of 10 frames: l = (1, 3) and (-2, -2, -2) -> shift (4 - 6) / 5, deviation sqrt((10 - 16 / 2 + 12 - 36 / 3) / 5)
    st.add_scores(4, 10, {"code_match": [4, 2], "mcd": [30.0, 50.0], "lsd": [10.0, 15.0], "f0_n": [2, 3], "f0_s1": [4.0, -6.0], "f0_s2": [10.0, 12.0],
                          "vuv": [1, 4], "voiced": [5, 10]})
    line = eval_conversion.format_line(st.num_samples, st.log_dict())
    assert line == ("2 samples: code_match=0.750000 mcd=4.000000 lsd=1.250000 f0_shift=-0.400000 "
                    f"f0_dev={math.sqrt(0.4):.6f} vuv_err=0.250000 voiced=0.750000")
    for reference in (False, True):
        st = eval_conversion.EvalState(reference=reference, pitch=True)
        st.add_scores(250, 401, pitch_scores(g, 3, reference))
        line = eval_conversion.format_line(st.num_samples, st.log_dict())
        m = TAIL.search(line)
        assert m and (m.group(5) is not None) == reference and PLAIN.match(line[:m.start()]), line
        for wrong in (batch_scores(g, 3, reference, False, False), pitch_scores(g, 3, not reference),   # no pitch keys; the other groups
                      {k: v for k, v in pitch_scores(g, 3, reference).items() if k != "vuv"}):
            with pytest.raises(ValueError):
                st.add_scores(250, 401, wrong)
        plain = eval_conversion.EvalState(reference=reference)   # pitch off: today's key set, and nothing else
        with pytest.raises(ValueError):
            plain.add_scores(250, 401, pitch_scores(g, 3, reference))
        plain.add_scores(250, 401, batch_scores(g, 3, reference, False, False))
        assert PLAIN.match(eval_conversion.format_line(3, plain.log_dict())) and not any("f0" in k or "vuv" in k for k in list(plain.sums) + list(plain.counts))
        with pytest.raises(ValueError):
            plain.merge(eval_conversion.EvalState(reference=reference, pitch=True))
    with pytest.raises(ValueError):   # a pitch state cannot score a batch without its PitchDistance
        eval_conversion.EvalState(pitch=True).add_batch(None, None, None, None, 0, 0, None)


def test_state_with_pitch_is_independent_of_batch_split_and_merge_order():
    import eval_conversion

    g = np.random.default_rng(12)
    scores = pitch_scores(g, 12, True, unvoiced_clip=5)
    scores["f0_n"][0], scores["f0_s1"][0], scores["f0_s2"][0] = 7, 7 * 1.1, 7 * 1.1 ** 2   # all l_f equal: the deviation may round below 0

    def build(cuts, order=None):
        states = []
        for lo, hi in zip((0,) + cuts, cuts + (12,)):
            st = eval_conversion.EvalState(reference=True, pitch=True)
            st.add_scores(250, 401, {k: v[lo:hi] for k, v in scores.items()})
            states.append(st.to_host())
        states = [states[i] for i in (order or range(len(states)))]
        merged = states[0]
        for other in states[1:]:
            merged.merge(other)
        return merged

    base = build(())
    n = sum(scores["f0_n"])
    within = sum(Fraction(q) - Fraction(s) ** 2 / c for c, s, q in zip(scores["f0_n"], scores["f0_s1"], scores["f0_s2"]) if c)
    log = base.log_dict()
    assert base.counts["f0_n"] == n and base.sums["f0_within"] == within and base.sums["f0_s1"] == sum(Fraction(s) for s in scores["f0_s1"])
    assert log["f0_shift"] == float(base.sums["f0_s1"] / n) and log["f0_dev"] == math.sqrt(float(within / n))
    assert log["vuv_err"] == sum(scores["vuv"]) / (12 * 401) and log["voiced"] == sum(scores["voiced"]) / (12 * 401)
    assert log["gap_vuv_err"] == sum(scores["gap_vuv"]) / (12 * 401)
    line = eval_conversion.format_line(base.num_samples, log)
    for cuts, order in (((6,), None), ((1, 2, 3), None), ((5, 6), (2, 0, 1)), ((4, 8), (1, 2, 0)), (tuple(range(1, 12)), tuple(reversed(range(12))))):
        m = build(cuts, order)
        assert m.sums == base.sums and m.counts == base.counts and m.log_dict() == log
        assert eval_conversion.format_line(m.num_samples, m.log_dict()) == line
    only = eval_conversion.EvalState(pitch=True)   # a pass whose only clip has no frame voiced in both: every ratio prints 0
    only.add_scores(250, 401, {"code_match": [1], "mcd": [1.0], "lsd": [1.0], "f0_n": [0], "f0_s1": [0.0], "f0_s2": [0.0], "vuv": [0], "voiced": [0]})
    assert eval_conversion.format_line(1, only.log_dict()).endswith(" f0_shift=0.000000 f0_dev=0.000000 vuv_err=0.000000 voiced=0.000000")
