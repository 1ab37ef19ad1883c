"""Conversion-quality evaluation, host side: the export and every argument refusal of `vqvs_spectral_distance`, the package's
constant tables against the reference's own derivation, the conditions the device test's gate rests on (tests/spectral_ref.py),
the mutants the gate must reject, and eval_conversion.py's state, line and flags (none of this needs a device)."""
import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import vq_voice_swap_amd
from vq_voice_swap_amd import SpectralDistance, VQVAE, _native, spectral_constants

import spectral_ref as sr
from mfcc_ref import FAMILIES, GATE_FACTOR
from util import flags_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["const float* d_a", "const float* d_b", "const float* d_window", "const double* d_twiddle", "const float* d_fb",
        "const float* d_dct", "double* d_mcd", "double* d_lsd", "int B", "int T", "int n_fft", "int hop", "int n_mels", "int n_ceps",
        "float eps", "void* stream"]


def test_symbol_is_exported_and_declared(lib_built):
    assert "vqvs_spectral_distance" in _native.EXPORTS and hasattr(lib_built, "vqvs_spectral_distance")
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    decl = re.search(r"int vqvs_spectral_distance\(([^;]*)\);", header)
    assert decl, "include/vqvs.h does not declare vqvs_spectral_distance"
    assert [a.strip() for a in " ".join(decl.group(1).split()).split(",")] == ARGS
    assert len(lib_built.vqvs_spectral_distance.argtypes) == len(ARGS)
    for name in ("SpectralDistance", "spectral_constants"):
        assert name in vq_voice_swap_amd.__all__ and hasattr(vq_voice_swap_amd, name)
    assert callable(VQVAE.code_agreement)


def test_entry_point_refuses_bad_arguments_without_a_device(lib_built):
    """Every refusal of include/vqvs.h with host-only pointers: a call that reached the device would fault on them, so VQVS_ERR_ARG
    proves it did not.  (The accepted argument set itself is never sent: it is what the device tests send.)"""
    L = lib_built
    sizes = dict(a=2 * 64 * 4, b=2 * 64 * 4, window=16 * 4, twiddle=16 * 16, fb=9 * 128 * 4, dct=128 * 64 * 4, mcd=2 * 8, lsd=2 * 8)
    keep = {k: (C.c_char * n)() for k, n in sizes.items()}
    ptr = {k: C.cast(v, C.c_void_p) for k, v in keep.items()}
    ok = dict(ptr, B=2, T=64, n_fft=16, hop=8, n_mels=4, n_ceps=2, eps=1e-6)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_spectral_distance(a["a"], a["b"], a["window"], a["twiddle"], a["fb"], a["dct"], a["mcd"], a["lsd"], a["B"], a["T"],
                                        a["n_fft"], a["hop"], a["n_mels"], a["n_ceps"], a["eps"], None)

    inside = lambda name, off=8: C.c_void_p(ptr[name].value + off)  # noqa: E731
    bad = [dict(a=None), dict(b=None), dict(window=None), dict(twiddle=None), dict(fb=None), dict(dct=None), dict(mcd=None, lsd=None),
           dict(B=0), dict(B=-1), dict(B=65536),
           dict(T=8), dict(T=0), dict(T=-64), dict(T=(1 << 30) + 1),
           dict(n_fft=17), dict(n_fft=14), dict(n_fft=0), dict(n_fft=514), dict(n_fft=513), dict(n_fft=-16),
           dict(hop=0), dict(hop=-8), dict(hop=17),
           dict(n_mels=0), dict(n_mels=-4), dict(n_mels=129),
           dict(n_ceps=1), dict(n_ceps=0), dict(n_ceps=5), dict(n_ceps=65, n_mels=128), dict(n_ceps=65, n_mels=65),
           dict(eps=0.0), dict(eps=-1e-6), dict(eps=float("inf")), dict(eps=float("nan")),
           # an output inside an input, or the other output
           dict(mcd=inside("a")), dict(lsd=inside("a")), dict(mcd=inside("b", 2 * 64 * 4 - 8)), dict(lsd=inside("b")),
           dict(mcd=inside("window")), dict(lsd=inside("twiddle")), dict(mcd=inside("fb", 0)), dict(lsd=inside("dct", 0)),
           dict(lsd=ptr["mcd"]), dict(mcd=inside("lsd")),
           # one output may be NULL: everything else is still checked
           dict(mcd=None, B=0), dict(lsd=None, T=8), dict(lsd=None, a=None), dict(mcd=None, lsd=inside("a"))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.vqvs_last_error(), kw
    for kw, text in ((dict(B=65536), b"65535"), (dict(T=8), b"reflect"), (dict(n_fft=17), b"n_fft=17"), (dict(hop=17), b"hop=17"),
                     (dict(n_mels=129), b"n_mels=129"), (dict(n_ceps=65, n_mels=128), b"n_ceps=65"), (dict(eps=0.0), b"eps"),
                     (dict(mcd=None, lsd=None), b"both NULL"), (dict(a=None), b"non-NULL"), (dict(lsd=ptr["mcd"]), b"overlap"),
                     (dict(T=(1 << 30) + 1), b"2^30")):
        assert call(**kw) == -1 and text in L.vqvs_last_error(), (kw, L.vqvs_last_error())


def test_wrapper_checks_raise_before_a_device():
    d = SpectralDistance()
    x = torch.zeros(2, 1, 800)
    for a, b in ((x, torch.zeros(2, 1, 801)), (x, torch.zeros(3, 1, 800)), (x[:, 0], x),       # shapes differ
                 (x.double(), x.double()), (x, x.half()), (x.int(), x.int()),                 # dtypes
                 (torch.zeros(800), torch.zeros(800)), (torch.zeros(2, 2, 800), torch.zeros(2, 2, 800)),  # ranks
                 (torch.zeros(2, 1, 200), torch.zeros(2, 1, 200)), (torch.zeros(0, 1, 800), torch.zeros(0, 1, 800))):
        with pytest.raises(ValueError):
            d(a, b)
    for a, b in ((x, x), (x[:, 0], x[:, 0])):  # nothing left to object to but the device: there is no CPU path
        with pytest.raises(_native.NativeError):
            d(a, b)
    for kw in (dict(n_fft=401), dict(n_fft=1024), dict(hop=0), dict(hop=401), dict(n_mels=129), dict(n_ceps=1), dict(n_ceps=41),
               dict(eps=0.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            SpectralDistance(**kw)
    assert d.frames(64000) == 401 and d.frames(1119) == 7


@pytest.mark.parametrize("cfg", sr.CONFIGS)
def test_constants_equal_the_reference_derivation(cfg):
    """The package's tables against tests/spectral_ref.py's own formulation: equal to float32 rounding (one float32 ulp of the
    table's largest entry; measured: bitwise equal), the float64 twiddle table to a few float64 ulps."""
    n_fft, _, n_mels, n_ceps = cfg
    got = spectral_constants(sr.SAMPLE_RATE, n_fft, n_mels, n_ceps)
    win, fb, dct, tw = sr.constants(cfg)
    for name, want in (("window", win), ("fb", fb), ("dct", dct)):
        assert got[name].dtype == np.float32 and got[name].shape == want.shape, name
        assert np.abs(got[name].astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23 * np.abs(want).max(), name
    assert got["twiddle"].dtype == np.float64 and got["twiddle"].shape == (n_fft, 2)
    assert np.abs(got["twiddle"] - tw).max() <= 4 * 2.0 ** -53
    # what the tables are: a periodic Hann window, triangles of height <= 1 that cover the band, orthonormal DCT columns
    assert got["window"][0] == 0.0 and got["window"][n_fft // 2] == 1.0 and np.allclose(got["window"][1:], got["window"][1:][::-1])
    assert got["fb"].min() >= 0.0 and got["fb"].max() <= 1.0 and not got["fb"][0].any()
    assert np.abs(got["dct"].astype(np.float64).T @ got["dct"].astype(np.float64) - np.eye(n_ceps)).max() < 1e-6


@pytest.mark.parametrize("cfg", sr.CONFIGS)
def test_gate_conditions_hold_for_every_case(cfg):
    """For every case of the device test: 8 E_model <= cap, and E_model > 0 unless the clip's b IS its a (then reference, emulation
    and gate are exactly 0: the device must return 0.0)."""
    worst, worst_per_frame = 0.0, 0.0
    for T, family, pairing in itertools.product(sr.lengths(cfg), FAMILIES, sr.PAIRINGS):
        c = sr.case(family, T, cfg, pairing)
        assert c.frames == T // cfg[1] + 1 and c.cap == 1e-3 * c.frames
        same = (c.a == c.b).all(1).numpy()
        assert same.all() == (pairing == "same") or family == "tone_silence_square"
        for out in ("mcd", "lsd"):
            e, ref = c.e_model[out], c.ref[out]
            assert e.shape == ref.shape == (3,) and np.isfinite(ref).all()
            assert (GATE_FACTOR * e <= c.cap).all(), (cfg, T, family, pairing, out, GATE_FACTOR * e / c.cap)
            assert ((e > 0) != same).all(), (cfg, T, family, pairing, out, e, same)
            assert (ref[same] == 0.0).all() and (ref[~same] > 0.0).all()
            assert (c.gate[out] == GATE_FACTOR * e).all()
            worst, worst_per_frame = max(worst, float((GATE_FACTOR * e / c.cap).max())), max(worst_per_frame, float((e / c.frames).max()))
    print(f"{cfg}: largest 8 E_model / cap = {worst:.3f}, largest E_model = {worst_per_frame:.3e} dB per frame")


MUTANT_LENGTHS = (0, 1, 2, 5, 6)  # indices into spectral_ref.lengths: the five short ones


@pytest.mark.parametrize("cfg", sr.CONFIGS)
def test_every_mutant_lies_100_gates_from_the_reference(cfg):
    """The gate rejects each deliberate error with a factor of 100 to spare -- on some clip of the case, in an output the error
    applies to -- on at least three cases of every configuration."""
    hits = {m: 0 for m in sr.MUTANTS}
    cases = 0
    for i, family, pairing in itertools.product(MUTANT_LENGTHS, FAMILIES, ("roll", "perturb")):
        c = sr.case(family, sr.lengths(cfg)[i], cfg, pairing)
        cases += 1
        for m in sr.MUTANTS:
            got = c.mutant(m)
            for out in ("mcd", "lsd"):
                d, gate = np.abs(got[out] - c.ref[out]), c.gate[out]
                if out not in sr.MUTANT_OUTPUTS.get(m, ("mcd", "lsd")):
                    assert (d == 0).all(), (m, out)  # the error does not apply to this output
            if any((np.abs(got[out] - c.ref[out])[c.gate[out] > 0] >= 100 * c.gate[out][c.gate[out] > 0]).any()
                   for out in sr.MUTANT_OUTPUTS.get(m, ("mcd", "lsd"))):
                hits[m] += 1
    print(f"{cfg}: cases rejected with a factor of 100, of {cases}: {hits}")
    assert all(n >= 3 for n in hits.values()), hits


# ---------------------------------------------------------------- eval_conversion.py
def test_script_flags_and_refusals(capsys):
    import eval_conversion
    import eval_vqvae

    common = flags_of(eval_vqvae.arg_parser())
    assert flags_of(eval_conversion.arg_parser()) == sorted(common + ["--sampler", "--eta", "--sample-steps", "--target", "--reference-steps",
                                                                      "--reference-sampler", "--classifier"])
    a = eval_conversion.parse_args(["vqvae.pt", "tones"])
    assert (a.batch_size, a.precision, a.seed, a.max_samples, a.dist_backend) == (4, "fp32", 0, None, "nccl")
    assert (a.sampler, a.eta, a.sample_steps, a.target, a.reference_steps, a.reference_sampler, a.classifier) == \
        ("ddpm", 0.0, 100, "other", None, "ddpm", None)
    a = eval_conversion.parse_args(["--sampler", "ddim", "--eta", "0.5", "--target", "2", "--reference-steps", "100", "--reference-sampler", "dpmpp",
                                    "--classifier", "clf.pt", "--sample-steps", "25", "vqvae.pt", "tones"])
    assert (a.sampler, a.eta, a.target, a.reference_steps, a.reference_sampler, a.classifier, a.sample_steps) == ("ddim", 0.5, 2, 100, "dpmpp", "clf.pt", 25)
    assert eval_conversion.parse_args(["--target", "same", "vqvae.pt", "tones"]).target == "same"
    for argv, text in ((["--sampler", "dpmpp", "--eta", "0.5"], "--eta belongs to --sampler ddim"), (["--eta", "0.5"], "--eta belongs to --sampler ddim"),
                       (["--sampler", "ddim", "--eta", "-0.1"], "negative"), (["--reference-steps", "0"], "--reference-steps"),
                       (["--reference-steps", "-3"], "--reference-steps"), (["--sample-steps", "0"], "--sample-steps"),
                       (["--target", "nobody"], "--target"), (["--sampler", "euler"], "--sampler"), (["--reference-sampler", "euler"], "--reference-sampler")):
        with pytest.raises(SystemExit):
            eval_conversion.parse_args(argv + ["vqvae.pt", "tones"])
        assert text in capsys.readouterr().err, argv
    # the label count comes from the data: refused before the model loads (the checkpoint does not exist)
    eval_conversion.check_target("other", 2), eval_conversion.check_target("same", 1), eval_conversion.check_target(2, 3)
    for target, n in (("other", 1), (3, 3), (-1, 3)):
        with pytest.raises(SystemExit, match="--target"):
            eval_conversion.check_target(target, n)
    env = {k: os.environ.pop(k) for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK") if k in os.environ}
    try:
        with pytest.raises(SystemExit, match="--target 100000 is outside the labels"):
            eval_conversion.main(["--target", "100000", os.path.join(ROOT, "no-such-checkpoint.pt"), "tones"])
    finally:
        os.environ.update(env)


def test_target_labels_use_wrong_labels_for_other():
    import eval_conversion
    import eval_vqvae

    assert eval_conversion.wrong_labels is eval_vqvae.wrong_labels
    labels = torch.tensor([0, 1, 2, 2, 1, 0])
    for seed, first in ((0, 0), (1, 6), (7, 12)):
        other = eval_conversion.target_labels(labels, "other", 3, seed, first)
        assert torch.equal(other, eval_vqvae.wrong_labels(labels, 3, seed, first)) and (other != labels).all()
    assert eval_conversion.target_labels(labels, "same", 3, 0, 0) is labels
    assert torch.equal(eval_conversion.target_labels(labels, 2, 3, 0, 0), torch.full_like(labels, 2))


LINE = re.compile(r"^(\d+) samples: code_match=(\d\.\d{6}) mcd=(\d+\.\d{6}) lsd=(\d+\.\d{6})"
                  r"( ref_code_match=\d\.\d{6} ref_mcd=\d+\.\d{6} ref_lsd=\d+\.\d{6} gap_mcd=\d+\.\d{6} gap_lsd=\d+\.\d{6})?"
                  r"( target_acc=\d\.\d{6} target_nll=\d+\.\d{6}( source_acc=\d\.\d{6})?)?$")


def batch_scores(g, n, reference, classifier, same, codes=250, frames=401):
    """Random per-clip results whose float additions round differently in different orders."""
    s = {"code_match": g.integers(0, codes + 1, n).tolist(), "mcd": (g.random(n) * 10.0 ** g.integers(-8, 8, n)).tolist(),
         "lsd": (g.random(n) * 10.0 ** g.integers(-8, 8, n)).tolist()}
    if reference:
        s["ref_code_match"] = g.integers(0, codes + 1, n).tolist()
        for key in ("ref_mcd", "ref_lsd", "gap_mcd", "gap_lsd"):
            s[key] = (g.random(n) * 10.0 ** g.integers(-8, 8, n)).tolist()
    if classifier:
        s["target_correct"], s["target_nll"] = g.integers(0, 2, n).tolist(), (g.random(n) * 10.0 ** g.integers(-8, 8, n)).tolist()
        if not same:
            s["source_correct"] = g.integers(0, 2, n).tolist()
    return s


def test_format_line_and_optional_groups():
    import eval_conversion

    st = eval_conversion.EvalState()
    assert st.log_dict() == {"code_match": 0.0, "mcd": 0.0, "lsd": 0.0}  # an empty state
    assert eval_conversion.format_line(0, st.log_dict()) == "0 samples: code_match=0.000000 mcd=0.000000 lsd=0.000000"
    st.add_scores(4, 10, {"code_match": [4, 2], "mcd": [30.0, 50.0], "lsd": [10.0, 15.0]})
    assert (st.num_samples, st.codes, st.frames) == (2, 8, 20)
    assert eval_conversion.format_line(st.num_samples, st.log_dict()) == "2 samples: code_match=0.750000 mcd=4.000000 lsd=1.250000"
    g = np.random.default_rng(5)
    for reference, classifier, same in itertools.product((False, True), repeat=3):
        st = eval_conversion.EvalState(reference=reference, classifier=classifier, same=same)
        empty = st.log_dict()
        st.add_scores(250, 401, batch_scores(g, 3, reference, classifier, same))
        log = st.log_dict()
        assert list(log) == list(empty)
        want = ["code_match", "mcd", "lsd"] + (["ref_code_match", "ref_mcd", "ref_lsd", "gap_mcd", "gap_lsd"] if reference else []) + \
            ((["target_acc", "target_nll"] + ([] if same else ["source_acc"])) if classifier else [])
        assert list(log) == want
        line = eval_conversion.format_line(st.num_samples, log)
        m = LINE.match(line)
        assert m and int(m.group(1)) == 3, line
        assert (m.group(5) is not None) == reference and (m.group(6) is not None) == classifier
        assert (m.group(7) is not None) == (classifier and not same)
        with pytest.raises(ValueError):  # a batch that does not carry exactly the configured groups
            st.add_scores(250, 401, batch_scores(g, 3, not reference, classifier, same))


def test_merging_shards_in_any_order_is_exact():
    import eval_conversion

    g = np.random.default_rng(3)
    shards = [batch_scores(g, 5, True, True, False) for _ in range(3)]

    def build(order):
        states = []
        for i in order:
            st = eval_conversion.EvalState(reference=True, classifier=True)
            st.add_scores(250, 401, shards[i])
            states.append(st.to_host())
        merged = states[0]
        for other in states[1:]:
            merged.merge(other)
        return merged

    base = build((0, 1, 2))
    assert (base.num_samples, base.codes, base.frames) == (15, 15 * 250, 15 * 401)
    for key in base.sums:
        assert base.sums[key] == sum(Fraction(v) for sh in shards for v in sh[key]) and isinstance(base.sums[key], Fraction)
    assert base.counts["code_match"] == sum(sum(sh["code_match"]) for sh in shards)
    for order in itertools.permutations(range(3)):
        m = build(order)
        assert m.sums == base.sums and m.counts == base.counts and (m.num_samples, m.codes, m.frames) == (15, 15 * 250, 15 * 401)
        assert m.log_dict() == base.log_dict()
        assert eval_conversion.format_line(m.num_samples, m.log_dict()) == eval_conversion.format_line(base.num_samples, base.log_dict())
    with pytest.raises(ValueError):
        build((0,)).merge(eval_conversion.EvalState())
