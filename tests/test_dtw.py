"""MCD-DTW, host side: the reference itself against brute-force enumeration (tests/dtw_ref.py), the condition the device test's
exact comparisons rest on, the exports and every argument refusal of `vqvs_mel_cepstra` and `vqvs_dtw_distance`, the wrappers'
checks, and eval_parallel.py's pairs file, flags, state and merged line (none of this needs a device)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import vq_voice_swap_amd
from vq_voice_swap_amd import AlignedDistance, PitchDistance, SpectralDistance, _native, dtw_distance

import dtw_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CEPSTRA_ARGS = ["const float* d_x", "const int* d_len", "const float* d_window", "const double* d_twiddle", "const float* d_fb",
                "const float* d_dct", "float* d_ceps", "float* d_logmel", "int* d_frames", "int B", "int T", "int n_fft", "int hop", "int n_mels",
                "int n_ceps", "float eps", "void* stream"]
DTW_ARGS = ["const float* d_ca", "const float* d_cb", "const int* d_fa", "const int* d_fb", "const double* d_ta", "const double* d_tb",
            "double* d_cost", "int* d_steps", "long long* d_track_counts", "double* d_track_sums", "int B", "int Fa_max", "int Fb_max", "int n_ceps",
            "void* stream"]


# ---------------------------------------------------------------- the reference
def test_reference_equals_brute_force_for_every_small_shape():
    """Every Fa, Fb <= 5, with tracks: the DP's cost is the minimum over all monotone paths bit for bit (rounding is monotone, so
    the minimum of the rounded sums is reached cell by cell), the minimum is unique on these inputs, and steps, both, vuv and the
    two sums are those of that path."""
    for Fa, Fb in itertools.product(range(1, 6), repeat=2):
        ca, cb = dr.noise_cepstra(Fa, 5, 10 * Fa + Fb), dr.noise_cepstra(Fb, 5, 1000 + 10 * Fa + Fb)
        ta, tb = dr.noise_track(Fa, 7 * Fa + Fb), dr.noise_track(Fb, 500 + 7 * Fa + Fb)
        paths = sorted(dr.brute_force(ca, cb, ta, tb))
        assert len(paths) == delannoy(Fa - 1, Fb - 1)
        assert len(paths) == 1 or paths[0][0] < paths[1][0], (Fa, Fb)
        ref = dr.dtw_ref(ca, cb, ta, tb)
        assert (ref["cost"], ref["steps"], ref["both"], ref["vuv"], ref["s1"], ref["s2"]) == paths[0], (Fa, Fb)
        plain = dr.dtw_ref(ca, cb)
        assert (plain["cost"], plain["steps"]) == paths[0][:2] and (plain["both"], plain["vuv"], plain["s1"], plain["s2"]) == (0, 0, 0.0, 0.0)
        assert plain["margin"] == ref["margin"] and (ref["margin"] > 0 or min(Fa, Fb) == 1)


def delannoy(m, n):
    return 1 if m == 0 or n == 0 else delannoy(m - 1, n) + delannoy(m, n - 1) + delannoy(m - 1, n - 1)


def test_reference_tie_break_and_self_distance():
    """d(a, a): cost exactly 0 along the diagonal and steps = F, for noise and for constant cepstra, where EVERY path costs 0 and
    only the tie-break (diagonal first) decides; with the order reversed the path would have 2 F - 1 cells."""
    for F in (1, 2, 9):
        for ca in (dr.noise_cepstra(F, 5, F), np.ones((F, 5), dtype=np.float32)):
            t = dr.noise_track(F, F)
            ref = dr.dtw_ref(ca, ca, t, t)
            finite = int(np.isfinite(t).sum())
            assert (ref["cost"], ref["steps"], ref["both"], ref["vuv"], ref["s1"], ref["s2"]) == (0.0, F, finite, 0, 0.0, 0.0)
    flat = np.ones((4, 5), dtype=np.float32)
    ref = dr.dtw_ref(flat, np.ones((7, 5), dtype=np.float32))
    assert (ref["cost"], ref["steps"], ref["margin"]) == (0.0, 7, 0.0)   # diagonal while it can, then along j
    # a hand-made case: a = (0, 1), b = (0, 0, 1) in coefficient 1 -> the path (0,0) (0,1) (1,2) of cost 0, found over (0,0) (1,1) (1,2)
    a, b = np.zeros((2, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.float32)
    a[1, 1] = b[2, 1] = 1.0
    ref = dr.dtw_ref(a, b, np.array([1.0, np.nan]), np.array([3.0, 4.0, 5.0]))
    assert (ref["cost"], ref["steps"], ref["both"], ref["vuv"], ref["s1"], ref["s2"]) == (0.0, 3, 2, 1, 5.0, 13.0)
    shifted = a.copy()
    shifted[:, 0] = 5.0   # coefficient 0 is left out
    assert dr.local_cost(a, b)[0, 2] == dr.DB * np.sqrt(2.0) and np.array_equal(dr.local_cost(shifted, b), dr.local_cost(a, b))


def test_device_cases_have_no_near_tie():
    """The condition of the device test's exact comparisons: on its inputs no cell's two cheapest predecessors lie within 1000 x
    the cost bound of each other, so no correct implementation's rounding can choose another predecessor."""
    cases = list(zip(dr.SHAPES, dr.dtw_inputs())) + list(zip(dr.LONG_SHAPES, dr.dtw_inputs(shapes=dr.LONG_SHAPES)))
    cases += [((129, 70), dr.dtw_inputs(dr.CFG_DEFAULT[3], ((129, 70),))[0])]
    for (Fa, Fb), (ca, cb, ta, tb, ref) in cases:
        bound = dr.bound_factor(ca.shape[1], Fa, Fb)
        print(f"({Fa}, {Fb}): smallest margin {ref['margin']:.3e}, bound {bound:.3e}")
        assert ref["margin"] >= dr.MARGIN_FACTOR * bound or min(Fa, Fb) == 1, (Fa, Fb, ref["margin"])
        assert ref["steps"] >= max(Fa, Fb) and ref["both"] + ref["vuv"] <= ref["steps"] and ref["both"] > 0
        swapped = dr.dtw_ref(cb, ca, tb, ta)   # the tie-break is not symmetric, but without near-ties the path is
        assert swapped["cost"] == ref["cost"] and swapped["steps"] == ref["steps"] and swapped["s1"] == -ref["s1"]


# ---------------------------------------------------------------- the ABI
def declared(name):
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    decl = re.search(rf"int {name}\(([^;]*)\);", header)
    assert decl, f"include/vqvs.h does not declare {name}"
    return [a.strip() for a in " ".join(decl.group(1).split()).split(",")]


def test_symbols_are_exported_and_declared(lib_built):
    for name, args in (("vqvs_mel_cepstra", CEPSTRA_ARGS), ("vqvs_dtw_distance", DTW_ARGS)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        assert declared(name) == args and len(getattr(lib_built, name).argtypes) == len(args)
    for name in ("AlignedDistance", "dtw_distance"):
        assert name in vq_voice_swap_amd.__all__ and hasattr(vq_voice_swap_amd, name)


def test_mel_cepstra_refuses_bad_arguments_without_a_device(lib_built):
    """With host-only pointers: a call that reached the device would fault on them, so VQVS_ERR_ARG proves it did not."""
    L = lib_built
    sizes = dict(x=2 * 64 * 4, len=2 * 4, window=16 * 4, twiddle=16 * 16, fb=9 * 128 * 4, dct=128 * 64 * 4, ceps=2 * 9 * 64 * 4,
                 logmel=2 * 9 * 128 * 4, frames=2 * 4)
    keep = {k: (C.c_char * n)() for k, n in sizes.items()}
    ptr = {k: C.cast(v, C.c_void_p) for k, v in keep.items()}
    ok = dict(ptr, B=2, T=64, n_fft=16, hop=8, n_mels=4, n_ceps=2, eps=1e-6)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_mel_cepstra(a["x"], a["len"], a["window"], a["twiddle"], a["fb"], a["dct"], a["ceps"], a["logmel"], a["frames"], a["B"],
                                  a["T"], a["n_fft"], a["hop"], a["n_mels"], a["n_ceps"], a["eps"], None)

    inside = lambda name, off=8: C.c_void_p(ptr[name].value + off)  # noqa: E731
    bad = [dict(x=None), dict(len=None), dict(window=None), dict(twiddle=None), dict(fb=None), dict(dct=None), dict(ceps=None), dict(frames=None),
           dict(B=0), dict(B=-1), dict(B=65536), dict(T=8), dict(T=0), dict(T=-64), dict(T=(1 << 30) + 1),
           dict(n_fft=17), dict(n_fft=14), dict(n_fft=0), dict(n_fft=514), dict(hop=0), dict(hop=-8), dict(hop=17),
           dict(n_mels=0), dict(n_mels=129), dict(n_ceps=1), dict(n_ceps=5), dict(n_ceps=65, n_mels=128),
           dict(eps=0.0), dict(eps=-1e-6), dict(eps=float("inf")), dict(eps=float("nan")),
           # an output inside an input or another output
           dict(ceps=inside("x")), dict(logmel=inside("x")), dict(frames=inside("x", 4)), dict(ceps=inside("len", 0)), dict(frames=ptr["len"]),
           dict(ceps=inside("window")), dict(logmel=inside("twiddle")), dict(ceps=inside("fb", 0)), dict(frames=inside("dct", 0)),
           dict(logmel=ptr["ceps"]), dict(frames=inside("ceps")), dict(frames=inside("logmel", 4)),
           # logmel may be NULL: everything else is still checked
           dict(logmel=None, B=0), dict(logmel=None, x=None), dict(logmel=None, frames=inside("ceps"))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.vqvs_last_error(), kw
    for kw, text in ((dict(B=65536), b"65535"), (dict(T=8), b"reflect"), (dict(n_fft=17), b"n_fft=17"), (dict(hop=17), b"hop=17"),
                     (dict(n_ceps=65, n_mels=128), b"n_ceps=65"), (dict(eps=0.0), b"eps"), (dict(x=None), b"non-NULL"),
                     (dict(ceps=None), b"non-NULL"), (dict(logmel=ptr["ceps"]), b"overlap")):
        assert call(**kw) == -1 and text in L.vqvs_last_error(), (kw, L.vqvs_last_error())


def test_dtw_distance_refuses_bad_arguments_without_a_device(lib_built):
    L = lib_built
    sizes = dict(ca=2 * 9 * 5 * 4, cb=2 * 7 * 5 * 4, fa=2 * 4, fb=2 * 4, ta=2 * 9 * 8, tb=2 * 7 * 8, cost=2 * 8, steps=2 * 4, counts=2 * 16, sums=2 * 16)
    keep = {k: (C.c_char * n)() for k, n in sizes.items()}
    ptr = {k: C.cast(v, C.c_void_p) for k, v in keep.items()}
    ok = dict(ptr, B=2, Fa=9, Fb=7, n_ceps=5)
    plain = dict(ta=None, tb=None, counts=None, sums=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_dtw_distance(a["ca"], a["cb"], a["fa"], a["fb"], a["ta"], a["tb"], a["cost"], a["steps"], a["counts"], a["sums"], a["B"],
                                   a["Fa"], a["Fb"], a["n_ceps"], None)

    inside = lambda name, off=8: C.c_void_p(ptr[name].value + off)  # noqa: E731
    bad = [dict(ca=None), dict(cb=None), dict(fa=None), dict(fb=None), dict(cost=None), dict(steps=None),
           dict(plain, ca=None), dict(plain, steps=None),
           dict(ta=None), dict(tb=None), dict(counts=None), dict(sums=None),                       # exactly one of a pair
           dict(counts=None, sums=None), dict(ta=None, tb=None),                                   # tracks without outputs, outputs without tracks
           dict(plain, ta=ptr["ta"]), dict(plain, sums=ptr["sums"]), dict(ta=None, sums=None),
           dict(B=0), dict(B=-1), dict(B=65536), dict(Fa=0), dict(Fa=-1), dict(Fa=2049), dict(Fb=0), dict(Fb=2049),
           dict(n_ceps=1), dict(n_ceps=0), dict(n_ceps=65), dict(plain, B=0), dict(plain, Fb=2049), dict(plain, n_ceps=65),
           # an output inside an input or another output
           dict(cost=inside("ca")), dict(steps=inside("cb")), dict(counts=inside("ta")), dict(sums=inside("tb", 0)), dict(cost=ptr["fa"]),
           dict(steps=ptr["fb"]), dict(steps=inside("cost")), dict(sums=ptr["counts"]), dict(counts=inside("cost", 0)), dict(sums=inside("steps", 0)),
           dict(plain, cost=inside("ca")), dict(plain, steps=inside("cost"))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.vqvs_last_error(), kw
    for kw, text in ((dict(B=65536), b"65535"), (dict(Fa=2049), b"Fa_max=2049"), (dict(Fb=0), b"Fb_max=0"), (dict(n_ceps=65), b"n_ceps=65"),
                     (dict(ta=None), b"both or neither"), (dict(sums=None), b"both or neither"), (dict(ta=None, tb=None), b"if and only if"),
                     (dict(counts=None, sums=None), b"if and only if"), (dict(ca=None), b"non-NULL"), (dict(steps=inside("cost")), b"overlap")):
        assert call(**kw) == -1 and text in L.vqvs_last_error(), (kw, L.vqvs_last_error())


def test_wrapper_checks_raise_before_a_device():
    d = SpectralDistance()
    x = torch.zeros(2, 1, 800)
    for bad, lengths in ((x.double(), [800, 800]), (torch.zeros(800), [800]), (torch.zeros(2, 2, 800), [800, 800]), (x.numpy(), [800, 800]),
                         (x, [800]), (x, [800, 801]), (x, [200, 800]), (x, [800.0, 800]), (x, torch.tensor([800.0, 800.0])), (x, 800),
                         (torch.zeros(2, 200), [200, 200])):
        with pytest.raises(ValueError):
            d.cepstra(bad, lengths)
    with pytest.raises(_native.NativeError):   # nothing left to object to but the device: there is no CPU path
        d.cepstra(x, [800, 201])
    c = torch.zeros(2, 9, 13)
    for args in ((c, [9, 9], torch.zeros(3, 9, 13), [9, 9, 9]), (c, [9, 9], torch.zeros(2, 9, 12), [9, 9]), (c.double(), [9, 9], c.double(), [9, 9]),
                 (c[0], [9], c[0], [9]), (c, [9, 10], c, [9, 9]), (c, [0, 9], c, [9, 9]), (c, [9], c, [9, 9]),
                 (torch.zeros(2, 2049, 13), [9, 9], c, [9, 9]), (torch.zeros(2, 9, 1), [9, 9], torch.zeros(2, 9, 1), [9, 9])):
        with pytest.raises(ValueError):
            dtw_distance(*args)
    t = torch.zeros(2, 9, dtype=torch.float64)
    for ta, tb in ((t, None), (None, t), (t.float(), t.float()), (t, torch.zeros(2, 8, dtype=torch.float64))):
        with pytest.raises(ValueError):
            dtw_distance(c, [9, 9], c, [9, 9], ta, tb)
    with pytest.raises(_native.NativeError):
        dtw_distance(c, [9, 9], c, [9, 9])
    with pytest.raises(ValueError):   # one track value per cepstral frame
        AlignedDistance(SpectralDistance(), PitchDistance(hop=80))
    with pytest.raises(ValueError):
        AlignedDistance(SpectralDistance(hop=80))(torch.zeros(1, 2048 * 80), [800], torch.zeros(1, 800), [800])   # more than 2048 frames
    a = AlignedDistance()
    assert a.pitch is None and a.spectral.hop == 160 and a.max_samples() == 2048 * 160 - 1
    with pytest.raises(ValueError):
        a(x, [800, 800], torch.zeros(3, 1, 800), [800, 800, 800])


# ---------------------------------------------------------------- eval_parallel.py
def test_flags():
    import eval_parallel

    a = eval_parallel.parse_args(["pairs.tsv", "data", "--checkpoint", "m.pt"])
    assert (a.pairs, a.data_dir, a.checkpoint, a.converted_dir, a.pitch, a.max_pairs) == ("pairs.tsv", "data", "m.pt", None, False, None)
    assert (a.sampler, a.eta, a.sample_steps, a.window_seconds, a.overlap_seconds, a.window_batch, a.pack_windows, a.seed, a.precision) == \
        ("ddpm", 0.0, 100, 4.0, 0.4, 64, 512, 0, "fp32")   # convert_dataset.py's defaults
    b = eval_parallel.parse_args(["pairs.tsv", "data", "--converted-dir", "out", "--pitch", "--max-pairs", "3", "--pack-windows", "7"])
    assert (b.checkpoint, b.converted_dir, b.pitch, b.max_pairs, b.pack_windows) == (None, "out", True, 3, 7)
    c = eval_parallel.parse_args(["p", "d", "--checkpoint", "m.pt", "--sampler", "dpmpp", "--sample-steps", "25", "--precision", "fp16"])
    assert (c.sampler, c.sample_steps, c.precision) == ("dpmpp", 25, "fp16")
    import convert_dataset

    shared = {"--sampler", "--eta", "--sample-steps", "--window-seconds", "--overlap-seconds", "--window-batch", "--pack-windows", "--precision", "--seed"}
    flags = lambda parser: {s for act in parser._actions for s in act.option_strings}  # noqa: E731
    assert shared <= flags(eval_parallel.arg_parser()) and shared <= flags(convert_dataset.arg_parser())
    for argv in (["p", "d"], ["p", "d", "--checkpoint", "m.pt", "--converted-dir", "out"], ["p", "--checkpoint", "m.pt"],
                 ["p", "d", "--checkpoint", "m.pt", "--eta", "0.5"], ["p", "d", "--checkpoint", "m.pt", "--sampler", "ddim", "--eta", "-1"],
                 ["p", "d", "--checkpoint", "m.pt", "--max-pairs", "0"], ["p", "d", "--converted-dir", "o", "--pack-windows", "0"],
                 ["p", "d", "--checkpoint", "m.pt", "--sample-steps", "0"]):
        with pytest.raises(SystemExit):
            eval_parallel.parse_args(argv)


def test_pairs_file_and_every_refusal(tmp_path):
    import eval_parallel
    from vq_voice_swap_amd.audio import ChunkWriter

    data, out = tmp_path / "data", tmp_path / "out"
    lengths = {"s/a.wav": 4000, "s/b.wav": 201, "t/a.wav": 5000, "t/b.wav": 2048 * 160 - 1, "t/short.wav": 200, "t/long.wav": 2048 * 160}
    for rel, n in lengths.items():
        os.makedirs(data / os.path.dirname(rel), exist_ok=True)
        w = ChunkWriter(str(data / rel), 16000)
        w.write(np.zeros(n, dtype=np.float32))
        w.close()
    (data / "t" / "broken.wav").write_bytes(b"not a wave file")
    os.makedirs(out / "s")
    w = ChunkWriter(str(out / "s" / "a.wav"), 16000)
    w.write(np.zeros(4000, dtype=np.float32))
    w.close()
    table = tmp_path / "pairs.tsv"

    def read(text, **kw):
        table.write_text(text)
        return eval_parallel.read_pairs(str(table), str(data), **kw)

    good = "# source, target, label\n\ns/a.wav\tt/a.wav\t2\ns/b.wav\tt/b.wav\t0\n"
    assert read(good, num_labels=3) == [("s/a.wav", "t/a.wav", 2, 4000), ("s/b.wav", "t/b.wav", 0, 201)]
    assert read(good) == read(good, num_labels=3) and read(good, max_pairs=1) == [("s/a.wav", "t/a.wav", 2, 4000)]
    assert read(good + "s/a.wav\tt/missing.wav\t0\n", max_pairs=2) == read(good)   # lines past --max-pairs are not looked at
    assert read("s/a.wav\tt/a.wav\t1\n", converted_dir=str(out)) == [("s/a.wav", "t/a.wav", 1, 4000)]
    for text, line, what, kw in (
            (good + "s/a.wav t/a.wav 2\n", 5, "expected", {}), (good + "s/a.wav\tt/a.wav\n", 5, "expected", {}),
            (good + "s/a.wav\tt/a.wav\t2\textra\n", 5, "expected", {}), ("\tt/a.wav\t2\n", 1, "expected", {}),
            (good + "s/a.wav\tt/a.wav\tbob\n", 5, "label", {}), (good + "s/a.wav\tt/a.wav\t-1\n", 5, "label", {}),
            (good, 3, "label 2 outside the model's 0..1", dict(num_labels=2)),
            ("s/a.wav\tt/missing.wav\t0\n", 1, "no file", {}), ("s/none.wav\tt/a.wav\t0\n", 1, "no file", {}),
            (good + "s/a.wav\tt/short.wav\t0\n", 5, "200 samples", {}), (good + "s/a.wav\tt/long.wav\t0\n", 5, "2048 frames", {}),
            (good + "s/a.wav\tt/broken.wav\t0\n", 5, "cannot read", {}),
            (good, 4, "no file", dict(converted_dir=str(out))),           # s/b.wav was not converted
            ("# nothing\n\n", None, "no pairs", {})):
        with pytest.raises(ValueError) as e:
            read(text, **kw)
        assert what in str(e.value) and (line is None or f"pairs.tsv:{line}:" in str(e.value)), (text, str(e.value))
    # the script ends with that message before it asks for a device
    table.write_text(good + "s/a.wav\tt/missing.wav\t0\n")
    with pytest.raises(SystemExit) as e:
        eval_parallel.main([str(table), str(data), "--converted-dir", str(out)])
    assert "pairs.tsv:4: no file" in str(e.value)   # (line 3's converted file is there; line 4's is the first thing missing)


def pair_scores(g, n, pitch, unvoiced=None):
    """Random per-pair results as `score_pack` returns them; pair `unvoiced` has no cell voiced in both."""
    import eval_parallel

    s = {}
    for p in eval_parallel.SIDES:
        longer = g.integers(1, 400, n)
        steps = longer + g.integers(0, 100, n)
        s[p + "longer"], s[p + "steps"], s[p + "cost"] = longer.tolist(), steps.tolist(), (steps * g.uniform(3.0, 9.0, n)).tolist()
        if pitch:
            cnt = g.integers(1, longer + 1)
            if unvoiced is not None:
                cnt[unvoiced] = 0
            mean, spread = g.normal(0.0, 3.0, n), g.random(n)
            s[p + "f0_n"], s[p + "vuv"] = cnt.tolist(), g.integers(0, longer + 1).tolist()
            s[p + "f0_s1"] = np.where(cnt > 0, cnt * mean, 0.0).tolist()
            s[p + "f0_s2"] = np.where(cnt > 0, cnt * (mean ** 2 + spread ** 2), 0.0).tolist()
    return s


NUMBER = r"-?\d+\.\d{6}"
LINE = re.compile(rf"^(\d+) pairs: mcd_dtw=({NUMBER}) src_mcd_dtw=({NUMBER}) gain=({NUMBER}) stretch=({NUMBER})"
                  rf"( f0_shift_dtw={NUMBER} f0_dev_dtw={NUMBER} vuv_err_dtw={NUMBER} src_f0_shift_dtw={NUMBER} src_f0_dev_dtw={NUMBER} src_vuv_err_dtw={NUMBER})?$")


@pytest.mark.parametrize("pitch", [False, True])
def test_merged_line_is_independent_of_ranks_and_pack_budget(pitch):
    """Eleven pairs of 1..5 windows: packed under two budgets, dealt to 1, 2 and 3 simulated ranks, each rank's packs folded into
    its own state and the states merged in rank order -- one line, character for character."""
    import eval_parallel
    from fractions import Fraction
    from vq_voice_swap_amd.corpus import deal_packs, make_packs

    g = np.random.default_rng(21)
    n = 11
    scores = pair_scores(g, n, pitch, unvoiced=4)
    windows = g.integers(1, 6, n).tolist()

    def run(budget, world):
        states = []
        for rank in range(world):
            st = eval_parallel.ParallelState(pitch=pitch)
            for pack in deal_packs(make_packs(windows, budget), rank, world):
                st.add_scores({k: [v[i] for i in pack] for k, v in scores.items()})
            states.append(st)
        for other in states[1:]:
            states[0].merge(other)
        return states[0]

    base = run(512, 1)
    line = eval_parallel.format_line(base.num_pairs, base.log_dict())
    m = LINE.match(line)
    assert m and int(m.group(1)) == n and (m.group(6) is not None) == pitch, line
    log = base.log_dict()
    cost, src = (sum(Fraction(c) for c in scores[p + "cost"]) for p in eval_parallel.SIDES)
    assert log["mcd_dtw"] == float(cost / sum(scores["steps"])) and log["src_mcd_dtw"] == float(src / sum(scores["src_steps"]))
    assert log["gain"] == float(src / sum(scores["src_steps"]) - cost / sum(scores["steps"]))
    assert log["stretch"] == sum(scores["steps"]) / sum(scores["longer"])
    if pitch:
        assert log["f0_shift_dtw"] == float(sum(Fraction(s) for s in scores["f0_s1"]) / sum(scores["f0_n"]))
        assert log["src_vuv_err_dtw"] == sum(scores["src_vuv"]) / sum(scores["src_steps"])
    for budget, world in itertools.product((512, 4), (1, 2, 3)):
        st = run(budget, world)
        assert st.sums == base.sums and st.counts == base.counts
        assert eval_parallel.format_line(st.num_pairs, st.log_dict()) == line, (budget, world)
    assert len(make_packs(windows, 4)) > 3 > len(make_packs(windows, 512))
    empty = eval_parallel.ParallelState(pitch=pitch)
    assert LINE.match(eval_parallel.format_line(0, empty.log_dict())) and not any(empty.log_dict().values())
    for wrong in (pair_scores(g, 3, not pitch), {k: v for k, v in pair_scores(g, 3, pitch).items() if k != "src_steps"}):
        with pytest.raises(ValueError):
            empty.add_scores(wrong)
    with pytest.raises(ValueError):
        empty.merge(eval_parallel.ParallelState(pitch=not pitch))
