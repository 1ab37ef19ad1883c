"""CPU half of the pointwise tests (tests/pointwise_ref.py): the formulas of csrc/common.hpp restated in float32 meet every gate the GPU
file holds the kernels to, the float32 oracle sits far inside its bounds, the two debug entries are declared, exported and refuse bad
arguments -- and the gates BITE: defects planted in copies of the reference are rejected by the per-entry bounds.

Planted defects, and whether today's whole-tensor gates (rel_rms < 1e-4 in fp32 mode, < 4e-3 in fp16 mode, tests/test_parity_gpu.py) would
have let them through.  Stem and head are measured at the shape of today's only tap test, test_unet32_forward_and_taps (base 32,
T = 64000, B = 2); the figures are the ones this file prints:
  stem, left neighbour dropped at t = 256 (one row per clip)     rel_rms 2.2e-3   fp16 gate LETS IT THROUGH (the fp32 gate sees it)
  stem, last row reads the next clip instead of zero             rel_rms 1.5e-3   fp16 gate LETS IT THROUGH
  head, left neighbour dropped at t = 256 (one sample per clip)  rel_rms 4.7e-3   AT the fp16 gate: seen or not by the data's luck
  head, last row reads the next clip instead of zero             rel_rms 2.1e-3   fp16 gate LETS IT THROUGH
  head, GroupNorm statistics over the first tile only            rel_rms 3e-2 .. 7e-2 at T = 770: a whole-tensor error, both gates see it
  FiLM (a | b) halves swapped for clip 32 of 33                  no test reads FiLM rows; only the B = 64 forward (batch invariance, minutes) reaches a
  clip 32 given clip 0's embedding                               second clip tile at all: NOT SEEN by any value check
  label clamped one short of the table's end                     test_time_embedding_vs_golden uses three labels: LET THROUGH unless one is the last
  degree-6 coefficients where degree 7 is claimed                |error| <= 5.7e-4 on O(1) activations, a seventh of the fp16 gate: LETS IT THROUGH
Every one of them is rejected by the per-entry bounds, by a factor of 8 (the GELU coefficients) to 10^5."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as pw
from oracle import ref_cpu
from vq_voice_swap_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_REL, FP16_REL = 1e-4, 4e-3  # today's whole-tensor gates (tests/test_parity_gpu.py)


# ------------------------------------------------------------------------------------------------------------------ the library side
def test_entry_points_are_declared_and_exported(lib_built):
    header = " ".join(open(os.path.join(ROOT, "include", "vqvs.h")).read().split())
    for name, nargs in (("vqvs_debug_gelu", 5), ("vqvs_debug_read_film", 3)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(getattr(lib_built, name).argtypes), name
    assert _native.GELU_FORMS == pw.FORMS
    src = open(os.path.join(ROOT, "vq_voice_swap_amd", "csrc", "common.hpp")).read()
    named = re.search(r"\(tests/(\w+\.py)", src)
    assert named and os.path.exists(os.path.join(ROOT, "tests", named.group(1))), "common.hpp's GELU comment must name a test that exists"


def test_entry_points_refuse_bad_arguments_without_a_device(lib_built):
    L = lib_built
    buf = C.cast((C.c_float * 8)(), C.c_void_p)
    assert L.vqvs_debug_read_film(None, 1, buf) == -1 and L.vqvs_last_error()
    for args in ((None, buf, 8, 0), (buf, None, 8, 0), (buf, buf, 0, 0), (buf, buf, -1, 0), (buf, buf, (1 << 30) + 1, 0), (buf, buf, 8, 5), (buf, buf, 8, -1)):
        assert L.vqvs_debug_gelu(*args, None) == -1 and L.vqvs_last_error(), args


# ------------------------------------------------------------------------------------------------------------------ Stage A
@pytest.fixture(scope="module")
def gx():
    return pw.gelu_inputs()


def test_gelu_inputs_are_the_cases_the_issue_sets(gx):
    assert gx.dtype == np.float32 and len(gx) == 2 ** 20 + 1 + 5 * 129 + 10
    assert gx[0] == -8.0 and gx[2 ** 20] == 8.0 and gx[2 ** 19] == 0.0
    for c in (4.0, -4.0, 8.0, -8.0):
        near = pw._around(c)
        assert len(set(near.tolist())) == 129 and np.float32(c) in near
        assert np.nextafter(np.float32(c), np.float32(np.inf)) in near and near.min() < c < near.max()
    assert np.float32(2.0 ** -149) in gx and np.float32(65504.0) in gx and np.float32(-3.0e4) in gx
    assert np.signbit(gx[-1]) and gx[-1] == 0.0


@pytest.mark.parametrize("name", list(pw.FORMS))
def test_float32_formulas_meet_the_gates(gx, name):
    """The gates are attainable: the formulas themselves, restated in float32, meet them (and reproduce common.hpp's figures)."""
    form = pw.FORMS[name]
    got, want, gate = pw.gelu_formula(gx, form), pw.gelu_want(gx, form), pw.gelu_gate(gx, form)
    a = np.abs(gx.astype(np.float64))
    err = np.abs(got.astype(np.float64) - want)
    e, share, i = pw.worst(got, want, gate)
    print(f"[formula] {name}: max |err| on [-8, 8] {err[a <= 8].max():.3e}, on [-4, 4] {err[a <= 4].max():.3e}, tail {(err[a > 8] / a[a > 8]).max():.3e} |v|, "
          f"share {share:.3f} at {gx[i]}")
    assert share <= 1.0
    if form in pw.COMMON_HPP:  # common.hpp's statement, to its two digits
        assert err[a <= 8].max() <= pw.COMMON_HPP[form] * 1.005
    if form == 3:
        assert err[a <= 4].max() <= pw.COMMON_HPP["3inner"] * 1.005


def test_gates_are_common_hpps_statements_rounded_up():
    src = open(os.path.join(ROOT, "vq_voice_swap_amd", "csrc", "common.hpp")).read()
    for fig in ("8.7e-7", "5.7e-4", "4.4e-5", "3.4e-4"):
        assert fig in src, fig
    assert (pw.GELU_GATE[0], pw.GELU_GATE[1], pw.GELU_GATE[2], pw.GELU_GATE_INNER[3], pw.GELU_GATE[3]) == (1e-6, 1e-6, 6e-4, 5e-5, 3.5e-4)
    assert pw.GELU_GATE[4] == 1e-6 and pw.GELU_TAIL == {0: 2.0 ** -22, 1: 2.0 ** -22, 2: 2.0 ** -9, 3: 2.0 ** -12}
    assert pw.HEAD_GELU == {"fp32": (8.7e-7, 8.7e-7), "fp16": (4.4e-5, 3.4e-4)} and pw.EMB_CAP == 2e-5 and pw.FORM01_ULPS == 2
    x = np.array([0.0, 3.9, 4.0, 4.1, 8.0, 8.5, -100.0], dtype=np.float32)
    assert np.allclose(pw.gelu_gate(x, 3), [5e-5, 5e-5, 5e-5, 3.5e-4, 3.5e-4, 8.5 * 2.0 ** -12, 100 * 2.0 ** -12], rtol=1e-6)
    assert np.allclose(pw.gelu_gate(x, 4), 1e-6)


def test_specials_of_the_float32_formulas():
    x = np.array([np.nan, 0.0, -0.0, 1e-40, -1e-40], dtype=np.float32)
    for form in pw.FORMS.values():
        got = pw.gelu_formula(x, form)
        assert np.isnan(got[0]) and (np.abs(got[1:].astype(np.float64) - pw.gelu_want(x[1:], form)) <= pw.gelu_gate(x[1:], form)).all()
    ref = torch.nn.functional.gelu(torch.tensor([float("inf"), float("-inf")]))
    print("[inf] torch float32 gelu(+inf, -inf) =", ref.tolist())


def test_degree_6_coefficients_do_not_pass_for_degree_7(gx):
    got = pw.gelu_formula(gx, 3, poly7=(0.0,) + pw.POLY6)  # planted: the degree-6 fit where degree 7 is claimed
    want = pw.gelu_want(gx, 3)
    e, share, i = pw.worst(got, want, pw.gelu_gate(gx, 3))
    err = np.abs(got.astype(np.float64) - want)
    e8 = err[np.abs(gx) <= 8].max()
    print(f"[defect] degree 6 for degree 7: max |err| on [-8, 8] {e8:.3e} (on [-4, 4]: {err[np.abs(gx) <= 4].max():.3e}), share {share:.1f}")
    assert share > 5.0
    assert e8 < FP16_REL  # an absolute error below the fp16 gate on O(1) activations: the whole-tensor gate lets it through


# ------------------------------------------------------------------------------------------------------------------ Stage B
@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(base, labels=True, **kw):
        k = (base, labels, tuple(sorted(kw.items())))
        if k not in cache:
            cache[k] = pw.make_model(base, labels=labels, **kw)
        return cache[k]

    return get


def test_clip_inputs_are_the_cases_the_issue_sets(lib_built):
    ts, labels, vec = pw.clip_inputs(33, 32)
    assert ts[:13].tolist() == [float(np.float32(v)) for v in pw.TS_HEAD] and ts[13].item() == float(np.float32(27 / 40)) and len(set(ts.tolist())) == 33
    assert labels.tolist() == [i % 4 for i in range(33)] and vec.shape == (33, 128) and 0.25 < vec.std().item() < 0.35
    assert pw.EMB_BASES == (32, 64, 96, 128, 256, 40) and pw.FILM_B == (1, 31, 32, 33, 65)
    assert pw.STEM_BASES == (32, 64, 96, 128) and pw.STEM_T == (2, 254, 256, 258, 770) and pw.STEM_B == (1, 3)
    assert pw.phys_index(40, 160).tolist()[:6] == [0, 1, 2, 3, 4, 8] and pw.phys_index(96, 10).tolist() == list(range(10))


@pytest.mark.parametrize("path", ["labels", "vectors", "none"])
@pytest.mark.parametrize("base", pw.EMB_BASES)
def test_embedding_reference_and_bound(models, base, path, lib_built):
    m = models(base, labels=path != "none")
    c = pw.emb_case(m, 33, path)
    print(f"[emb] base {base} {path}: E_ref {c['eref']:.2e}, max |want| {c['want'].abs().max():.3f}, bound {c['bound'].min():.2e} .. {c['bound'].max():.2e}")
    assert c["eref"] <= pw.EREF_MAX  # (the issue's condition on a case: if a new case breaks it, change the case, not the gate)
    assert pw.U * c["want"].abs().max() <= c["eref"] and (c["bound"] <= pw.EMB_CAP).all() and (c["bound"] >= 8 * c["eref"]).all()
    sd32 = pw.state(m, torch.float32)
    got32 = pw.embedding(sd32, c["ts"], c["labels"], c["vectors"])
    if path != "vectors":  # the restatement IS the oracle in float32 ...
        assert torch.equal(got32, ref_cpu.unet_embedding(sd32, c["ts"], c["labels"]))
        # ... and in float64 differs from it only by where the argument is rounded
        assert (c["want"] - ref_cpu.unet_embedding(pw.state(m), c["ts"].double(), c["labels"])).abs().max() < 2e-5
    assert pw.worst(got32.numpy(), c["want"].numpy(), c["bound"][None].expand_as(c["want"]).numpy())[1] < 0.2
    if path == "labels":  # planted: the label clamped one short of the table's end
        bad = pw.embedding(pw.state(m), c["ts"], c["labels"], clamp_labels_to=pw.NUM_LABELS - 2)
        e, share, i = pw.worst(bad.numpy(), c["want"].numpy(), c["bound"][None].expand_as(c["want"]).numpy())
        assert share > 1e3 and i // c["want"].shape[1] in range(3, 33, 4), (e, share)
        seen = c["labels"] <= pw.NUM_LABELS - 2  # clips whose labels stay below the table's end see nothing
        assert torch.equal(bad[seen], c["want"][seen])


# ------------------------------------------------------------------------------------------------------------------ Stage C
@pytest.mark.parametrize("base", (32, 96, 40))
def test_film_reference_bound_and_planted_defects(models, base, lib_built):
    m = models(base)
    ts, labels, _ = pw.clip_inputs(33)
    sd32 = pw.state(m, torch.float32)
    emb = pw.embedding(sd32, ts, labels)
    want, bound = pw.film_ref(m, emb)
    names = [n for n, _ in pw.film_blocks(base)]
    got32 = F.linear(F.gelu(emb), torch.cat([sd32[f"predictor.{n}.cond_layers.1.weight"] for n in names]),
                     torch.cat([sd32[f"predictor.{n}.cond_layers.1.bias"] for n in names]))
    e, share, _ = pw.worst(got32.numpy(), want.numpy(), bound.numpy())
    print(f"[film] base {base}: float32 oracle error {e:.2e}, share {share:.3f}, rows reach {want.abs().max():.2f}, R = {want.shape[1]}")
    assert share < 0.1 and want.shape[1] == sum(2 * c for _, c in pw.film_blocks(base))
    idx, R = pw.film_index(base)
    assert len(idx) == want.shape[1] and len(set(idx.tolist())) == len(idx) and int(idx.max()) < R
    from enroll_ref import film_rows
    assert [(n, c) for n, _r, c in film_rows(dict(base=base, topo=pw.TOPO))] == pw.film_blocks(base)  # the layout enroll_ref describes
    for defect in ("swap32", "emb0"):
        bad, _ = pw.film_ref(m, emb, defect)
        e, share, i = pw.worst(bad.numpy(), want.numpy(), bound.numpy())
        print(f"[defect] film {defect}: max |err| {e:.3f}, share {share:.0f}")
        assert share > 1e3 and i // want.shape[1] == 32 and torch.equal(bad[:32], want[:32])


# ------------------------------------------------------------------------------------------------------------------ Stage D
def _stem32(m, x, cond=None):
    sd = pw.state(m, torch.float32)
    got = F.conv1d(x, sd["predictor.in_conv.weight"], sd["predictor.in_conv.bias"], padding=1)
    if cond is not None:
        got = got + F.interpolate(F.conv1d(cond, sd["predictor.cond_proj.weight"], sd["predictor.cond_proj.bias"], padding=1), x.shape[-1])
    return got


@pytest.mark.parametrize("key", [32, 96, "in3", "cond"])
def test_stem_reference_bound_and_planted_defects(models, key, lib_built):
    kw = dict(pw.EXTRA[key]) if key in pw.EXTRA else dict(base=key)
    m = models(kw.pop("base"), **kw)
    B, T = 3, 770
    x = pw.wave((B, m.in_channels, T), 11)
    cond = pw.wave((B, m.cond_channels, pw.COND_LEN), 12) if m.cond_channels else None
    r = pw.stem_ref(m, x, cond)
    got = _stem32(m, x, cond)
    s32 = pw.worst(got.numpy(), r["want"].numpy(), r["bound32"].numpy())[1]
    s16 = pw.worst(got.half().float().numpy(), r["want"].numpy(), r["bound16"].numpy())[1]
    print(f"[stem] {key}: float32 oracle share {s32:.3f}; rounded to half, share of the fp16 bound {s16:.3f}")
    assert s32 <= 1.0 and s16 <= 1.0
    assert (r["bound16"] >= r["bound32"] - 1e-30).all()
    if cond is not None:  # the rows of the conditioning follow PyTorch's nearest rule, which neither equals nor divides T here
        assert T % pw.COND_LEN and pw.COND_LEN != T
    for defect in ("left256", "right_end"):
        bad = pw.stem_ref(m, x, cond, defect)["want"]
        for mode, bound in (("fp32", r["bound32"]), ("fp16", r["bound16"])):
            e, share, i = pw.worst(bad.numpy(), r["want"].numpy(), bound.numpy())
            t = int(np.unravel_index(i, tuple(bad.shape))[2])
            assert share > 50 and t == (256 if defect == "left256" else T - 1), (key, defect, mode, share)


def test_single_row_defects_pass_todays_fp16_gate(models, lib_built):
    """At the shape of today's tap test (base 32, T = 64000, B = 2) a single wrong row is invisible to rel_rms < 4e-3."""
    m = models(32)
    B, T = 2, 64000
    x = pw.wave((B, 1, T), 21)
    good = pw.stem_ref(m, x)
    tap = pw.wave((B, 32, T), 22)
    sd = pw.state(m)
    hgood = pw.head_eval(sd, tap.double())[0]
    for defect in ("left256", "right_end"):
        rs = pw.rel_rms(pw.stem_ref(m, x, defect=defect)["want"].numpy(), good["want"].numpy())
        rh = pw.rel_rms(pw.head_eval(sd, tap.double(), defect)[0].numpy(), hgood.numpy())
        print(f"[defect] {defect} at T = 64000, B = 2: rel_rms stem {rs:.2e}, head {rh:.2e} (fp16 gate {FP16_REL:.0e}, fp32 gate {FP32_REL:.0e})")
        assert rs < FP16_REL  # the stem's: let through in the benchmarked mode ...
        assert rh < 1.5 * FP16_REL  # ... the head's: at the gate itself (one output channel: a row is one sample of 64000)
        assert rs > FP32_REL and rh > FP32_REL  # (the fp32 gate would have seen them)
        e, share, _ = pw.worst(pw.stem_ref(m, x, defect=defect)["want"].numpy(), good["want"].numpy(), good["bound16"].numpy())
        assert share > 50  # ... and rejected entry by entry at the same shape


@pytest.mark.parametrize("key", [32, 96])
def test_head_reference_bound_and_planted_defects(models, key, lib_built):
    m = models(key)
    B, T = 3, 770
    tap = 0.3 + 1.5 * pw.wave((B, key, T), 31)
    sd32 = pw.state(m, torch.float32)
    got = pw.head_eval(sd32, tap)[0]
    for mode in ("fp32", "fp16"):
        r = pw.head_ref(m, tap.half().float() if mode == "fp16" else tap, mode)
        g = pw.head_eval(sd32, tap.half().float())[0] if mode == "fp16" else got
        share = pw.worst(g.numpy(), r["want"].numpy(), r["bound"].numpy())[1]
        print(f"[head] base {key} {mode}: float32 oracle share {share:.4f}, E_ref {r['eref']:.2e}, bound {r['bound'].min():.2e} .. {r['bound'].max():.2e}")
        assert share < 0.2 and torch.isfinite(r["bound"]).all()
        for defect in ("left256", "right_end", "stats256"):
            bad = pw.head_ref(m, tap.half().float() if mode == "fp16" else tap, mode, defect=defect)["want"]
            e, share, i = pw.worst(bad.numpy(), r["want"].numpy(), r["bound"].numpy())
            print(f"[defect] head {defect} {mode}: max |err| {e:.3f}, share {share:.0f}, rel_rms at T = 770 {pw.rel_rms(bad.numpy(), r['want'].numpy()):.2e}")
            assert share > 20, (key, mode, defect, share)
            if defect != "stats256":
                assert int(np.unravel_index(i, tuple(bad.shape))[2]) == (256 if defect == "left256" else T - 1)


def test_head_bound_follows_the_taps_that_exist_and_the_clamp(models, lib_built):
    m = models(32)
    tap = pw.wave((1, 32, 258), 41)
    tap[0, 3, 100] = 40.0  # one |u| beyond the polynomial forms' clamp
    r16, r32 = pw.head_ref(m, tap, "fp16"), pw.head_ref(m, tap, "fp32")
    w = pw.state(m)["predictor.out.1.weight"].abs()
    sumw = torch.stack([w[0, :, 1:].sum(), w[0].sum(), w[0, :, :2].sum()])  # first row, interior, last row
    _, u, _ = pw.head_eval(pw.state(m), tap.double())
    far = (u.abs().amax(dim=1)[0] > 4).nonzero().flatten().tolist()
    assert 100 in far
    stat16 = r16["bound"] - 8 * r16["eref"]
    stat32 = r32["bound"] - 8 * r32["eref"]
    extra = stat32[0, 0] - 8.7e-7 * torch.where(torch.arange(258) == 0, sumw[0], torch.where(torch.arange(258) == 257, sumw[2], sumw[1]))
    assert (extra > 0).all()  # the statistics term
    lo = 4.4e-5 * sumw[1] + extra[50]
    assert abs(stat16[0, 0, 50] - lo) < 1e-7 * lo and stat16[0, 0, 100] > 3.4e-4 * sumw[1] and stat16[0, 0, 99] > 3.4e-4 * sumw[1]


# ------------------------------------------------------------------------------------------------------------------ the recorded run
def test_recorded_margins_cover_every_case_and_stay_inside_their_bounds():
    import json

    recs = [json.loads(ln) for ln in open(os.path.join(ROOT, "profiles", pw.MARGINS))]
    by = {}
    for r in recs:
        by.setdefault(r["test"], {})[r["case"]] = r
    assert set(by["pointwise.gelu"]) == set(pw.FORMS)
    assert set(by["pointwise.embedding"]) == {f"base{b}.{p}" for b in pw.EMB_BASES for p in ("labels", "vectors", "none")}
    assert set(by["pointwise.film"]) == {f"base{b}.B{n}" for b in pw.EMB_BASES for n in pw.FILM_B}
    shapes = {k: [(T, B) for T in pw.STEM_T for B in pw.STEM_B] for k in pw.STEM_BASES + ("in3",)}
    shapes["cond"] = [(pw.COND_T, B) for B in pw.STEM_B]
    want = {f"{k}.{mode}.T{T}.B{B}" for k, tb in shapes.items() for T, B in tb for mode in ("fp32", "fp16")}
    assert set(by["pointwise.stem"]) == want and set(by["pointwise.head"]) == want
    for r in recs:
        assert 0.0 <= r["share_of_bound"] <= 1.0, r
    for r in by["pointwise.embedding"].values():
        assert r["e_ref"] <= pw.EREF_MAX and r["bound_max"] <= pw.EMB_CAP
