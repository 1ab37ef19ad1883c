"""CPU half of the GroupNorm tests (tests/groupnorm_ref.py): the float64 reference is the oracle's group_norm, the bound arithmetic holds
against float32 emulations of the producers' three summation orders, the debug entries are declared, exported and refuse bad arguments
-- and the bounds BITE: every defect planted in a copy of the reference exceeds its bound by a factor of at least 4 at the shapes
tests/test_groupnorm_gpu.py runs (the factors are printed; the factor is a condition on the shapes, not a measurement: a defect caught
by less means the shape is too long for it)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import groupnorm_ref as gr
import pointwise_ref as pw
from oracle import ref_cpu
from vq_voice_swap_amd import _native
from vq_voice_swap_amd.det_init import det_tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4.0


def affine(C, tag="t"):
    return det_tensor(f"gn.{tag}.{C}.weight", (C,)), det_tensor(f"gn.{tag}.{C}.bias", (C,))


def film_rows(B, C, tag="t"):
    f = 0.3 * pw.wave((B, 2 * C), 4242 + C)
    return f[:, :C], f[:, C:]


def form_of(z, form):
    return {"n01": z, "x1e-3": z * 1e-3, "x30": z * 30.0, "dc80": 4.0 + 0.05 * z}[form]


# ------------------------------------------------------------------------------------------------------------------ the library side
def test_entry_points_are_declared_exported_and_refuse_bad_arguments(lib_built):
    header = " ".join(open(os.path.join(ROOT, "include", "vqvs.h")).read().split())
    for name, nargs in (("vqvs_debug_gn_count", 1), ("vqvs_debug_gn_info", 7), ("vqvs_debug_gn_read", 7), ("vqvs_debug_xform_count", 1),
                        ("vqvs_debug_xform_info", 5), ("vqvs_debug_xform_read", 6)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(getattr(lib_built, name).argtypes), name
    L = lib_built
    buf = C.cast((C.c_float * 8)(), C.c_void_p)
    info = (C.c_int64 * 24)()
    assert L.vqvs_debug_gn_count(None) == 0 and L.vqvs_debug_xform_count(None) == 0
    assert L.vqvs_debug_gn_info(None, 0, 1, 1, None, 0, info) == -1 and L.vqvs_last_error()
    assert L.vqvs_debug_gn_read(None, 0, 1, 1, 0, 0, buf) == -1 and L.vqvs_debug_xform_info(None, 0, 1, 1, info) == -1
    assert L.vqvs_debug_xform_read(None, 0, 1, 1, 0, buf) == -1


def test_the_cases_are_the_ones_the_issue_sets():
    c = gr.BLOCK_CASES
    assert list(c) == ["c32_L200", "c64_L592", "c96_L300", "c128to256_L131", "c256_d16_L255", "c256_d16_L256", "c512_d8_L250", "c64_avg", "c128_up",
                       "c512_avg_L254"]
    assert c["c32_L200"][:6] == (32, 32, 1.0, 1, 200, 3) and c["c64_L592"][:6] == (64, 64, 1.0, 2, 592, 3)
    assert c["c96_L300"][:6] == (96, 96, 1.0, 1, 300, 3) and c["c128to256_L131"][:6] == (128, 256, 1.0, 1, 131, 3)
    assert c["c256_d16_L255"][:6] == (256, 256, 1.0, 16, 255, 3) and c["c256_d16_L256"][:6] == (256, 256, 1.0, 16, 256, 3)
    assert c["c512_d8_L250"][:6] == (512, 512, 1.0, 8, 250, 2) and c["c64_avg"][:6] == (64, 64, 0.5, 1, 504, 3)
    assert c["c128_up"][:6] == (128, 128, 2.0, 1, 126, 3) and c["c512_avg_L254"] == (512, 512, 0.5, 1, 254, 3, ("fp32",))
    assert gr.REFUSED_AS_THE_ISSUE_STATES_THEM == ((64, 128, 0.5), (128, 64, 2.0), (256, 512, 0.5))  # (resizing blocks keep their width)
    assert all(v[6] == ("fp32", "fp16") for k, v in c.items() if k != "c512_avg_L254")
    assert gr.FORMS == ("n01", "x1e-3", "x30", "dc80") and gr.GN_TABLE_CASES == ("c64_L592", "c128to256_L131", "c512_d8_L250", "c64_avg")
    x, e = gr.block_input("c32_L200", "dc80")
    assert x.shape == (3, 32, 200) and e.shape == (3, 128) and 70 < (x.mean() / x.std()).item() < 90
    xl, el = gr.long_input("c32_L200")
    assert xl.shape == (4, 32, 496) and el.shape == (4, 128)
    m = gr.MODEL_CASES
    assert m["unet32"][1:4] == (dict(base_channels=32, channel_mult=(1, 2, 2), middle_dilations=(2,), depth_mult=1, num_labels=3), 1024, ("fp32", "fp16"))
    assert m["unet48"][1]["base_channels"] == 48 and m["unet48"][2] == 512
    assert m["unet32_wide"][1]["channel_mult"] == (1, 8, 16) and m["unet32_wide"][2:4] == (1024, ("fp16",))
    assert m["classifier32"][1] == dict(base_channels=32, channel_mult=(1, 2, 2, 4), output_mult=8, depth_mult=1) and m["classifier32"][2] == 592
    xd = gr.model_input("unet32_dc")
    assert xd.shape == (2, 1, 1024) and abs(xd.mean().item() - 0.5) < 1e-3 and abs(xd.std().item() - 0.01) < 1e-3
    assert set(gr.PRODUCERS) == {"ntc_stats", "conv_ws (2-byte modes)", "conv_ws fp32 form, conv_mfma (fp32 mode)", "conv_mfma (2-byte modes)", "in_conv"}
    assert "unrounded" in gr.PRODUCERS["in_conv"]["values"] and gr.PRODUCERS["ntc_stats"]["values"] == "stored"


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("C,L", [(32, 200), (96, 300), (512, 250), (128, 131)])
def test_reference_is_the_oracles_group_norm_in_float64(C, L):
    x = (0.3 + 1.5 * pw.wave((3, C, L), 51)).double()
    gw, gb = affine(C)
    sd = {"g.weight": gw.double(), "g.bias": gb.double()}
    want = ref_cpu.group_norm(x, sd, "g")
    groups = ref_cpu.gn_groups(C)
    t = gr.tensor_totals(x, L)
    c = gr.coefficients(t["s1"], t["s2"], groups, (C // groups) * L, gw, gb)
    got = x * c["scale"][:, :, None] + c["shift"][:, :, None]
    err = (got - want).abs().max().item()
    print(f"[oracle] C={C} L={L} groups={groups}: max |scale x + shift - group_norm64| = {err:.2e}")
    assert err < 1e-11
    # with FiLM: h (a + 1) + b, as unet.py:311-314
    fa, fb = film_rows(3, C)
    cf = gr.coefficients(t["s1"], t["s2"], groups, (C // groups) * L, gw, gb, fa, fb)
    wantf = want * (fa.double()[:, :, None] + 1.0) + fb.double()[:, :, None]
    assert ((x * cf["scale"][:, :, None] + cf["shift"][:, :, None]) - wantf).abs().max().item() < 1e-11


def test_reference_at_a_padded_width_and_over_a_concatenation(lib_built):
    """Physical channels in blocks of 4 of which 3 are real (base 48 -> 64): groups and count from the REAL width; two sources."""
    B, L, real = 2, 300, 96  # 2 x 48
    xr = pw.wave((B, real, L), 52).double()
    gw, gb = affine(real)
    want = ref_cpu.group_norm(xr, {"g.weight": gw.double(), "g.bias": gb.double()}, "g")
    idx = pw.phys_index(48, real)
    P = 128
    x = torch.zeros(B, P, L, dtype=torch.float64)
    x[:, idx] = xr
    gwp, gbp = torch.zeros(P), torch.zeros(P)
    gwp[idx], gbp[idx] = gw, gb
    groups = ref_cpu.gn_groups(real)
    assert groups == 32 and P // groups == 4 and real // groups == 3
    # two sources of 64 physical channels each, as a decoder block sees torch.cat([h, skip])
    t0, t1 = gr.tensor_totals(x[:, :64], L), gr.tensor_totals(x[:, 64:], L)
    c = gr.coefficients(torch.cat([t0["s1"], t1["s1"]], 1), torch.cat([t0["s2"], t1["s2"]], 1), groups, 3 * L, gwp, gbp)
    got = (x * c["scale"][:, :, None] + c["shift"][:, :, None])[:, idx]
    assert (got - want).abs().max().item() < 1e-11
    assert (c["scale"][:, [i for i in range(P) if i not in set(idx.tolist())]] == 0).all()  # pad channels: gamma = 0


# ------------------------------------------------------------------------------------------------------------------ stage (a)
@pytest.mark.parametrize("order", ["sequential", "pairwise", "sliced"])
def test_partial_bounds_hold_for_float32_tile_sums_in_every_order(order):
    worst = 0.0
    for C, L, rows in ((32, 200, 256), (32, 592, 252), (8, 1024, 256), (16, 250, 124), (16, 255, 255)):
        z = pw.wave((2, C, L), 60 + L)
        for form in gr.FORMS:
            x = form_of(z, form)
            parts = gr.tile_sums32(x, rows, order)
            assert parts.shape == (2, (L + rows - 1) // rows, C, 2)
            got = gr.partial_totals(parts)
            t = gr.tensor_totals(x, min(rows, L))
            s1 = gr.worst_share(got[:, :, 0], t["s1"], t["d1"])[1]
            s2 = gr.worst_share(got[:, :, 1], t["s2"], t["d2"])[1]
            worst = max(worst, s1, s2)
            assert s1 <= 1.0 and s2 <= 1.0, (order, C, L, rows, form, s1, s2)
    print(f"[partials] {order}: largest share of gamma_n sum|x| / gamma_(n+1) sum x^2 over the shapes and forms: {worst:.3f}")


def test_the_stem_sums_unrounded_values_and_its_reference_is_the_float64_stem():
    """in_conv_kernel in a 2-byte mode: float32 v summed before store8 rounds it.  The float64 stem holds those sums; the stored halves
    do not (which is why the stored tensor is not this producer's reference)."""
    B, T, Cb = 2, 1024, 32
    x = pw.wave((B, 1, T), 70)
    w, b = det_tensor("in_conv.weight", (Cb, 1, 3)), det_tensor("in_conv.bias", (Cb,))
    v32 = F.conv1d(x, w, b, padding=1)
    parts = gr.tile_sums32(v32, 256, "sliced")
    got = gr.partial_totals(parts)
    t = gr.stem_totals(w, b, x)
    s1, s2 = gr.worst_share(got[:, :, 0], t["s1"], t["d1"])[1], gr.worst_share(got[:, :, 1], t["s2"], t["d2"])[1]
    stored = gr.tensor_totals(v32.half().float(), 256)
    h1, h2 = gr.worst_share(got[:, :, 0], stored["s1"], stored["d1"])[1], gr.worst_share(got[:, :, 1], stored["s2"], stored["d2"])[1]
    print(f"[stem] unrounded float32 sums: share of the float64-stem bound {s1:.3f} / {s2:.3f}; of the stored halves' gamma bound {h1:.2f} / {h2:.2f}")
    assert s1 <= 1.0 and s2 <= 1.0
    assert (t["d1"] < 2.5 * stored["d1"]).all()  # as sharp as any other producer's bound, not 2^-11 wide


def test_a_producer_that_sums_unrounded_values_and_the_storage_rounding_term():
    """conv_mfma_kernel in a 2-byte mode: float32 sums of v, stored halves.  The stored tensor's gamma bound does not hold them; with
    the storage-rounding term it does, and a miscounted row at such a source still exceeds the bound by the factor."""
    B, C, L, rows = 2, 64, 512, 254  # block 2 of the base-32 models at T = 1024
    v = pw.wave((B, C, L), 72)
    parts = gr.tile_sums32(v, rows, "sliced")
    got = gr.partial_totals(parts)
    x = v.half().float()
    plain, loose = gr.tensor_totals(x, rows), gr.unrounded_totals(x, rows)
    p2 = gr.worst_share(got[:, :, 1], plain["s2"], plain["d2"])[1]
    l1, l2 = gr.worst_share(got[:, :, 0], loose["s1"], loose["d1"])[1], gr.worst_share(got[:, :, 1], loose["s2"], loose["d2"])[1]
    print(f"[unrounded] share of the stored tensor's gamma bound {p2:.1f}; with the storage-rounding term {l1:.3f} / {l2:.3f}")
    assert p2 > 1.0 and l1 <= 1.0 and l2 <= 1.0
    gw, gb = affine(C)
    fa, fb = film_rows(B, C)
    groups = ref_cpu.gn_groups(C)
    info = info_of([x], (rows,), groups, (C // groups) * L)
    r = gr.gn_case([x], [parts], info, gw, gb, fa, fb, totals=["unrounded"])
    c, bd = r["b2"]
    nxt = torch.roll(x.double(), -1, dims=0)[:, :, 0]
    bad = gr.coefficients(got[:, :, 0] + nxt, got[:, :, 1] + nxt * nxt, groups, info["count"], gw, gb, fa, fb)
    assert defect_factor("conv_mfma source, 64 x 512: one row past L", bad["scale"], bad["shift"], c, bd) >= FACTOR


def test_whole_clip_form_is_recognised_from_the_partials():
    x = pw.wave((2, 8, 250), 71)
    one = gr.tile_sums32(x, 250)
    whole = torch.cat([one, torch.zeros_like(one)], dim=1)  # tile_rows 240: two statistics tiles, the second zero-filled
    assert gr.rows_per_partial(whole, 250, 240) == (250, True)
    assert gr.rows_per_partial(gr.tile_sums32(x, 240), 250, 240) == (240, False)
    assert gr.rows_per_partial(one, 250, 254) == (250, False)


# ------------------------------------------------------------------------------------------------------------------ stage (b)
def emulate(xs, rows, gw, gb, fa, fb, groups, count, orders=("sequential", "pairwise")):
    """What the library makes of stored sources xs: float32 partials in the producers' orders, float64 coefficients, float32 tables."""
    parts = [gr.tile_sums32(x, r, o) for x, r, o in zip(xs, rows, orders)]
    tot = [gr.partial_totals(p) for p in parts]
    c = gr.coefficients(torch.cat([t[:, :, 0] for t in tot], 1), torch.cat([t[:, :, 1] for t in tot], 1), groups, count, gw, gb, fa, fb)
    return parts, torch.stack([c["scale"].float(), c["shift"].float()], dim=2), torch.stack([c["mean"].float(), c["rstd"].float()], dim=2)


def info_of(xs, rows, groups, count):
    return dict(groups=groups, count=count, srcs=[dict(C=x.shape[1], rows=x.shape[2], tile_rows=r, ntiles=(x.shape[2] + r - 1) // r) for x, r in zip(xs, rows)])


GEOM = [  # (id, C per source, L, rows per tile per source, real base / physical base) -- GroupNorm 1 and 2 of the cases of section 4
    ("c32_L200", (32,), 200, (256,), None), ("c64_L592", (64,), 592, (252,), None), ("c96_L300", (96,), 300, (254,), None),
    ("c128_L131", (128,), 131, (256,), None), ("c256_L255", (256,), 255, (255,), None), ("c512_L250", (512,), 250, (250,), None),
    ("c64_L504", (64,), 504, (256,), None), ("c128_L126", (128,), 126, (256,), None), ("c256_L253", (256,), 253, (256,), None),
    ("unet32_stem_T1024", (32,), 1024, (256,), None), ("unet32_cat_T1024", (32, 32), 1024, (254, 256), None),
    ("unet48_cat_T512", (64, 64), 512, (254, 256), (48, 64)),
]


@pytest.mark.parametrize("form", gr.FORMS)
@pytest.mark.parametrize("geom", GEOM, ids=[g[0] for g in GEOM])
def test_coefficient_bounds_hold_for_an_emulated_library_and_cover_every_input_form(geom, form, lib_built):
    _id, Cs, L, rows, pad = geom
    B, Ctot = 2, sum(Cs)
    xs = [form_of(pw.wave((B, C, L), 80 + i), form).half().float() for i, C in enumerate(Cs)]
    gw, gb = affine(Ctot)
    if pad:  # pad channels are exact zeros with zero affine parameters
        keep = torch.zeros(Ctot, dtype=torch.bool)
        keep[pw.phys_index(pad[0], Ctot * pad[0] // pad[1])] = True
        gw, gb = gw * keep, gb * keep
        for i, C in enumerate(Cs):
            xs[i] = xs[i] * keep[sum(Cs[:i]):sum(Cs[:i]) + C][None, :, None]
    Creal = Ctot * pad[0] // pad[1] if pad else Ctot
    groups = ref_cpu.gn_groups(Creal)
    count = (Creal // groups) * L
    fa, fb = film_rows(B, Ctot)
    parts, ss, mr = emulate(xs, rows, gw, gb, fa, fb, groups, count)
    r = gr.gn_case(xs, parts, info_of(xs, rows, groups, count), gw, gb, fa, fb)
    for stage in ("b1", "b2"):
        c, bd = r[stage]
        assert torch.isfinite(bd["scale"]).all() and torch.isfinite(bd["shift"]).all(), (geom[0], form, stage)  # the bound covers the form
        shares = [gr.worst_share(ss[:, :, 0], c["scale"], bd["scale"])[1], gr.worst_share(ss[:, :, 1], c["shift"], bd["shift"])[1],
                  gr.worst_share(mr[:, :, 0], c["mean"], bd["mean"])[1], gr.worst_share(mr[:, :, 1], c["rstd"], bd["rstd"])[1]]
        assert max(shares) <= 1.0, (geom[0], form, stage, shares)
    rel = (r["b2"][1]["scale"] / r["b2"][0]["scale"].abs().clamp(min=1e-30))[:, gw != 0].max().item()
    print(f"[bound] {geom[0]} {form}: end-to-end bound of scale, relative, at most {rel:.2e}")
    assert rel < (0.5 if form == "dc80" else 1e-3)


# ------------------------------------------------------------------------------------------------------------------ planted defects
def flat_read(parts, nt_read, C_read, c_of, B):
    """What gn_prepare's address arithmetic p[b * nt * C + t * C + c] reads from a source's partials [B, ntiles, C, 2] laid out flat,
    with `nt_read` tiles assumed and channel indices c_of [C_read]: totals [B, C_read, 2] (reads past the end: zeros)."""
    flat = torch.cat([parts.double().reshape(-1, 2), torch.zeros(4 * parts.shape[1] * parts.shape[2], 2, dtype=torch.float64)])
    C = parts.shape[2]
    out = torch.zeros(B, C_read, 2, dtype=torch.float64)
    for b in range(B):
        for t in range(nt_read):
            out[b] += flat[(b * nt_read + t) * C + c_of]
    return out


def defect_factor(name, got_scale, got_shift, c, bd):
    f = max(gr.worst_share(got_scale, c["scale"], bd["scale"])[1], gr.worst_share(got_shift, c["shift"], bd["shift"])[1])
    print(f"[defect] {name}: exceeds its bound by a factor of {f:.1f}")
    return f


def setup(Cs, L, rows, form="n01", pad=None, seed=90):
    B, Ctot = 3, sum(Cs)
    xs = [form_of(pw.wave((B, C, L), seed + i), form).half().float() for i, C in enumerate(Cs)]
    gw, gb = affine(Ctot)
    Creal = Ctot * pad[0] // pad[1] if pad else Ctot
    if pad:
        keep = torch.zeros(Ctot, dtype=torch.bool)
        keep[pw.phys_index(pad[0], Creal)] = True
        gw, gb = gw * keep, gb * keep
        xs = [x * keep[sum(Cs[:i]):sum(Cs[:i]) + x.shape[1]][None, :, None] for i, x in enumerate(xs)]
    groups = ref_cpu.gn_groups(Creal)
    count = (Creal // groups) * L
    fa, fb = film_rows(B, Ctot)
    parts = [gr.tile_sums32(x, r, "pairwise") for x, r in zip(xs, rows)]
    r = gr.gn_case(xs, parts, info_of(xs, rows, groups, count), gw, gb, fa, fb)
    tot = torch.cat([gr.partial_totals(p) for p in parts], dim=1)  # [B, Ctot, 2]
    return dict(xs=xs, parts=parts, tot=tot, gw=gw, gb=gb, fa=fa, fb=fb, groups=groups, count=count, want=r["b2"], B=B, L=L, rows=rows)


def coef(s, tot=None, **kw):
    tot = s["tot"] if tot is None else tot
    args = dict(groups=s["groups"], count=s["count"], gw=s["gw"], gb=s["gb"], fa=s["fa"], fb=s["fb"])
    args.update(kw)
    c = gr.coefficients(tot[:, :, 0], tot[:, :, 1], args.pop("groups"), args.pop("count"), args.pop("gw"), args.pop("gb"), args.pop("fa"), args.pop("fb"), **args)
    return c["scale"], c["shift"]


ROW_GEOM = [g for g in GEOM if len(g[1]) == 1]


@pytest.mark.parametrize("geom", ROW_GEOM, ids=[g[0] for g in ROW_GEOM])
def test_defect_a_miscounted_row(geom):
    """One row past L counted in the ragged tile (the next clip's first row sits there); one halo row counted twice (the first row of
    the last tile, which the tile before it staged as halo)."""
    _id, Cs, L, rows, _pad = geom
    s = setup(Cs, L, rows)
    x = s["xs"][0].double()
    nxt = torch.roll(x, -1, dims=0)[:, :, 0]
    past = s["tot"] + torch.stack([nxt, nxt * nxt], dim=2)
    assert defect_factor(f"{geom[0]}: one row past L", *coef(s, past), *s["want"]) >= FACTOR
    t0 = ((L - 1) // rows[0]) * rows[0]
    halo = x[:, :, max(t0, 1)]
    twice = s["tot"] + torch.stack([halo, halo * halo], dim=2)
    assert defect_factor(f"{geom[0]}: one halo row twice", *coef(s, twice), *s["want"]) >= FACTOR


def test_defect_inv_count_from_the_padded_width(lib_built):
    s = setup((64, 64), 512, (254, 256), pad=(48, 64))
    assert s["groups"] == 32 and s["count"] == 3 * 512
    assert defect_factor("unet48 cat: inv_count from the padded width", *coef(s, count=4 * 512), *s["want"]) >= FACTOR
    s1 = setup((64,), 512, (256,), pad=(48, 64))
    assert s1["groups"] == 16 and defect_factor("unet48 stem: inv_count from the padded width", *coef(s1, count=4 * 512), *s1["want"]) >= FACTOR
    assert defect_factor("unet48 stem: group count from the padded width", *coef(s1, groups=32, count=2 * 512), *s1["want"]) >= FACTOR


def test_defect_group_boundaries_off_by_one_at_cpg_3():
    s = setup((96,), 300, (254,))
    assert 96 // s["groups"] == 3
    assert defect_factor("c96_L300: group boundaries off by one channel", *coef(s, group_shift=1), *s["want"]) >= FACTOR


def test_defects_of_the_second_source(lib_built):
    for name, Cs, L, rows, pad in (("unet32_cat_T1024", (32, 32), 1024, (254, 256), None), ("unet48_cat_T512", (64, 64), 512, (254, 256), (48, 64))):
        s = setup(Cs, L, rows, pad=pad)
        B, C0, C1 = s["B"], Cs[0], Cs[1]
        nt0, nt1 = s["parts"][0].shape[1], s["parts"][1].shape[1]
        assert nt0 != nt1  # (the two producers tile differently: the case reaches "its own ntiles")
        first = gr.partial_totals(s["parts"][0])
        at_c = flat_read(s["parts"][1], nt1, C1, torch.arange(C1) + C0, B)  # channel c, not c - C0
        assert defect_factor(f"{name}: second source read at c", *coef(s, torch.cat([first, at_c], 1)), *s["want"]) >= FACTOR
        other_nt = flat_read(s["parts"][1], nt0, C1, torch.arange(C1), B)  # the first source's ntiles
        assert defect_factor(f"{name}: second source over the first's ntiles", *coef(s, torch.cat([first, other_nt], 1)), *s["want"]) >= FACTOR


@pytest.mark.parametrize("geom", ROW_GEOM, ids=[g[0] for g in ROW_GEOM])
def test_defects_of_film_eps_and_a_stale_tile(geom):
    _id, Cs, L, rows, _pad = geom
    s = setup(Cs, L, rows)
    assert defect_factor(f"{geom[0]}: FiLM applied to scale only", *coef(s, film_scale_only=True), *s["want"]) >= FACTOR
    q = setup(Cs, L, rows, form="x1e-3")  # var << eps: the form of section 4 that makes eps decide
    assert defect_factor(f"{geom[0]}: eps left out (input x 1e-3)", *coef(q, eps=0.0), *q["want"]) >= FACTOR
    # a longer earlier call (2 L + 96 rows of 3 N(0, 1)) left one more tile behind this call's last one
    old = gr.tile_sums32(3.0 * pw.wave((s["B"], Cs[0], 2 * L + 96), 99), rows[0], "pairwise")
    nt = s["parts"][0].shape[1]
    assert old.shape[1] > nt
    assert defect_factor(f"{geom[0]}: a stale tile of a longer call", *coef(s, s["tot"] + old[:, nt].double()), *s["want"]) >= FACTOR


# ------------------------------------------------------------------------------------------------------------------ stage (c)
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("C,Lin,avg", [(512, 250, False), (256, 253, True), (64, 592, False)])
def test_xform_reference_bound_and_planted_defect(C, Lin, avg, mode):
    B = 2
    x = (0.2 + 1.3 * pw.wave((B, C, Lin), 77)).half().float()
    table = torch.stack([1.0 + 0.1 * pw.wave((B, C), 78), 0.3 * pw.wave((B, C), 79)], dim=2)
    want, bound = gr.xform_ref(x, table, avg, mode)
    assert want.shape == (B, C, Lin // 2 if avg else Lin)  # (an odd input length drops its last row)
    # the kernel's formula in float32: fma, the mode's GELU form, [mean of two rows], one rounding to the storage type
    u = pw._fma(x.numpy(), table[:, :, 0:1].numpy(), table[:, :, 1:2].numpy())
    g = torch.from_numpy(pw.gelu_formula(u, gr.GELU_FORM[mode]))
    if avg:
        g = (g[:, :, 0:2 * (Lin // 2):2] + g[:, :, 1:2 * (Lin // 2):2]) * 0.5
    got = g.half().float() if mode == "fp16" else g
    e, share, where = gr.worst_share(got, want, bound)
    print(f"[xform] C={C} Lin={Lin} avg={avg} {mode}: float32 formula error {e:.2e}, share {share:.3f}")
    assert share <= 1.0
    if avg:
        bad, _ = gr.xform_ref(x, table, avg, mode, rows_from=-1)
        f = gr.worst_share(bad, want, bound)[1]
        print(f"[defect] xform C={C} Lin={Lin} {mode}: averaging rows 2t - 1, 2t exceeds the bound by a factor of {f:.0f}")
        assert f >= FACTOR
        keep, _ = gr.xform_ref(x[:, :, :Lin - 1] if Lin & 1 else x, table, avg, mode)
        assert torch.equal(keep, want)


# ------------------------------------------------------------------------------------------------------------------ the recorded run
def test_recorded_margins_cover_every_case_and_stay_inside_their_bounds():
    path = os.path.join(ROOT, "profiles", gr.MARGINS)
    recs = [json.loads(ln) for ln in open(path)]
    gn = [r for r in recs if r["test"] == "groupnorm.gn"]
    cases = {r["case"] for r in gn}
    want = {f"{c}.{m}" for c, v in list(gr.BLOCK_CASES.items()) + [(c, (0,) * 6 + (v[3],)) for c, v in gr.MODEL_CASES.items()] for m in v[6]}
    assert all(r["forms"] == list(gr.FORMS) for r in gn if r["case"].split(".")[0] in gr.BLOCK_CASES)
    assert cases == want, (sorted(want - cases), sorted(cases - want))
    for r in recs:
        for k, v in r.items():
            if k.startswith("share"):
                assert all(0.0 <= x <= 1.0 for x in (v if isinstance(v, list) else [v])), r
    dc = [r for r in gn if "ratio_to_torch_float32" in r]
    assert {r["case"].split(".")[0] for r in dc} >= set(gr.BLOCK_CASES) | {"unet32_dc"}
