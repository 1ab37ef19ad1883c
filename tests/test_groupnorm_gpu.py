"""GroupNorm's statistics and coefficients on the device against float64, entry by entry (cases, references and bounds:
tests/groupnorm_ref.py), through the debug entries vqvs_debug_gn_* / vqvs_debug_xform_* of a debug_taps handle.

  per GroupNorm  (a) the tile partials' totals against the stored sources; (b1) the (scale, shift) [and (mean, rstd)] table against the
                 float64 coefficients of the kernel's own partials; (b2) against those of the stored sources
  per xform      (c) its output against gelu(scale x + shift) [avg-pooled] of the kernel's own table and the stored input
  block cases    four input forms each; run again on the same handle straight after a longer, larger forward: every read-back array
                 bitwise equal (stale partials); the flags show which builder made the table
  both builders  gn_prepare_kernel and the convolution's own gn_table, one interpreter each: outputs bitwise equal per clip
  range guard    the 9e8 threshold from both sides, seen by either copy of the guard

Each GroupNorm's largest share of each bound is recorded under VQVS_MARGINS_DIR (profiles/groupnorm_margins.jsonl)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import groupnorm_ref as gr
import pointwise_ref as pw
from util import record_margin
from vq_voice_swap_amd import Classifier, UNetPredictor, _native
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.unet import ResBlockModule, pad_blocks, pad_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sig3(v):
    return float(f"{v:.3g}")


_block_recs = {}  # (case.mode, gn) -> the records of the input forms so far; written as one record with the last form


def emit(rec, forms=None):
    """A whole model's record at once; a block case's GroupNorm as one record over its input forms (groupnorm_ref.merge_records)."""
    if forms is None:
        return record_margin(gr.MARGINS, rec)
    print("[form] " + json.dumps(rec))
    got = _block_recs.setdefault((rec["case"].rsplit(".", 1)[0], rec["gn"]), [])
    got.append(rec)
    if rec["case"].endswith("." + forms[-1]):
        record_margin(gr.MARGINS, gr.merge_records(got))


def audit(h, B, T, mode, sd, case, stem=None, dc=False, forms=None):
    """Stages (a), (b), (c) of every GroupNorm and xform entry of the last forward.  stem: (tap, totals) of the in_conv output in a
    2-byte mode.  Returns (failures, every read-back array in order)."""
    fails, arrays, tables = [], [], []
    film = h.read_film(B) if any(h.gn_info(i, B, T)["film"] for i in range(h.gn_count())) else None
    for i in range(h.gn_count()):
        info = h.gn_info(i, B, T)
        ns = len(info["srcs"])
        xs = [h.gn_source(i, B, T, s) for s in range(ns)]
        ps = [h.gn_partials(i, B, T, s) for s in range(ns)]
        ss = h.gn_table(i, B, T)
        mr = h.gn_table(i, B, T, mean_rstd=True) if info["has_mr"] else None
        arrays += xs + ps + [ss] + ([mr] if mr is not None else [])
        tables.append(ss)
        Ct = info["Ctot"]
        gw, gb = sd[info["name"] + ".weight"].float(), sd[info["name"] + ".bias"].float()
        fa = fb = None
        if info["film"]:
            fa, fb = film[:, info["film_off"]:info["film_off"] + Ct], film[:, info["film_off"] + Ct:info["film_off"] + 2 * Ct]
        # a source whose producer summed unrounded float32 values: the stem has the float64 stem, a convolution the storage-rounding term
        totals = [stem[1] if stem is not None and x.shape == stem[0].shape and torch.equal(x, stem[0]) else
                  ("unrounded" if mode != "fp32" and not sr["sums_stored"] else None) for x, sr in zip(xs, info["srcs"])]
        if stem is not None:
            assert all(not sr["sums_stored"] for t, sr in zip(totals, info["srcs"]) if isinstance(t, dict)), info
        r = gr.gn_case(xs, ps, info, gw, gb, fa, fb, totals)
        # one compact record per GroupNorm: the largest share of each bound (three digits), and where the largest of each stage sits
        rec = dict(test="groupnorm.gn", case=case, gn=i, name=info["name"], fused=int(info["fused"]), n=[a["n"] for a in r["a"]])
        if any(totals):
            rec["ref"] = ["float64 stem" if isinstance(t, dict) else (t or "stored") for t in totals]
        if any(a["whole_clip"] for a in r["a"]):
            rec["whole_clip"] = True
        shares = {}
        for s, a in enumerate(r["a"]):
            for k, col in (("s1", 0), ("s2", 1)):
                e, sh, w = gr.worst_share(a["got"][:, :, col], a[k], a["d" + k[1]])
                shares[f"share_a_{k}_src{s}"] = (sh, w, e)
        group_of = r["b1"][0]["group_of"]
        for st in ("b1", "b2"):
            c, bd = r[st]
            e, sh, w = gr.worst_share(ss[:, :, 0], c["scale"], bd["scale"])
            shares[f"share_{st}_scale"] = (sh, w, e)
            e, sh, w = gr.worst_share(ss[:, :, 1], c["shift"], bd["shift"])
            shares[f"share_{st}_shift"] = (sh, w, e)
            if mr is not None:
                e, sh, w = gr.worst_share(mr[:, :, 0], c["mean"][:, group_of], bd["mean"][:, group_of])
                shares[f"share_{st}_mean"] = (sh, w, e)
                e, sh, w = gr.worst_share(mr[:, :, 1], c["rstd"][:, group_of], bd["rstd"][:, group_of])
                shares[f"share_{st}_rstd"] = (sh, w, e)
        for k, (sh, w, e) in shares.items():
            if not sh <= 1.0:
                fails.append(f"{case} gn {i} {info['name']}: {k} = {sh:.3g} at {w} (|error| {e:.3g})")
        for st in ("a", "b1", "b2"):
            of = {k[len("share_") + len(st) + 1:]: v for k, v in shares.items() if k.startswith(f"share_{st}_")}
            top = max(of, key=lambda k: of[k][0] if of[k][0] == of[k][0] else float("inf"))
            rec["share_" + st] = [sig3(v[0]) for v in of.values()]  # (a: s1, s2 per source; b1, b2: scale, shift[, mean, rstd])
            if st != "b1":  # (where b1's largest sits is the fall of a float32 rounding: not recorded)
                rec["at_" + st] = [top] + of[top][1]
        if dc:  # recorded, not gated: the kernel's coefficient error against torch's own float32 group_norm statistics' (two-pass)
            c2 = r["b2"][0]
            x32 = torch.cat(xs, dim=1).float()
            _o, m32, r32 = torch.native_group_norm(x32, None, None, B, Ct, x32.shape[2], info["groups"], gr.EPS)
            if info["count"] != (Ct // info["groups"]) * x32.shape[2]:  # (a padded handle: torch counts the zero channels too)
                m32 = r32 = None
            if m32 is not None:
                sc = gr.f64(r32)[:, group_of] * gr.f64(gw) * ((gr.f64(fa) + 1.0) if fa is not None else 1.0)
                live = gw != 0
                ek = ((gr.f64(ss[:, :, 0]) - c2["scale"]).abs() / c2["scale"].abs().clamp(min=1e-30))[:, live].max().item()
                et = ((sc - c2["scale"]).abs() / c2["scale"].abs().clamp(min=1e-30))[:, live].max().item()
                rec["scale_rel_err"], rec["torch_float32_scale_rel_err"] = sig3(ek), sig3(et)
                rec["ratio_to_torch_float32"] = sig3(ek / max(et, 2.0 ** -60))
        emit(rec, forms)
    for j in range(h.xform_count()):
        xi = h.xform_info(j, B, T)
        xin, xout = h.xform_tensor(j, B, T, False), h.xform_tensor(j, B, T, True)
        arrays += [xout]
        tab = tables[xi["gn"]][:, xi["ss_c0"]:xi["ss_c0"] + xi["C"]]
        want, bound = gr.xform_ref(xin, tab, xi["avg"], mode)
        ok_shape = tuple(xout.shape) == tuple(want.shape) and tables[xi["gn"]].shape[1] == xi["ss_stride"]
        e, sh, w = gr.worst_share(xout, want, bound) if ok_shape else (float("nan"), float("inf"), [])
        record_margin(gr.MARGINS, dict(test="groupnorm.xform", case=case, xform=j, share_c=sig3(sh), at_c=w, **xi))
        if not sh <= 1.0:
            fails.append(f"{case} xform {j} {xi}: share {sh:.3g} at {w} (|error| {e:.3g})")
    return fails, arrays


# ------------------------------------------------------------------------------------------------------------------ single blocks
@functools.lru_cache(maxsize=None)
def block_model(case, mode):
    cin, cout, scale, dil, L, B, _modes = gr.BLOCK_CASES[case]
    m = ResBlockModule(cin, gr.EMB, cout, scale, dil)
    det_init_((f"gn.{case}." + k, v) for k, v in m.block.state_dict().items())
    m.set_precision(mode)
    m.debug_taps = True
    m.handle(DEV, B + 1, 2 * L + 96)  # built once, for the longer and larger forward too
    return m


def expect_fused(info, mode, xform_gns, i):
    cpg = info["Ctot"] // info["groups"]
    return (mode == "fp16" and info["Ctot"] % 64 == 0 and info["srcs"][0]["C"] % 64 == 0 and cpg & (cpg - 1) == 0 and not info["has_mr"]
            and i not in xform_gns and max(s["ntiles"] for s in info["srcs"]) <= 32)


BLOCK_PARAMS = [(c, m, f) for c, v in gr.BLOCK_CASES.items() for m in v[6] for f in gr.FORMS]


@pytest.mark.parametrize("case,mode,form", BLOCK_PARAMS, ids=[".".join(p) for p in BLOCK_PARAMS])
def test_block_groupnorms_vs_float64(lib_built, case, mode, form):
    cin, cout, scale, dil, L, B, _modes = gr.BLOCK_CASES[case]
    m = block_model(case, mode)
    h = m._handle
    x, e = gr.block_input(case, form)
    xl, el = gr.long_input(case)
    h.status()
    m(x.to(DEV), e.to(DEV))
    assert m._handle is h and h.status() == 0
    fails, first = audit(h, B, L, mode, m.block.state_dict(), f"{case}.{mode}.{form}", dc=form == "dc80", forms=gr.FORMS)
    # the flags: which builder made each table, and the xform entries the case is meant to reach
    infos = [h.gn_info(i, B, L) for i in range(h.gn_count())]
    xf = [h.xform_info(j, B, L) for j in range(h.xform_count())]
    assert [g["name"] for g in infos] == ["pre_cond.0.0", "pre_cond.3"] and infos[1]["film"] and not infos[0]["film"]
    assert infos[0]["srcs"][0]["tile_rows"] == 256  # (ntc_stats)
    assert all(s_["sums_stored"] for g in infos for s_ in g["srcs"]) or (mode == "fp16" and cin == 32 and cout == 64)
    for i, g in enumerate(infos):
        assert g["fused"] == expect_fused(g, mode, {x_["gn"] for x_ in xf}, i), (case, mode, i, g)
    if mode == "fp16" and cin >= 64 and cin % 64 == 0:
        assert infos[0]["fused"], infos[0]
    want_xf = {"c512_d8_L250": [(0, False), (1, False)], "c512_avg_L254": [(0, True), (1, False)]}.get(case, []) if mode == "fp32" else []
    if mode == "fp32" and cout >= 512:
        assert [(x_["gn"], x_["avg"]) for x_ in xf] == want_xf, xf
    if mode == "fp16":
        assert xf == []
    if case == "c512_avg_L254":
        assert xf[0]["Lin"] == 254 and xf[0]["Lout"] == 127
    if case in ("c256_d16_L255", "c256_d16_L256") and mode == "fp16":  # conv 1's tiles are 254 rows in the 2-byte modes: GroupNorm 2 adds two statistics tiles
        assert infos[1]["srcs"][0]["ntiles"] == 2  # (whether one workgroup tile wrote both is recorded: srcs[].whole_clip)
    # the same call again, straight after a forward of B + 1 clips of 2 L + 96 rows on the same handle
    m(xl.to(DEV), el.to(DEV))
    h.status()
    m(x.to(DEV), e.to(DEV))
    assert m._handle is h and h.status() == 0
    second = []
    for i, g in enumerate(infos):
        ns = len(g["srcs"])
        second += [h.gn_source(i, B, L, s) for s in range(ns)] + [h.gn_partials(i, B, L, s) for s in range(ns)] + [h.gn_table(i, B, L)]
        second += [h.gn_table(i, B, L, mean_rstd=True)] if g["has_mr"] else []
    second += [h.xform_tensor(j, B, L, True) for j in range(len(xf))]
    assert len(first) == len(second)
    for k, (a, b) in enumerate(zip(first, second)):
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
            fails.append(f"{case}.{mode}.{form}: read-back array {k} of shape {tuple(a.shape)} changed after a longer forward "
                         f"({int((a.view(torch.int32) != b.view(torch.int32)).sum())} entries)")
    assert not fails, "\n".join(fails)


def test_a_resizing_block_keeps_its_width(lib_built):
    """The three resizing blocks of the issue's table change their width; the library builds none of them (groupnorm_ref.BLOCK_CASES)."""
    for cin, cout, scale in gr.REFUSED_AS_THE_ISSUE_STATES_THEM:
        m = ResBlockModule(cin, gr.EMB, cout, scale, 1)
        with pytest.raises(_native.NativeArgumentError, match="cannot change channels"):
            m.handle(DEV, 1, 256)
    m = ResBlockModule(512, gr.EMB, 512, 0.5, 1)  # ... nor an avg-pooled block at the issue's odd length
    with pytest.raises(_native.NativeArgumentError, match="needs even L"):
        m(torch.zeros(1, 512, 253, device=DEV), torch.zeros(1, gr.EMB, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ whole models
@functools.lru_cache(maxsize=None)
def whole_model(case, mode):
    kind, kw, T, _modes, _form = gr.MODEL_CASES[case]
    m = UNetPredictor(**kw) if kind == "unet" else Classifier(5, **kw)
    det_init_((f"gn.{case.split('_')[0]}." + k, v) for k, v in m.state_dict().items())
    m.eval()
    m.set_precision(mode)
    m.debug_taps = True
    return m


MODEL_PARAMS = [(c, m) for c, v in gr.MODEL_CASES.items() for m in v[3]]


@pytest.mark.parametrize("case,mode", MODEL_PARAMS, ids=[".".join(p) for p in MODEL_PARAMS])
def test_model_groupnorms_vs_float64(lib_built, case, mode):
    kind, kw, T, _modes, form = gr.MODEL_CASES[case]
    B = gr.B_MODEL
    m = whole_model(case, mode)
    x = gr.model_input(case)
    ts, labels, _ = pw.clip_inputs(B)
    if kind == "unet":
        m(x.to(DEV), ts.to(DEV), labels=(labels % kw["num_labels"]).to(DEV))
    else:
        m(x.to(DEV), ts.to(DEV))
    h = m._handle
    assert h.status() == 0
    sd = m.state_dict()
    q, qp = pad_blocks(kw["base_channels"])
    if q != qp:
        sd = pad_state(sd, _native.param_table(h.cfg), q, qp)
    stem = None
    if mode != "fp32":
        key = [k for k in sd if k.endswith("in_conv.weight")][0]
        names = [n for n, _c, _l in h.taps()]
        tap = h.read_tap([i for i, n in enumerate(names) if n.endswith("in_conv")][0], B, T)
        stem = (tap, gr.stem_totals(sd[key], sd[key[:-6] + "bias"], x))
    fails, _arrays = audit(h, B, T, mode, sd, f"{case}.{mode}", stem=stem, dc=form == "dc")
    infos = [h.gn_info(i, B, T) for i in range(h.gn_count())]
    xf = [h.xform_info(j, B, T) for j in range(h.xform_count())]
    two = [g for g in infos if len(g["srcs"]) == 2]
    if kind == "unet":
        assert len(two) >= len(kw["channel_mult"]) and infos[-1]["name"] == "out.0.0" and not infos[-1]["film"]
        assert any(g["srcs"][0]["ntiles"] != g["srcs"][1]["ntiles"] for g in two)  # (a second source with its own ntiles)
        assert not any(g["has_mr"] for g in infos)
        if mode == "fp16":
            assert any(g["fused"] and g["Ctot"] >= 64 for g in infos)
            assert not infos[0]["srcs"][0]["sums_stored"]  # (the stem)
            if kw["base_channels"] == 32:  # 32 -> 64 channels: conv 1 is a single K chunk, which runs on conv_mfma_kernel
                assert [g["name"] for g in infos if not g["srcs"][0]["sums_stored"] and len(g["srcs"]) == 1 and g["name"].endswith("pre_cond.3")]
        else:
            assert not any(g["fused"] for g in infos) and all(s_["sums_stored"] for g in infos for s_ in g["srcs"])
    else:
        assert all(g["has_mr"] and not g["fused"] for g in infos) and not two
    if case == "unet48":  # groups and counts from the real width, channels from the physical one
        g0 = infos[0]
        assert (g0["Ctot"], g0["groups"], g0["count"]) == (64, 16, 3 * T)
    if case == "unet32_wide":
        assert any(x_["ss_c0"] != 0 and len(infos[x_["gn"]]["srcs"]) == 2 for x_ in xf), xf
    if stem is not None:
        assert infos[0]["srcs"][0]["tile_rows"] == 256
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------------ one interpreter per run
_stopped = []  # set by the first child that did not end cleanly: nothing further is started on the GPU


def child(spec, tmp_path, name, gn_env, seconds=240):
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]} ended without a clean exit, nothing further runs on the GPU")
    out = tmp_path / (name + ".pt")
    env = {k: v for k, v in os.environ.items() if k != "VQVS_WS_GN"}
    if gn_env is not None:
        env["VQVS_WS_GN"] = gn_env
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.join(ROOT, "tests", "groupnorm_child.py"), json.dumps(spec), str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    if r.returncode != 0 or "GN_CHILD_OK" not in r.stdout:
        _stopped.append(name)
        pytest.fail(f"{name}: exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}")
    return torch.load(out, weights_only=False)


@pytest.mark.parametrize("case", gr.GN_TABLE_CASES)
def test_both_table_builders_give_the_same_bits(lib_built, case, tmp_path):
    """The convolution's own gn_table (default) against gn_prepare_kernel (VQVS_WS_GN=0) on the same partials, fp16: the output is
    expected bitwise equal per clip -- both evaluate the same float64 expressions and differ only in the order of float64 additions."""
    a = child(dict(what="table", case=case), tmp_path, case + ".default", None)
    b = child(dict(what="table", case=case), tmp_path, case + ".gn0", "0")
    assert any(a["fused"]) and not any(b["fused"]), (a["fused"], b["fused"])  # each run used the builder it is meant to
    assert a["status"] == 0 and b["status"] == 0
    for pa, pb in zip(a["partials"][0], b["partials"][0]):  # GroupNorm 1 reads the same partials in both runs
        assert torch.equal(pa, pb)
    differ = (a["out"] != b["out"]).flatten(1).any(dim=1)
    chans = (a["out"] != b["out"]).any(dim=2)
    print(f"[builders] {case}: clips that differ {differ.nonzero().flatten().tolist()}, (clip, channel) pairs {int(chans.sum())} of {chans.numel()}")
    assert not differ.any(), (case, differ.nonzero().flatten().tolist(), chans.nonzero().tolist()[:20])


@pytest.mark.parametrize("gn_env", [None, "0"], ids=["gn_table", "gn_prepare"])
def test_range_guard_threshold_in_either_copy(lib_built, gn_env, tmp_path):
    """256 rows of +-1800 sum to 8.3e8 < 9e8: status 0.  +-1900: 9.2e8: bit 1 and not bit 0.  Nothing overflows (1900 is well inside fp16)."""
    lo = child(dict(what="guard", magnitude=1800), tmp_path, f"guard1800.{gn_env}", gn_env)
    hi = child(dict(what="guard", magnitude=1900), tmp_path, f"guard1900.{gn_env}", gn_env)
    for r in (lo, hi):
        assert r["fused"][0] == (gn_env is None), r["fused"]  # the copy of the guard that saw the tile
        assert r["infos"][0]["srcs"][0]["ntiles"] == 1 and bool(torch.isfinite(r["out"]).all())
    p = hi["partials"][0][0]
    assert float(p[:, 0, :, 1].min()) >= 9.0e8 and float(lo["partials"][0][0][:, 0, :, 1].max()) < 9.0e8
    assert lo["status"] == 0, lo["status"]
    assert hi["status"] & 2 and not hi["status"] & 1, hi["status"]
