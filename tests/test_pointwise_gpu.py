"""The non-convolution kernels of a UNet forward against float64, entry by entry (cases, references and bounds: tests/pointwise_ref.py).

  Stage A  the GELU device functions of csrc/common.hpp through vqvs_debug_gelu
  Stage B  time_embed_kernel: label table, vector per clip, no labels; widths up to the kernel's E = 1024 and a padded one
  Stage C  film_kernel: every row, one / full / one-into-the-second / three clip tiles
  Stage D  in_conv_kernel and out_conv_kernel / out_conv_rows_kernel from the debug taps, around the 256-row tile ends

Each test records its largest error and the largest share of its bound under VQVS_MARGINS_DIR (profiles/pointwise_margins.jsonl)."""
import functools

import numpy as np
import pytest
import torch

import pointwise_ref as pw
from util import record_margin
from vq_voice_swap_amd import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ("fp32", "fp16")


def record(test, case, err, share, where, **more):
    record_margin(pw.MARGINS, dict(test="pointwise." + test, case=case, max_err=err, share_of_bound=share, where=where, **more))


@functools.lru_cache(maxsize=None)
def model_of(key, mode, labels=True, taps=False):
    """One module per (model, precision, labels, taps) for the whole file: its handle is built once, at the largest batch and length."""
    kw = dict(pw.EXTRA[key]) if key in pw.EXTRA else dict(base=key)
    m = pw.make_model(kw.pop("base"), labels=labels, **kw)
    m.set_precision(mode)
    m.debug_taps = taps
    return m


# ------------------------------------------------------------------------------------------------------------------ Stage A
@functools.lru_cache(maxsize=None)
def gelu_run(form):
    x = pw.gelu_inputs()
    return x, _native.debug_gelu(torch.from_numpy(x).to(DEV), form).cpu().numpy()


@pytest.mark.parametrize("name", list(pw.FORMS))
def test_gelu_forms_vs_float64(lib_built, name):
    form = pw.FORMS[name]
    x, got = gelu_run(form)
    want, gate = pw.gelu_want(x, form), pw.gelu_gate(x, form)
    a = np.abs(x.astype(np.float64))
    err = np.abs(got.astype(np.float64) - want)
    e, share, i = pw.worst(got, want, gate)
    inner = float(err[a <= 4.0].max())
    tail = float((err[a > 8.0] / a[a > 8.0]).max())
    record("gelu", name, float(err[a <= 8.0].max()), share, float(x[i]), max_err_inner4=inner, max_tail_rel=tail)
    assert share <= 1.0, (name, e, share, float(x[i]))
    # what csrc/common.hpp states about the form (the gates are these figures rounded up)
    if form in pw.COMMON_HPP:
        assert float(err[a <= 8.0].max()) <= pw.GELU_GATE[form]
    if form == 3:
        assert inner <= pw.GELU_GATE_INNER[3]


def test_gelu_specials_and_agreement(lib_built):
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1e-40, -1e-40, 3.0], device=DEV)  # (odd tail for the pair forms below)
    out = {name: _native.debug_gelu(x, form).cpu().numpy() for name, form in pw.FORMS.items()}
    for name, form in pw.FORMS.items():
        assert np.isnan(out[name][0]), name
        want, gate = pw.gelu_want(x.cpu().numpy()[3:], form), pw.gelu_gate(x.cpu().numpy()[3:], form)
        assert (np.abs(out[name][3:].astype(np.float64) - want) <= gate).all(), name
        odd = _native.debug_gelu(x[3:], form).cpu().numpy()  # 5 values: the last pair's partner is padding
        assert np.array_equal(odd, out[name][3:]), name
    g0, g1 = gelu_run(0)[1], gelu_run(1)[1]
    ulps = np.abs(g0.astype(np.float64) - g1.astype(np.float64)) / np.spacing(np.maximum(np.abs(g0), np.abs(g1)) + np.float32(1e-45)).astype(np.float64)
    record("gelu_forms_0_1", "agreement", float(np.abs(g0.astype(np.float64) - g1).max()), float(ulps.max()) / pw.FORM01_ULPS, float(gelu_run(0)[0][int(ulps.argmax())]),
           bitwise=bool(np.array_equal(g0, g1)), at_inf={n: [float(out[n][1]), float(out[n][2])] for n in pw.FORMS})
    assert ulps.max() <= pw.FORM01_ULPS


def test_debug_gelu_arguments(lib_built):
    x = torch.zeros(4, device=DEV)
    L = _native.lib()
    assert L.vqvs_debug_gelu(x.data_ptr(), x.data_ptr(), 4, 5, None) == -1 and "form" in _native.last_error()
    assert L.vqvs_debug_gelu(x.data_ptr(), x.data_ptr(), 0, 0, None) == -1 and "n=" in _native.last_error()


# ------------------------------------------------------------------------------------------------------------------ Stage B
def forward(m, B, T, ts, labels=None, vectors=None, cond=None, seed=7800):
    Cin = m.in_channels
    x = pw.wave((B, Cin, T), seed + 13 * B + T)
    out = m(x.to(DEV), ts.to(DEV), cond=None if cond is None else cond.to(DEV), labels=None if labels is None else labels.to(DEV),
            vectors=None if vectors is None else vectors.to(DEV))
    return x, out.cpu()


def read_emb(m, B):
    """The conditioning vector at the real width, and the largest |pad entry|."""
    e = m._handle.read_embedding(B)
    idx = pw.phys_index(m.base_channels, 4 * m.base_channels)
    pad = torch.ones(e.shape[1], dtype=torch.bool)
    pad[idx] = False
    return e[:, idx], float(e[:, pad].abs().max()) if pad.any() else 0.0


@pytest.mark.parametrize("path", ["labels", "vectors", "none"])
@pytest.mark.parametrize("base", pw.EMB_BASES)
def test_embedding_vs_float64(lib_built, base, path):
    B = 33
    got = {}
    c = pw.emb_case(model_of(base, MODES[0], labels=path != "none"), B, path)
    for mode in MODES:
        m = model_of(base, mode, labels=path != "none")
        forward(m, B, 2, c["ts"], c["labels"], c["vectors"])
        got[mode], pad = read_emb(m, B)
        assert pad == 0.0, (base, path, mode, pad)
    assert c["eref"] <= pw.EREF_MAX
    e, share, i = pw.worst(got["fp32"].numpy(), c["want"].numpy(), c["bound"][None, :].expand_as(c["want"]).numpy())
    record("embedding", f"base{base}.{path}", e, share, [i // got["fp32"].shape[1], i % got["fp32"].shape[1]], e_ref=c["eref"],
           bound_max=float(c["bound"].max()))
    assert share <= 1.0, (base, path, e, share)
    assert torch.equal(got["fp32"], got["fp16"]), (base, path)  # the buffers are float32 in both modes


# ------------------------------------------------------------------------------------------------------------------ Stage C
def read_film(m, B):
    f = m._handle.read_film(B)
    idx, R = pw.film_index(m.base_channels)
    assert f.shape[1] == R
    pad = torch.ones(R, dtype=torch.bool)
    pad[idx] = False
    return f[:, idx], float(f[:, pad].abs().max()) if pad.any() else 0.0


@pytest.mark.parametrize("B", [65, 1, 31, 32, 33])  # (the largest first: the handle is built once)
@pytest.mark.parametrize("base", pw.EMB_BASES)
def test_film_rows_vs_float64(lib_built, base, B):
    m = model_of(base, "fp16")
    ts, labels, _ = pw.clip_inputs(B)
    forward(m, B, 2, ts, labels)
    emb, _ = read_emb(m, B)
    got, pad = read_film(m, B)
    assert pad == 0.0
    want, bound = pw.film_ref(m, emb)
    e, share, i = pw.worst(got.numpy(), want.numpy(), bound.numpy())
    record("film", f"base{base}.B{B}", e, share, [i // got.shape[1], i % got.shape[1]], rows=got.shape[1])
    assert share <= 1.0, (base, B, e, share, divmod(i, got.shape[1]))


@pytest.mark.parametrize("base", pw.EMB_BASES)
def test_film_rows_do_not_depend_on_the_batch(lib_built, base):
    m = model_of(base, "fp16")
    ts, labels, _ = pw.clip_inputs(65)
    forward(m, 65, 2, ts, labels)
    full = m._handle.read_film(65)
    m32 = model_of(base, "fp32")
    forward(m32, 65, 2, ts, labels)
    assert torch.equal(m32._handle.read_film(65), full)  # float32 in both modes
    for b in (0, 31, 32, 33, 64):
        forward(m, 1, 2, ts[b:b + 1], labels[b:b + 1])
        assert torch.equal(m._handle.read_film(1)[0], full[b]), (base, b)


# ------------------------------------------------------------------------------------------------------------------ Stage D
@functools.lru_cache(maxsize=None)
def tap_run(key, mode, T, B):
    """(x, cond, in_conv tap, last block's tap, output) of one forward with debug taps, on the CPU."""
    m = model_of(key, mode, taps=True)
    if m._handle is None:
        m.handle(DEV, max(pw.STEM_B), max(pw.STEM_T))
    ts, labels, _ = pw.clip_inputs(B)
    cond = pw.wave((B, m.cond_channels, pw.COND_LEN), 7900 + B) if m.cond_channels else None
    x, out = forward(m, B, T, ts, labels, cond=cond)
    h = m._handle
    names = [n for n, _c, _l in h.taps()]
    return x, cond, h.read_tap(names.index("in_conv"), B, T), h.read_tap(len(names) - 1, B, T), out


def stem_cases(key):
    return [(T, B) for T in ((pw.COND_T,) if key == "cond" else pw.STEM_T) for B in pw.STEM_B]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", list(pw.STEM_BASES) + list(pw.EXTRA))
def test_stem_vs_float64(lib_built, key, mode):
    for T, B in stem_cases(key):
        x, cond, tap, _last, _out = tap_run(key, mode, T, B)
        r = pw.stem_ref(model_of(key, mode, taps=True), x, cond)
        bound = r["bound32" if mode == "fp32" else "bound16"]
        e, share, i = pw.worst(tap.numpy(), r["want"].numpy(), bound.numpy())
        where = list(np.unravel_index(i, tuple(tap.shape)))
        record("stem", f"{key}.{mode}.T{T}.B{B}", e, share, [int(v) for v in where], rel_rms=pw.rel_rms(tap.numpy(), r["want"].numpy()))
        assert share <= 1.0, (key, mode, T, B, e, share, where)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", list(pw.STEM_BASES) + list(pw.EXTRA))
def test_head_vs_float64(lib_built, key, mode):
    for T, B in stem_cases(key):
        _x, _cond, _tap, last, out = tap_run(key, mode, T, B)
        m = model_of(key, mode, taps=True)
        r = pw.head_ref(m, last, mode)
        e, share, i = pw.worst(out.numpy(), r["want"].numpy(), r["bound"].numpy())
        where = list(np.unravel_index(i, tuple(out.shape)))
        record("head", f"{key}.{mode}.T{T}.B{B}", e, share, [int(v) for v in where], e_ref=r["eref"], rel_rms=pw.rel_rms(out.numpy(), r["want"].numpy()))
        assert share <= 1.0, (key, mode, T, B, e, share, where)
