"""The C boundary has one declaration, include/vqvs.h: the parser that turns it into ctypes prototypes (vq_voice_swap_amd/_abi.py) on
literal header text, and the header against the built library -- every declared function is exported and bound, and every exported
vqvs_* symbol is declared."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from vq_voice_swap_amd import _abi, _native

VP = C.c_void_p

TEXT = """
/* a comment with a ; and a vqvs_ghost(int x); inside */
#ifndef VQVS_H
#define VQVS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define VQVS_OK 0
#define VQVS_ERR_ARG (-1)     /* a comment that runs
                                 over two lines */
#define VQVS_FLAG 2u
typedef struct vqvs_model vqvs_model;
typedef struct vqvs_cfg {
  int32_t kind;          /* VQVS_KIND_* */
  int32_t rb_cin, rb_cout, rb_resize /*0 none*/;
  int32_t reserved[5];
  int32_t channel_mult[12];
} vqvs_cfg;
int vqvs_param_count(const vqvs_cfg* cfg);
int vqvs_param_info(const vqvs_cfg* cfg, int index, char* name_out, int name_cap, int64_t shape_out[4], int* ndim_out);
int vqvs_model_create(const vqvs_cfg* cfg, const float* const* h_params, int n_params, int device, vqvs_model** out);
void vqvs_model_destroy(vqvs_model* m);
int64_t vqvs_model_device_bytes(const vqvs_model* m);
int vqvs_step(const float* d_x, float* d_out, const uint8_t* d_keep, const int32_t* d_first, int B,
              uint32_t flags, float scale, uint64_t seed,
              int64_t row_len, void* stream);
int vqvs_pitch(const float* a, long long* counts, double* sums, double eps, unsigned* h_status, unsigned long long* h_counters);
const char* vqvs_last_error(void);
#ifdef __cplusplus
}
#endif
#endif /* VQVS_H */
"""


def test_parser_reads_every_form_the_header_uses():
    class Cfg(C.Structure):
        pass

    abi = _abi.parse(TEXT, Cfg)
    i, f = C.c_int, abi.functions
    assert list(f) == ["vqvs_param_count", "vqvs_param_info", "vqvs_model_create", "vqvs_model_destroy", "vqvs_model_device_bytes",
                       "vqvs_step", "vqvs_pitch", "vqvs_last_error"]  # header order; nothing from inside a comment
    assert f["vqvs_param_count"] == (i, [C.POINTER(Cfg)])
    assert f["vqvs_param_info"] == (i, [C.POINTER(Cfg), i, C.c_char_p, i, VP, VP])  # int64_t shape_out[4], int* ndim_out
    assert f["vqvs_model_create"] == (i, [C.POINTER(Cfg), VP, i, i, C.POINTER(VP)])  # const float* const*, vqvs_model**
    assert f["vqvs_model_destroy"] == (None, [VP])
    assert f["vqvs_model_device_bytes"] == (C.c_int64, [VP])
    assert f["vqvs_step"] == (i, [VP, VP, VP, VP, i, C.c_uint32, C.c_float, C.c_uint64, C.c_int64, VP])  # a multi-line declaration
    assert f["vqvs_pitch"] == (i, [VP, VP, VP, C.c_double, VP, VP])  # long long*, double*, double, unsigned*, unsigned long long*
    assert f["vqvs_last_error"] == (C.c_char_p, [])  # (void)
    assert abi.constants == {"VQVS_OK": 0, "VQVS_ERR_ARG": -1, "VQVS_FLAG": 2}  # VQVS_H has no value: not a constant
    assert [(n, getattr(t, "_length_", 0)) for n, t in abi.cfg_fields] == [("kind", 0), ("rb_cin", 0), ("rb_cout", 0), ("rb_resize", 0),
                                                                            ("reserved", 5), ("channel_mult", 12)]
    assert all((t._type_ if n in ("reserved", "channel_mult") else t) is C.c_int32 for n, t in abi.cfg_fields)
    own = _abi.parse(TEXT).functions["vqvs_param_count"][1][0]  # without a struct type of the caller's: one with the parsed fields
    assert C.sizeof(own._type_) == 4 * (4 + 5 + 12)


@pytest.mark.parametrize("text, named", [
    ("int vqvs_f(const float* d_x, size_t n);", "size_t n"),  # an unknown scalar
    ("int vqvs_f(struct foo* p);", "struct foo* p"),  # an unknown pointer
    ("int vqvs_f(const float** d_x);", "const float** d_x"),  # only vqvs_model** is a pointer to a pointer
    ("int vqvs_f(int);", "int"),  # a parameter without a name: its type cannot be told from its name
    ("int vqvs_f(int32_t n);", "int32_t n"),  # a scalar the header does not use
    ("size_t vqvs_f(int n);", "size_t vqvs_f"),  # an unknown return type
    ("float* vqvs_f(int n);", "float* vqvs_f"),
    ("int other_f(int n);", "other_f"),  # not a vqvs_ entry
    ("static const int vqvs_x = 3;", "vqvs_x"),  # not a prototype
    ("#define VQVS_SCALE 1.5f", "VQVS_SCALE"),  # not an integer constant
    ("typedef struct vqvs_cfg { int32_t kind; float scale; } vqvs_cfg;", "float scale"),
    ("typedef struct vqvs_cfg { int32_t mult[VQVS_MAX_LEVELS]; } vqvs_cfg;", "mult[VQVS_MAX_LEVELS]"),
])
def test_parser_refuses_what_it_does_not_know(text, named):
    """No default type: the error names the declaration."""
    with pytest.raises(ValueError) as e:
        _abi.parse(text)
    assert named in str(e.value), str(e.value)


def test_missing_header_is_a_native_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, "HEADER", str(tmp_path / "include" / "vqvs.h"))
    with pytest.raises(_native.NativeError, match=re.escape(str(tmp_path / "include" / "vqvs.h"))):
        _native._read_header()


def _code():
    """The header without comments and preprocessor lines."""
    with open(_native.HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))


def test_every_declared_function_is_bound_as_declared(lib_built):
    """Against the header's own text, by a count that does not go through the parser: the parameters between a declaration's
    parentheses, split on commas."""
    flat = " ".join(_code().split())
    assert _native.EXPORTS == list(_native.ABI.functions) and len(_native.EXPORTS) >= 77
    for name, (restype, argtypes) in _native.ABI.functions.items():
        fn = getattr(lib_built, name)  # every parsed function is an attribute of lib()
        decl = re.search(r"([\w ]+?\*?) ?\b%s ?\(([^)]*)\) ?;" % name, flat)
        assert decl, name
        params = [] if decl.group(2).strip() == "void" else decl.group(2).split(",")
        assert len(fn.argtypes) == len(argtypes) == len(params), name
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
        want = {"void": None, "const char*": C.c_char_p, "int64_t": C.c_int64, "int": C.c_int}[decl.group(1).strip()]
        assert fn.restype is want, name


def test_every_exported_symbol_is_declared(lib_built):
    """The direction the per-feature tests do not look in: a vqvs_* symbol the library defines and the header does not declare."""
    if shutil.which("nm") is None:
        pytest.skip("nm (binutils) is not installed: the library's dynamic symbols cannot be listed")
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("vqvs_")}
    assert exported, "nm lists no vqvs_* symbol"
    assert exported == set(_native.EXPORTS), (sorted(exported - set(_native.EXPORTS)), sorted(set(_native.EXPORTS) - exported))


def test_cfg_and_constants_are_the_headers(lib_built):
    body = re.search(r"typedef struct vqvs_cfg \{(.*?)\} vqvs_cfg;", _code(), flags=re.S).group(1)
    slots = 0
    for stmt in body.split(";"):  # `int32_t a, b, c` is three slots, `int32_t x[12]` twelve
        if stmt.strip():
            assert stmt.split()[0] == "int32_t", stmt
            slots += sum(int(n) if n else 1 for n in re.findall(r"\w+\s*(?:\[(\d+)\])?\s*(?:,|$)", stmt.strip()[len("int32_t"):].strip()))
    assert C.sizeof(_native.Cfg) == 4 * slots == 192
    assert (_native.KIND_PREDICTOR, _native.KIND_PREDICTOR_GRAD, _native.PREC_F16, _native.MAX_LEVELS) == (0, 6, 2, 12)
    assert (_native.DDPM_SIGMA_LARGE, _native.DDPM_CONSTRAIN, _native.DDIM_CONSTRAIN, _native.DDIM_INVERT, _native.ERR_ARG) == (1, 2, 2, 4, -1)
    with pytest.raises(ValueError, match="at most 12 levels"):
        _native.Cfg().set_topology((1,) * 13, 2, ())


def test_pad_blocks_is_the_librarys(lib_built):
    """vqvs_pad_blocks: the rule as include/vqvs.h words it, and its refusals; vq_voice_swap_amd.unet.pad_blocks returns it."""
    from vq_voice_swap_amd.unet import pad_blocks

    for real in list(range(1, 300)) + [1000, 1024]:
        q, qp = C.c_int(), C.c_int()
        assert lib_built.vqvs_pad_blocks(real, C.byref(q), C.byref(qp)) == 0
        k = min(5, (real & -real).bit_length() - 1)
        assert q.value << k == real and (q.value & 1 or k == 5)
        if real % 32 == 0:
            assert qp.value == q.value
        else:
            phys = qp.value << k
            assert qp.value & (qp.value - 1) == 0 and qp.value >= q.value and phys % 32 == 0  # a power of two, wide enough
            assert qp.value // 2 < q.value or (phys // 2) % 32  # ... and the smallest such
        assert pad_blocks(real) == (q.value, qp.value)
    q = C.c_int()
    for args in ((0, C.byref(q), C.byref(q)), (-32, C.byref(q), C.byref(q)), (48, None, C.byref(q)), (48, C.byref(q), None)):
        assert lib_built.vqvs_pad_blocks(*args) == _native.ERR_ARG
    with pytest.raises(ValueError):
        pad_blocks(0)
