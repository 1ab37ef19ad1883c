"""
ctypes binding of the C-ABI library `libvqvs_hip.so` (declared in include/vqvs.h).

There is no CPU fallback: if the library is missing, cannot be loaded, or a call
fails, this module raises.  The library is built in-tree by `build()` (hipcc,
--offload-arch=gfx950) so it travels with the source tree.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, List, Optional, Sequence, Tuple

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VQVS_LIB_PATH") or os.path.join(_HERE, "libvqvs_hip.so")  # override: instrumented builds (tools/)
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "vqvs.h"))  # the tree travels whole (csrc/Makefile depends on this path too)


class NativeError(RuntimeError):
    pass


class Cfg(C.Structure):
    """vqvs_cfg; its fields are the header's (set below)."""

    def set_topology(self, channel_mult, depth_mult, dilations):
        """Describe a UNet other than the reference's default one (unet.py:17-30, 188-196)."""
        if len(channel_mult) > MAX_LEVELS or len(dilations) > MAX_LEVELS:
            raise ValueError(f"the gfx950 library builds at most {MAX_LEVELS} levels and {MAX_LEVELS} middle / output dilations")
        self.topology_set = 1
        self.n_levels = len(channel_mult)
        for i, m in enumerate(channel_mult):
            self.channel_mult[i] = int(m)
        self.depth_mult = int(depth_mult)
        self.n_dilations = len(dilations)
        for i, d in enumerate(dilations):
            self.dilations[i] = int(d)


def _read_header() -> _abi.Abi:
    try:
        with open(HEADER) as f:
            return _abi.parse(f.read(), Cfg)
    except OSError as e:
        raise NativeError(f"cannot read the library's header {HEADER}: {e}") from e


# One declaration of the boundary: the prototypes, the VQVS_* constants (KIND_*, PREC_*, DDPM_*, DDIM_*, ERR_*, MAX_LEVELS: bound here
# under their names without the prefix) and the fields of vqvs_cfg all come from include/vqvs.h.
ABI = _read_header()
Cfg._fields_ = ABI.cfg_fields
EXPORTS = list(ABI.functions)
globals().update({name[len("VQVS_"):]: value for name, value in ABI.constants.items()})
STREAM_STEP, STREAM_XT, STREAM_LOSS, STREAM_KEEP = 0, 1, 2, 3  # stream ids of the noise generator (csrc/philox.hpp)
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "float32": PREC_F32, "bf16": PREC_BF16, "bfloat16": PREC_BF16,
              "fp16": PREC_F16, "f16": PREC_F16, "float16": PREC_F16, "half": PREC_F16}

_lib = None


class NativeArgumentError(NativeError, ValueError):
    """VQVS_ERR_ARG: the library refused the arguments on the host, before it touched the device.  A ValueError, as the
    reference raises for shape problems, and a NativeError like every other error the library reports."""


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into libvqvs_hip.so (in-tree)."""
    cmd = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=not verbose)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise NativeError("building libvqvs_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C vq_voice_swap_amd/csrc`). There is no CPU fallback for the sampling hot path."
        )
    if os.environ.get("HIP_FORCE_DEV_KERNARG") is None:
        import warnings

        warnings.warn("HIP_FORCE_DEV_KERNARG is not set: the HIP runtime keeps kernel arguments in host memory and every launch of the "
                      "sampler starts with loads across PCIe (~2 % slower, DESIGN.md section 7).  Set HIP_FORCE_DEV_KERNARG=1 in the "
                      "process environment before the first HIP call (bench.py and the sample_*.py scripts do).", RuntimeWarning, stacklevel=2)
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI.functions.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise NativeError(f"{LIB_PATH} does not export {name}, which {HEADER} declares: rebuild the library") from None
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def last_error() -> str:
    return (lib().vqvs_last_error() or b"").decode("utf-8", "replace")


def check(rc: int) -> None:
    """Map the ABI's error codes to the exception types the reference raises
    (AssertionError for the forward-argument asserts of unet.py:126-131, ValueError for
    shape problems -- NativeArgumentError, which is a NativeError too --, RuntimeError for HIP failures)."""
    if rc == 0:
        return
    msg = last_error()
    if rc == ERR_ARG:
        if msg.startswith("must provide"):
            raise AssertionError(msg)
        raise NativeArgumentError(msg)
    raise NativeError(f"libvqvs_hip error {rc}: {msg}")


def param_table(cfg: Cfg) -> List[Tuple[str, Tuple[int, ...]]]:
    L = lib()
    n = L.vqvs_param_count(C.byref(cfg))
    if n < 0:
        check(n)
    out = []
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 4)()
    nd = C.c_int()
    for i in range(n):
        check(L.vqvs_param_info(C.byref(cfg), i, name, 256, shape, C.byref(nd)))
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(nd.value))))
    return out


def _stream_ptr() -> int:
    import torch

    return torch.cuda.current_stream().cuda_stream


def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


class Handle:
    """Owns one `vqvs_model*`."""

    def __init__(self, cfg: Cfg, state: Dict[str, "object"], prefix: str, device_index: int):
        import torch

        self.cfg = cfg
        self.device_index = device_index
        table = param_table(cfg)
        keep = []
        ptrs = (C.c_void_p * len(table))()
        for i, (name, shape) in enumerate(table):
            key = prefix + name
            if key not in state:
                raise KeyError(f"state dict has no parameter {key!r} required by the gfx950 model")
            t = state[key].detach().to(device="cpu", dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"parameter {key}: expected shape {shape}, got {tuple(t.shape)}")
            keep.append(t)
            ptrs[i] = t.data_ptr()
        h = C.c_void_p()
        check(lib().vqvs_model_create(C.byref(cfg), ptrs, len(table), device_index, C.byref(h)))
        self._h = h
        del keep

    @property
    def ptr(self):
        return self._h

    def status(self) -> int:
        """Device status word (vqvs_model_status): read and cleared; synchronises the device."""
        w = C.c_uint(0)
        check(lib().vqvs_model_status(self.ptr, C.byref(w)))
        return int(w.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().vqvs_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- introspection
    def device_bytes(self) -> int:
        return int(lib().vqvs_model_device_bytes(self._h))

    def kernel_count(self) -> int:
        return int(lib().vqvs_forward_kernel_count(self._h))

    def model_bytes(self, B: int, T: int) -> int:
        return int(lib().vqvs_forward_model_bytes(self._h, B, T))

    def flops(self, B: int, T: int) -> int:
        return int(lib().vqvs_forward_flops(self._h, B, T))

    def set_profiling(self, on: bool) -> None:
        check(lib().vqvs_set_profiling(self._h, 1 if on else 0))

    def op_info(self, B: int, T: int) -> List[Tuple[str, int, int]]:
        """(kind, algorithmic bytes, flops) of every kernel one forward enqueues."""
        L = lib()
        kind = C.create_string_buffer(64)
        by, fl = C.c_int64(), C.c_int64()
        out = []
        for i in range(self.kernel_count()):
            check(L.vqvs_op_info(self._h, i, kind, 64, C.byref(by), C.byref(fl), B, T))
            out.append((kind.value.decode(), by.value, fl.value))
        return out

    def op_desc(self) -> List[str]:
        buf = C.create_string_buffer(256)
        out = []
        for i in range(self.kernel_count()):
            check(lib().vqvs_op_desc(self._h, i, buf, 256))
            out.append(buf.value.decode())
        return out

    def profile_read(self) -> List[float]:
        n = self.kernel_count()
        buf = (C.c_float * n)()
        r = lib().vqvs_profile_read(self._h, buf, n)
        if r < 0:
            check(r)
        return [float(buf[i]) for i in range(r)]

    def taps(self) -> List[Tuple[str, int, int]]:
        L = lib()
        n = L.vqvs_debug_tap_count(self._h)
        name = C.create_string_buffer(256)
        ch, ls = C.c_int(), C.c_int()
        out = []
        for i in range(n):
            check(L.vqvs_debug_tap_info(self._h, i, name, 256, C.byref(ch), C.byref(ls)))
            out.append((name.value.decode(), ch.value, ls.value))
        return out

    def read_embedding(self, B: int):
        """Conditioning vector [B, 4*base] of the last forward (time embedding [+ class embedding])."""
        import torch

        out = torch.empty(B, 4 * self.cfg.base_channels, dtype=torch.float32)
        r = lib().vqvs_debug_read_embedding(self._h, B, out.data_ptr())
        if r < 0:
            check(r)
        return out[:, :r]

    def _read_film_rows(self, entry, B: int):
        import torch

        R = sum(shape[0] for name, shape in param_table(self.cfg) if name.endswith("cond_layers.1.bias"))  # 2 * cout rows per block
        out = torch.empty(B, R, dtype=torch.float32)
        r = entry(self._h, B, out.data_ptr())
        if r < 0:
            check(r)
        assert r == R, (r, R)
        return out

    def read_dfilm(self, B: int):
        """d mse_b / d (FiLM rows) [B, R] of the last `vqvs_unet_embed_grad` on a predictor-gradient handle: per clip the (d a | d b)
        rows of every ResBlock in the order down, middle, up."""
        return self._read_film_rows(lib().vqvs_debug_read_dfilm, B)

    def read_film(self, B: int):
        """FiLM rows [B, R] of the last forward: per clip the (a | b) rows of every ResBlock in the order down, middle, up (the
        handle's physical widths)."""
        return self._read_film_rows(lib().vqvs_debug_read_film, B)

    # ---- GroupNorm / xform entries of a debug_taps handle, as the last forward at (B, T) ran them (include/vqvs.h)
    def gn_count(self) -> int:
        return int(lib().vqvs_debug_gn_count(self._h))

    def gn_info(self, i: int, B: int, T: int) -> dict:
        name = C.create_string_buffer(256)
        v = (C.c_int64 * 24)()
        check(lib().vqvs_debug_gn_info(self._h, i, B, T, name, 256, v))
        srcs = [dict(C=int(v[8 + 4 * s]), rows=int(v[9 + 4 * s]), tile_rows=int(v[10 + 4 * s]), ntiles=int(v[11 + 4 * s]), sums_stored=bool(v[16 + s]))
                for s in range(int(v[5]))]
        return dict(name=name.value.decode(), Ctot=int(v[0]), groups=int(v[1]), count=int(v[2]), film=bool(v[3]), film_off=int(v[4]),
                    has_mr=bool(v[6]), fused=bool(v[7]), srcs=srcs)

    def _gn_read(self, i: int, B: int, T: int, what: int, src: int, shape):
        import torch

        out = torch.empty(*shape, dtype=torch.float32)
        check(lib().vqvs_debug_gn_read(self._h, i, B, T, what, src, out.data_ptr()))
        return out

    def gn_source(self, i: int, B: int, T: int, src: int = 0):
        """Source `src` of GroupNorm i as stored, float32 [B, C, rows]."""
        s = self.gn_info(i, B, T)["srcs"][src]
        return self._gn_read(i, B, T, 0, src, (B, s["C"], s["rows"]))

    def gn_partials(self, i: int, B: int, T: int, src: int = 0):
        """Its tile partials (sum x, sum x^2), float32 [B, ntiles, C, 2]."""
        s = self.gn_info(i, B, T)["srcs"][src]
        return self._gn_read(i, B, T, 1, src, (B, s["ntiles"], s["C"], 2))

    def gn_table(self, i: int, B: int, T: int, mean_rstd: bool = False):
        """(scale, shift) -- or (mean, rstd) -- of GroupNorm i, float32 [B, Ctot, 2]."""
        return self._gn_read(i, B, T, 3 if mean_rstd else 2, 0, (B, self.gn_info(i, B, T)["Ctot"], 2))

    def xform_count(self) -> int:
        return int(lib().vqvs_debug_xform_count(self._h))

    def xform_info(self, i: int, B: int, T: int) -> dict:
        v = (C.c_int64 * 8)()
        check(lib().vqvs_debug_xform_info(self._h, i, B, T, v))
        return dict(gn=int(v[0]), C=int(v[1]), Lin=int(v[2]), Lout=int(v[3]), avg=bool(v[4]), ss_stride=int(v[5]), ss_c0=int(v[6]))

    def xform_tensor(self, i: int, B: int, T: int, output: bool):
        import torch

        x = self.xform_info(i, B, T)
        out = torch.empty(B, x["C"], x["Lout"] if output else x["Lin"], dtype=torch.float32)
        check(lib().vqvs_debug_xform_read(self._h, i, B, T, 1 if output else 0, out.data_ptr()))
        return out

    def read_tap(self, i: int, B: int, T: int):
        import torch

        _, ch, _ls = self.taps()[i]
        Lx = lib().vqvs_debug_tap_rows(self._h, i, T)
        if Lx < 0:
            check(Lx)
        out = torch.empty(B, ch, Lx, dtype=torch.float32)
        check(lib().vqvs_debug_read_tap(self._h, i, B, T, out.data_ptr()))
        return out


GELU_FORMS = {"gelu_f": 0, "exact": 1, "poly6": 2, "poly7": 3, "grad": 4}


def debug_gelu(x, form: int):
    """The library's GELU device function number `form` (vqvs_debug_gelu: 0 gelu_f, 1..3 gelu2 exact / degree 6 / degree 7 on pairs,
    4 gelu_grad_f) of a float32 tensor on a ROCm device, element by element."""
    import torch

    require_cuda(x)
    x = x.detach().to(torch.float32).contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(lib().vqvs_debug_gelu(x.data_ptr(), out.data_ptr(), x.numel(), int(form), _stream_ptr()))
    return out


_range_checked = {}


def check_index_range(t, n: int, what: str) -> None:
    """Raise IndexError, as nn.Embedding / F.embedding do (reference unet.py:45, vq.py:108), when an index tensor holds
    values outside [0, n).  The kernels clamp instead of faulting, which would turn a caller bug into plausible audio.
    The check costs one device->host sync, so the SAME tensor object at the same version (the labels of a sampling loop, passed
    again every step) is not checked twice; a new tensor -- even one the allocator places at the old address -- always is."""
    import weakref

    prev = _range_checked.get(what)
    if prev is not None and prev[0]() is t and prev[1:] == (t._version, t.numel(), n):
        return
    if t.numel():
        lo, hi = int(t.min().item()), int(t.max().item())
        if lo < 0 or hi >= n:
            raise IndexError(f"{what}: index out of range (values span [{lo}, {hi}], valid range is [0, {n - 1}])")
    _range_checked[what] = (weakref.ref(t), t._version, t.numel(), n)


def require_cuda(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NativeError(
                "the gfx950 sampling path needs tensors on a ROCm device (got a CPU tensor); "
                "there is deliberately no CPU fallback"
            )
