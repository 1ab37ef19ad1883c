"""
The C boundary, read from its one declaration: include/vqvs.h -> ctypes prototypes, the VQVS_* constants and the fields of vqvs_cfg.

`parse` knows exactly the declaration forms the header uses.  Anything else -- a parameter or return type outside the map below, a
statement that is not a prototype -- raises and names the declaration: a guessed prototype would marshal garbage into a kernel launch.
"""

from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, NamedTuple, Optional, Tuple

SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "unsigned": C.c_uint32, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double}
RETURNS = {"void": None, "const char*": C.c_char_p, "int64_t": C.c_int64, "int": C.c_int}


class Abi(NamedTuple):
    functions: Dict[str, Tuple[Optional[type], List[type]]]  # name -> (restype, argtypes), in header order
    constants: Dict[str, int]  # "VQVS_KIND_PREDICTOR" -> 0, ...
    cfg_fields: List[Tuple[str, type]]  # the _fields_ of vqvs_cfg


def _argtype(param: str, cfg: type, decl: str) -> type:
    """The ctypes type of one parameter.  Tensors come in as data_ptr() integers, and byref() objects and ctypes arrays are accepted
    wherever a c_void_p stands."""
    m = re.fullmatch(r"(.*?)\s*\b(\w+)\s*(\[\d+\])?", param)  # type, name, array suffix
    ctype = re.sub(r"\s*\*\s*", "*", m.group(1)) + ("*" if m.group(3) else "") if m else ""
    if ctype in SCALARS:
        return SCALARS[ctype]
    if ctype == "const vqvs_cfg*":
        return C.POINTER(cfg)
    if ctype == "char*":
        return C.c_char_p
    if ctype == "vqvs_model**":
        return C.POINTER(C.c_void_p)
    if re.fullmatch(r"(const )?(void|float|double|int|unsigned|long long|unsigned long long|u?int(8|32|64)_t|vqvs_model)\*( ?const\*)?", ctype):
        return C.c_void_p
    raise ValueError(f"vqvs.h: parameter {param!r} of `{decl}` has a type this binding does not know")


def parse(text: str, cfg: Optional[type] = None) -> Abi:
    """Parse the text of vqvs.h.  `cfg`: the ctypes.Structure that `const vqvs_cfg*` parameters point to (its _fields_ are the
    caller's to set, from the result); None: one is made here."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants, code = {}, []
    for line in text.splitlines():
        m = re.fullmatch(r"\s*#\s*define\s+(VQVS_\w+)\s+\(?(-?\d+)u?\)?\s*", line)
        if m:
            constants[m.group(1)] = int(m.group(2))
        elif re.match(r"\s*#\s*define\s+VQVS_\w+\s+\S", line):
            raise ValueError(f"vqvs.h: `{line.strip()}` is not an integer constant")
        elif not line.lstrip().startswith("#"):
            code.append(line)
    text = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', " ", "\n".join(code), flags=re.M)  # the __cplusplus wrapper

    cfg_fields = []
    m = re.search(r"typedef\s+struct\s+vqvs_cfg\s*\{(.*?)\}\s*vqvs_cfg\s*;", text, flags=re.S)
    if m:
        text = text[:m.start()] + text[m.end():]
        for stmt in filter(None, (" ".join(s.split()) for s in m.group(1).split(";"))):
            if not stmt.startswith("int32_t "):
                raise ValueError(f"vqvs.h: vqvs_cfg member `{stmt}` is not int32_t")
            for item in stmt[len("int32_t "):].split(","):
                f = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", item)
                if not f:
                    raise ValueError(f"vqvs.h: vqvs_cfg member `{stmt}`: cannot read `{item.strip()}`")
                cfg_fields.append((f.group(1), C.c_int32 * int(f.group(2)) if f.group(2) else C.c_int32))
    if cfg is None:
        cfg = type("vqvs_cfg", (C.Structure,), {"_fields_": cfg_fields})

    functions = {}
    for decl in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        if decl == "typedef struct vqvs_model vqvs_model":
            continue
        m = re.fullmatch(r"(.*?)\s*\b(vqvs_\w+)\s*\((.*)\)", decl)
        ret = re.sub(r"\s*\*\s*", "*", m.group(1)) if m else None
        if ret not in RETURNS:
            raise ValueError(f"vqvs.h: `{decl}` is not a prototype with a return type this binding knows")
        params = [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")]
        functions[m.group(2)] = (RETURNS[ret], [_argtype(p, cfg, decl) for p in params])
    return Abi(functions, constants, cfg_fields)
