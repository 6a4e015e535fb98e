"""include/f110qp.h as the binding tests read it: every declared function with its parameter types, and the ctypes
type a parameter type is bound as (tests/test_capi_families.py, tests/test_capi_abi.py)."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "f110qp.h")
CONFIG = re.compile(r"const f110qp_(\w+)_config\*")
ANY_CONFIG = re.compile(r"(?:const )?f110qp_(?:(\w+)_)?config\*")  # f110qp_config* and the out parameters too
SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "const char*": C.c_char_p}


def declarations():
    """{symbol: [parameter type, ...]} of every function the header declares, comments stripped."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(f110qp_\w+)\(([^()]*)\);", text):
        out[name] = [re.sub(r"\s*\b\w+(\[\d*\])?$", r"\1", " ".join(p.split())) for p in params.split(",")]
    return out


def ctype_of(capi, decl):
    """The ctypes type of a parameter declared as `decl`; c_void_p for every pointer and array that is neither a
    config nor a C string."""
    if decl in ("f110qp_ctx*", "void*"):
        return C.c_void_p
    m = ANY_CONFIG.fullmatch(decl)
    if m:
        return C.POINTER(getattr(capi, (m.group(1) or "").capitalize() + "Config"))
    if decl in SCALARS:
        return SCALARS[decl]
    assert decl.endswith("*") or decl.endswith("]"), decl
    return C.c_void_p
