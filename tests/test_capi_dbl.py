"""The double-precision input entry points of the C ABI, without a GPU: exported symbols, argument
checks equal to the float twins', the header as C and C++, and the binding's float64-only rule."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL = ("f110qp_solve_batch_dbl", "f110qp_solve_batch_dev_dbl", "f110qp_solve_batch_dev_sync_dbl",
       "f110qp_solve_grouped_dbl", "f110qp_solve_grouped_dev_dbl")
# (float twin, _dbl entry point, arguments after (ctx, batch), index of num_groups among them or None)
TWINS = [("f110qp_solve_batch_ex", "f110qp_solve_batch_dbl", 10, None),
         ("f110qp_solve_batch_ex_dev", "f110qp_solve_batch_dev_dbl", 11, None),
         ("f110qp_solve_batch_dev_sync", "f110qp_solve_batch_dev_sync_dbl", 9, None),
         ("f110qp_solve_grouped_ex", "f110qp_solve_grouped_dbl", 12, 5),
         ("f110qp_solve_grouped_ex_dev", "f110qp_solve_grouped_dev_dbl", 13, 5)]


def test_symbols_declared_bound_and_exported_by_both_libraries(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    declared = set(re.findall(r"\b(f110qp_[a-z_]+)\(", hdr))
    for name in DBL:
        assert name in declared and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6  # additive: the ABI version stays


@pytest.mark.parametrize("twin,dbl,nargs,gpos", TWINS, ids=[t[1] for t in TWINS])
def test_argument_checks_match_the_float_twin(capi, twin, dbl, nargs, gpos):
    L = capi.load()
    s = capi.Solver(capi.default_config(20))
    g = capi.Solver(capi.default_config(20, gap_mode=capi.GAP_ACTIVE))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)

    def args(fill, hs=None):
        a = [fill] * nargs
        a[3] = hs
        if gpos is not None:
            a[gpos - 1], a[gpos] = p, 2  # group, num_groups
        return a

    for fn in (getattr(L, twin), getattr(L, dbl)):
        assert fn(s._h, 0, *args(None)) == capi.OK  # batch 0: a no-op
        assert fn(s._h, -1, *args(None)) == capi.ERR_INVALID
        assert fn(None, 4, *args(None)) == capi.ERR_INVALID
        assert fn(s._h, 4, *args(None)) == capi.ERR_INVALID
        assert "non-NULL" in capi.last_error()
        assert fn(g._h, 4, *args(p)) == capi.ERR_INVALID
        assert "halfspace" in capi.last_error()
        if gpos is not None:
            a = args(p)
            a[gpos - 1] = None  # group
            assert fn(s._h, 4, *a) == capi.ERR_INVALID
            a = args(p)
            a[gpos] = 0  # num_groups
            assert fn(s._h, 4, *a) == capi.ERR_INVALID
    s.close()
    g.close()


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_header_declares_the_dbl_calls_in_c_and_cpp(tmp_path, lang, cc):
    """A translation unit that takes the address of every _dbl entry point with its documented
    signature compiles as C and as C++."""
    import shutil

    assert shutil.which(cc) is not None, f"{cc} not installed"
    src = tmp_path / ("use." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "f110qp.h"\n'
                   "typedef int (*host_fn)(f110qp_ctx*, int, const double*, const double*, const double*,\n"
                   "    const float*, float*, float*, int*, int*, double*, double*);\n"
                   "typedef int (*sync_fn)(f110qp_ctx*, int, const double*, const double*, const double*,\n"
                   "    const float*, float*, float*, int*, int*, void*);\n"
                   "host_fn a = f110qp_solve_batch_dbl;\nsync_fn b = f110qp_solve_batch_dev_sync_dbl;\n"
                   "int v = F110QP_API_VERSION;\n")
    subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_binding_takes_float64_only(capi):
    s = capi.Solver(capi.default_config(4))
    x0, ul, xr = np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((2, 4, 3))
    for bad in (x0.astype(np.float32), x0.tolist()):
        with pytest.raises(capi.F110QPError, match="x0 must be a float64"):
            s.solve_dbl(bad, ul, xr)
    with pytest.raises(capi.F110QPError, match="u_lin must be a float64"):
        s.solve_dbl(x0, ul.astype(np.float32), xr)
    with pytest.raises(capi.F110QPError, match="x_ref must be a float64"):
        s.solve_grouped_dbl(x0, ul, xr.astype(np.float32), np.zeros(2, np.int32))
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(64, dtype=torch.float32), torch.zeros(64, dtype=torch.float64)
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(capi.F110QPError, match="x0 must be torch.float64"):
        s.solve_dev_dbl(t32[:6].view(2, 3), t64, t64, None, t32, t32, i32)
    with pytest.raises(capi.F110QPError, match="x_ref must be torch.float64"):
        s.solve_grouped_dev_dbl(t64[:6].view(2, 3), t64, t32, None, i32, 1, t32, t32, i32)
    with pytest.raises(capi.F110QPError, match="u_out must be torch.float32"):
        s.solve_dev_dbl(t64[:6].view(2, 3), t64, t64, None, t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="no obj / cost"):
        s.solve_dev_dbl(t64[:6].view(2, 3), t64, t64, None, t32, t32, i32, obj=t64, sync=True)
    s.close()
