"""Every binding load() sets against include/f110qp.h (CPU only; the library has to load, no device is opened): for
each exported symbol the argtypes have the header's parameter count, and each has the class of the header's type.
int / unsigned / float / double / const char* are c_int / c_uint / c_float / c_double / c_char_p, a config pointer is
POINTER of capi's structure of that name, any other pointer or array is c_void_p or a POINTER(...) (load() uses both).
A miscounted list is no Python error: the call would misread its stack on the device."""
import ctypes as C

from capi_header import ctype_of, declarations


def parameters(decl, name):
    return [d for d in decl[name] if d]  # f(void) parses as one empty type


def is_pointer(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_exported_is_what_the_header_declares(capi):
    decl = declarations()
    assert len(capi.EXPORTED) == len(set(capi.EXPORTED))
    assert sorted(set(decl) - set(capi.EXPORTED)) == [], "declared in the header, missing from capi.EXPORTED"
    assert sorted(set(capi.EXPORTED) - set(decl)) == [], "in capi.EXPORTED, not declared in the header"


def test_every_symbol_with_parameters_is_bound(capi):
    lib, decl = capi.load(), declarations()
    unbound = [n for n in capi.EXPORTED if parameters(decl, n) and getattr(lib, n).argtypes is None]
    assert unbound == [], "the header gives these parameters, load() gives them no argtypes"


def test_argtypes_have_the_headers_count_and_classes(capi):
    lib, decl = capi.load(), declarations()
    checked = 0
    for name in capi.EXPORTED:
        got = getattr(lib, name).argtypes
        if got is None:
            continue
        params = parameters(decl, name)
        assert len(got) == len(params), f"{name}: {len(got)} argtypes, the header declares {len(params)} parameters"
        for i, (g, d) in enumerate(zip(got, params)):
            want = ctype_of(capi, d)
            ok = is_pointer(g) if want is C.c_void_p else g is want
            assert ok, f"{name}: parameter {i} ({d}) is bound as {g.__name__}, want {want.__name__}"
        checked += 1
    print(f"{checked} symbols checked against the header")
    # the solve entry points, the closed loops, the world families and the rest: nothing quietly dropped out
    assert checked == sum(1 for n in capi.EXPORTED if parameters(decl, n))


def test_the_solve_table_is_the_headers_solve_entry_points(capi):
    decl = declarations()
    assert sorted(r.symbol for r in capi.SOLVE_CALLS) == sorted(n for n in decl if n.startswith("f110qp_solve_"))
    for r in capi.SOLVE_CALLS:
        params = decl[r.symbol]
        assert params[2] == {"f32": "const float*", "f64": "const double*"}[r.fin], r.symbol  # x0
        assert ("int" in params[2:]) == r.grouped, r.symbol  # num_groups, the only int behind batch
        assert (params[-1] == "void*") == r.dev, r.symbol  # the stream
        assert params.count("double*") == 2 * r.ex, r.symbol  # obj, cost
        assert r.sync == ("_sync" in r.symbol)
