"""The world families' bindings against include/f110qp.h (CPU only): the argument lists load() sets are the
header's, parameter by parameter; the table's configs stand in the header's order; every public rollout wrapper
refuses a wrong type in each of its config slots, naming the slot, before it reads an array."""
import inspect
import re

import pytest
from capi_header import CONFIG, ctype_of, declarations

FAMILIES = ("world", "race", "contact", "body", "walls", "refresh", "noisy", "grid")


def family_symbols(capi):
    fam = "|".join(FAMILIES)
    pat = re.compile(rf"f110qp_(rollout_({fam})(_dev)?|cast_scans(_\w+)?_dev|clearance(_\w+)?_dev)")
    return [n for n in capi.EXPORTED if pat.fullmatch(n)]


def test_the_symbols_are_the_sixteen_six_and_four(capi):
    names = family_symbols(capi)
    assert len(names) == 26 and len(set(names)) == 26
    assert sum("rollout" in n for n in names) == 16 and sum("cast_scans" in n for n in names) == 6


def test_argtypes_are_the_header_declarations(capi):
    lib, decl = capi.load(), declarations()
    for name in family_symbols(capi):
        want = [ctype_of(capi, d) for d in decl[name]]
        got = list(getattr(lib, name).argtypes)
        assert len(got) == len(want), f"{name}: {len(got)} argtypes, the header declares {len(want)} parameters"
        for i, (g, w) in enumerate(zip(got, want)):
            assert g is w, f"{name}: parameter {i} ({decl[name][i]}) is bound as {g.__name__}, want {w.__name__}"


def test_the_tables_configs_stand_in_the_headers_order(capi):
    configs = [m.group(1) for m in map(CONFIG.fullmatch, declarations()["f110qp_rollout_grid_dev"]) if m]
    assert configs[:3] == ["rollout", "scan", "replan"]
    want = [getattr(capi, k.capitalize() + "Config") for k in configs[3:]]
    assert [f.cfg for f in capi.WORLD_FAMILIES] == want
    assert tuple(f.name for f in capi.WORLD_FAMILIES) == FAMILIES


WRAPPERS = [f"rollout_{f}{d}" for d in ("_dev", "") for f in FAMILIES]


@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_a_wrong_config_type_names_its_slot(capi, wrapper):
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    call = getattr(s, wrapper)
    given = set(inspect.signature(call).parameters)
    # wc is read, not type-checked; a host wrapper builds its walls config itself
    slots = [f for f in capi.WORLD_FAMILIES[1:] if f.arg in given]
    family = wrapper[len("rollout_"):].replace("_dev", "")
    upto = FAMILIES.index(family) + 1
    want = [f for f in capi.WORLD_FAMILIES[1:upto] if wrapper.endswith("_dev") or f.arg != "walls"]
    assert slots == want
    required = [n for n, p in inspect.signature(call).parameters.items() if p.default is inspect.Parameter.empty]
    for bad in slots:
        for wrong in (None, 3, capi.default_world_config()):
            args = {n: None for n in required}
            args.update({f.arg: f.cfg() for f in slots})
            args[bad.arg] = wrong
            with pytest.raises(capi.F110QPError, match=rf"\b{bad.arg} (must be )?a {bad.cfg.__name__}\b"):
                call(**args)
    s.close()
