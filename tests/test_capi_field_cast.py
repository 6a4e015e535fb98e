"""The raster LiDAR through the distance field in the C ABI (f110qp_grid_cast_dev, f110qp_rollout_field[_dev])
without a GPU: the exported symbols, their argument lists against the header, and every argument rule the calls add
to the grid family's, each of which answers with its text before the first device call."""
import ctypes as C
import os

import capi_header
import numpy as np
import pytest
from test_capi_grid import grid_rules
from test_capi_noise import noise_rules
from test_capi_walls import wall_rules
from test_capi_world import ref, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD = ("f110qp_grid_cast_dev", "f110qp_rollout_field_dev", "f110qp_rollout_field")
TWIN = {"f110qp_grid_cast_dev": "f110qp_cast_scans_grid_dev", "f110qp_rollout_field_dev": "f110qp_rollout_grid_dev",
        "f110qp_rollout_field": "f110qp_rollout_grid"}
MAX_SIDE = 32768


def test_symbols_version_and_rule(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in FIELD:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    assert "F1. A beam against the grid through its field" in hdr
    assert hdr.index("D4. Lookup of a point") < hdr.index("F1. A beam against the grid through its field")
    assert len(capi.WORLD_FAMILIES) == 8, "the calls are the grid family's: no ninth row"


def test_argument_lists_are_the_headers(capi):
    decl = capi_header.declarations()
    for name in FIELD:
        want = [capi_header.ctype_of(capi, d) for d in decl[name]]
        for lib in (capi.load(), capi.load(test=True)):
            assert list(getattr(lib, name).argtypes) == want, name
    # the grid family's lists with const int* d2 behind grid and int* visits behind ranges
    cast, twin = decl["f110qp_grid_cast_dev"], decl["f110qp_cast_scans_grid_dev"]
    k = twin.index("const unsigned char*") + 1
    assert cast == twin[:k] + ["const int*"] + twin[k:k + 1] + ["int*"] + twin[k + 1:]
    assert twin[k] == "float*" and twin[k + 1] == "void*"
    roll, twin = decl["f110qp_rollout_field_dev"], decl["f110qp_rollout_grid_dev"]
    k = twin.index("const unsigned char*") + 1
    assert roll == twin[:k] + ["const int*"] + twin[k:]
    assert decl["f110qp_rollout_field"] == decl["f110qp_rollout_grid"], "the host caller needs nothing new"


def field_rules(capi, call):
    """The two rules the field adds behind the grid's; call(gc=..., grid=..., d2=...) -> return code."""
    for over in (dict(width=MAX_SIDE + 1, height=1), dict(width=1, height=MAX_SIDE + 1), dict(width=40000, height=40000)):
        assert call(gc=capi.default_grid_config(**over)) == capi.ERR_INVALID, over
        assert "32768" in capi.last_error() and "width and height" in capi.last_error()
    assert call(gc=capi.default_grid_config(width=MAX_SIDE, height=2), batch=0) == capi.OK, "the limit itself is valid"


def test_cast_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    sc, wc = scan(capi), capi.default_world_config(num_circles=5)
    race, body = capi.default_race_config(group_size=2), capi.default_body_config()
    ok, quiet, room = capi.default_walls_config(num_segments=3), capi.default_noise_config(), \
        capi.default_grid_config(width=8, height=6)

    def cast(walls=ok, segments=p, batch=4, body=body, race=race, wc=wc, circles=p, noise=quiet, tick=0, sc=sc,
             lst=None, count=None, gc=room, grid=p, d2=p, ranges=p, visits=p, x=p):
        return L.f110qp_grid_cast_dev(ref(sc), ref(wc), ref(race), ref(body), ref(walls), ref(noise), ref(gc), batch,
                                      tick, lst, count, x, circles, segments, grid, d2, ranges, visits, None)

    # the new rules, with their texts, and their place behind the grid's
    field_rules(capi, cast)
    assert cast(d2=None) == capi.ERR_INVALID and "needs d2" in capi.last_error()
    assert cast(d2=None, batch=0) == capi.ERR_INVALID and "needs d2" in capi.last_error(), "before the empty batch"
    assert cast(d2=None, grid=None) == capi.ERR_INVALID and "needs the grid" in capi.last_error(), "the grid's first"
    assert cast(d2=None, gc=capi.default_grid_config(width=MAX_SIDE + 1, height=1)) == capi.ERR_INVALID
    assert "32768" in capi.last_error(), "the side before d2"
    assert cast(gc=capi.default_grid_config(width=MAX_SIDE + 1, height=1, resolution=0.0)) == capi.ERR_INVALID
    assert "resolution" in capi.last_error(), "the grid's rules before the side"
    # an empty map needs neither array, and visits may be NULL
    assert cast(batch=0, gc=capi.default_grid_config(), grid=None, d2=None) == capi.OK
    assert cast(batch=0, gc=capi.default_grid_config(width=5, height=0), grid=None, d2=None, visits=None) == capi.OK
    assert cast(batch=0, visits=None) == capi.OK
    # visits NULL passes every check: the first complaint of a call without x is x's, not visits'
    assert cast(visits=None, x=None) == capi.ERR_INVALID and "x/ranges" in capi.last_error()
    assert cast(visits=None, ranges=None) == capi.ERR_INVALID and "x/ranges" in capi.last_error()
    # every rule of the grid cast still answers
    grid_rules(capi, cast, 5 + 2 + 3)
    wall_rules(capi, cast, 4)
    noise_rules(capi, cast, 4)
    assert cast(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
    assert cast(race=None) == capi.ERR_INVALID and "race config" in capi.last_error()
    assert cast(wc=None) == capi.ERR_INVALID and "world config" in capi.last_error()
    assert cast(batch=3) == capi.ERR_INVALID and "group_size" in capi.last_error()
    assert cast(batch=-1) == capi.ERR_INVALID and "batch" in capi.last_error()
    assert cast(noise=None, gc=None) == capi.ERR_INVALID and "noise config" in capi.last_error(), "noise before grid"
    for t in (-1, -(2 ** 31)):
        assert cast(tick=t) == capi.ERR_INVALID and "tick" in capi.last_error()
    assert cast(sc=None) == capi.ERR_INVALID and "scan config" in capi.last_error()
    assert cast(lst=p) == capi.ERR_INVALID and "together" in capi.last_error()
    assert cast(batch=0) == capi.OK


@pytest.mark.parametrize("name", ["f110qp_rollout_field_dev", "f110qp_rollout_field"])
def test_rollout_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    rc, rp = capi.default_rollout_config(ticks=3), capi.default_replan_config(num_waypoints=4)
    sc, wc = scan(capi), capi.default_world_config(num_circles=5)
    race, cc, body = capi.default_race_config(group_size=2), capi.default_contact_config(), capi.default_body_config()
    ok, every, quiet = capi.default_walls_config(num_segments=3), capi.default_refresh_config(every=1), \
        capi.default_noise_config()
    room = capi.default_grid_config(width=8, height=6)

    def call(walls=ok, segments=p, batch=4, body=body, cc=cc, rf=every, noise=quiet, gc=room, grid=p, d2=p, patch=None):
        # the grid rollout's arrays (test_capi_grid.py) with d2 behind grid in the device call
        a = [p] * 5 + [segments, grid] + [p] * 4 + [None] * 11 + [p, None, p] + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        if dev:
            a.insert(7, d2)
        return fn(s._h, ref(rc), ref(sc), ref(rp), ref(wc), ref(race), ref(cc), ref(body), ref(walls), ref(rf),
                  ref(noise), ref(gc), batch, *a)

    field_rules(capi, call)
    if dev:
        assert call(d2=None) == capi.ERR_INVALID and "needs d2" in capi.last_error()
        assert call(d2=None, batch=0) == capi.ERR_INVALID and "needs d2" in capi.last_error()
        assert call(d2=None, grid=None) == capi.ERR_INVALID and "needs the grid" in capi.last_error()
        assert call(batch=0, gc=capi.default_grid_config(), grid=None, d2=None) == capi.OK
    grid_rules(capi, call, 5 + 2 + 3)
    noise_rules(capi, call, 4)
    assert call(rf=None) == capi.ERR_INVALID and "refresh config" in capi.last_error()
    wall_rules(capi, call, 4)
    assert call(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
    assert call(cc=None) == capi.ERR_INVALID and "contact config" in capi.last_error()
    assert call(patch={22: None}) == capi.ERR_INVALID and "clear_traj" in capi.last_error()
    assert call(patch={24: None}) == capi.ERR_INVALID and "crash_tick" in capi.last_error()
    assert call(patch={7: None}) == capi.ERR_INVALID and "x_traj" in capi.last_error()
    assert call(batch=0) == capi.OK
    s.close()


def test_binding_checks(capi):
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    cfg = (capi.default_race_config(), capi.default_contact_config(), capi.default_body_config())
    with pytest.raises(capi.F110QPError, match="GridConfig"):
        s.rollout_field(None, None, None, None, None, None, *cfg, capi.default_refresh_config(),
                        capi.default_noise_config(), None, None, None, None, 1)
    with pytest.raises(capi.F110QPError, match="GridConfig"):
        s.rollout_field_dev(None, None, None, None, *cfg, capi.default_walls_config(), capi.default_refresh_config(),
                            capi.default_noise_config(), 3, *[None] * 14)
    with pytest.raises(capi.F110QPError, match="GridConfig"):
        capi.grid_cast_dev(None, None, capi.default_race_config(), capi.default_body_config(),
                           capi.default_walls_config(), capi.default_noise_config(), 3, 0, *[None] * 6)
    s.close()
