"""The raster-map entry points of the C ABI (f110qp_default_grid_config, f110qp_cast_scans_grid_dev,
f110qp_clearance_grid_dev, f110qp_rollout_grid[_dev]) without a GPU: exported symbols, the default, the struct layout
against the header, and every argument rule, each of which answers before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from test_capi_noise import noise_rules
from test_capi_walls import wall_rules
from test_capi_world import ref, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = ("f110qp_default_grid_config", "f110qp_cast_scans_grid_dev", "f110qp_clearance_grid_dev",
        "f110qp_rollout_grid_dev", "f110qp_rollout_grid")
INT_MAX = 2 ** 31 - 1


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in GRID:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    for rule in ("G1. A beam against the grid", "G2. The rectangle against the grid"):
        assert rule in hdr


def test_default_and_layout(capi):
    g = capi.GridConfig(width=9, height=9, origin_x=9.0, origin_y=9.0, resolution=9.0, reach=9.0)
    capi.load().f110qp_default_grid_config(C.byref(g))
    assert (g.width, g.height, g.origin_x, g.origin_y, g.resolution, g.reach) == (0, 0, 0.0, 0.0, 0.05, 1.0)
    capi.load().f110qp_default_grid_config(None)  # a NULL config is ignored
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} f110qp_grid_config;", hdr).group(1)
    fields = []
    for t, names in re.findall(r"^\s*(int|double)\s+([\w, ]+);", body, re.M):
        fields += [(n.strip(), {"int": C.c_int, "double": C.c_double}[t]) for n in names.split(",")]
    assert fields == list(capi.GridConfig._fields_)
    assert C.sizeof(capi.GridConfig) == 40
    from f110qp import workload
    k = capi.grid_config_of(workload.GridSpec(7, 5, -1.5, 2.0, 0.1, 0.4))
    assert (k.width, k.height, k.origin_x, k.origin_y, k.resolution, k.reach) == (7, 5, -1.5, 2.0, 0.1, 0.4)


def grid_rules(capi, call, obstacles):
    """The grid rules shared by the four calls; call(gc=..., grid=...) -> return code. obstacles: C + G + S."""
    def cfg(**over):
        return capi.default_grid_config(**{**dict(width=8, height=6), **over})

    assert call(gc=None) == capi.ERR_INVALID and "grid config" in capi.last_error()
    for k in ("width", "height"):
        for v in (-1, -(2 ** 31)):
            assert call(gc=cfg(**{k: v})) == capi.ERR_INVALID, (k, v)
            assert "width and height" in capi.last_error()
    assert call(gc=cfg(), grid=None) == capi.ERR_INVALID and "needs the grid" in capi.last_error()
    for v in (0.0, -0.05, float("inf"), float("nan")):
        assert call(gc=cfg(resolution=v)) == capi.ERR_INVALID, v
        assert "resolution" in capi.last_error()
    for v in (-1e-300, -1.0, float("inf"), float("nan")):
        assert call(gc=cfg(reach=v)) == capi.ERR_INVALID, v
        assert "reach" in capi.last_error()
    for k in ("origin_x", "origin_y"):
        for v in (float("inf"), -float("inf"), float("nan")):
            assert call(gc=cfg(**{k: v})) == capi.ERR_INVALID, (k, v)
            assert "origin" in capi.last_error()
    assert call(gc=cfg(width=INT_MAX - obstacles + 1, height=1)) == capi.ERR_INVALID and "fit an int" in capi.last_error()
    assert call(gc=cfg(width=65536, height=65536)) == capi.ERR_INVALID and "fit an int" in capi.last_error()


def test_cast_and_clearance_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    sc, wc = scan(capi), capi.default_world_config(num_circles=5)
    race, body = capi.default_race_config(group_size=2), capi.default_body_config()
    ok, quiet, room = capi.default_walls_config(num_segments=3), capi.default_noise_config(), \
        capi.default_grid_config(width=8, height=6)

    def cast(walls=ok, segments=p, batch=4, body=body, race=race, wc=wc, circles=p, noise=quiet, tick=0, sc=sc,
             lst=None, count=None, gc=room, grid=p):
        return L.f110qp_cast_scans_grid_dev(ref(sc), ref(wc), ref(race), ref(body), ref(walls), ref(noise), ref(gc),
                                            batch, tick, lst, count, p, circles, segments, grid, p, None)

    def clear(walls=ok, segments=p, batch=4, body=body, race=race, wc=wc, circles=p, gc=room, grid=p, rows=1):
        return L.f110qp_clearance_grid_dev(ref(wc), ref(race), ref(body), ref(walls), ref(gc), batch, rows, p, circles,
                                           segments, grid, p, None, None)

    for call in (cast, clear):
        grid_rules(capi, call, 5 + 2 + 3)
        wall_rules(capi, call, 4)  # every rule of the walls calls still answers
        assert call(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
        assert call(race=None) == capi.ERR_INVALID and "race config" in capi.last_error()
        assert call(wc=None) == capi.ERR_INVALID and "world config" in capi.last_error()
        assert call(batch=3) == capi.ERR_INVALID and "group_size" in capi.last_error()
        assert call(batch=-1) == capi.ERR_INVALID and "batch" in capi.last_error()
        # the grid is checked where the batch is empty; the walls' rules come first
        assert call(batch=0, gc=None) == capi.ERR_INVALID and "grid config" in capi.last_error()
        assert call(walls=None, gc=None) == capi.ERR_INVALID and "walls config" in capi.last_error()
        assert call(batch=0) == capi.OK
        assert call(batch=0, gc=capi.default_grid_config(), grid=None) == capi.OK, "an empty map needs no array"
        assert call(batch=0, gc=capi.default_grid_config(width=5, height=0), grid=None) == capi.OK
    noise_rules(capi, cast, 4)
    assert cast(noise=None, gc=None) == capi.ERR_INVALID and "noise config" in capi.last_error(), "noise before grid"
    for t in (-1, -(2 ** 31)):
        assert cast(tick=t) == capi.ERR_INVALID and "tick" in capi.last_error()
    assert cast(sc=None) == capi.ERR_INVALID and "scan config" in capi.last_error()
    assert cast(lst=p) == capi.ERR_INVALID and "together" in capi.last_error()
    assert clear(rows=0) == capi.ERR_INVALID and "rows" in capi.last_error()


@pytest.mark.parametrize("name", ["f110qp_rollout_grid_dev", "f110qp_rollout_grid"])
def test_rollout_grid_validation_errors_touch_no_device(capi, name):
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

    def call(walls=ok, segments=p, batch=4, body=body, cc=cc, rf=every, noise=quiet, gc=room, grid=p, patch=None):
        # 0 table, 1 waypoints, 2 x_ref, 3 have_path, 4 circles, 5 segments, 6 grid, 7 x_traj, 8 u_lin_traj,
        # 9 u_applied, 10 status_traj, then the optional iters .. ranges_traj (11), clear_traj, nearest_traj,
        # crash_tick[, stream]
        a = [p] * 5 + [segments, grid] + [p] * 4 + [None] * 11 + [p, None, p] + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(s._h, ref(rc), ref(sc), ref(rp), ref(wc), ref(race), ref(cc), ref(body), ref(walls), ref(rf),
                  ref(noise), ref(gc), batch, *a)

    grid_rules(capi, call, 5 + 2 + 3)
    assert call(gc=None, batch=0) == capi.ERR_INVALID and "grid config" in capi.last_error()
    # every check of the noisy call
    noise_rules(capi, call, 4)
    assert call(rf=None) == capi.ERR_INVALID and "refresh config" in capi.last_error()
    assert call(rf=capi.default_refresh_config(every=-1)) == capi.ERR_INVALID and "every" in capi.last_error()
    wall_rules(capi, call, 4)
    assert call(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
    assert call(cc=None) == capi.ERR_INVALID and "contact config" in capi.last_error()
    assert call(patch={22: None}) == capi.ERR_INVALID and "clear_traj" in capi.last_error()
    assert call(patch={24: None}) == capi.ERR_INVALID and "crash_tick" in capi.last_error()
    assert call(patch={7: None}) == capi.ERR_INVALID and "x_traj" in capi.last_error()
    assert call(batch=0) == capi.OK
    assert call(batch=0, gc=capi.default_grid_config(), grid=None) == capi.OK
    s.close()


def test_binding_checks(capi):
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    cfg = (capi.default_race_config(), capi.default_contact_config(), capi.default_body_config())
    with pytest.raises(capi.F110QPError, match="GridConfig"):
        s.rollout_grid(None, None, None, None, None, None, *cfg, capi.default_refresh_config(),
                       capi.default_noise_config(), None, None, None, None, 1)
    with pytest.raises(capi.F110QPError, match="GridConfig"):
        s.rollout_grid_dev(None, None, None, None, *cfg, capi.default_walls_config(), capi.default_refresh_config(),
                           capi.default_noise_config(), 3, *[None] * 13)
    s.close()
