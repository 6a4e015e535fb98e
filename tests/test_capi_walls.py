"""The straight-wall entry points of the C ABI (f110qp_default_walls_config, f110qp_cast_scans_walls_dev,
f110qp_clearance_walls_dev, f110qp_rollout_walls[_dev]) without a GPU: exported symbols, the defaults, the struct
layout against the header, and every wall rule, each of which answers before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from test_capi_world import ref, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALLS = ("f110qp_default_walls_config", "f110qp_cast_scans_walls_dev", "f110qp_clearance_walls_dev",
         "f110qp_rollout_walls_dev", "f110qp_rollout_walls")


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in WALLS:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive


def test_defaults_and_layout(capi):
    w = capi.default_walls_config()
    assert (w.num_segments, w.wall_rows) == (0, 1)
    w = capi.default_walls_config(num_segments=9, wall_rows=4)
    assert (w.num_segments, w.wall_rows) == (9, 4)
    capi.load().f110qp_default_walls_config(None)  # a NULL config is ignored
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} f110qp_walls_config;", hdr).group(1)
    fields = re.findall(r"^\s*(int|double|float)\s+(\w+);", body, re.M)
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(capi.WallsConfig._fields_)
    assert C.sizeof(capi.WallsConfig) == 8


def wall_rules(capi, call, B):
    """The wall rules shared by the four calls; call(walls=..., segments=...) -> return code."""
    assert call(walls=None) == capi.ERR_INVALID
    assert "walls config" in capi.last_error()
    assert call(walls=capi.default_walls_config(num_segments=-1)) == capi.ERR_INVALID
    assert "num_segments" in capi.last_error()
    for rows in (0, 2, B + 1, -1):
        assert call(walls=capi.default_walls_config(num_segments=3, wall_rows=rows)) == capi.ERR_INVALID, rows
        assert "wall_rows" in capi.last_error()
    assert call(walls=capi.default_walls_config(num_segments=3), segments=None) == capi.ERR_INVALID
    assert "segments" in capi.last_error()
    assert call(walls=capi.default_walls_config(num_segments=2 ** 31 - 3)) == capi.ERR_INVALID
    assert "fit an int" in capi.last_error()


def test_cast_and_clearance_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    sc, wc = scan(capi), capi.default_world_config(num_circles=5)
    race, body, ok = capi.default_race_config(group_size=2), capi.default_body_config(), capi.default_walls_config(num_segments=3)

    def cast(walls=ok, segments=p, batch=4, body=body, race=race, wc=wc, circles=p):
        return L.f110qp_cast_scans_walls_dev(ref(sc), ref(wc), ref(race), ref(body), ref(walls), batch, None, None, p,
                                             circles, segments, p, None)

    def clear(walls=ok, segments=p, batch=4, body=body, race=race, wc=wc, circles=p, rows=2):
        return L.f110qp_clearance_walls_dev(ref(wc), ref(race), ref(body), ref(walls), batch, rows, p, circles, segments,
                                            p, None, None)

    for call in (cast, clear):
        wall_rules(capi, call, 4)
        # the twin's rules still answer
        assert call(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
        assert call(race=None) == capi.ERR_INVALID and "race config" in capi.last_error()
        assert call(wc=None) == capi.ERR_INVALID and "world config" in capi.last_error()
        assert call(batch=3) == capi.ERR_INVALID and "group_size" in capi.last_error()
        # batch 0 is valid with and without segments and circles
        assert call(batch=0) == capi.OK
        assert call(batch=0, walls=capi.default_walls_config(), segments=None) == capi.OK
        assert call(batch=0, wc=capi.default_world_config(), circles=None) == capi.OK
    assert clear(rows=0) == capi.ERR_INVALID and "rows" in capi.last_error()


@pytest.mark.parametrize("name", ["f110qp_rollout_walls_dev", "f110qp_rollout_walls"])
def test_rollout_walls_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    rc, rp = capi.default_rollout_config(ticks=3), capi.default_replan_config(num_waypoints=4)
    sc, wc = scan(capi), capi.default_world_config(num_circles=5)
    race, cc, body = capi.default_race_config(group_size=2), capi.default_contact_config(), capi.default_body_config()
    ok = capi.default_walls_config(num_segments=3)

    def call(walls=ok, segments=p, batch=4, body=body, cc=cc, patch=None):
        # 0 table, 1 waypoints, 2 x_ref, 3 have_path, 4 circles, 5 segments, 6 x_traj, 7 u_lin_traj, 8 u_applied,
        # 9 status_traj, then the optional iters .. ranges_traj (11), clear_traj, nearest_traj, crash_tick[, stream]
        a = [p] * 5 + [segments] + [p] * 4 + [None] * 11 + [p, None, p] + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(s._h, ref(rc), ref(sc), ref(rp), ref(wc), ref(race), ref(cc), ref(body), ref(walls), batch, *a)

    wall_rules(capi, call, 4)
    assert call(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
    assert call(cc=None) == capi.ERR_INVALID and "contact config" in capi.last_error()
    assert call(patch={21: None}) == capi.ERR_INVALID and "clear_traj" in capi.last_error()
    assert call(patch={23: None}) == capi.ERR_INVALID and "crash_tick" in capi.last_error()
    assert call(batch=0) == capi.OK
    assert call(batch=0, walls=capi.default_walls_config(), segments=None) == capi.OK
    s.close()


def test_binding_checks(capi):
    with pytest.raises(capi.F110QPError):
        capi._wall_spec(capi.default_world_config(), None)
    assert capi._wall_spec(capi.default_walls_config(), None)[-1] is True  # S = 0: the segments may be None
    assert capi._wall_spec(capi.default_walls_config(num_segments=3, wall_rows=2), None)[2] == 24
