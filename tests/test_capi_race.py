"""The race entry points of the C ABI (f110qp_default_race_config, f110qp_cast_scans_race_dev,
f110qp_rollout_race[_dev]) without a GPU: exported symbols, the defaults, every argument rule (each answers
before the first device call) and the bindings' own checks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from test_capi_world import NOT_FINITE, ref, scan, world_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RACE = ("f110qp_default_race_config", "f110qp_cast_scans_race_dev", "f110qp_rollout_race_dev", "f110qp_rollout_race")


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in RACE:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    assert "} f110qp_race_config;" in hdr


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_header_compiles_with_the_race_calls(tmp_path, lang, cc):
    """The header as C and as C++ (test_capi_dbl.py's pattern), in a program that names the race calls."""
    assert shutil.which(cc) is not None, f"{cc} not installed"
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "f110qp.h"\nint main(void) { f110qp_race_config r; f110qp_default_race_config(&r);\n'
                   "  return f110qp_cast_scans_race_dev(0, 0, &r, 0, 0, 0, 0, 0, 0, 0) + (sizeof(r) == 24 ? 0 : 1)\n"
                   "    + (&f110qp_rollout_race_dev != 0) + (&f110qp_rollout_race != 0); }\n")
    subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-Wno-address", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_default_race_config(capi):
    r = capi.default_race_config()
    assert (r.group_size, r.car_radius, r.center_offset) == (1, 0.3, 0.1651)
    r = capi.default_race_config(group_size=4, center_offset=0.0)
    assert (r.group_size, r.car_radius, r.center_offset) == (4, 0.3, 0.0)
    capi.load().f110qp_default_race_config(None)  # a NULL config is ignored
    assert C.sizeof(capi.RaceConfig) == 24
    junk = capi.RaceConfig()
    C.memset(C.byref(junk), 0xFF, C.sizeof(junk))
    capi.load().f110qp_default_race_config(C.byref(junk))  # zeroes first: the padding too
    assert bytes(junk) == bytes(capi.default_race_config())


def race_rules(capi, call, B):
    """The rules on the race shared by the three calls; call(race=..., batch=...) -> return code."""
    assert call(race=None) == capi.ERR_INVALID
    assert "race config" in capi.last_error()
    for G in (0, -1, -B):
        assert call(race=capi.default_race_config(group_size=G)) == capi.ERR_INVALID, G
        assert "group_size" in capi.last_error()
    for G in (B - 1, B + 1, 2 * B):
        assert call(race=capi.default_race_config(group_size=G)) == capi.ERR_INVALID, G
        assert "multiple of group_size" in capi.last_error()
    for v in NOT_FINITE + [0.0, -0.3]:
        assert call(race=capi.default_race_config(group_size=2, car_radius=v)) == capi.ERR_INVALID, v
        assert "car_radius" in capi.last_error()
    for v in NOT_FINITE:
        assert call(race=capi.default_race_config(group_size=2, center_offset=v)) == capi.ERR_INVALID, v
        assert "center_offset" in capi.last_error()
    # the rules hold at batch 0 too (0 is a multiple of every G), and nothing is launched there
    assert call(batch=0, race=None) == capi.ERR_INVALID
    assert call(batch=0, race=capi.default_race_config(group_size=0)) == capi.ERR_INVALID
    assert call(batch=0, race=capi.default_race_config(group_size=7, center_offset=-0.2)) == capi.OK


def test_cast_scans_race_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    sc_ok, wc_ok = scan(capi, scan_rows=7), capi.default_world_config(num_circles=5)
    race_ok = capi.default_race_config(group_size=2)

    def call(sc=sc_ok, wc=wc_ok, race=race_ok, batch=4, lst=None, count=None, x=p, circles=p, ranges=p):
        return L.f110qp_cast_scans_race_dev(ref(sc), ref(wc), ref(race), batch, lst, count, x, circles, ranges, None)

    world_rules(capi, call, 4)
    race_rules(capi, call, 4)
    assert call(sc=None) == capi.ERR_INVALID
    assert call(sc=scan(capi, num_ranges=0)) == capi.ERR_INVALID and call(sc=scan(capi, num_ranges=65536)) == capi.ERR_INVALID
    assert call(sc=scan(capi, angle_increment=0.0)) == capi.ERR_INVALID
    assert "angle_increment" in capi.last_error()
    assert call(lst=p) == capi.ERR_INVALID and "together" in capi.last_error()
    assert call(count=p) == capi.ERR_INVALID and "together" in capi.last_error()
    assert call(x=None) == capi.ERR_INVALID and call(ranges=None) == capi.ERR_INVALID
    assert "non-NULL" in capi.last_error()
    assert call(batch=-1) == capi.ERR_INVALID
    # no static circle: circles may be NULL; with circles announced it may not
    assert call(batch=0, wc=capi.default_world_config(), circles=None) == capi.OK
    assert call(wc=capi.default_world_config(num_circles=1), circles=None) == capi.ERR_INVALID
    big = capi.default_world_config(num_circles=2**31 - 1)
    assert call(wc=big, race=capi.default_race_config(group_size=4)) == capi.ERR_INVALID
    assert "does not fit" in capi.last_error()


@pytest.mark.parametrize("name", ["f110qp_rollout_race_dev", "f110qp_rollout_race"])
def test_rollout_race_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok, rp_ok = capi.default_rollout_config(ticks=3), capi.default_replan_config(num_waypoints=4)
    sc_ok, wc_ok = scan(capi, scan_rows=7), capi.default_world_config(num_circles=5)
    race_ok = capi.default_race_config(group_size=2)

    def call(rc=ok, sc=sc_ok, rp=rp_ok, wc=wc_ok, race=race_ok, batch=4, patch=None, ctx=s._h, circles=p):
        # 0 table, 1 waypoints, 2 x_ref, 3 have_path, 4 circles, 5 x_traj, 6 u_lin_traj, 7 u_applied, 8 status_traj,
        # then the optional arrays of f110qp_rollout_world[_dev]
        a = [p] * 4 + [circles] + [p] * 4 + [None] * 11 + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(ctx, ref(rc), ref(sc), ref(rp), ref(wc), ref(race), batch, *a)

    world_rules(capi, call, 4)
    race_rules(capi, call, 4)
    # the checks f110qp_rollout_world[_dev] makes
    s1 = capi.Solver(capi.default_config(1, x_ref_points=50))
    assert call(ctx=s1._h) == capi.ERR_INVALID and "horizon" in capi.last_error()
    s1.close()
    for pts in (0, 20, 49, 51):
        s2 = capi.Solver(capi.default_config(20, x_ref_points=pts))
        assert call(ctx=s2._h) == capi.ERR_INVALID and "x_ref_points" in capi.last_error()
        s2.close()
    for d in (0.0, -1.0, float("nan"), float("inf")):
        assert call(rp=capi.default_replan_config(replan_dist=d)) == capi.ERR_INVALID
        assert "replan_dist" in capi.last_error()
    assert call(rp=capi.default_replan_config(num_waypoints=-1)) == capi.ERR_INVALID
    assert call(rp=capi.default_replan_config(steer_discrete=0)) == capi.ERR_INVALID
    assert call(rc=capi.default_rollout_config(ticks=0)) == capi.ERR_INVALID and "ticks" in capi.last_error()
    assert call(rc=capi.default_rollout_config(ticks=3, plant_dt=-1.0)) == capi.ERR_INVALID
    assert call(rc=None) == capi.ERR_INVALID and call(sc=None) == capi.ERR_INVALID and call(rp=None) == capi.ERR_INVALID
    assert call(sc=scan(capi, num_ranges=0)) == capi.ERR_INVALID
    assert call(sc=scan(capi, angle_increment=-1.0)) == capi.ERR_INVALID
    assert call(ctx=None) == capi.ERR_INVALID and call(batch=-1) == capi.ERR_INVALID
    for k in (0, 1, 2, 3, 5, 6, 7, 8):  # every required pointer (4, the circles, is a world rule)
        assert call(patch={k: None}) == capi.ERR_INVALID, k
        assert "non-NULL" in capi.last_error()
    if dev:
        off = C.c_void_p(buf.ctypes.data + 4)
        assert call(patch={7: off}) == capi.ERR_INVALID and "aligned" in capi.last_error()  # u_applied
        assert call(patch={11: off}) == capi.ERR_INVALID and "aligned" in capi.last_error()  # u_plan
    assert call(batch=0) == capi.OK
    s.close()


def test_binding_checks_types_and_shapes(capi):
    s = capi.Solver(capi.default_config(4, x_ref_points=6))
    rp = capi.default_replan_config(traj_discrete=6, steer_discrete=2, num_waypoints=3)
    sc = scan(capi, num_ranges=8)
    x0, ul, tab, wp = np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((3, 6, 3)), np.zeros((3, 2))
    ci = np.zeros((5, 3))
    race = capi.default_race_config(group_size=2)
    with pytest.raises(capi.F110QPError, match="race must be a RaceConfig"):
        s.rollout_race(x0, ul, ci, None, sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="group_size must be >= 1 and divide B = 2"):
        s.rollout_race(x0, ul, ci, capi.default_race_config(group_size=3), sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="group_size must be >= 1"):
        s.rollout_race(x0, ul, ci, capi.default_race_config(group_size=0), sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="x0 must be a float64"):
        s.rollout_race(x0.astype(np.float32), ul, ci, race, sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="ticks must be >= 1"):
        s.rollout_race(x0, ul, ci, race, sc, rp, tab, wp, 0)
    with pytest.raises(capi.F110QPError, match="circles must be a float64"):
        s.rollout_race(x0, ul, ci.astype(np.float32), race, sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="one world or B"):
        s.rollout_race(x0, ul, np.zeros((3, 5, 3)), race, sc, rp, tab, wp, 2)
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.float64)
    i32 = torch.zeros(16, dtype=torch.int32)
    rc, w = capi.default_rollout_config(ticks=2), capi.default_world_config(num_circles=5)
    xr, xt = t64[:36].view(2, 6, 3), t64[:18].view(3, 2, 3)
    args = (rc, sc, rp, w, race, t64, t64, xr, i32, t64, xt, t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="race must be a RaceConfig"):
        s.rollout_race_dev(rc, sc, rp, w, w, *args[5:])
    with pytest.raises(capi.F110QPError, match="group_size must be >= 1 and divide B = 2"):
        s.rollout_race_dev(rc, sc, rp, w, capi.default_race_config(group_size=4), *args[5:])
    with pytest.raises(capi.F110QPError, match="x_traj must be \\[ticks"):
        s.rollout_race_dev(*args[:10], t64[:12].view(2, 2, 3), *args[11:])
    with pytest.raises(capi.F110QPError, match="circles must be torch.float64"):
        s.rollout_race_dev(*args[:9], t32, *args[10:])
    with pytest.raises(capi.F110QPError, match="circles holds"):
        s.rollout_race_dev(*args[:9], t64[:14], *args[10:])
    with pytest.raises(capi.F110QPError, match="ranges_traj must be torch.float32"):
        s.rollout_race_dev(*args, ranges_traj=t64)
    with pytest.raises(capi.F110QPError, match="ranges_traj holds"):
        s.rollout_race_dev(*args, ranges_traj=t32[:31])
    x = t64[:6].view(2, 3)
    with pytest.raises(capi.F110QPError, match="group_size must be >= 1 and divide B = 2"):
        capi.cast_scans_race_dev(sc, w, capi.default_race_config(group_size=3), x, t64, t32)
    with pytest.raises(capi.F110QPError, match="ranges holds"):
        capi.cast_scans_race_dev(sc, w, race, x, t64, t32[:15])
    with pytest.raises(capi.F110QPError, match="list must be torch.int32"):
        capi.cast_scans_race_dev(sc, w, race, x, t64, t32, list_=t32, count=i32)
    with pytest.raises(capi.F110QPError, match="x must be torch.float64"):
        capi.cast_scans_race_dev(sc, w, race, t32[:6].view(2, 3), t64, t32)
    with pytest.raises(capi.F110QPError, match="circles must be torch.float64"):
        capi.cast_scans_race_dev(sc, w, race, x, t32, t32)
    s.close()
