"""The simulated-LiDAR entry points of the C ABI (f110qp_default_world_config, f110qp_cast_scans_dev,
f110qp_rollout_world[_dev]) without a GPU: exported symbols, the defaults, every argument rule (each answers
before the first device call), the bindings' own checks, workload.make_world and the numpy oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import world_cases as wc_

from f110qp import workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = ("f110qp_default_world_config", "f110qp_cast_scans_dev", "f110qp_rollout_world_dev", "f110qp_rollout_world")
NOT_FINITE = [float("nan"), float("inf"), float("-inf")]


def scan(capi, **over):
    kw = dict(num_ranges=64, angle_min=-2.0, angle_increment=0.0625, angle_max=2.0)
    kw.update(over)
    return capi.default_scan_config(**kw)


def ref(v):
    return C.byref(v) if v is not None else None


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in WORLD:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    assert f"#define F110QP_CAST_CIRCLE_TILE {capi.CAST_CIRCLE_TILE}" in hdr and wc_.TILE == capi.CAST_CIRCLE_TILE


def test_default_world_config(capi):
    w = capi.default_world_config()
    assert (w.num_circles, w.world_rows, w.lidar_offset, w.max_range) == (0, 1, 0.275, 10.0)
    w = capi.default_world_config(num_circles=7, world_rows=3, max_range=4.0)
    assert (w.num_circles, w.world_rows, w.lidar_offset, w.max_range) == (7, 3, 0.275, 4.0)
    capi.load().f110qp_default_world_config(None)  # a NULL config is ignored
    assert C.sizeof(capi.WorldConfig) == 24
    assert (wc_.LIDAR_OFFSET, wc_.MAX_RANGE) == (0.275, 10.0)


def world_rules(capi, call, B):
    """The rules on the world shared by the three calls; call(wc=..., circles=...) -> return code."""
    ok = capi.default_world_config(num_circles=5)
    assert call(wc=None) == capi.ERR_INVALID
    assert "world config" in capi.last_error()
    for rows in (0, 2, B + 1, -1):
        assert call(wc=capi.default_world_config(num_circles=5, world_rows=rows)) == capi.ERR_INVALID, rows
        assert "world_rows" in capi.last_error()
    assert call(wc=capi.default_world_config(num_circles=-1)) == capi.ERR_INVALID
    assert "num_circles" in capi.last_error()
    assert call(wc=ok, circles=None) == capi.ERR_INVALID
    assert "circles" in capi.last_error()
    for v in NOT_FINITE + [0.0, -1.0]:
        assert call(wc=capi.default_world_config(num_circles=5, max_range=v)) == capi.ERR_INVALID, v
        assert "max_range" in capi.last_error()
    for v in NOT_FINITE:
        assert call(wc=capi.default_world_config(num_circles=5, lidar_offset=v)) == capi.ERR_INVALID, v
        assert "lidar_offset" in capi.last_error()


def test_cast_scans_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    sc_ok, wc_ok = scan(capi, scan_rows=7), capi.default_world_config(num_circles=5)  # scan_rows is not read

    def call(sc=sc_ok, wc=wc_ok, batch=4, lst=None, count=None, x=p, circles=p, ranges=p):
        return L.f110qp_cast_scans_dev(ref(sc), ref(wc), batch, lst, count, x, circles, ranges, None)

    world_rules(capi, call, 4)
    assert call(sc=None) == capi.ERR_INVALID
    assert call(sc=scan(capi, num_ranges=0)) == capi.ERR_INVALID and call(sc=scan(capi, num_ranges=65536)) == capi.ERR_INVALID
    assert call(sc=scan(capi, angle_increment=0.0)) == capi.ERR_INVALID
    assert "angle_increment" in capi.last_error()
    assert call(lst=p) == capi.ERR_INVALID  # a list without a count
    assert "together" in capi.last_error()
    assert call(count=p) == capi.ERR_INVALID  # a count without a list
    assert "together" in capi.last_error()
    assert call(x=None) == capi.ERR_INVALID and call(ranges=None) == capi.ERR_INVALID
    assert "non-NULL" in capi.last_error()
    assert call(batch=-1) == capi.ERR_INVALID
    assert call(batch=0, wc=capi.default_world_config(num_circles=5)) == capi.OK
    assert call(batch=0, wc=capi.default_world_config(), circles=None) == capi.OK


@pytest.mark.parametrize("name", ["f110qp_rollout_world_dev", "f110qp_rollout_world"])
def test_rollout_world_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok, rp_ok = capi.default_rollout_config(ticks=3), capi.default_replan_config(num_waypoints=4)
    sc_ok, wc_ok = scan(capi, scan_rows=7), capi.default_world_config(num_circles=5)  # scan_rows is not read

    def call(rc=ok, sc=sc_ok, rp=rp_ok, wc=wc_ok, batch=4, patch=None, ctx=s._h, circles=p):
        # 0 table, 1 waypoints, 2 x_ref, 3 have_path, 4 circles, 5 x_traj, 6 u_lin_traj, 7 u_applied, 8 status_traj,
        # then the optional iters, cost, u_plan, x_plan, hs_traj, kind, plan_status, best_traj, best_global, pose,
        # ranges_traj[, stream]
        a = [p] * 4 + [circles] + [p] * 4 + [None] * 11 + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(ctx, ref(rc), ref(sc), ref(rp), ref(wc), batch, *a)

    world_rules(capi, call, 4)
    # the checks f110qp_rollout_replan_dev makes
    s1 = capi.Solver(capi.default_config(1, x_ref_points=50))
    assert call(ctx=s1._h) == capi.ERR_INVALID
    assert "horizon" in capi.last_error()
    s1.close()
    for pts in (0, 20, 49, 51):
        s2 = capi.Solver(capi.default_config(20, x_ref_points=pts))
        assert call(ctx=s2._h) == capi.ERR_INVALID
        assert "x_ref_points" in capi.last_error()
        s2.close()
    for d in (0.0, -1.0, float("nan"), float("inf")):
        assert call(rp=capi.default_replan_config(replan_dist=d)) == capi.ERR_INVALID
        assert "replan_dist" in capi.last_error()
    assert call(rp=capi.default_replan_config(num_waypoints=-1)) == capi.ERR_INVALID
    assert call(rp=capi.default_replan_config(steer_discrete=0)) == capi.ERR_INVALID
    assert call(rc=capi.default_rollout_config(ticks=0)) == capi.ERR_INVALID
    assert "ticks" in capi.last_error()
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
        assert call(patch={7: off}) == capi.ERR_INVALID  # u_applied
        assert "aligned" in capi.last_error()
        assert call(patch={11: off}) == capi.ERR_INVALID  # u_plan
        assert "aligned" in capi.last_error()
    for rows in (0, 2, 3, -1):  # scan_rows is not read: any value passes (batch 0 launches nothing)
        assert call(sc=scan(capi, scan_rows=rows), batch=0, wc=capi.default_world_config(num_circles=5, world_rows=1)) == capi.OK
    assert call(batch=0, wc=capi.default_world_config(num_circles=5, world_rows=0)) == capi.OK
    s.close()


def test_binding_checks_types_and_shapes(capi):
    s = capi.Solver(capi.default_config(4, x_ref_points=6))
    rp = capi.default_replan_config(traj_discrete=6, steer_discrete=2, num_waypoints=3)
    sc = scan(capi, num_ranges=8)
    x0, ul, tab, wp = np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((3, 6, 3)), np.zeros((3, 2))
    ci = np.zeros((5, 3))
    with pytest.raises(capi.F110QPError, match="x0 must be a float64"):
        s.rollout_world(x0.astype(np.float32), ul, ci, sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="ticks must be >= 1"):
        s.rollout_world(x0, ul, ci, sc, rp, tab, wp, 0)
    with pytest.raises(capi.F110QPError, match="circles must be a float64"):
        s.rollout_world(x0, ul, ci.astype(np.float32), sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="circles must be a float64"):
        s.rollout_world(x0, ul, np.zeros((5, 2)), sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="one world or B"):
        s.rollout_world(x0, ul, np.zeros((3, 5, 3)), sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="waypoints must hold"):
        s.rollout_world(x0, ul, ci, sc, rp, tab, wp[:2], 2)
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.float64)
    i32 = torch.zeros(16, dtype=torch.int32)
    rc, w = capi.default_rollout_config(ticks=2), capi.default_world_config(num_circles=5)
    xr, xt = t64[:36].view(2, 6, 3), t64[:18].view(3, 2, 3)
    args = (rc, sc, rp, w, t64, t64, xr, i32, t64, xt, t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="x_traj must be \\[ticks"):
        s.rollout_world_dev(*args[:9], t64[:12].view(2, 2, 3), *args[10:])
    with pytest.raises(capi.F110QPError, match="circles must be torch.float64"):
        s.rollout_world_dev(*args[:8], t32, *args[9:])
    with pytest.raises(capi.F110QPError, match="circles holds"):
        s.rollout_world_dev(*args[:8], t64[:14], *args[9:])
    with pytest.raises(capi.F110QPError, match="world_rows must be 1 or B"):
        s.rollout_world_dev(rc, sc, rp, capi.default_world_config(num_circles=5, world_rows=3), *args[4:])
    with pytest.raises(capi.F110QPError, match="ranges_traj must be torch.float32"):
        s.rollout_world_dev(*args, ranges_traj=t64)
    with pytest.raises(capi.F110QPError, match="ranges_traj holds"):
        s.rollout_world_dev(*args, ranges_traj=t32[:31])
    with pytest.raises(capi.F110QPError, match="ranges holds"):
        capi.cast_scans_dev(sc, w, t64[:6].view(2, 3), t64, t32[:15])
    with pytest.raises(capi.F110QPError, match="list must be torch.int32"):
        capi.cast_scans_dev(sc, w, t64[:6].view(2, 3), t64, t32, list_=t32, count=i32)
    with pytest.raises(capi.F110QPError, match="x must be torch.float64"):
        capi.cast_scans_dev(sc, w, t32[:6].view(2, 3), t64, t32)
    s.close()


def test_make_world_is_drive_streams_world():
    """make_world(seed, obstacles) returns the circles drive_stream(seed=seed, obstacles=obstacles) scans:
    every scan of the stream is reproduced from them (the stream keeps the 200 nearest circles of each
    pose), bit for bit."""
    for seed, obstacles in ((0, 40), (5, 40), (3, 7)):
        w = workload.make_world(seed, obstacles)
        assert w.shape == (1000 + obstacles, 3) and w.dtype == np.float64 and w.flags.c_contiguous
        assert (w[:1000, 2] == 0.12).all() and (w[1000:, 2] >= 0.15).all() and (w[1000:, 2] <= 0.3).all()
        d = workload.drive_stream(4, seed=seed, obstacles=obstacles)
        pose = d["pose"]
        yaw = np.arctan2(pose[:, 2], pose[:, 3]) * 2.0
        ang = yaw[:, None] + (d["angle_min"] + d["angle_inc"] * np.arange(1080, dtype=np.float64))[None, :]
        lx, ly = pose[:, 0] + 0.275 * np.cos(yaw), pose[:, 1] + 0.275 * np.sin(yaw)
        near = np.argsort(np.hypot(w[None, :, 0] - lx[:, None], w[None, :, 1] - ly[:, None]), axis=1)[:, :200]
        r = workload._ray_circles(lx, ly, ang, w[near, 0], w[near, 1], w[near, 2], 10.0).astype(np.float32)
        agree = r == d["ranges"]
        # yaw is recovered from the pose's quaternion: a beam can move by a rounding of the angle
        assert agree.mean() >= 0.999 and np.abs(r - d["ranges"]).max() <= 1e-5, (seed, agree.mean())


def test_oracle_restates_ray_circles():
    """The test oracle is workload._ray_circles on the header's angles: C = 0, a shared world and per-car
    worlds, and the classifier's counts the hand-made cases and the track world were checked with."""
    g = wc_.geometry(65)
    x = wc_.poses_near_origin(3, 1, wc_.YAWS)
    assert (wc_.oracle_scan(x, np.zeros((0, 3)), g, 65) == np.float32(10.0)).all()
    w = wc_.random_world(40, 2)
    one = wc_.oracle_scan(x, w, g, 65)
    per = wc_.oracle_scan(x, np.ascontiguousarray(np.tile(w[None], (3, 1, 1))), g, 65)
    assert one.dtype == np.float32 and (one == per).all() and (one < 10.0).any() and (one == 10.0).any()
    for kind in ("2pi", "270"):
        g = wc_.geometry(1080, kind)
        for name, (xs, ci, _) in wc_.hand_cases(g, 1080).items():
            assert wc_.grazing(xs, ci, g, 1080).sum() <= 1, (kind, name)
    g = wc_.geometry(1080)
    assert wc_.grazing(wc_.track_poses(64), wc_.track_world(), g, 1080).sum() == 0
