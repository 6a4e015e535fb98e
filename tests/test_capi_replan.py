"""The re-planning closed-loop entry points of the C ABI (f110qp_default_replan_config,
f110qp_plan_listed_dev, f110qp_replan_start_dev, f110qp_advance_replan_dev, f110qp_rollout_replan[_dev])
without a GPU: exported symbols, the defaults, and the argument checks, every one of which answers before
the first device call."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAN = ("f110qp_default_replan_config", "f110qp_plan_listed_dev", "f110qp_replan_start_dev",
          "f110qp_advance_replan_dev", "f110qp_rollout_replan_dev", "f110qp_rollout_replan")


def scan(capi, **over):
    kw = dict(num_ranges=64, angle_min=-2.0, angle_increment=0.0625, angle_max=2.0)
    kw.update(over)
    return capi.default_scan_config(**kw)


def test_symbols_constants_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in REPLAN:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    for name, v in (("TICK_MPC", 0), ("TICK_PLAN", 1), ("TICK_HOLD", 2), ("TICK_PLAN_FAILED", 3), ("NO_SOLVE", 0)):
        assert getattr(capi, name) == v and f"#define F110QP_{name} {v}" in hdr
    # no status a solve reports is NO_SOLVE
    assert capi.NO_SOLVE not in (capi.SOLVED, capi.SOLVED_INACCURATE, capi.MAX_ITER, capi.PRIMAL_INFEASIBLE,
                                 capi.NUMERICAL)


def test_default_replan_config(capi):
    rp = capi.default_replan_config()
    assert rp.replan_dist == 1.98 and rp.num_waypoints == 0  # src/project.cpp:182
    ref = capi.default_plan_config()
    for f, _ in capi.PlanConfig._fields_:
        assert getattr(rp.plan, f) == getattr(ref, f), f
    assert rp.plan.traj_discrete == 50 and rp.plan.steer_discrete == 30
    rp = capi.default_replan_config(replan_dist=1.5, num_waypoints=7, traj_discrete=20)
    assert (rp.replan_dist, rp.num_waypoints, rp.plan.traj_discrete, rp.plan.steer_discrete) == (1.5, 7, 20, 30)
    capi.load().f110qp_default_replan_config(None)  # a NULL config is ignored
    assert C.sizeof(capi.ReplanConfig) == 8 + C.sizeof(capi.PlanConfig) + 8


BAD_DIST = [0.0, -1.0, float("nan"), float("inf")]


@pytest.mark.parametrize("name", ["f110qp_rollout_replan_dev", "f110qp_rollout_replan"])
def test_rollout_replan_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok, sc_ok, rp_ok = capi.default_rollout_config(ticks=3), scan(capi), capi.default_replan_config(num_waypoints=4)

    def call(rc=ok, sc=sc_ok, rp=rp_ok, batch=4, patch=None, ctx=s._h):
        # table, waypoints, x_ref, have_path, ranges, x_traj, u_lin_traj, u_applied, status_traj, then the
        # optional iters, cost, u_plan, x_plan, hs_traj, kind, plan_status, best_traj, best_global, pose[, stream]
        a = [p] * 9 + [None] * 10 + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        ref = lambda v: C.byref(v) if v is not None else None  # noqa: E731
        return fn(ctx, ref(rc), ref(sc), ref(rp), batch, *a)

    for N in (1,):  # horizon 1: the index model has no counterpart of f110qp_advance_dev's N = 1 rule
        s1 = capi.Solver(capi.default_config(N, x_ref_points=50))
        assert call(ctx=s1._h) == capi.ERR_INVALID
        assert "horizon" in capi.last_error()
        s1.close()
    for pts in (0, 20, 49, 51):  # x_ref_points != traj_discrete (0 means N = 20)
        s2 = capi.Solver(capi.default_config(20, x_ref_points=pts))
        assert call(ctx=s2._h) == capi.ERR_INVALID
        assert "x_ref_points" in capi.last_error()
        s2.close()
    assert call(rp=capi.default_replan_config(traj_discrete=49)) == capi.ERR_INVALID
    assert "x_ref_points" in capi.last_error()
    for rows in (0, 2, 4, -1):  # ticks = 3: only 1 and 3 are rows
        assert call(sc=scan(capi, scan_rows=rows)) == capi.ERR_INVALID
        assert "scan_rows" in capi.last_error()
    assert call(sc=scan(capi, scan_rows=3), batch=0) == capi.OK
    for d in BAD_DIST:
        assert call(rp=capi.default_replan_config(replan_dist=d)) == capi.ERR_INVALID
        assert "replan_dist" in capi.last_error()
    assert call(rp=capi.default_replan_config(num_waypoints=-1)) == capi.ERR_INVALID
    assert call(rp=capi.default_replan_config(steer_discrete=0)) == capi.ERR_INVALID  # the plan config's own checks
    assert call(rc=capi.default_rollout_config(ticks=0)) == capi.ERR_INVALID
    assert "ticks" in capi.last_error()
    assert call(rc=capi.default_rollout_config(ticks=3, plant_dt=-1.0)) == capi.ERR_INVALID
    assert call(rc=None) == capi.ERR_INVALID and call(sc=None) == capi.ERR_INVALID and call(rp=None) == capi.ERR_INVALID
    assert "replan config" in capi.last_error()
    assert call(sc=scan(capi, num_ranges=0)) == capi.ERR_INVALID
    assert call(ctx=None) == capi.ERR_INVALID and call(batch=-1) == capi.ERR_INVALID
    for k in range(9):  # every required pointer
        assert call(patch={k: None}) == capi.ERR_INVALID, k
        assert "non-NULL" in capi.last_error()
    if dev:
        off = C.c_void_p(buf.ctypes.data + 4)
        assert call(patch={7: off}) == capi.ERR_INVALID  # u_applied
        assert "aligned" in capi.last_error()
        assert call(patch={11: off}) == capi.ERR_INVALID  # u_plan
        assert "aligned" in capi.last_error()
    assert call(batch=0) == capi.OK
    s.close()


def test_parts_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p, q = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2048)
    rc, sc, rp = capi.default_rollout_config(ticks=0), scan(capi, scan_rows=7), capi.default_replan_config(num_waypoints=4)
    ref = lambda v: C.byref(v) if v is not None else None  # noqa: E731

    def listed(rp=rp, sc=sc, batch=4, patch=None):
        a = [p] * 11 + [None]  # list, count, pose, ranges, table, waypoints, x_ref, plan_status, best_traj, best_global
        for k, v in (patch or {}).items():
            a[k] = v
        return L.f110qp_plan_listed_dev(ref(rp), ref(sc), batch, *a[:10], a[11])

    assert listed(rp=None) == capi.ERR_INVALID and listed(sc=None) == capi.ERR_INVALID
    assert listed(sc=scan(capi, angle_increment=0.0)) == capi.ERR_INVALID
    assert "angle_increment" in capi.last_error()
    for d in BAD_DIST:
        assert listed(rp=capi.default_replan_config(replan_dist=d)) == capi.ERR_INVALID
    assert listed(batch=-1) == capi.ERR_INVALID
    for k in range(10):
        assert listed(patch={k: None}) == capi.ERR_INVALID, k
    assert listed(batch=0) == capi.OK

    def start(rp=rp, sc=sc, batch=4, patch=None):
        a = [p, p, p, p, q, q, q, q, q, None]  # x, have_path, x_ref, gap, pose, kind, list, count, hs, stream
        for k, v in (patch or {}).items():
            a[k] = v
        return L.f110qp_replan_start_dev(ref(rp), ref(sc), batch, *a)

    assert start(rp=None) == capi.ERR_INVALID
    assert start(sc=None) == capi.ERR_INVALID  # hs asks for the scan geometry
    assert start(patch={3: None}) == capi.ERR_INVALID
    assert "gap" in capi.last_error()
    for k in (0, 1, 2, 4, 5, 6, 7):
        assert start(patch={k: None}) == capi.ERR_INVALID, k
    assert start(batch=-1) == capi.ERR_INVALID and start(batch=0) == capi.OK

    def step(rc=rc, rp=rp, sc=sc, batch=4, horizon=20, patch=None):
        # 0 x, 1 kind, 2 u_plan, 3 status, 4 plan_status, 5 x_ref, 6 gap, 7 u_held, 8 held_len, 9 held_idx, 10 have_path,
        # 11 x_next, 12 u_lin_next, 13 u_applied, 14 pose_next, 15 kind_next, 16 next_list, 17 next_count, 18 hs_next
        a = [p] * 11 + [q, q, None, q, q, q, q, q, None]
        for k, v in (patch or {}).items():
            a[k] = v
        return L.f110qp_advance_replan_dev(ref(rc), ref(rp), ref(sc), batch, horizon, *a)

    assert step(rc=None) == capi.ERR_INVALID and step(rp=None) == capi.ERR_INVALID and step(sc=None) == capi.ERR_INVALID
    assert step(rc=capi.default_rollout_config(car_length=0.0)) == capi.ERR_INVALID
    for h in (0, 1, 49):
        assert step(horizon=h) == capi.ERR_INVALID
        assert "horizon" in capi.last_error()
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 14):
        assert step(patch={k: None}) == capi.ERR_INVALID, k
        assert "non-NULL" in capi.last_error()
    assert step(patch={16: None}) == capi.ERR_INVALID and step(patch={17: None}) == capi.ERR_INVALID
    assert "kind_next" in capi.last_error()
    assert step(patch={6: None}) == capi.ERR_INVALID
    assert "gap" in capi.last_error()
    assert step(patch={11: p}) == capi.ERR_INVALID  # x_next aliases x
    assert "alias" in capi.last_error()
    for k in (2, 7, 13):
        assert step(patch={k: C.c_void_p(buf.ctypes.data + 4)}) == capi.ERR_INVALID
        assert "aligned" in capi.last_error()
    assert step(batch=-1) == capi.ERR_INVALID and step(batch=0) == capi.OK


def test_binding_checks_types_and_shapes(capi):
    s = capi.Solver(capi.default_config(4, x_ref_points=6))
    rp = capi.default_replan_config(traj_discrete=6, steer_discrete=2, num_waypoints=3)
    sc = scan(capi, num_ranges=8)
    x0, ul, tab, wp = np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((3, 6, 3)), np.zeros((3, 2))
    with pytest.raises(capi.F110QPError, match="x0 must be a float64"):
        s.rollout_replan(x0.astype(np.float32), ul, np.zeros((2, 8)), sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="ticks must be >= 1"):
        s.rollout_replan(x0, ul, np.zeros((2, 8)), sc, rp, tab, wp, 0)
    with pytest.raises(capi.F110QPError, match="ranges must hold"):
        s.rollout_replan(x0, ul, np.zeros((2, 7)), sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="waypoints must hold"):
        s.rollout_replan(x0, ul, np.zeros((2, 8)), sc, rp, tab, wp[:2], 2)
    with pytest.raises(capi.F110QPError, match="scan_rows must be 1 or ticks"):
        s.rollout_replan(x0, ul, np.zeros((3, 2, 8)), scan(capi, num_ranges=8, scan_rows=3), rp, tab, wp, 2)
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.float64)
    i32 = torch.zeros(16, dtype=torch.int32)
    rc = capi.default_rollout_config(ticks=2)
    xr, xt, rg = t64[:36].view(2, 6, 3), t64[:18].view(3, 2, 3), t32[:16].view(1, 2, 8)
    args = (rc, sc, rp, t64, t64, xr, i32, rg, xt, t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="x_traj must be \\[ticks"):
        s.rollout_replan_dev(*args[:8], t64[:12].view(2, 2, 3), *args[9:])
    with pytest.raises(capi.F110QPError, match="have_path must be torch.int32"):
        s.rollout_replan_dev(*args[:6], t32, *args[7:])
    with pytest.raises(capi.F110QPError, match="pose_traj holds"):
        s.rollout_replan_dev(*args, pose_traj=t64[:23])
    with pytest.raises(capi.F110QPError, match="kind_traj must be torch.int32"):
        s.rollout_replan_dev(*args, kind_traj=t32)
    with pytest.raises(capi.F110QPError, match="x_ref must be torch.float64"):
        capi.plan_listed_dev(rp, sc, i32, i32, t64[:8].view(2, 4), t32, t64, t64, t32, i32, i32, i32)
    with pytest.raises(capi.F110QPError, match="kind must be torch.int32"):
        capi.replan_start_dev(rp, sc, t64[:6].view(2, 3), i32, t64, None, t64, t32, i32, i32)
    with pytest.raises(capi.F110QPError, match="u_held must be torch.float32"):
        capi.advance_replan_dev(rc, rp, sc, 4, t64[:6].view(2, 3), i32, t32, i32, i32, t64, t64, i32, i32, i32, t64,
                                t64, t64)
    s.close()


def test_product_library_reads_no_environment_knob(capi):
    """The product library still holds no F110QP_ string (its behaviour is the config alone)."""
    with open(capi.LIB_PATH, "rb") as f:
        assert b"F110QP_" not in f.read()
