"""The contact entry points of the C ABI (f110qp_clearance_dev, f110qp_default_contact_config,
f110qp_rollout_contact[_dev]) without a GPU: exported symbols, the defaults, every argument rule (each answers
before the first device call) and the bindings' own checks."""
import ctypes as C
import os

import numpy as np
import pytest
from test_capi_race import race_rules
from test_capi_world import NOT_FINITE, ref, scan, world_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTACT = ("f110qp_clearance_dev", "f110qp_default_contact_config", "f110qp_rollout_contact_dev", "f110qp_rollout_contact")


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in CONTACT:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    assert "} f110qp_contact_config;" in hdr
    assert "#define F110QP_TICK_CRASHED 4" in hdr and capi.TICK_CRASHED == 4


def test_default_contact_config(capi):
    c = capi.default_contact_config()
    assert (c.stop_on_contact, c.margin) == (0, 0.0)
    c = capi.default_contact_config(stop_on_contact=1, margin=0.05)
    assert (c.stop_on_contact, c.margin) == (1, 0.05)
    capi.load().f110qp_default_contact_config(None)  # a NULL config is ignored
    assert C.sizeof(capi.ContactConfig) == 16
    junk = capi.ContactConfig()
    C.memset(C.byref(junk), 0xFF, C.sizeof(junk))
    capi.load().f110qp_default_contact_config(C.byref(junk))  # zeroes first: the padding too
    assert bytes(junk) == bytes(16)


def test_clearance_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    wc_ok, race_ok = capi.default_world_config(num_circles=5), capi.default_race_config(group_size=2)

    def call(wc=wc_ok, race=race_ok, batch=4, rows=3, x=p, circles=p, clearance=p, nearest=None):
        return L.f110qp_clearance_dev(ref(wc), ref(race), batch, rows, x, circles, clearance, nearest, None)

    world_rules(capi, call, 4)
    race_rules(capi, call, 4)
    for rows in (0, -1):
        assert call(rows=rows) == capi.ERR_INVALID and "rows" in capi.last_error()
        assert call(rows=rows, batch=0) == capi.ERR_INVALID
    assert call(x=None) == capi.ERR_INVALID and "non-NULL" in capi.last_error()
    assert call(clearance=None) == capi.ERR_INVALID and "non-NULL" in capi.last_error()
    assert call(batch=-1) == capi.ERR_INVALID
    assert call(batch=0) == capi.OK
    # no static circle: circles may be NULL; with circles announced it may not
    assert call(batch=0, wc=capi.default_world_config(), circles=None) == capi.OK
    assert call(wc=capi.default_world_config(num_circles=1), circles=None) == capi.ERR_INVALID


@pytest.mark.parametrize("name", ["f110qp_rollout_contact_dev", "f110qp_rollout_contact"])
def test_rollout_contact_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok, rp_ok = capi.default_rollout_config(ticks=3), capi.default_replan_config(num_waypoints=4)
    sc_ok, wc_ok = scan(capi, scan_rows=7), capi.default_world_config(num_circles=5)
    race_ok, cc_ok = capi.default_race_config(group_size=2), capi.default_contact_config()

    def call(rc=ok, sc=sc_ok, rp=rp_ok, wc=wc_ok, race=race_ok, cc=cc_ok, batch=4, patch=None, ctx=s._h, circles=p):
        # 0 table, 1 waypoints, 2 x_ref, 3 have_path, 4 circles, 5 x_traj, 6 u_lin_traj, 7 u_applied, 8 status_traj,
        # 9..19 the optional arrays of f110qp_rollout_race[_dev], 20 clear_traj, 21 nearest_traj, 22 crash_tick
        a = [p] * 4 + [circles] + [p] * 4 + [None] * 11 + [p, None, p] + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(ctx, ref(rc), ref(sc), ref(rp), ref(wc), ref(race), ref(cc), batch, *a)

    world_rules(capi, call, 4)
    race_rules(capi, call, 4)
    assert call(cc=None) == capi.ERR_INVALID and "contact config" in capi.last_error()
    for v in (2, -1):
        assert call(cc=capi.default_contact_config(stop_on_contact=v)) == capi.ERR_INVALID
        assert "stop_on_contact" in capi.last_error()
    for v in NOT_FINITE:
        assert call(cc=capi.default_contact_config(margin=v)) == capi.ERR_INVALID and "margin" in capi.last_error()
    assert call(batch=0, cc=None) == capi.ERR_INVALID
    for k in (20, 22):
        assert call(patch={k: None}) == capi.ERR_INVALID and "clear_traj/crash_tick" in capi.last_error()
    # the checks f110qp_rollout_race[_dev] makes
    s1 = capi.Solver(capi.default_config(1, x_ref_points=50))
    assert call(ctx=s1._h) == capi.ERR_INVALID and "horizon" in capi.last_error()
    s1.close()
    s2 = capi.Solver(capi.default_config(20, x_ref_points=20))
    assert call(ctx=s2._h) == capi.ERR_INVALID and "x_ref_points" in capi.last_error()
    s2.close()
    assert call(rp=capi.default_replan_config(replan_dist=0.0)) == capi.ERR_INVALID
    assert call(rc=capi.default_rollout_config(ticks=0)) == capi.ERR_INVALID and "ticks" in capi.last_error()
    assert call(rc=None) == capi.ERR_INVALID and call(sc=None) == capi.ERR_INVALID and call(rp=None) == capi.ERR_INVALID
    assert call(sc=scan(capi, num_ranges=0)) == capi.ERR_INVALID
    assert call(ctx=None) == capi.ERR_INVALID and call(batch=-1) == capi.ERR_INVALID
    for k in (0, 1, 2, 3, 5, 6, 7, 8):
        assert call(patch={k: None}) == capi.ERR_INVALID, k
        assert "non-NULL" in capi.last_error()
    if dev:
        off = C.c_void_p(buf.ctypes.data + 4)
        assert call(patch={7: off}) == capi.ERR_INVALID and "aligned" in capi.last_error()  # u_applied
    assert call(batch=0) == capi.OK
    s.close()


def test_binding_checks_types_and_shapes(capi):
    s = capi.Solver(capi.default_config(4, x_ref_points=6))
    rp = capi.default_replan_config(traj_discrete=6, steer_discrete=2, num_waypoints=3)
    sc = scan(capi, num_ranges=8)
    x0, ul, tab, wp = np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((3, 6, 3)), np.zeros((3, 2))
    ci = np.zeros((5, 3))
    race, cc = capi.default_race_config(group_size=2), capi.default_contact_config()
    with pytest.raises(capi.F110QPError, match="cc a ContactConfig"):
        s.rollout_contact(x0, ul, ci, race, None, sc, rp, tab, wp, 2)
    with pytest.raises(capi.F110QPError, match="group_size must be >= 1 and divide B = 2"):
        s.rollout_contact(x0, ul, ci, capi.default_race_config(group_size=3), cc, sc, rp, tab, wp, 2)
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.float64)
    i32 = torch.zeros(16, dtype=torch.int32)
    rc, w = capi.default_rollout_config(ticks=2), capi.default_world_config(num_circles=5)
    xr, xt = t64[:36].view(2, 6, 3), t64[:18].view(3, 2, 3)
    args = (rc, sc, rp, w, race, cc, t64, t64, xr, i32, t64, xt, t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="cc a ContactConfig"):
        s.rollout_contact_dev(rc, sc, rp, w, race, race, *args[6:], t64, i32)
    with pytest.raises(capi.F110QPError, match="clear_traj must be torch.float64"):
        s.rollout_contact_dev(*args, t32, i32)
    with pytest.raises(capi.F110QPError, match="clear_traj holds"):
        s.rollout_contact_dev(*args, t64[:5], i32)
    with pytest.raises(capi.F110QPError, match="crash_tick holds"):
        s.rollout_contact_dev(*args, t64, i32[:1])
    with pytest.raises(capi.F110QPError, match="nearest_traj must be torch.int32"):
        s.rollout_contact_dev(*args, t64, i32, nearest_traj=t32)
    x = t64[:12].view(2, 2, 3)
    with pytest.raises(capi.F110QPError, match="group_size must be >= 1 and divide B = 2"):
        capi.clearance_dev(w, capi.default_race_config(group_size=3), x, t64, t64)
    with pytest.raises(capi.F110QPError, match="clearance holds"):
        capi.clearance_dev(w, race, x, t64, t64[:3])
    with pytest.raises(capi.F110QPError, match="nearest must be torch.int32"):
        capi.clearance_dev(w, race, x, t64, t64, nearest=t64)
    with pytest.raises(capi.F110QPError, match="x must be torch.float64"):
        capi.clearance_dev(w, race, t32[:12].view(2, 2, 3), t64, t64)
    with pytest.raises(capi.F110QPError, match=r"x must be \[rows, B, 3\]"):
        capi.clearance_dev(w, race, t64[:12].view(3, 4), t64, t64)
    s.close()
