"""The rectangular-body entry points of the C ABI (f110qp_default_body_config, f110qp_clearance_body_dev,
f110qp_cast_scans_body_dev, f110qp_rollout_body[_dev]) without a GPU: exported symbols, the defaults and every
argument rule (each answers before the first device call)."""
import ctypes as C
import os

import numpy as np
import pytest
from test_capi_race import race_rules
from test_capi_world import NOT_FINITE, ref, scan, world_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY = ("f110qp_default_body_config", "f110qp_clearance_body_dev", "f110qp_cast_scans_body_dev",
        "f110qp_rollout_body_dev", "f110qp_rollout_body")


def body_rules(capi, call):
    """The rules on the body shared by the calls; call(body=...) -> return code."""
    assert call(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
    for v in NOT_FINITE + [0.0, -0.29]:
        assert call(body=capi.default_body_config(half_length=v)) == capi.ERR_INVALID, v
        assert "half_length" in capi.last_error()
        assert call(body=capi.default_body_config(half_width=v)) == capi.ERR_INVALID, v
        assert "half_width" in capi.last_error()
    assert call(body=None, batch=0) == capi.ERR_INVALID


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in BODY:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive
    assert "} f110qp_body_config;" in hdr


def test_default_body_config(capi):
    b = capi.default_body_config()
    assert (b.half_length, b.half_width) == (0.29, 0.155)
    b = capi.default_body_config(half_length=0.5)
    assert (b.half_length, b.half_width) == (0.5, 0.155)
    capi.load().f110qp_default_body_config(None)  # a NULL config is ignored
    assert C.sizeof(capi.BodyConfig) == 16
    junk = capi.BodyConfig()
    C.memset(C.byref(junk), 0xFF, C.sizeof(junk))
    capi.load().f110qp_default_body_config(C.byref(junk))
    assert bytes(junk) == bytes(capi.default_body_config())


def test_clearance_body_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    wc_ok, race_ok, body_ok = capi.default_world_config(num_circles=5), capi.default_race_config(group_size=2), \
        capi.default_body_config()

    def call(wc=wc_ok, race=race_ok, body=body_ok, batch=4, rows=3, x=p, circles=p, clearance=p, nearest=None):
        return L.f110qp_clearance_body_dev(ref(wc), ref(race), ref(body), batch, rows, x, circles, clearance, nearest, None)

    world_rules(capi, call, 4)
    race_rules(capi, call, 4)
    body_rules(capi, call)
    for rows in (0, -1):
        assert call(rows=rows) == capi.ERR_INVALID and "rows" in capi.last_error()
    assert call(x=None) == capi.ERR_INVALID and "non-NULL" in capi.last_error()
    assert call(clearance=None) == capi.ERR_INVALID and "non-NULL" in capi.last_error()
    assert call(batch=-1) == capi.ERR_INVALID
    assert call(batch=0) == capi.OK
    assert call(batch=0, wc=capi.default_world_config(), circles=None) == capi.OK
    assert call(wc=capi.default_world_config(num_circles=1), circles=None) == capi.ERR_INVALID


def test_cast_scans_body_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    sc_ok, wc_ok = scan(capi), capi.default_world_config(num_circles=5)
    race_ok, body_ok = capi.default_race_config(group_size=2), capi.default_body_config()

    def call(sc=sc_ok, wc=wc_ok, race=race_ok, body=body_ok, batch=4, list_=None, count=None, x=p, circles=p, ranges=p):
        return L.f110qp_cast_scans_body_dev(ref(sc), ref(wc), ref(race), ref(body), batch, list_, count, x, circles,
                                            ranges, None)

    world_rules(capi, call, 4)
    race_rules(capi, call, 4)
    body_rules(capi, call)
    assert call(sc=None) == capi.ERR_INVALID and call(sc=scan(capi, num_ranges=0)) == capi.ERR_INVALID
    assert call(list_=p) == capi.ERR_INVALID and "together" in capi.last_error()
    assert call(count=p) == capi.ERR_INVALID and "together" in capi.last_error()
    assert call(x=None) == capi.ERR_INVALID and call(ranges=None) == capi.ERR_INVALID
    assert call(batch=-1) == capi.ERR_INVALID
    assert call(batch=0) == capi.OK


@pytest.mark.parametrize("name", ["f110qp_rollout_body_dev", "f110qp_rollout_body"])
def test_rollout_body_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok, rp_ok = capi.default_rollout_config(ticks=3), capi.default_replan_config(num_waypoints=4)
    sc_ok, wc_ok = scan(capi, scan_rows=7), capi.default_world_config(num_circles=5)
    race_ok, cc_ok, body_ok = capi.default_race_config(group_size=2), capi.default_contact_config(), capi.default_body_config()

    def call(rc=ok, sc=sc_ok, rp=rp_ok, wc=wc_ok, race=race_ok, cc=cc_ok, body=body_ok, batch=4, patch=None, ctx=s._h,
             circles=p):
        # the array order of f110qp_rollout_contact[_dev]: 20 clear_traj, 21 nearest_traj, 22 crash_tick
        a = [p] * 4 + [circles] + [p] * 4 + [None] * 11 + [p, None, p] + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(ctx, ref(rc), ref(sc), ref(rp), ref(wc), ref(race), ref(cc), ref(body), batch, *a)

    world_rules(capi, call, 4)
    race_rules(capi, call, 4)
    body_rules(capi, call)
    assert call(cc=None) == capi.ERR_INVALID and "contact config" in capi.last_error()
    assert call(cc=capi.default_contact_config(stop_on_contact=2)) == capi.ERR_INVALID
    for v in NOT_FINITE:
        assert call(cc=capi.default_contact_config(margin=v)) == capi.ERR_INVALID and "margin" in capi.last_error()
    for k in (20, 22):
        assert call(patch={k: None}) == capi.ERR_INVALID and "clear_traj/crash_tick" in capi.last_error()
    s1 = capi.Solver(capi.default_config(1, x_ref_points=50))
    assert call(ctx=s1._h) == capi.ERR_INVALID and "horizon" in capi.last_error()
    s1.close()
    assert call(rc=capi.default_rollout_config(ticks=0)) == capi.ERR_INVALID and "ticks" in capi.last_error()
    assert call(rc=None) == capi.ERR_INVALID and call(sc=None) == capi.ERR_INVALID and call(rp=None) == capi.ERR_INVALID
    assert call(ctx=None) == capi.ERR_INVALID and call(batch=-1) == capi.ERR_INVALID
    for k in (0, 1, 2, 3, 5, 6, 7, 8):
        assert call(patch={k: None}) == capi.ERR_INVALID, k
        assert "non-NULL" in capi.last_error()
    if dev:
        off = C.c_void_p(buf.ctypes.data + 4)
        assert call(patch={7: off}) == capi.ERR_INVALID and "aligned" in capi.last_error()  # u_applied
    assert call(batch=0) == capi.OK
    s.close()


def test_binding_checks(capi):
    torch = pytest.importorskip("torch")
    t64 = torch.zeros(256, dtype=torch.float64)
    w, race = capi.default_world_config(num_circles=5), capi.default_race_config(group_size=2)
    x = t64[:12].view(2, 2, 3)
    with pytest.raises(capi.F110QPError, match="body must be a BodyConfig"):
        capi.clearance_body_dev(w, race, race, x, t64, t64)
    with pytest.raises(capi.F110QPError, match="clearance holds"):
        capi.clearance_body_dev(w, race, capi.default_body_config(), x, t64, t64[:3])
    with pytest.raises(capi.F110QPError, match="body must be a BodyConfig"):
        capi.cast_scans_body_dev(scan(capi), w, race, None, x[0], t64, t64)
