"""The refreshed-scan entry points of the C ABI (f110qp_default_refresh_config, f110qp_gap_refresh_dev,
f110qp_rollout_refresh[_dev]) without a GPU: exported symbols, the default, the struct layout against the header,
and every argument rule, each of which answers before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from test_capi_walls import wall_rules
from test_capi_world import ref, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFRESH = ("f110qp_default_refresh_config", "f110qp_gap_refresh_dev", "f110qp_rollout_refresh_dev",
           "f110qp_rollout_refresh")


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in REFRESH:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive


def test_default_and_layout(capi):
    rf = capi.RefreshConfig(every=9)
    capi.load().f110qp_default_refresh_config(C.byref(rf))
    assert rf.every == 0, "the default zeroes the struct"
    assert capi.default_refresh_config().every == 0 and capi.default_refresh_config(every=5).every == 5
    capi.load().f110qp_default_refresh_config(None)  # a NULL config is ignored
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} f110qp_refresh_config;", hdr).group(1)
    fields = re.findall(r"^\s*(int|double|float)\s+(\w+);", body, re.M)
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(capi.RefreshConfig._fields_)
    assert C.sizeof(capi.RefreshConfig) == 4


def test_gap_refresh_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok = scan(capi)

    def call(sc=ok, batch=4, ranges=p, states=p, gap=p, hs=p):
        return L.f110qp_gap_refresh_dev(ref(sc), batch, ranges, states, gap, hs, None)

    assert call(sc=None) == capi.ERR_INVALID and "scan config" in capi.last_error()
    for k in ("ranges", "states", "gap", "hs"):
        assert call(**{k: None}) == capi.ERR_INVALID, k
        assert "non-NULL" in capi.last_error()
    for batch in (0, -1):
        assert call(batch=batch) == capi.ERR_INVALID, batch
        assert "batch" in capi.last_error()
    # every sc rule of f110qp_gap_search_dev
    for nr in (0, -1, 65536):
        assert call(sc=scan(capi, num_ranges=nr)) == capi.ERR_INVALID, nr
        assert L.f110qp_gap_search_dev(ref(scan(capi, num_ranges=nr)), 4, p, p, None) == capi.ERR_INVALID
        assert "num_ranges" in capi.last_error()
    for inc in (0.0, -0.1, float("nan")):
        assert call(sc=scan(capi, angle_increment=inc)) == capi.ERR_INVALID, inc
        assert "angle_increment" in capi.last_error()
    # scan_rows is not read
    assert call(sc=scan(capi, scan_rows=7), batch=0) == capi.ERR_INVALID and "batch" in capi.last_error()


@pytest.mark.parametrize("name", ["f110qp_rollout_refresh_dev", "f110qp_rollout_refresh"])
def test_rollout_refresh_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    rc, rp = capi.default_rollout_config(ticks=3), capi.default_replan_config(num_waypoints=4)
    sc, wc = scan(capi), capi.default_world_config(num_circles=5)
    race, cc, body = capi.default_race_config(group_size=2), capi.default_contact_config(), capi.default_body_config()
    ok, every = capi.default_walls_config(num_segments=3), capi.default_refresh_config(every=1)

    def call(walls=ok, segments=p, batch=4, body=body, cc=cc, rf=every, patch=None):
        # 0 table, 1 waypoints, 2 x_ref, 3 have_path, 4 circles, 5 segments, 6 x_traj, 7 u_lin_traj, 8 u_applied,
        # 9 status_traj, then the optional iters .. ranges_traj (11), clear_traj, nearest_traj, crash_tick[, stream]
        a = [p] * 5 + [segments] + [p] * 4 + [None] * 11 + [p, None, p] + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(s._h, ref(rc), ref(sc), ref(rp), ref(wc), ref(race), ref(cc), ref(body), ref(walls), ref(rf), batch,
                  *a)

    assert call(rf=None) == capi.ERR_INVALID and "refresh config" in capi.last_error()
    for k in (-1, -(2 ** 31)):
        assert call(rf=capi.default_refresh_config(every=k)) == capi.ERR_INVALID, k
        assert "every" in capi.last_error()
    # rf is checked where no row is computed and where the batch is empty
    assert call(rf=None, batch=0) == capi.ERR_INVALID and "refresh config" in capi.last_error()
    # every check of the walls call
    wall_rules(capi, call, 4)
    assert call(body=None) == capi.ERR_INVALID and "body config" in capi.last_error()
    assert call(cc=None) == capi.ERR_INVALID and "contact config" in capi.last_error()
    assert call(patch={21: None}) == capi.ERR_INVALID and "clear_traj" in capi.last_error()
    assert call(patch={23: None}) == capi.ERR_INVALID and "crash_tick" in capi.last_error()
    assert call(patch={6: None}) == capi.ERR_INVALID and "x_traj" in capi.last_error()
    for k in (0, 1, 2 ** 31 - 1):
        assert call(batch=0, rf=capi.default_refresh_config(every=k)) == capi.OK, k
    s.close()


def test_binding_checks(capi):
    s = capi.Solver(capi.default_config(20, x_ref_points=50))
    cfg = (capi.default_race_config(), capi.default_contact_config(), capi.default_body_config())
    with pytest.raises(capi.F110QPError, match="RefreshConfig"):
        s.rollout_refresh(None, None, None, None, *cfg, capi.default_walls_config(), None, None, None, None, 1)
    with pytest.raises(capi.F110QPError, match="RefreshConfig"):
        s.rollout_refresh_dev(None, None, None, None, *cfg, capi.default_walls_config(), 3, *[None] * 12)
    s.close()
