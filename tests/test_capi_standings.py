"""The standings entry points of the C ABI (f110qp_path_lengths, f110qp_progress_dev, f110qp_standings_dev,
f110qp_race_standings) without a GPU: exported symbols, every argument rule (each answers before the first
device call: on a machine without a device anything later would be F110QP_ERR_HIP), f110qp_path_lengths against
the oracle, and the bindings' own checks."""
import ctypes as C
import os

import numpy as np
import pytest
import standings_cases as sc_
from test_capi_world import NOT_FINITE, ref

from f110qp import workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDINGS = ("f110qp_path_lengths", "f110qp_progress_dev", "f110qp_standings_dev", "f110qp_race_standings")


def test_symbols_and_version(capi):
    hdr = open(os.path.join(ROOT, "include", "f110qp.h")).read()
    for name in STANDINGS:
        assert name + "(" in hdr and name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6 and "#define F110QP_API_VERSION 6" in hdr  # additive


def invalid(capi, rc, word):
    assert rc == capi.ERR_INVALID, rc
    assert word in capi.last_error(), capi.last_error()


def race_rules(capi, call, B):
    """test_capi_race.race_rules for calls that refuse an empty batch."""
    invalid(capi, call(race=None), "race config")
    for G in (0, -1, -B):
        invalid(capi, call(race=capi.default_race_config(group_size=G)), "group_size")
    for G in (B - 1, B + 1, 2 * B):
        invalid(capi, call(race=capi.default_race_config(group_size=G)), "multiple of group_size")
    for v in NOT_FINITE + [0.0, -0.3]:
        invalid(capi, call(race=capi.default_race_config(group_size=2, car_radius=v)), "car_radius")
    for v in NOT_FINITE:
        invalid(capi, call(race=capi.default_race_config(group_size=2, center_offset=v)), "center_offset")


def shape_rules(capi, call):
    for v in (0, -1):
        invalid(capi, call(batch=v), "batch")
        invalid(capi, call(rows=v), "rows")
    invalid(capi, call(batch=1 << 16, rows=1 << 15), "too large")


@pytest.fixture
def host():
    buf = np.zeros(4096, np.float64)
    return buf, C.c_void_p(buf.ctypes.data)


def test_path_lengths_rules_and_bits(capi):
    L = capi.load()
    wp = np.ascontiguousarray(workload.track_waypoints())
    cum = np.zeros(501)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    invalid(capi, L.f110qp_path_lengths(None, 500, p(cum)), "non-NULL")
    invalid(capi, L.f110qp_path_lengths(p(wp), 500, None), "non-NULL")
    for W in (1, 0, -3):
        invalid(capi, L.f110qp_path_lengths(p(wp), W, p(cum)), "num_waypoints")
    dup = sc_.duplicate_case().wp
    bad = sc_.bad_waypoint_cases()[0].wp
    for w in (wp, sc_.ellipse(2), sc_.ellipse(3), sc_.rectangle(), dup, bad, wp * 1e160):
        for lib in (False, True):
            got = np.full(len(w) + 2, -7.0)
            assert capi.load(test=lib).f110qp_path_lengths(p(np.ascontiguousarray(w)), len(w), p(got)) == capi.OK
            assert sc_.same(got[:-1], workload.path_lengths(w)) and got[-1] == -7.0
        assert sc_.same(capi.path_lengths(w), workload.path_lengths(w))
    assert capi.path_lengths(dup)[11] == capi.path_lengths(dup)[10], "a duplicated waypoint adds nothing"
    assert capi.path_lengths(sc_.ellipse(2))[2] == 2 * capi.path_lengths(sc_.ellipse(2))[1]
    with pytest.raises(capi.F110QPError, match="float64"):
        capi.path_lengths(wp.astype(np.float32))
    with pytest.raises(capi.F110QPError, match="at least 2"):
        capi.path_lengths(wp[:1])


def test_progress_validation_errors_touch_no_device(capi, host):
    _, p = host

    def call(batch=4, rows=3, x=p, wp=p, cum=p, W=5, seg=None, s=p, lateral=None):
        return capi.load().f110qp_progress_dev(batch, rows, x, wp, cum, W, seg, s, lateral, None)

    shape_rules(capi, call)
    for W in (1, 0, -1):
        invalid(capi, call(W=W), "num_waypoints")
    for k in ("x", "wp", "cum", "s"):
        invalid(capi, call(**{k: None}), "non-NULL")


def test_standings_validation_errors_touch_no_device(capi, host):
    _, p = host
    race_ok = capi.default_race_config(group_size=2)

    def call(race=race_ok, batch=4, rows=3, s=p, L=70.0, dist=p, lap=None, rank=p):
        return capi.load().f110qp_standings_dev(ref(race), batch, rows, s, L, dist, lap, rank, None)

    shape_rules(capi, call)
    race_rules(capi, call, 4)
    for v in NOT_FINITE + [0.0, -1.0]:
        invalid(capi, call(L=v), "path_length")
    for k in ("s", "dist", "rank"):
        invalid(capi, call(**{k: None}), "non-NULL")


def test_race_standings_validation_errors_touch_no_device(capi, host):
    buf, p = host
    race_ok = capi.default_race_config(group_size=2)
    wp_ok = np.ascontiguousarray(sc_.ellipse(5))

    def call(race=race_ok, batch=4, rows=3, x=p, wp=C.c_void_p(wp_ok.ctypes.data), W=5, seg=None, s=p, lateral=None,
             dist=p, lap=None, rank=p):
        return capi.load().f110qp_race_standings(ref(race), batch, rows, x, wp, W, seg, s, lateral, dist, lap, rank)

    shape_rules(capi, call)
    race_rules(capi, call, 4)
    for W in (1, 0, -1):
        invalid(capi, call(W=W), "num_waypoints")
    for k in ("x", "wp", "s", "dist", "rank"):
        invalid(capi, call(**{k: None}), "non-NULL")
    # the path's length, computed by the call: all waypoints in one place (0), or a non-finite one (NaN)
    invalid(capi, call(wp=p), "path_length")
    bad = np.ascontiguousarray(sc_.bad_waypoint_cases()[0].wp)
    invalid(capi, call(wp=C.c_void_p(bad.ctypes.data), W=len(bad)), "path_length")
    assert not buf.any(), "nothing was written"


def test_binding_checks_types_and_shapes(capi):
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.float64)
    i32 = torch.zeros(64, dtype=torch.int32)
    x, wp, race = t64[:24].view(2, 4, 3), t64[:10].view(5, 2), capi.default_race_config(group_size=2)
    with pytest.raises(capi.F110QPError, match=r"x must be \[rows, B, 3\]"):
        capi.progress_dev(t64[:24].view(6, 4), wp, t64, t64)
    with pytest.raises(capi.F110QPError, match="x must be torch.float64"):
        capi.progress_dev(t32[:24].view(2, 4, 3), wp, t64, t64)
    with pytest.raises(capi.F110QPError, match="waypoints must be"):
        capi.progress_dev(x, t64[:2].view(1, 2), t64, t64)
    with pytest.raises(capi.F110QPError, match="cum holds"):
        capi.progress_dev(x, wp, t64[:5], t64)
    with pytest.raises(capi.F110QPError, match="s holds"):
        capi.progress_dev(x, wp, t64, t64[:7])
    with pytest.raises(capi.F110QPError, match="seg must be torch.int32"):
        capi.progress_dev(x, wp, t64, t64, seg=t64)
    with pytest.raises(capi.F110QPError, match="lateral holds"):
        capi.progress_dev(x, wp, t64, t64, lateral=t64[:7])
    s = t64[:8].view(2, 4)
    with pytest.raises(capi.F110QPError, match="group_size must be >= 1 and divide B = 4"):
        capi.standings_dev(capi.default_race_config(group_size=3), s, 70.0, t64, i32)
    with pytest.raises(capi.F110QPError, match="rank must be torch.int32"):
        capi.standings_dev(race, s, 70.0, t64, t64)
    with pytest.raises(capi.F110QPError, match="dist holds"):
        capi.standings_dev(race, s, 70.0, t64[:7], i32)
    with pytest.raises(capi.F110QPError, match="lap holds"):
        capi.standings_dev(race, s, 70.0, t64, i32, lap=i32[:7])
    with pytest.raises(capi.F110QPError, match="group_size must be >= 1 and divide B = 4"):
        capi.race_standings(capi.default_race_config(group_size=3), np.zeros((2, 4, 3)), sc_.ellipse(5))
    with pytest.raises(capi.F110QPError, match=r"x must be \[rows, B, 3\]"):
        capi.race_standings(race, np.zeros((2, 4)), sc_.ellipse(5))
