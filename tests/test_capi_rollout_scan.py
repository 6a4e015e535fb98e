"""The scan-rollout entry points of the C ABI (f110qp_find_half_spaces_dev_dbl, f110qp_gap_search_dev,
f110qp_half_space_rows_dev, f110qp_advance_scan_dev, f110qp_rollout_scan[_dev]) without a GPU: exported
symbols, the default scan config and the argument checks, every one of which answers before the first
device call."""
import ctypes as C

import numpy as np
import pytest

SCAN = ("f110qp_find_half_spaces_dev_dbl", "f110qp_default_scan_config", "f110qp_gap_search_dev",
        "f110qp_half_space_rows_dev", "f110qp_advance_scan_dev", "f110qp_rollout_scan_dev", "f110qp_rollout_scan")


def scan(capi, **over):
    kw = dict(num_ranges=64, angle_min=-2.0, angle_increment=0.0625, angle_max=2.0)
    kw.update(over)
    return capi.default_scan_config(**kw)


def test_symbols_exported_by_both_libraries(capi):
    for name in SCAN:
        assert name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6  # additive: the ABI version stays


def test_default_scan_config(capi):
    sc = capi.default_scan_config()
    assert (sc.ftg_thresh, sc.divider, sc.buffer, sc.scan_rows) == (3.0, 1.5, 3.0, 1)
    assert (sc.num_ranges, sc.angle_min, sc.angle_increment, sc.angle_max) == (0, 0.0, 0.0, 0.0)
    sc = capi.default_scan_config(num_ranges=1080, scan_rows=4, buffer=2.0)
    assert (sc.num_ranges, sc.scan_rows, sc.buffer, sc.divider) == (1080, 4, 2.0, 1.5)
    capi.load().f110qp_default_scan_config(None)  # a NULL config is ignored
    assert C.sizeof(capi.ScanConfig) == 32 and capi.GAP_RECORD_DTYPE.itemsize == 16


BAD_SCANS = [(dict(num_ranges=0), "num_ranges"), (dict(num_ranges=65536), "num_ranges"),
             (dict(angle_increment=0.0), "angle_increment"), (dict(angle_increment=-0.1), "angle_increment"),
             (dict(angle_increment=float("nan")), "angle_increment")]


@pytest.mark.parametrize("name", ["f110qp_rollout_scan_dev", "f110qp_rollout_scan"])
def test_rollout_scan_validation_errors_touch_no_device(capi, name):
    fn = getattr(capi.load(), name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok, sc_ok = capi.default_rollout_config(ticks=3), scan(capi)

    def call(rc=ok, sc=sc_ok, batch=4, patch=None, ctx=s._h):
        # x_ref, ranges, x_traj, u_lin_traj, u_applied, status_traj, iters, cost, u_plan, x_plan, hs_traj[, stream]
        a = [p, p, p, p, p, p, None, None, None, None, None] + ([None] if dev else [])
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(ctx, C.byref(rc) if rc is not None else None, C.byref(sc) if sc is not None else None, batch, *a)

    assert call(rc=capi.default_rollout_config(ticks=0)) == capi.ERR_INVALID
    assert "ticks" in capi.last_error()
    assert call(rc=capi.default_rollout_config(ticks=3, plant_dt=-1.0)) == capi.ERR_INVALID
    assert "plant_dt" in capi.last_error()
    assert call(rc=None) == capi.ERR_INVALID and call(sc=None) == capi.ERR_INVALID
    assert "scan config" in capi.last_error()
    assert call(ctx=None) == capi.ERR_INVALID and call(batch=-1) == capi.ERR_INVALID
    for rows in (0, 2, 4, -1):  # ticks = 3: only 1 and 3 are rows
        assert call(sc=scan(capi, scan_rows=rows)) == capi.ERR_INVALID
        assert "scan_rows" in capi.last_error()
    for over, word in BAD_SCANS:
        assert call(sc=scan(capi, **over)) == capi.ERR_INVALID
        assert word in capi.last_error()
    for k in (0, 2, 3, 4, 5):  # x_ref, x_traj, u_lin_traj, u_applied, status_traj
        assert call(patch={k: None}) == capi.ERR_INVALID
        assert "non-NULL" in capi.last_error()
    for ctx in (s, capi.Solver(capi.default_config(20, gap_mode=capi.GAP_ACTIVE))):  # either gap mode
        assert call(patch={1: None}, ctx=ctx._h) == capi.ERR_INVALID
        assert "ranges" in capi.last_error()
    if dev:  # (the host-pointer call stages into buffers of its own: any host alignment will do)
        off = C.c_void_p(buf.ctypes.data + 4)
        assert call(patch={8: off}) == capi.ERR_INVALID  # u_plan
        assert "aligned" in capi.last_error()
        assert call(patch={4: off}) == capi.ERR_INVALID  # u_applied
        assert "aligned" in capi.last_error()
    assert call(batch=0) == capi.OK  # batch 0: a no-op
    assert call(batch=0, sc=scan(capi, scan_rows=3)) == capi.OK
    s.close()


def test_advance_scan_validation_errors_touch_no_device(capi):
    fn = capi.load().f110qp_advance_scan_dev
    buf = np.zeros(4096, np.float64)
    p, q = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2048)
    ok, sc_ok = capi.default_rollout_config(ticks=0), scan(capi, scan_rows=7)  # neither is read here

    def call(rc=ok, sc=sc_ok, batch=4, horizon=20, patch=None):
        a = [p, p, p, p, q, q, None, q, None]  # x, u_plan, status, gap, x_next, u_lin_next, u_applied, hs_next, stream
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(C.byref(rc) if rc is not None else None, C.byref(sc) if sc is not None else None, batch, horizon, *a)

    assert call(rc=None) == capi.ERR_INVALID and call(sc=None) == capi.ERR_INVALID
    assert call(rc=capi.default_rollout_config(car_length=0.0)) == capi.ERR_INVALID
    for over, word in BAD_SCANS:
        assert call(sc=scan(capi, **over)) == capi.ERR_INVALID
        assert word in capi.last_error()
    assert call(batch=-1) == capi.ERR_INVALID
    assert call(horizon=0) == capi.ERR_INVALID and call(horizon=49) == capi.ERR_INVALID
    for k in (0, 1, 2, 4, 5):
        assert call(patch={k: None}) == capi.ERR_INVALID
    for k in (3, 7):  # gap, hs_next
        assert call(patch={k: None}) == capi.ERR_INVALID
        assert "gap/hs_next" in capi.last_error()
    assert call(patch={4: p}) == capi.ERR_INVALID  # x_next aliases x
    assert "alias" in capi.last_error()
    assert call(patch={1: C.c_void_p(buf.ctypes.data + 4)}) == capi.ERR_INVALID
    assert "aligned" in capi.last_error()
    assert call(batch=0) == capi.OK


def test_search_rows_and_dbl_validation_errors_touch_no_device(capi):
    L = capi.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok = scan(capi)
    for over, word in BAD_SCANS:
        bad = scan(capi, **over)
        assert L.f110qp_gap_search_dev(C.byref(bad), 4, p, p, None) == capi.ERR_INVALID
        assert word in capi.last_error()
        assert L.f110qp_half_space_rows_dev(C.byref(bad), 4, p, p, p, None) == capi.ERR_INVALID
        assert word in capi.last_error()
    assert L.f110qp_gap_search_dev(None, 4, p, p, None) == capi.ERR_INVALID
    assert L.f110qp_gap_search_dev(C.byref(ok), -1, p, p, None) == capi.ERR_INVALID
    assert L.f110qp_gap_search_dev(C.byref(ok), 4, None, p, None) == capi.ERR_INVALID
    assert L.f110qp_gap_search_dev(C.byref(ok), 4, p, None, None) == capi.ERR_INVALID
    assert "gap_out" in capi.last_error()
    assert L.f110qp_gap_search_dev(C.byref(ok), 0, None, None, None) == capi.OK
    assert L.f110qp_half_space_rows_dev(None, 4, p, p, p, None) == capi.ERR_INVALID
    assert L.f110qp_half_space_rows_dev(C.byref(ok), -1, p, p, p, None) == capi.ERR_INVALID
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert L.f110qp_half_space_rows_dev(C.byref(ok), 4, *a, None) == capi.ERR_INVALID
    assert L.f110qp_half_space_rows_dev(C.byref(ok), 0, None, None, None, None) == capi.OK
    dbl = L.f110qp_find_half_spaces_dev_dbl
    g = (-2.0, 0.0625, 2.0, 3.0, 1.5, 3.0)
    assert dbl(4, p, p, 0, *g, p, None, None, None) == capi.ERR_INVALID
    assert dbl(4, p, p, 65536, *g, p, None, None, None) == capi.ERR_INVALID
    assert dbl(-1, p, p, 64, *g, p, None, None, None) == capi.ERR_INVALID
    assert dbl(4, p, p, 64, -2.0, 0.0, 2.0, 3.0, 1.5, 3.0, p, None, None, None) == capi.ERR_INVALID
    assert "angle_increment" in capi.last_error()
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert dbl(4, a[0], a[1], 64, *g, a[2], None, None, None) == capi.ERR_INVALID
    assert dbl(0, None, None, 64, *g, None, None, None, None) == capi.OK


def test_binding_checks_types_and_shapes(capi):
    s = capi.Solver(capi.default_config(4))
    x0, ul, xr = np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((2, 4, 3))
    sc = scan(capi, num_ranges=8)
    with pytest.raises(capi.F110QPError, match="x0 must be a float64"):
        s.rollout_scan(x0.astype(np.float32), ul, xr, np.zeros((2, 8)), sc, 2)
    with pytest.raises(capi.F110QPError, match="ticks must be >= 1"):
        s.rollout_scan(x0, ul, xr, np.zeros((2, 8)), sc, 0)
    with pytest.raises(capi.F110QPError, match="ranges must hold"):
        s.rollout_scan(x0, ul, xr, np.zeros((2, 7)), sc, 2)
    with pytest.raises(capi.F110QPError, match="scan_rows must be 1 or ticks"):
        s.rollout_scan(x0, ul, xr, np.zeros((3, 2, 8)), scan(capi, num_ranges=8, scan_rows=3), 2)
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.float64)
    i32 = torch.zeros(16, dtype=torch.int32)
    rc = capi.default_rollout_config(ticks=2)
    xr64, xt, rg = t64[:24].view(2, 4, 3), t64[:18].view(3, 2, 3), t32[:16].view(1, 2, 8)
    with pytest.raises(capi.F110QPError, match="x_traj must be \\[ticks"):
        s.rollout_scan_dev(rc, sc, xr64, rg, t64[:12].view(2, 2, 3), t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="ranges must be \\[scan_rows"):
        s.rollout_scan_dev(rc, sc, xr64, t32[:16].view(2, 8), xt, t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="ranges must be torch.float32"):
        s.rollout_scan_dev(rc, sc, xr64, t64[:16].view(1, 2, 8), xt, t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="hs_traj holds"):
        s.rollout_scan_dev(rc, sc, xr64, rg, xt, t64, t32, i32, hs_traj=t32[:23])
    with pytest.raises(capi.F110QPError, match="gap must be torch.int32"):
        capi.advance_scan_dev(rc, sc, 4, t64[:6].view(2, 3), t32, i32, t32, t64, t64, t32)
    with pytest.raises(capi.F110QPError, match="states must be torch.float64"):
        capi.find_half_spaces_dev_dbl(t32[:6].view(2, 3), t32[:16].view(2, 8), -2.0, 0.5, 2.0, t32)
    with pytest.raises(capi.F110QPError, match="gap_out holds"):
        capi.gap_search_dev(sc, t32[:16].view(2, 8), i32[:7])
    with pytest.raises(capi.F110QPError, match="states must be torch.float64"):
        capi.half_space_rows_dev(sc, i32, t32[:6].view(2, 3), t32)
    s.close()


def test_product_library_reads_no_environment_knob(capi):
    """The product library still holds no F110QP_ string (its behaviour is the config alone)."""
    with open(capi.LIB_PATH, "rb") as f:
        assert b"F110QP_" not in f.read()
