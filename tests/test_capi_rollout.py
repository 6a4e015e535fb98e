"""The closed-loop entry points of the C ABI (f110qp_advance_dev, f110qp_rollout_dev, f110qp_rollout)
without a GPU: exported symbols, the default rollout config and the argument checks, every one of
which answers before the first device call."""
import ctypes as C
import math

import numpy as np
import pytest

ROLLOUT = ("f110qp_advance_dev", "f110qp_rollout_dev", "f110qp_rollout")


def test_symbols_exported_by_both_libraries(capi):
    for name in ROLLOUT + ("f110qp_default_rollout_config",):
        assert name in capi.EXPORTED
        assert getattr(capi.load(), name) is not None
        assert getattr(capi.load(test=True), name) is not None
    assert capi.load().f110qp_version() == 6  # additive: the ABI version stays


def test_default_rollout_config(capi):
    rc = capi.default_rollout_config()
    assert (rc.plant_dt, rc.car_length, rc.v_lin, tuple(rc.fail_u)) == (0.01, 0.35, 4.5, (0.5, 0.0))
    assert rc.ticks == 1
    rc = capi.default_rollout_config(ticks=7, plant_dt=0.02, fail_u=(1.0, 0.1))
    assert (rc.ticks, rc.plant_dt, tuple(rc.fail_u), rc.car_length) == (7, 0.02, (1.0, 0.1), 0.35)
    capi.load().f110qp_default_rollout_config(None)  # a NULL config is ignored


def _rollout_args(p, dev):
    # x_ref, halfspace, x_traj, u_lin_traj, u_applied, status_traj, iters, cost, u_plan, x_plan[, stream]
    return [p, None, p, p, p, p, None, None, None, None] + ([None] if dev else [])


@pytest.mark.parametrize("name", ["f110qp_rollout_dev", "f110qp_rollout"])
def test_rollout_validation_errors_touch_no_device(capi, name):
    L = capi.load()
    fn = getattr(L, name)
    dev = name.endswith("_dev")
    s = capi.Solver(capi.default_config(20))
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    ok = capi.default_rollout_config(ticks=2)

    def call(rc, batch=4, patch=None, ctx=s._h):
        a = _rollout_args(p, dev)
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(ctx, C.byref(rc) if rc is not None else None, batch, *a)

    for rc, word in ((capi.default_rollout_config(ticks=0), "ticks"),
                     (capi.default_rollout_config(ticks=2, plant_dt=math.nan), "plant_dt"),
                     (capi.default_rollout_config(ticks=2, plant_dt=math.inf), "plant_dt"),
                     (capi.default_rollout_config(ticks=2, plant_dt=-0.01), "plant_dt"),
                     (capi.default_rollout_config(ticks=2, car_length=0.0), "car_length"),
                     (capi.default_rollout_config(ticks=2, car_length=math.nan), "car_length"),
                     (capi.default_rollout_config(ticks=2, v_lin=math.nan), "v_lin"),
                     (capi.default_rollout_config(ticks=2, fail_u=(math.inf, 0.0)), "fail_u")):
        assert call(rc) == capi.ERR_INVALID
        assert word in capi.last_error()
    assert call(None) == capi.ERR_INVALID
    assert call(ok, ctx=None) == capi.ERR_INVALID
    assert call(ok, batch=-1) == capi.ERR_INVALID
    for k in (0, 2, 3, 4, 5):  # x_ref, x_traj, u_lin_traj, u_applied, status_traj
        assert call(ok, patch={k: None}) == capi.ERR_INVALID
        assert "non-NULL" in capi.last_error()
    assert call(ok, batch=0) == capi.OK  # batch 0: a no-op
    g = capi.Solver(capi.default_config(20, gap_mode=capi.GAP_ACTIVE))
    assert call(ok, ctx=g._h) == capi.ERR_INVALID  # gap rows without half-spaces
    assert "halfspace" in capi.last_error()
    g.close()
    s.close()


def test_advance_validation_errors_touch_no_device(capi):
    fn = capi.load().f110qp_advance_dev
    buf = np.zeros(4096, np.float64)
    p, q = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2048)
    ok = capi.default_rollout_config(ticks=0)  # ticks is not read here

    def call(rc, batch=4, horizon=20, patch=None):
        a = [p, p, p, q, q, None, None]  # x, u_plan, status, x_next, u_lin_next, u_applied, stream
        for k, v in (patch or {}).items():
            a[k] = v
        return fn(C.byref(rc) if rc is not None else None, batch, horizon, *a)

    assert call(None) == capi.ERR_INVALID
    assert call(capi.default_rollout_config(plant_dt=math.nan)) == capi.ERR_INVALID
    assert call(capi.default_rollout_config(car_length=0.0)) == capi.ERR_INVALID
    assert call(ok, batch=-1) == capi.ERR_INVALID
    assert call(ok, horizon=0) == capi.ERR_INVALID
    assert call(ok, horizon=49) == capi.ERR_INVALID
    for k in range(5):
        assert call(ok, patch={k: None}) == capi.ERR_INVALID
    assert call(ok, patch={3: p}) == capi.ERR_INVALID  # x_next aliases x
    assert "alias" in capi.last_error()
    assert call(ok, patch={1: C.c_void_p(buf.ctypes.data + 4)}) == capi.ERR_INVALID
    assert "aligned" in capi.last_error()
    assert call(ok, batch=0) == capi.OK


def test_binding_checks_types_and_shapes(capi):
    s = capi.Solver(capi.default_config(4))
    x0, ul, xr = np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((2, 4, 3))
    with pytest.raises(capi.F110QPError, match="x0 must be a float64"):
        s.rollout(x0.astype(np.float32), ul, xr, 2)
    with pytest.raises(capi.F110QPError, match="ticks must be >= 1"):
        s.rollout(x0, ul, xr, 0)
    torch = pytest.importorskip("torch")
    t32, t64 = torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.float64)
    i32 = torch.zeros(16, dtype=torch.int32)
    rc = capi.default_rollout_config(ticks=2)
    xr64, xt = t64[:24].view(2, 4, 3), t64[:18].view(3, 2, 3)
    with pytest.raises(capi.F110QPError, match="x_traj must be \\[ticks"):
        s.rollout_dev(rc, xr64, None, t64[:12].view(2, 2, 3), t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="x_ref must be torch.float64"):
        s.rollout_dev(rc, t32[:24].view(2, 4, 3), None, xt, t64, t32, i32)
    with pytest.raises(capi.F110QPError, match="u_applied must be torch.float32"):
        s.rollout_dev(rc, xr64, None, xt, t64, t64, i32)
    with pytest.raises(capi.F110QPError, match="status_traj holds"):
        s.rollout_dev(rc, xr64, None, xt, t64, t32, i32[:3])
    with pytest.raises(capi.F110QPError, match="x_next must be torch.float64"):
        capi.advance_dev(rc, 4, t64[:6].view(2, 3), t32, i32, t32, t64)
    s.close()
