"""The device-resident closed loop (f110qp_advance_dev, f110qp_rollout_dev, f110qp_rollout) on MI355X.

Every check is per tick, on the inputs the device itself recorded (x_traj[t], u_lin_traj[t]), so no
closed-loop drift enters a tolerance:
  solve    oracle.solve on the recorded doubles: equal status, and
           |u_plan[t,b] - u*|_inf / max(1, |u*|_inf) <= 2e-6 (U_TOL of test_gpu_dbl.py);
  inputs   u_applied[t] == u_plan[t,:,0] and u_lin_traj[t+1] == (4.5, float64(u_plan[t,:,1,1]))
           (u_plan[t,:,0,1] when N = 1) bit for bit; a car without a usable plan (status not SOLVED /
           SOLVED_INACCURATE) has a NaN plan, applies (0.5, 0) and linearises next at (4.5, 0);
  plant    x_traj[t+1] against x + dt (v cos, v sin, tan(steer) v / L) recomputed in numpy fp64 from
           x_traj[t] and the applied input, elementwise within 2 spacing(|expected|) + 2e-16. Derived,
           not measured: the increment is at most 0.06 in magnitude (4.5 x 0.01, and
           tan(0.43) x 4.5 / 0.35 x 0.01) and carries at most about 8 relative roundings (2-ulp device
           trig, the products, a possible fused multiply-add): 1.07e-16, doubled; on top the final
           add's rounding and one ulp of the result.
Start states: rollout_cases.start, a workload.make_batch batch widened to float64 with sub-float32-ulp
offsets (doubles that no float32 holds).
"""
import numpy as np
import pytest
import rollout_cases as rc_
from test_gpu_dbl import U_TOL

from f110qp import workload

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def solver(capi, N, gap=False, **cfg):
    return capi.Solver(capi.default_config(N, gap_mode=capi.GAP_ACTIVE if gap else capi.GAP_INACTIVE, **cfg))


KEYS = ("x_traj", "u_lin_traj", "u_applied", "status", "iters", "cost", "u_plan", "x_plan")


def buffers(torch, cuda, x0, ul, B, N, T, full=True):
    """Device arrays of a rollout_dev call, outputs pre-filled with a pattern no result holds."""
    e = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device=cuda)  # noqa: E731
    d = {"x_traj": e((T + 1, B, 3), torch.float64, -7.0), "u_lin_traj": e((T + 1, B, 2), torch.float64, -7.0),
         "u_applied": e((T, B, 2), torch.float32, -7.0), "status": e((T, B), torch.int32, 77)}
    d["x_traj"][0] = torch.from_numpy(x0).to(cuda)
    d["u_lin_traj"][0] = torch.from_numpy(ul).to(cuda)
    if full:
        d.update(iters=e((T, B), torch.int32, -7), cost=e((T, B), torch.float64, -7.0),
                 u_plan=e((T, B, N, 2), torch.float32, -7.0), x_plan=e((T, B, N + 1, 3), torch.float32, -7.0))
    return d


def rollout_dev(capi, cuda, s, x0, ul, xr, hs, T, full=True, stream=None, rc=None):
    """One Solver.rollout_dev call on fresh device arrays; returns the recorded arrays as numpy."""
    import torch

    B, N = x0.shape[0], s.horizon
    d = buffers(torch, cuda, x0, ul, B, N, T, full)
    xrd = torch.from_numpy(xr).to(cuda)
    hsd = None if hs is None else torch.from_numpy(np.ascontiguousarray(hs, np.float32)).to(cuda)
    cfg = rc if rc is not None else capi.default_rollout_config()
    cfg.ticks = T
    torch.cuda.synchronize(cuda)
    s.rollout_dev(cfg, xrd, hsd, d["x_traj"], d["u_lin_traj"], d["u_applied"], d["status"], d.get("iters"),
                  d.get("cost"), d.get("u_plan"), d.get("x_plan"), stream=stream)
    (stream or torch.cuda.current_stream(cuda)).synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def check_ticks(oracle, capi, out, xr, hs, N, gap=False, cars=None, what=""):
    """The per-tick checks of the module docstring on the recorded arrays of one rollout, for the
    cars in `cars` (default: all). Returns the oracle's statuses [T,B] and solutions."""
    xt, ult, ua, st, up = (out[k] for k in ("x_traj", "u_lin_traj", "u_applied", "status", "u_plan"))
    T, B = st.shape
    cars = np.arange(B) if cars is None else np.asarray(cars)
    prm = oracle.params(N)
    sts = np.zeros((T, B), np.int32)
    us, xs = np.zeros((T, B, N, 2)), np.zeros((T, B, N + 1, 3))
    worst_u = worst_x = 0.0
    for t in range(T):
        for b in cars:
            r = oracle.solve(prm, xt[t, b], ult[t, b], xr[b, :N], None if hs is None else hs[b], gap)
            sts[t, b], us[t, b], xs[t, b] = r["status"], r["u"], r["x"]
        assert (sts[t, cars] != oracle.UNCERTIFIED).all(), "the oracle has no answer for a recorded input"
        np.testing.assert_array_equal(st[t, cars], sts[t, cars], err_msg=f"{what} status, tick {t}")
        ok = np.zeros(B, bool)
        ok[cars] = sts[t, cars] == oracle.SOLVED
        bad = np.zeros(B, bool)
        bad[cars] = ~ok[cars]
        if ok.any():
            eu = np.abs(up[t, ok].astype(np.float64) - us[t, ok]).max(axis=(1, 2)) / \
                np.maximum(1.0, np.abs(us[t, ok]).max(axis=(1, 2)))
            worst_u = max(worst_u, float(eu.max()))
            assert eu.max() <= U_TOL, (what, t, float(eu.max()), int(np.argmax(eu)))
        # applied input and next linearisation input
        same_bits(ua[t, ok], up[t, ok, 0], f"{what} u_applied, tick {t}")
        nxt = up[t, :, 1 if N > 1 else 0, 1].astype(np.float64)
        want_ul = np.stack([np.full(B, rc_.V_LIN), nxt], 1)
        same_bits(ult[t + 1, ok], want_ul[ok], f"{what} u_lin_traj, tick {t + 1}")
        if bad.any():
            assert np.isnan(up[t, bad]).all(), (what, t)
            same_bits(ua[t, bad], np.tile(np.float32(rc_.FAIL_U), (int(bad.sum()), 1)), f"{what} fallback, tick {t}")
            same_bits(ult[t + 1, bad], np.tile([rc_.V_LIN, rc_.FAIL_U[1]], (int(bad.sum()), 1)),
                      f"{what} fallback u_lin, tick {t + 1}")
        # plant step
        exp = rc_.plant_step(xt[t, cars], ua[t, cars])
        err = np.abs(xt[t + 1, cars] - exp)
        bound = 2 * np.spacing(np.abs(exp)) + 2e-16
        worst_x = max(worst_x, float((err / bound).max()))
        assert (err <= bound).all(), (what, t, float((err / bound).max()))
    print(f"{what}: max u err {worst_u:.3e} (bound {U_TOL:.0e}), plant step at {worst_x:.3f} of its bound, "
          f"{int((sts[:, cars] == oracle.SOLVED).sum())} of {T * len(cars)} pairs SOLVED")
    return sts, us, xs


# ---- cases 1-7: the routes, box rows (always feasible: every pair is SOLVED) ---------------------

def _route(capi, B, backend=None, segmented=None):
    def proof(s):
        if backend is not None:
            assert s.backend_info(B)[0] == backend, s.backend_info(B)
        if segmented is not None:
            assert (s.lane_segments(B) > 1) == segmented, s.lane_segments(B)
    return proof


ROUTES = [
    ("base", 64, 20, 8, {}, lambda c: _route(c, 64, c.BACKEND_WAVE)),
    ("single car, partitioned horizon", 1, 20, 4, {}, lambda c: _route(c, 1, c.BACKEND_LANE, True)),
    ("1100 cars, ragged", 1100, 20, 3, {}, lambda c: _route(c, 1100, c.BACKEND_LANE)),
    ("1100 cars, sequential lane", 1100, 20, 3, {"F110QP_LANE_SEG": 1}, lambda c: _route(c, 1100, c.BACKEND_LANE, False)),
    ("wave N=8", 96, 8, 4, {"backend": "WAVE"}, lambda c: _route(c, 96, c.BACKEND_WAVE)),
    ("N=1", 33, 1, 3, {}, lambda c: _route(c, 33)),
    ("N=48", 40, 48, 2, {}, lambda c: _route(c, 40, c.BACKEND_LANE)),
]


@pytest.mark.parametrize("name,B,N,T,cfg,proof", ROUTES, ids=[r[0] for r in ROUTES])
def test_rollout_routes(oracle, capi, cuda, request, name, B, N, T, cfg, proof):
    """1: 64 x N=20 x 8 ticks, AUTO. 2: one car (partitioned-horizon kernel). 3: 1,100 cars, past
    F110QP_LANE_MIN_BATCH: the lane back end with a ragged last wave and a ragged plant-step
    workgroup, once as AUTO launches it (at this size still the partitioned-horizon kernel) and once
    on the sequential lane kernel (test build, F110QP_LANE_SEG = 1). 4: the wave back end at N = 8.
    5: N = 1, where u*_1 does not exist and the next steer is u*_0's. 6: the longest horizon."""
    for k in [k for k in cfg if k.startswith("F110QP_")]:
        request.getfixturevalue("knob")(k, cfg[k])  # (the other cases stay on the product library)
    cfg = {k: getattr(capi, "BACKEND_" + v) for k, v in cfg.items() if k == "backend"}
    x0, ul, xr = rc_.start(B, N, seed=100 + B % 97 + N)
    s = solver(capi, N, **cfg)
    proof(capi)(s)
    out = rollout_dev(capi, cuda, s, x0, ul, xr, None, T)
    s.close()
    sts, _, _ = check_ticks(oracle, capi, out, xr, None, N, what=name)
    assert (sts == oracle.SOLVED).all()
    same_bits(out["x_traj"][0], x0)
    same_bits(out["u_lin_traj"][0], ul)
    assert (out["iters"] > 0).all()


def test_rollout_x_ref_points_above_horizon(oracle, capi, cuda):
    """7: x_ref_points = 50 > N = 20, rows N..49 of x_ref NaN: never read."""
    B, N, T, P = 64, 20, 3, 50
    x0, ul, xr = rc_.start(B, N, seed=107, P=P)
    assert np.isnan(xr[:, N:]).all() and np.isfinite(xr[:, :N]).all()
    s = solver(capi, N, x_ref_points=P)
    out = rollout_dev(capi, cuda, s, x0, ul, xr, None, T)
    s.close()
    sts, _, _ = check_ticks(oracle, capi, out, xr, None, N, what="x_ref_points=50")
    assert (sts == oracle.SOLVED).all()


# ---- case 8: gap rows ----------------------------------------------------------------------------

def test_rollout_gap_rows(oracle, capi, cuda):
    """8: 64 x N=20 x 4 ticks, gap_mode ACTIVE, the half-spaces of a workload.make_scans scan at the
    tick-0 states (oracle, float32), held fixed. Seed rollout_cases.GAP_SEED = 2, the first seed from 1
    that passed rollout_cases.gap_seed_is_robust on the CPU and holds a non-SOLVED pair (251 SOLVED,
    5 PRIMAL_INFEASIBLE; seed 1 passed with all 256 SOLVED): in the oracle-driven loop (numpy plant, u
    rounded to float32) no (car, tick) changes oracle status when its x0 moves by +-1e-6 in any
    coordinate, none is left uncertified, and at least half of the pairs are SOLVED. Non-SOLVED pairs
    are checked too: equal status, NaN plan, fallback applied."""
    B, N, T = 64, 20, 4
    x0, ul, xr, hs = rc_.gap_case(oracle, rc_.GAP_SEED, B, N)
    s = solver(capi, N, gap=True)
    out = rollout_dev(capi, cuda, s, x0, ul, xr, hs, T)
    s.close()
    sts, _, _ = check_ticks(oracle, capi, out, xr, hs, N, gap=True, what="gap rows")
    assert (sts == oracle.SOLVED).mean() >= 0.5


# ---- case 9: the failure branch ------------------------------------------------------------------

def test_rollout_failure_branch(oracle, capi, cuda):
    """9: every fourth car's x_ref is all NaN. At every tick those cars are not SOLVED, their plan is
    NaN, they apply (0.5, 0), linearise next at (4.5, 0) and take the (0.5, 0) Euler step; the other
    cars pass the per-tick checks."""
    B, N, T = 64, 20, 3
    x0, ul, xr = rc_.start(B, N, seed=109)
    xr = xr.copy()
    dead = np.arange(B) % 4 == 0
    xr[dead] = np.nan
    s = solver(capi, N)
    out = rollout_dev(capi, cuda, s, x0, ul, xr, None, T)
    s.close()
    check_ticks(oracle, capi, out, xr, None, N, cars=np.flatnonzero(~dead), what="live cars")
    n = int(dead.sum())
    for t in range(T):
        st = out["status"][t, dead]
        assert (st != capi.SOLVED).all() and (st != capi.SOLVED_INACCURATE).all(), st
        assert np.isnan(out["u_plan"][t, dead]).all() and np.isnan(out["x_plan"][t, dead]).all()
        assert np.isnan(out["cost"][t, dead]).all()
        same_bits(out["u_applied"][t, dead], np.tile(np.float32([0.5, 0.0]), (n, 1)))
        same_bits(out["u_lin_traj"][t + 1, dead], np.tile([4.5, 0.0], (n, 1)))
        x = out["x_traj"][t, dead]
        exp = rc_.plant_step(x, np.tile([0.5, 0.0], (n, 1)))
        err = np.abs(out["x_traj"][t + 1, dead] - exp)
        assert (err <= 2 * np.spacing(np.abs(exp)) + 2e-16).all(), float(err.max())
        same_bits(out["x_traj"][t + 1, dead, 2], x[:, 2])  # tan(0) = 0: the heading stands


# ---- case 10: composition ------------------------------------------------------------------------

def test_rollout_is_solve_then_advance(capi, cuda):
    """10: rollout_dev with T = 4 equals, bit for bit in every output array, four manual rounds of
    solve_dev_dbl + advance_dev on the same stream; a second identical rollout_dev call equals the
    first."""
    import torch

    B, N, T = 64, 20, 4
    x0, ul, xr = rc_.start(B, N, seed=110)
    s = solver(capi, N)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    a = rollout_dev(capi, cuda, s, x0, ul, xr, None, T, stream=side)
    b = rollout_dev(capi, cuda, s, x0, ul, xr, None, T, stream=side)
    d = buffers(torch, cuda, x0, ul, B, N, T)
    xrd = torch.from_numpy(xr).to(cuda)
    rc = capi.default_rollout_config()
    torch.cuda.synchronize(cuda)
    for t in range(T):
        s.solve_dev_dbl(d["x_traj"][t], d["u_lin_traj"][t], xrd, None, d["u_plan"][t], d["x_plan"][t],
                        d["status"][t], d["iters"][t], stream=side, cost=d["cost"][t])
        capi.advance_dev(rc, N, d["x_traj"][t], d["u_plan"][t], d["status"][t], d["x_traj"][t + 1],
                         d["u_lin_traj"][t + 1], d["u_applied"][t], stream=side)
    side.synchronize()
    s.close()
    assert (a["status"] == capi.SOLVED).all()
    for k in KEYS:
        same_bits(a[k], b[k], f"second call, {k}")
        same_bits(a[k], d[k].cpu().numpy(), f"manual rounds, {k}")
    # the closed loop moved: the ticks are not copies of one another
    assert np.abs(a["x_traj"][1:] - a["x_traj"][:-1]).max(axis=(1, 2)).min() > 0.01
    assert (np.abs(a["u_plan"][1:] - a["u_plan"][:-1]).max(axis=(1, 2, 3)) > 0).all()


# ---- case 11: NULL options -----------------------------------------------------------------------

def test_rollout_null_options_and_cost(oracle, capi, cuda):
    """11: without u_plan / x_plan / iters_traj / cost_traj the call gives the same x_traj /
    u_lin_traj / u_applied / status_traj bits as the full call; cost_traj matches
    oracle.tracking_cost of the exact optimum of each recorded tick within 1e-6 max(1, cost), the
    bound of test_gpu_parity.py::test_objective_matches_oracle."""
    B, N, T = 64, 20, 3
    x0, ul, xr = rc_.start(B, N, seed=111)
    s = solver(capi, N)
    full = rollout_dev(capi, cuda, s, x0, ul, xr, None, T)
    lean = rollout_dev(capi, cuda, s, x0, ul, xr, None, T, full=False)
    s.close()
    assert set(lean) == {"x_traj", "u_lin_traj", "u_applied", "status"}
    for k in lean:
        same_bits(lean[k], full[k], k)
    sts, us, xs = check_ticks(oracle, capi, full, xr, None, N, what="full call")
    prm = oracle.params(N)
    for t in range(T):
        cr = oracle.tracking_cost(prm, us[t], xs[t], xr)
        err = np.abs(full["cost"][t] - cr)
        print(f"tick {t}: max cost err {err.max():.3e} at cost {cr[np.argmax(err)]:.3e}")
        assert (err <= 1e-6 * np.maximum(1.0, cr)).all(), float(err.max())


# ---- cases 12, 13: no hidden synchronisation, the host variant -----------------------------------

def test_rollout_host_variant_and_no_completion_word(capi, cuda):
    """12, 13: Solver.rollout returns the bits of rollout_dev for case 1 (64 x N=20 x 8 ticks), and
    neither call moves f110qp_sync_signals (a host solve on the same context does)."""
    B, N, T = 64, 20, 8
    x0, ul, xr = rc_.start(B, N, seed=100 + B % 97 + N)
    s = solver(capi, N)
    n0 = s.sync_signals()
    dev = rollout_dev(capi, cuda, s, x0, ul, xr, None, T)
    assert s.sync_signals() == n0
    host = s.rollout(x0, ul, xr, T, plans=True, objective=True)
    assert s.sync_signals() == n0
    lean = s.rollout(x0, ul, xr, T)
    assert s.sync_signals() == n0
    s.solve_dbl(x0, ul, xr)
    assert s.sync_signals() == n0 + 1  # the counter does move for a call that polls the word
    s.close()
    assert set(host) == set(KEYS) and set(lean) == {"x_traj", "u_lin_traj", "u_applied", "status", "iters"}
    for k in KEYS:
        same_bits(host[k], dev[k], f"host rollout, {k}")
    for k in lean:
        same_bits(lean[k], dev[k], f"lean host rollout, {k}")


# ---- case 14: float32 start ----------------------------------------------------------------------

def test_rollout_float32_start_matches_the_float_solve(capi, cuda):
    """14: a start (and reference) that is exactly float32-valued gives a tick-0 plan bit-identical
    to solve_dev on the float inputs (64 cars, AUTO: the wave back end, not the sequential
    float-LDS scratch mode the header exempts)."""
    import torch

    B, N, T = 64, 20, 2
    w = workload.make_batch(B, N, seed=114)
    s = solver(capi, N)
    assert s.backend_info(B)[0] == capi.BACKEND_WAVE
    out = rollout_dev(capi, cuda, s, *(w[k].astype(np.float64) for k in ("x0", "u_lin", "x_ref")), None, T)
    t = {k: torch.from_numpy(w[k]).to(cuda) for k in ("x0", "u_lin", "x_ref")}
    uo = torch.empty((B, N, 2), dtype=torch.float32, device=cuda)
    xo = torch.empty((B, N + 1, 3), dtype=torch.float32, device=cuda)
    st = torch.empty(B, dtype=torch.int32, device=cuda)
    it = torch.empty(B, dtype=torch.int32, device=cuda)
    s.solve_dev(t["x0"], t["u_lin"], t["x_ref"], None, uo, xo, st, it)
    torch.cuda.synchronize(cuda)
    s.close()
    assert (out["status"][0] == capi.SOLVED).all()
    same_bits(out["u_plan"][0], uo.cpu().numpy(), "tick-0 u_plan")
    same_bits(out["x_plan"][0], xo.cpu().numpy(), "tick-0 x_plan")
    np.testing.assert_array_equal(out["status"][0], st.cpu().numpy())
    np.testing.assert_array_equal(out["iters"][0], it.cpu().numpy())
