"""The fixed-length partitioned-horizon kernels (csrc/lane_seg_kernel.h, Q = 5: S = 4 segments of a
20-stage horizon in the heading frame, the stage loops unrolled, the lane's references, PDAS state
and feedback gains in registers) against the run-time-length kernel they replace and against the CPU
oracle, through the C ABI. Every case solves twice in the test build: on the new route and with
F110QP_SEG_FIXEDQ=0 (the parent's code path), and asserts which route each solver takes
(f110qp_lane_fixed_q), so that it cannot pass on the old kernel alone.

Bounds: status and iters identical; u and x against the oracle at the project's 1e-4 relative (the
check of tests/test_gpu_seg.py); route to route ROUTE_TOL. Both routes evaluate the same fp64
expressions and write float32, so only contraction and ordering could differ: the largest difference
measured over all cases of this file on an MI355X is MEASURED_ROUTE_DIFF = 0 (every output
bit-identical; also on 1,024 and 4,096 x N = 20); the bound is 4x that, capped at the 1e-6 DESIGN.md 5
records for this path, so the two routes must agree exactly.
"""
import numpy as np
import pytest

from f110qp import workload

from test_gpu_dbl import assert_parity, expected
from test_gpu_parity import TOL, rel_err

N = 20
MEASURED_ROUTE_DIFF = 0.0  # measured on an MI355X over every case below
ROUTE_TOL = min(4 * MEASURED_ROUTE_DIFF, 1e-6)
BATCHES = [1, 2, 3, 17, 130]  # one slot, a twin pair, duplicate lanes, a partial wave, two waves and a tail
INSIDE = dict(u_des=[4.0, 0.0])  # u_des[0] strictly inside the speed box [3.0, 4.5]: no twin start

_ref = {}


def batch(B, seed=7000, **kw):
    return workload.make_batch(B, N, seed=seed + B, heading="true", lateral=1.0, steer_range=0.6, **kw)


def oracle_ref(oracle, key, w, objective=False, **over):
    """The oracle's answer for a case, computed once and left unchanged."""
    if key not in _ref:
        r = oracle.solve_batch(oracle.params(N, **over), w["x0"], w["u_lin"], w["x_ref"][:, :N], objective=objective)
        for a in r:
            a.setflags(write=False)
        _ref[key] = r
    return _ref[key]


def both_routes(capi, knob, B, call, starts=None, **cfg):
    """call(solver) on the fixed-length route and on the run-time-length one; the route, the segment
    count and (if given) the PDAS starts asserted on each solver."""
    out = {}
    for fq in ("1", "0"):
        knob("F110QP_SEG_FIXEDQ", fq)
        s = capi.Solver(capi.default_config(N, backend=capi.BACKEND_LANE, **cfg))
        assert s.test_build
        assert s.lane_segments(B) == 4
        assert s.lane_fixed_q(B) == (5 if fq == "1" else 0)
        if starts is not None:
            assert s.lane_starts(B) == starts
        out[fq] = call(s)
        s.close()
    return out["1"], out["0"]


def route_diff(new, old):
    """status and iters identical, u and x within ROUTE_TOL (figures printed before the assert)."""
    np.testing.assert_array_equal(new[2], old[2])
    np.testing.assert_array_equal(new[3], old[3])
    ok = new[2] == 1
    d = 0.0
    if ok.any():
        d = max(rel_err(new[0][ok], old[0][ok].astype(np.float64)).max(),
                rel_err(new[1][ok], old[1][ok].astype(np.float64)).max())
    print(f"route-to-route max rel diff {d:.3e}")
    assert d <= ROUTE_TOL, d
    return d


def oracle_parity(capi, out, ref, tol=TOL):
    ur, xr, sr = ref[0], ref[1], ref[2]
    np.testing.assert_array_equal(out[2], sr)
    ok = sr == capi.SOLVED
    assert ok.any()
    assert rel_err(out[0][ok], ur[ok]).max() <= tol and rel_err(out[1][ok], xr[ok]).max() <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("twin", [True, False])
@pytest.mark.parametrize("B", BATCHES)
def test_batches_twin_and_one_start(oracle, capi, knob, B, twin):
    w = batch(B)
    cfg = {} if twin else INSIDE
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"]),
                           starts=2 if twin else 1, **cfg)
    route_diff(new, old)
    ref = oracle_ref(oracle, ("b", B, twin), w, **cfg)
    assert (ref[2] == capi.SOLVED).all()
    oracle_parity(capi, new, ref)
    oracle_parity(capi, old, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kmax", ["0", "1", "2"])
def test_single_flip_passes(oracle, capi, knob, kmax):
    """Single least-index flips from pass kmax on: the segments that did not hold the QP's first flip
    put the replaced state back into the packed word."""
    B = 17
    knob("F110QP_LANE_KMAX", kmax)
    w = workload.make_batch(B, N, seed=7117, heading="true", lateral=1.5, steer_range=1.0)
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"]))
    route_diff(new, old)
    oracle_parity(capi, new, oracle_ref(oracle, ("flip",), w))


@pytest.mark.gpu
def test_non_finite_inputs(oracle, capi, knob):
    """NaN in x_ref at the first and at the last stage of a middle segment, NaN in x0: NUMERICAL and
    NaN outputs for that QP only; every other QP of its wave as in the clean solve."""
    B = 130
    w = batch(B)
    clean = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"]))[0]
    wb = {k: v.copy() for k, v in w.items()}
    wb["x_ref"][3, 5, 0] = np.nan    # first stage of segment 1
    wb["x_ref"][40, 14, 2] = np.nan  # last stage of segment 2
    wb["x0"][77, 1] = np.nan
    bad = np.array([3, 40, 77])
    new, old = both_routes(capi, knob, B, lambda s: s.solve(wb["x0"], wb["u_lin"], wb["x_ref"]))
    route_diff(new, old)
    good = np.setdiff1d(np.arange(B), bad)
    for out in (new, old):
        assert (out[2][bad] == capi.NUMERICAL).all() and (out[2][good] == capi.SOLVED).all()
        assert np.isnan(out[0][bad]).all() and np.isnan(out[1][bad]).all()
    for k in range(4):
        np.testing.assert_array_equal(new[k][good], clean[k][good])


@pytest.mark.gpu
@pytest.mark.parametrize("q", [[0.0, 0.0, 0.0], [1e-9, 1e-9, 0.0]])
def test_degenerate_bound(oracle, capi, knob, q):
    """The inputs of test_degenerate_bound_zero_multiplier: the speed on its bound with a zero
    multiplier."""
    B = 3
    w = workload.make_batch(B, N, seed=4500, heading="true", lateral=0.0, steer_range=0.0)
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"]), q=q)
    route_diff(new, old)
    assert (new[2] == capi.SOLVED).all()
    oracle_parity(capi, new, oracle_ref(oracle, ("deg", tuple(q)), w, q=q), tol=2e-6)


@pytest.mark.gpu
def test_warm_start_from_the_packed_word(oracle, capi, knob):
    """Three calls on the same inputs with warm_start = 1: the second and third are seeded from the
    first's write-back of the packed state word, on all 17 QPs, and give the first call's answers."""
    B = 17
    w = batch(B)

    def three(s):
        outs, hits = [], []
        for _ in range(3):
            outs.append(s.solve(w["x0"], w["u_lin"], w["x_ref"]))
            hits.append(s.warm_hits()[1])
        return outs, hits

    (new, hn), (old, ho) = both_routes(capi, knob, B, three, warm_start=1)
    assert hn == [0, B, B] and ho == [0, B, B]
    for k in (1, 2):
        np.testing.assert_array_equal(new[k][2], new[0][2])
        np.testing.assert_array_equal(new[k][0], new[0][0])
        np.testing.assert_array_equal(new[k][1], new[0][1])
        assert (new[k][3] <= new[0][3]).all()
        np.testing.assert_array_equal(new[k][3], old[k][3])
    route_diff(new[0], old[0])
    route_diff(new[2], old[2])
    oracle_parity(capi, new[2], oracle_ref(oracle, ("b", B, True), w))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 130])
def test_dbl_entry_point(oracle, capi, knob, B):
    """Doubles that no float32 holds, against the oracle on the doubles (test_gpu_dbl's inputs and
    bounds)."""
    exp = expected(oracle, B, N, 21, 0.0)
    new, old = both_routes(capi, knob, B, lambda s: s.solve_dbl(exp[0], exp[1], exp[2]))
    route_diff(new, old)
    assert_parity(capi, oracle, new, exp, "fixed-length")
    assert_parity(capi, oracle, old, exp, "run-time-length")


@pytest.mark.gpu
def test_x_ref_points_past_the_horizon(oracle, capi, knob):
    """x_ref rows of 50 points (the tick route's stride), the rows past the horizon NaN."""
    B = 17
    w = batch(B)
    xr = np.concatenate([w["x_ref"], np.full((B, 50 - N, 3), np.nan, np.float32)], 1)
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], xr), x_ref_points=50)
    route_diff(new, old)
    oracle_parity(capi, new, oracle_ref(oracle, ("b", B, True), w))


@pytest.mark.gpu
def test_objective_outputs(oracle, capi, knob):
    B = 17
    w = batch(B)
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"], objective=True))
    route_diff(new, old)
    ur, xr, sr, obr = oracle_ref(oracle, ("obj",), w, objective=True)
    np.testing.assert_array_equal(new[2], sr)
    for out in (new, old):
        np.testing.assert_allclose(out[4], obr, rtol=1e-6, atol=1e-6)
    cr = oracle.tracking_cost(oracle.params(N), ur, xr, w["x_ref"])
    assert (np.abs(new[5] - cr) <= 1e-6 * np.maximum(1.0, cr)).all()


def test_knob_is_the_test_builds_alone(capi, monkeypatch):
    """F110QP_SEG_FIXEDQ=0 moves the test build to the run-time-length kernel; the product library
    reads no environment and keeps the fixed-length one (create touches no device)."""
    cfg = capi.default_config(N)
    for env, want_test in ((None, 5), ("1", 5), ("0", 0)):
        if env is None:
            monkeypatch.delenv("F110QP_SEG_FIXEDQ", raising=False)
        else:
            monkeypatch.setenv("F110QP_SEG_FIXEDQ", env)
        for test_build, want in ((True, want_test), (False, 5)):
            s = capi.Solver(cfg, test_build=test_build)
            assert s.test_build == test_build
            assert s.lane_segments(1024) == 4 and s.lane_fixed_q(1024) == want
            assert s.lane_fixed_q(8192) == (want if s.lane_segments(8192) == 4 else 0)
            s.close()
    s = capi.Solver(capi.default_config(40), test_build=False)
    assert s.lane_fixed_q(8192) == 0  # N = 40: ten-stage segments
    s.close()
