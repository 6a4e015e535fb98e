"""The setup and the output sweep of the fixed-length partitioned-horizon kernels (csrc/lane_seg_kernel.h,
Q = 5): the lane's references loaded straight from global memory (no staging through LDS), the register
gains left uninitialised with the no-pass wave handled on its own, the packed state built from the twin
rule alone when a call moves no warm state, the twin owner picked by a DPP row move, the stores of a
lane grouped under one test.

Every case runs at N = 20 in the heading frame through the C ABI of the test build, asserts that AUTO
takes the fixed-length kernel (f110qp_lane_fixed_q == 5), and compares it bit for bit (status, iters, u, x,
NaNs included) with the run-time-length kernel (F110QP_SEG_FIXEDQ=0), whose setup and output the change
leaves alone, and against the CPU oracle at the 1e-4 relative bound of tests/test_gpu_seg.py.
"""
import numpy as np
import pytest

from f110qp import workload

from test_gpu_dbl import expected
from test_gpu_parity import TOL, rel_err

N = 20
_ref = {}


def batch(B, seed=8100):
    return workload.make_batch(B, N, seed=seed + B, heading="true", lateral=1.0, steer_range=0.6)


def oracle_ref(oracle, key, x0, ul, xr):
    """The oracle's (u, x, status) of a case, computed once and left unchanged."""
    if key not in _ref:
        r = oracle.solve_batch(oracle.params(N), x0, ul, xr[:, :N])
        for a in r:
            a.setflags(write=False)
        _ref[key] = r
    return _ref[key]


def both_routes(capi, knob, B, call, starts=None, **cfg):
    """call(solver) on the fixed-length route and on the run-time-length one, each route asserted."""
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


def same_bits(new, old):
    """status, iters, u and x identical, a NaN equal to a NaN."""
    np.testing.assert_array_equal(new[2], old[2])
    np.testing.assert_array_equal(new[3], old[3])
    for k in (0, 1):
        assert new[k].dtype == np.float32 and old[k].dtype == np.float32
        nn, no = np.isnan(new[k]), np.isnan(old[k])
        np.testing.assert_array_equal(nn, no)
        np.testing.assert_array_equal(new[k][~nn].view(np.uint32), old[k][~no].view(np.uint32))


def oracle_parity(capi, out, ref):
    ur, xr, sr = ref[0], ref[1], ref[2]
    np.testing.assert_array_equal(out[2], sr)
    ok = sr == capi.SOLVED
    assert ok.any()
    eu, ex = rel_err(out[0][ok], ur[ok]).max(), rel_err(out[1][ok], xr[ok]).max()
    print(f"oracle: max rel err u {eu:.3e} x {ex:.3e}")
    assert eu <= TOL and ex <= TOL
    if (~ok).any():
        assert np.isnan(out[0][~ok]).all() and np.isnan(out[1][~ok]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B,twin", [(1, True), (3, True), (9, True), (17, False)])
def test_partial_and_multiple_waves(oracle, capi, knob, B, twin):
    """One QP; an odd count in a partial wave (the lanes of the missing slots duplicate a valid QP and
    load its references); twin starts in two waves, the second nearly empty; the one-start kernel in
    two waves."""
    w = batch(B)
    if not twin:
        knob("F110QP_LANE_TWIN", 0)
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"]),
                           starts=2 if twin else 1)
    same_bits(new, old)
    ref = oracle_ref(oracle, ("b", B), w["x0"], w["u_lin"], w["x_ref"])
    assert (ref[2] == capi.SOLVED).all()
    oracle_parity(capi, new, ref)


@pytest.mark.gpu
def test_reference_stride(oracle, capi, knob):
    """x_ref rows of 50 points (stride 150 scalars, not 3 N), the 30 points past the horizon a large finite
    value: a load at the wrong stride solves another problem without raising NUMERICAL."""
    B = 9
    w = batch(B)
    xr = np.concatenate([w["x_ref"], np.full((B, 50 - N, 3), 3.0e30, np.float32)], 1)
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], xr), starts=2, x_ref_points=50)
    same_bits(new, old)
    oracle_parity(capi, new, oracle_ref(oracle, ("b", B), w["x0"], w["u_lin"], w["x_ref"]))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 9])
def test_double_inputs(oracle, capi, knob, B):
    """The *_dbl entry point: 8-byte references loaded per lane, the same code past the widening."""
    exp = expected(oracle, B, N, 31, 0.0)
    new, old = both_routes(capi, knob, B, lambda s: s.solve_dbl(exp[0], exp[1], exp[2]))
    same_bits(new, old)
    oracle_parity(capi, new, (exp[4], exp[5], exp[6]))


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [0, 5, 10, 15, 19])
def test_non_finite_reference_one_segment(oracle, capi, knob, stage):
    """A NaN in one stage's reference of QP 4 of 9 (every segment in turn, first and last stage of the
    horizon included): that QP alone NUMERICAL with NaN outputs, every other QP (its wave neighbours, the
    slots of its twin sibling, the second wave) as in the clean batch, bit for bit."""
    B, bad = 9, 4
    w = batch(B)
    xr = w["x_ref"].copy()
    xr[bad, stage, stage % 3] = np.nan
    clean = _ref.get("clean")
    if clean is None:
        clean = _ref["clean"] = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"]))[0]
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], xr), starts=2)
    same_bits(new, old)
    good = np.setdiff1d(np.arange(B), [bad])
    assert new[2][bad] == capi.NUMERICAL and (new[2][good] == capi.SOLVED).all()
    assert np.isnan(new[0][bad]).all() and np.isnan(new[1][bad]).all()
    same_bits([a[good] for a in new], [a[good] for a in clean])
    ref = oracle_ref(oracle, ("b", B), w["x0"], w["u_lin"], w["x_ref"])
    oracle_parity(capi, [a[good] for a in new], [a[good] for a in ref])


@pytest.mark.gpu
def test_one_pass_budget(oracle, capi, knob):
    """The smallest pass budget the API takes is one pass (F110QP_LANE_PASSCAP >= 1, max_iter >= 1; no
    call can ask for zero): whatever one pass leaves, status, iters and outputs are the other route's."""
    B = 9
    w = batch(B)
    knob("F110QP_LANE_PASSCAP", 1)
    new, old = both_routes(capi, knob, B, lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"]), starts=2)
    same_bits(new, old)
    assert (new[3] <= 1).all()
    ns = new[2] != capi.SOLVED
    assert (new[2][ns] == capi.MAX_ITER).all()
    assert np.isnan(new[0][ns]).all() and np.isnan(new[1][ns]).all()
    ref = oracle_ref(oracle, ("b", B), w["x0"], w["u_lin"], w["x_ref"])
    ok = ~ns
    if ok.any():  # a QP that one pass solves is the optimum
        assert rel_err(new[0][ok], ref[0][ok]).max() <= TOL and rel_err(new[1][ok], ref[1][ok]).max() <= TOL


@pytest.mark.gpu
def test_wave_that_runs_no_pass(oracle, capi, knob):
    """Every QP of the wave non-finite: the pass loop ends before its first pass, the register gains were
    never written, and the wave reports NUMERICAL, zero iterations and NaN everywhere."""
    B = 3
    w = batch(B)
    x0 = w["x0"].copy()
    x0[:, 1] = np.nan
    new, old = both_routes(capi, knob, B, lambda s: s.solve(x0, w["u_lin"], w["x_ref"]), starts=2)
    same_bits(new, old)
    assert (new[2] == capi.NUMERICAL).all() and (new[3] == 0).all()
    assert np.isnan(new[0]).all() and np.isnan(new[1]).all()


@pytest.mark.gpu
def test_warm_state_on_the_same_kernel(oracle, capi, knob):
    """Two consecutive ticks of a stream whose linearisation keys repeat (the c5_straight pattern),
    warm_start = 1: the first call writes keys and active sets, the second is seeded from them on every QP
    (f110qp_warm_hits), and both calls are the other route's bit for bit. The second tick solved cold (no
    warm state: the packed state word built from the twin rule alone) gives the same optimum."""
    B = 9
    ticks = workload.make_stream(B, N, 2, seed=8200)

    def two(s):
        outs, hits = [], []
        for t in ticks:
            outs.append(s.solve(t["x0"], t["u_lin"], t["x_ref"]))
            hits.append(s.warm_hits()[1])
        return outs, hits

    (new, hn), (old, ho) = both_routes(capi, knob, B, two, starts=2, warm_start=1)
    assert hn == [0, B] and ho == [0, B]
    for k, t in enumerate(ticks):
        same_bits(new[k], old[k])
        oracle_parity(capi, new[k], oracle_ref(oracle, ("warm", k), t["x0"], t["u_lin"], t["x_ref"]))
    assert (new[1][3] <= new[0][3]).all()
    cold = both_routes(capi, knob, B, lambda s: s.solve(ticks[1]["x0"], ticks[1]["u_lin"], ticks[1]["x_ref"]), starts=2)
    same_bits(cold[0], cold[1])
    oracle_parity(capi, cold[0], oracle_ref(oracle, ("warm", 1), ticks[1]["x0"], ticks[1]["u_lin"], ticks[1]["x_ref"]))
