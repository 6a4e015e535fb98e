"""The fixed-length segment kernels (csrc/lane_seg_kernel.h, Q = 5) with the pass loop's LDS round
trips taken out: every per-stage value of the forward sweep (K 6, k 2, the lam-gains F 6) lives in
registers (all 14; the partial schemes are retired), so that the pass loop reads LDS for code-table
entries only. The fixed-length route must give the run-time-length route's bits
(F110QP_SEG_FIXEDQ=0 in the test build: the Q = 0 kernel, whose text did not change) and the oracle's answer at the tolerance of the other seg tests (TOL, and
test_gpu_dbl's bound on the double inputs). All cases N = 20, S = 4.

Pass budgets: the ABI takes no zero budget (max_iter >= 1, F110QP_LANE_PASSCAP in 1 .. 999; a cap of 0
is "no cap", the kernel's pass_cap = 0), so the smallest budget is max_iter = 1 with the cap left at 0
and single flips from the first pass (F110QP_LANE_KMAX=0: max_pass = max(max_iter, kmax) = 1), and
the wave that runs no pass at all (ran == false: NaNs stored without a gain being read) is the wave
whose QPs are all non-finite.

Measured on an MI355X over every case of this file: route-to-route difference 0 (bit-identical)."""
import numpy as np
import pytest

from f110qp import workload

from test_gpu_dbl import assert_parity, expected
from test_gpu_parity import TOL, rel_err
from test_gpu_seg_ends import batch, lane, oracle_ref, parity
from test_gpu_seg_issue import bit_equal, routes, sequential

pytestmark = pytest.mark.gpu

N = 20
INSIDE = dict(u_des=[4.0, 0.0])  # strictly inside the speed box [3.0, 4.5]


@pytest.mark.parametrize("dbl", [False, True], ids=["float", "dbl"])
@pytest.mark.parametrize("twin", ["1", "0"])
@pytest.mark.parametrize("B", [1, 5, 37])
def test_batches(oracle, capi, knob, B, twin, dbl):
    """One slot, duplicate lanes, a partly filled last wave; twin starts and one start."""
    knob("F110QP_LANE_TWIN", twin)
    if dbl:
        exp = expected(oracle, B, N, 41, 0.0)
        new, old = routes(capi, knob, N, None, B, call=lambda s: s.solve_dbl(exp[0], exp[1], exp[2]))
        bit_equal(new, old)
        assert_parity(capi, oracle, new, exp, "register gains")
    else:
        w = batch(B, N)
        new, old = routes(capi, knob, N, w, B)
        bit_equal(new, old)
        parity(capi, new, oracle_ref(oracle, ("box", N, B), N, w))


def test_one_two_and_three_passes_in_one_wave(oracle, capi, knob):
    """QPs that converge after 1, 2 and 3 passes planted next to each other in one wave (one start, 16
    slots): the wave sweeps on after the early ones have converged and rewrites their register gains
    from an unchanged state word, so their outputs and pass counts stay the sequential kernel's."""
    knob("F110QP_LANE_TWIN", "0")
    pool = [workload.make_batch(32, N, seed=9700, heading="true", lateral=0.0, steer_range=0.0),
            workload.make_batch(32, N, seed=9701, heading="true", lateral=0.3, steer_range=0.2),
            workload.make_batch(32, N, seed=9702, heading="true", lateral=1.5, steer_range=1.0)]
    wp = {k: np.concatenate([p[k] for p in pool]) for k in ("x0", "u_lin", "x_ref")}
    seq_pool = sequential(capi, knob, ("pool",), N, wp, 96, **INSIDE)
    it = seq_pool[3]
    print("pool pass counts:", np.bincount(it))
    pick = []
    for passes in (1, 2, 3):
        idx = np.flatnonzero((it == passes) & (seq_pool[2] == capi.SOLVED))
        assert len(idx) >= 2, (passes, np.bincount(it))
        pick += [idx[0], idx[1]]
    order = [pick[k] for k in (4, 0, 2, 5, 1, 3)]  # 3, 1, 2, 3, 1, 2 passes: early and late mixed
    w = {k: np.ascontiguousarray(v[order]) for k, v in wp.items()}
    B = len(order)
    knob("F110QP_LANE_SEG", "0")  # (sequential() left F110QP_LANE_SEG=1 set: back to auto for the routes)
    new, old = routes(capi, knob, N, w, B, **INSIDE)
    bit_equal(new, old)
    np.testing.assert_array_equal(new[3], np.array([3, 1, 2, 3, 1, 2]))
    np.testing.assert_array_equal(new[3], it[order])
    assert (new[2] == capi.SOLVED).all()
    parity(capi, new, oracle_ref(oracle, ("planted",), N, w, **INSIDE))
    # each QP as in the pool's own solve by the sequential kernel (fp64 rounding apart)
    assert rel_err(new[0], seq_pool[0][order].astype(np.float64)).max() <= 1e-6


@pytest.mark.parametrize("twin", ["1", "0"])
def test_smallest_pass_budget(oracle, capi, knob, twin):
    """max_iter = 1, the pass cap left at 0, single flips from the first pass: one pass and no more;
    what it leaves (MAX_ITER and NaN for most QPs) is the other route's."""
    B = 9
    knob("F110QP_LANE_TWIN", twin)
    knob("F110QP_LANE_KMAX", "0")
    w = batch(B, N)
    new, old = routes(capi, knob, N, w, B, max_iter=1)
    bit_equal(new, old)
    assert (new[3] <= 1).all()
    ns = new[2] != capi.SOLVED
    assert ns.any() and (new[2][ns] == capi.MAX_ITER).all()
    assert np.isnan(new[0][ns]).all() and np.isnan(new[1][ns]).all()


def test_wave_that_runs_no_pass(oracle, capi, knob):
    """Every QP of the wave non-finite, max_iter = 1: no pass runs (ran == false), no register gain was
    written, and the output sweep stores NaN without reading one."""
    B = 5
    w = batch(B, N)
    x0 = w["x0"].copy()
    x0[:, 0] = np.inf
    new, old = routes(capi, knob, N, dict(w, x0=x0), B, max_iter=1)
    bit_equal(new, old)
    assert (new[2] == capi.NUMERICAL).all() and (new[3] == 0).all()
    assert np.isnan(new[0]).all() and np.isnan(new[1]).all()


@pytest.mark.parametrize("twin", ["1", "0"])
def test_one_non_finite_qp_in_a_wave(oracle, capi, knob, twin):
    """One QP's reference non-finite (a stage of segment 2): NUMERICAL and NaN for it alone; the QPs that
    share its wave keep the clean batch's bits."""
    B, bad = 7, 3
    knob("F110QP_LANE_TWIN", twin)
    w = batch(B, N)
    clean, _ = routes(capi, knob, N, w, B)
    xr = w["x_ref"].copy()
    xr[bad, 12, 1] = np.nan
    new, old = routes(capi, knob, N, dict(w, x_ref=xr), B)
    bit_equal(new, old)
    good = np.setdiff1d(np.arange(B), [bad])
    assert new[2][bad] == capi.NUMERICAL and (new[2][good] == capi.SOLVED).all()
    assert np.isnan(new[0][bad]).all() and np.isnan(new[1][bad]).all()
    bit_equal([a[good] for a in new], [a[good] for a in clean])


def test_warm_traffic_then_cold(oracle, capi, knob):
    """warm_start = 1: the first call moves warm traffic and misses (the state word built stage by stage
    from the empty masks and the twin rule), the second hits on every QP (built from the masks the first
    wrote back). Then a solver without warm state (the word in closed form from the twin rule). The
    three ways of building the word feed the same register gains: every call both routes' bits, the same
    optimum."""
    B = 5
    w = batch(B, N)

    def pair(s):
        outs, hits = [], []
        for _ in range(2):
            outs.append(s.solve(w["x0"], w["u_lin"], w["x_ref"]))
            hits.append(s.warm_hits()[1])
        return outs, hits

    (new, hn), (old, ho) = routes(capi, knob, N, w, B, call=pair, warm_start=1)
    assert hn == [0, B] and ho == [0, B]
    bit_equal(new[0], old[0])
    bit_equal(new[1], old[1])
    cold, cold_old = routes(capi, knob, N, w, B)
    bit_equal(cold, cold_old)
    for k in (2, 0, 1):
        np.testing.assert_array_equal(new[1][k], new[0][k])
        np.testing.assert_array_equal(cold[k], new[0][k])
    assert (new[1][3] <= new[0][3]).all()
    ref = oracle_ref(oracle, ("box", N, B), N, w)
    parity(capi, new[1], ref)
    parity(capi, cold, ref)


@pytest.mark.parametrize("q", [[0.0, 0.0, 0.0], [1e-9, 1e-9, 0.0]])
def test_single_flip_copy_on_a_degenerate_bound(oracle, capi, knob, q):
    """max_iter above kmax on test_degenerate_bound's QPs (the speed on its bound with a zero multiplier).
    These QPs settle in one pass from either start (measured: one pass each at F110QP_LANE_KMAX=1), so a
    pass past kmax never runs on them unless kmax is 0: with F110QP_LANE_KMAX=0 every pass, the first
    included, is a single-flip pass (pass >= kmax), and the pass they run is the single-flip copy of the
    forward sweep, reading the same register gains."""
    B = 3
    knob("F110QP_LANE_KMAX", "0")
    w = workload.make_batch(B, N, seed=4500, heading="true", lateral=0.0, steer_range=0.0)
    new, old = routes(capi, knob, N, w, B, max_iter=60, q=q)
    bit_equal(new, old)
    assert (new[2] == capi.SOLVED).all()
    print("passes:", new[3])
    assert new[3].min() >= 1  # a pass ran on every QP, and at kmax = 0 each pass is a single-flip pass
    ur, xr, sr = oracle.solve_batch(oracle.params(N, q=q), w["x0"], w["u_lin"], w["x_ref"])[:3]
    np.testing.assert_array_equal(new[2], sr)
    assert rel_err(new[0], ur).max() <= 2e-6 and rel_err(new[1], xr).max() <= 2e-6


def test_single_flip_copy_after_a_pdas_pass(oracle, capi, knob):
    """F110QP_LANE_KMAX=1, max_iter = 60, one start, QPs with many active bounds: the first pass is a PDAS
    pass, every later one a single-flip pass on the gains the backward sweep just left in registers; some
    QP runs past kmax (asserted), and status and pass counts are the sequential kernel's."""
    B = 5
    knob("F110QP_LANE_KMAX", "1")
    knob("F110QP_LANE_TWIN", "0")
    w = batch(B, N)
    new, old = routes(capi, knob, N, w, B, max_iter=60)
    bit_equal(new, old)
    print("passes:", new[3])
    assert new[3].max() > 1  # the single-flip copy was executed
    assert (new[2] == capi.SOLVED).all()
    seq = sequential(capi, knob, ("flip5",), N, w, B, max_iter=60)
    np.testing.assert_array_equal(new[2], seq[2])
    np.testing.assert_array_equal(new[3], seq[3])
    parity(capi, new, oracle_ref(oracle, ("box", N, B), N, w))
