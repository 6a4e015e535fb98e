"""The fixed part of the fixed-length segment kernels (csrc/lane_seg_kernel.h, Q = 5): their two code
tables come from the solver's constant block (csrc/seg_tables.h, filled once per solver on the device)
instead of being built by every wave. Every case solves on that route and on the run-time-length route
of the test build (F110QP_SEG_FIXEDQ=0: its waves still build their own tables),
asserts which route each solver takes, and compares the two bit for bit: status, iters, u and x (NaNs
in the same places). Against the oracle at the tolerance of the other segment tests (TOL; test_gpu_dbl's
bound on the double inputs). All cases N = 20, S = 4, heading frame.

A stale or foreign block would change the bounds, the re-guess thresholds or the free masks of a solver:
the two-solver and the re-created-solver cases use boxes whose optima differ by far more than TOL
(asserted on the oracle's answers), so a solver reading the other's block cannot pass its own parity.
"""
import numpy as np
import pytest

from f110qp import workload

from test_gpu_dbl import assert_parity, dbl_batch
from test_gpu_parity import TOL, rel_err
from test_gpu_seg_ends import batch, lane, oracle_ref, parity
from test_gpu_seg_issue import bit_equal, routes

pytestmark = pytest.mark.gpu

N = 20
INSIDE = dict(u_des=[4.0, 0.0])  # strictly inside the speed box [3.0, 4.5]: no twin start
# a second box and other weights: the speed band and the steering limits narrower, u_des on the lower bound
OTHER = dict(u_min=[2.0, -0.2], u_max=[3.5, 0.25], u_des=[2.0, 0.0], r=[0.7, 0.3], q=[8.0, 8.0, 2.0])


_dbl = {}


def dbl_expected(oracle, B, twin, **cfg):
    """test_gpu_dbl's expected() for a config of this file: doubles that no float32 holds and the oracle's
    answer on them, computed once."""
    if (B, twin) not in _dbl:
        x0, ul, xr = dbl_batch(B, N, 61, 0.0)
        prm = oracle.params(N, **cfg)
        us, xs, st, ob = np.zeros((B, N, 2)), np.zeros((B, N + 1, 3)), np.zeros(B, np.int32), np.zeros(B)
        for b in range(B):
            r = oracle.solve(prm, x0[b], ul[b], xr[b], None, False)
            us[b], xs[b], st[b], ob[b] = r["u"], r["x"], r["status"], r["obj"]
        for a in (x0, ul, xr, us, xs, st, ob):
            a.setflags(write=False)
        _dbl[(B, twin)] = (x0, ul, xr, None, us, xs, st, ob)
    return _dbl[(B, twin)]


@pytest.mark.parametrize("dbl", [False, True], ids=["float", "dbl"])
@pytest.mark.parametrize("twin", [True, False], ids=["twin", "one_start"])
@pytest.mark.parametrize("B", [1, 5, 37])
def test_batches(oracle, capi, knob, B, twin, dbl):
    """One slot, duplicate lanes, a partly filled last wave; u_des on a speed bound (the shipped config,
    twin starts) and strictly inside the box (one start)."""
    cfg = {} if twin else INSIDE
    if dbl:
        exp = dbl_expected(oracle, B, twin, **cfg)
        new, old = routes(capi, knob, N, None, B, call=lambda s: s.solve_dbl(exp[0], exp[1], exp[2]), **cfg)
        bit_equal(new, old)
        assert_parity(capi, oracle, new, exp, "constant block")
    else:
        w = batch(B, N)
        s = lane(capi, N, **cfg)
        assert s.lane_starts(B) == (2 if twin else 1)
        s.close()
        new, old = routes(capi, knob, N, w, B, **cfg)
        bit_equal(new, old)
        parity(capi, new, oracle_ref(oracle, ("box", N, B, twin), N, w, **cfg))


def test_two_solvers_keep_their_own_tables(oracle, capi, knob):
    """Two solvers alive at once with different bounds and weights, called alternately, twice each."""
    B = 37
    w = batch(B, N)
    ra, rb = oracle_ref(oracle, ("box", N, B, True), N, w), oracle_ref(oracle, ("other", B), N, w, **OTHER)
    assert rel_err(ra[0], rb[0]).max() > 100 * TOL  # the two configs' optima are far apart
    knob("F110QP_SEG_FIXEDQ", "1")
    a, b = lane(capi, N), lane(capi, N, **OTHER)
    assert a.lane_fixed_q(B) == 5 and b.lane_fixed_q(B) == 5
    outs = [s.solve(w["x0"], w["u_lin"], w["x_ref"]) for s in (a, b, a, b)]
    a.close()
    b.close()
    for out, ref in zip(outs, (ra, rb, ra, rb)):
        parity(capi, out, ref)
    bit_equal(outs[0], outs[2])
    bit_equal(outs[1], outs[3])
    old_b = routes(capi, knob, N, w, B, **OTHER)[1]
    bit_equal(outs[1], old_b)


def test_destroyed_solver_leaves_no_stale_block(oracle, capi, knob):
    """A solver used and destroyed, then one with other bounds created (its block may take the freed
    address): the new solver's answers are its own config's."""
    B = 5
    w = batch(B, N)
    knob("F110QP_SEG_FIXEDQ", "1")
    first = lane(capi, N)
    out_a = first.solve(w["x0"], w["u_lin"], w["x_ref"])
    first.close()
    second = lane(capi, N, **OTHER)
    assert second.lane_fixed_q(B) == 5
    out_b = second.solve(w["x0"], w["u_lin"], w["x_ref"])
    second.close()
    parity(capi, out_a, oracle_ref(oracle, ("box", N, B, True), N, w))
    parity(capi, out_b, oracle_ref(oracle, ("other", B), N, w, **OTHER))
    bit_equal(out_b, routes(capi, knob, N, w, B, **OTHER)[1])


@pytest.mark.parametrize("name,over", [
    ("speed_pinned", dict(u_min=[4.0, -0.43], u_max=[4.0, 0.43])),       # u_min == u_max on the speed
    ("steer_pinned", dict(u_min=[3.0, 0.1], u_max=[4.5, 0.1])),          # ... on the steering angle
    ("far_bounds", dict(u_min=[-300.0, -0.43], u_max=[4.5, 200.0])),     # 1 + |bound| sets the tolerance
    ("no_bound", dict(u_min=[3.0, -1e30], u_max=[1e30, 0.43])),          # bound_scale's capped sum
])
def test_degenerate_and_far_bounds(oracle, capi, knob, name, over):
    B = 5
    w = batch(B, N)
    new, old = routes(capi, knob, N, w, B, **over)
    bit_equal(new, old)
    ref = oracle_ref(oracle, ("bounds", name), N, w, **over)
    ok = ref[2] == capi.SOLVED
    np.testing.assert_array_equal(new[2][ok], ref[2][ok])
    assert ok.any()
    eu, ex = rel_err(new[0][ok], ref[0][ok]).max(), rel_err(new[1][ok], ref[1][ok]).max()
    print(f"{name}: max rel err u {eu:.3e} x {ex:.3e}")
    assert eu <= TOL and ex <= TOL, (eu, ex)


def test_no_pass_runs(oracle, capi, knob):
    """Every QP of the wave non-finite: no pass runs, NUMERICAL and NaN on both routes; and the smallest
    pass budget the API takes (max_iter = 1, single flips from the first pass)."""
    B = 5
    w = batch(B, N)
    x0 = w["x0"].copy()
    x0[:, 0] = np.inf
    new, old = routes(capi, knob, N, dict(w, x0=x0), B, max_iter=1)
    bit_equal(new, old)
    assert (new[2] == capi.NUMERICAL).all() and (new[3] == 0).all()
    assert np.isnan(new[0]).all() and np.isnan(new[1]).all()
    knob("F110QP_LANE_KMAX", "0")
    new, old = routes(capi, knob, N, w, B, max_iter=1)
    bit_equal(new, old)
    assert (new[3] <= 1).all()


@pytest.mark.parametrize("B", [5, 37])
def test_one_non_finite_qp_among_finite_ones(oracle, capi, knob, B):
    """Its neighbours' outputs are those of the clean solve, its own NUMERICAL and NaN as on the other
    route."""
    w = batch(B, N)
    clean = routes(capi, knob, N, w, B)[0]
    xr = w["x_ref"].copy()
    xr[2, 7, 1] = np.nan
    new, old = routes(capi, knob, N, dict(w, x_ref=xr), B)
    bit_equal(new, old)
    good = np.setdiff1d(np.arange(B), [2])
    assert new[2][2] == capi.NUMERICAL and np.isnan(new[0][2]).all() and np.isnan(new[1][2]).all()
    for k in range(4):
        np.testing.assert_array_equal(new[k][good], clean[k][good])


def test_max_iter_unconverged(oracle, capi, knob):
    """F110QP_LANE_KMAX=1, one start, max_iter = 2 on the many-bound batch whose QPs need more than two
    passes (test_gpu_seg_issue.test_single_flip_passes_restore_the_state_word): MAX_ITER with whatever
    the second pass left, as on the other route."""
    B = 37
    knob("F110QP_LANE_KMAX", "1")
    knob("F110QP_LANE_TWIN", "0")
    w = batch(B, N)
    new, old = routes(capi, knob, N, w, B, max_iter=2)
    bit_equal(new, old)
    assert (new[2] == capi.MAX_ITER).any()


def test_x_ref_points_past_the_horizon(oracle, capi, knob):
    """x_ref rows of 50 points (the tick's stride), the rows past the horizon NaN."""
    B = 5
    w = batch(B, N)
    xr = np.concatenate([w["x_ref"], np.full((B, 50 - N, 3), np.nan, np.float32)], 1)
    new, old = routes(capi, knob, N, None, B, call=lambda s: s.solve(w["x0"], w["u_lin"], xr), x_ref_points=50)
    bit_equal(new, old)
    parity(capi, new, oracle_ref(oracle, ("box", N, B, True), N, w))


def test_objective_outputs(oracle, capi, knob):
    B = 5
    w = batch(B, N)
    new, old = routes(capi, knob, N, None, B,
                      call=lambda s: s.solve(w["x0"], w["u_lin"], w["x_ref"], objective=True))
    bit_equal(new, old)
    np.testing.assert_array_equal(new[4], old[4])
    np.testing.assert_array_equal(new[5], old[5])
    assert np.isfinite(new[4]).all() and (new[5] >= 0).all()


def test_warm_start_over_three_calls(oracle, capi, knob):
    """warm_start = 1, the key repeating on the second call and changed on the third; a fourth call repeats
    the third's key and is seeded from the masks the third stored. Answers, pass counts and hit counters of
    every call as on the other route."""
    B = 5
    w = batch(B, N)
    w3 = {k: v.copy() for k, v in w.items()}
    w3["u_lin"][:, 0] += 0.25

    def four(s):
        outs, hits = [], []
        for ww in (w, w, w3, w3):
            outs.append(s.solve(ww["x0"], ww["u_lin"], ww["x_ref"]))
            hits.append(s.warm_hits())
        return outs, hits

    (new, hn), (old, ho) = routes(capi, knob, N, None, B, call=four, warm_start=1)
    assert hn == ho
    assert [h[1] for h in hn] == [0, B, 0, B]
    for k in range(4):
        bit_equal(new[k], old[k])
    for k in (0, 1, 2):  # a seeded call gives the cold call's answers
        np.testing.assert_array_equal(new[3][k], new[2][k])


def test_second_stream_waits_for_the_fill(oracle, capi, knob, cuda):
    """A new solver's first two calls go out back to back on two streams, nothing synchronised between
    them: the second stream's kernel must wait for the block's fill on the first. Both give the host
    call's answers bit for bit."""
    import torch

    B = 37
    w = batch(B, N)
    knob("F110QP_SEG_FIXEDQ", "1")
    ref = lane(capi, N)
    want = ref.solve(w["x0"], w["u_lin"], w["x_ref"])
    ref.close()
    x0, ul, xr = (torch.from_numpy(w[k]).to(cuda) for k in ("x0", "u_lin", "x_ref"))
    outs = [dict(u=torch.zeros((B, N, 2), dtype=torch.float32, device=cuda),
                 x=torch.zeros((B, N + 1, 3), dtype=torch.float32, device=cuda),
                 st=torch.zeros((B,), dtype=torch.int32, device=cuda),
                 it=torch.zeros((B,), dtype=torch.int32, device=cuda)) for _ in range(2)]
    streams = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    torch.cuda.synchronize()
    s = lane(capi, N)
    assert s.lane_fixed_q(B) == 5
    for o, st in zip(outs, streams):
        s.solve_dev(x0, ul, xr, None, o["u"], o["x"], o["st"], o["it"], stream=st)
    torch.cuda.synchronize()
    s.close()
    for o in outs:
        bit_equal((o["u"].cpu().numpy(), o["x"].cpu().numpy(), o["st"].cpu().numpy(), o["it"].cpu().numpy()), want)
