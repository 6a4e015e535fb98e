"""The segment ends of the partitioned-horizon lane kernel at S <= 4 (csrc/lane_seg_kernel.h, step 2 of
the pass: the boundary problem over the segments eliminated from both ends, S / 2 - 1 shared steps,
one meet, S / 2 - 1 shared back-substitution steps; numpy model tests/diag_seg_ends_model.py) against
the CPU oracle, the sequential lane kernel and the run-time-length route, through the C ABI.
F110QP_LANE_SEG forces S in the test build. Small shapes: two-stage segments, uneven splits with 1, 2
and 3 longer segments, the fixed-length route (N = 20), a lone QP, a partly filled wave and more than
one wave. The oracle's answer for a batch is computed once and shared by the cases that use it."""
import numpy as np
import pytest

from f110qp import workload

from test_gpu_parity import TOL, check, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (2, 3), (2, 5), (4, 8), (4, 9), (4, 10), (4, 11), (4, 17), (4, 20)]
BATCHES = [1, 5, 37]
WEIGHTS = dict(q=[3.0, 7.0, 2.0], r=[0.5, 1.5], u_des=[3.7, 0.05], u_min=[3.5, -0.2], u_max=[4.0, 0.2])

_ref = {}


def batch(B, N, seed=8800):
    """Many active bounds on both faces."""
    return workload.make_batch(B, N, seed=seed + 100 * N + B, heading="true", lateral=1.5, steer_range=1.0)


def oracle_ref(oracle, key, N, w, **over):
    if key not in _ref:
        r = oracle.solve_batch(oracle.params(N, **over), w["x0"], w["u_lin"], w["x_ref"])
        for a in r:
            a.setflags(write=False)
        _ref[key] = r
    return _ref[key]


def lane(capi, N, **cfg):
    return capi.Solver(capi.default_config(N, backend=capi.BACKEND_LANE, **cfg))


def solve(capi, N, w, B, segs=None, **cfg):
    s = lane(capi, N, **cfg)
    assert s.test_build
    if segs is not None:
        assert s.lane_segments(B) == segs
    out = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    return out


def parity(capi, out, ref, tol=TOL):
    u, x, st = out[0], out[1], out[2]
    ur, xr, sr = ref
    np.testing.assert_array_equal(st, sr)
    assert (sr == capi.SOLVED).all()
    eu, ex = rel_err(u, ur).max(), rel_err(x, xr).max()
    print(f"max rel err u {eu:.3e} x {ex:.3e}")
    assert eu <= tol and ex <= tol, (eu, ex)


@pytest.mark.parametrize("twin", ["0", "1"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("S,N", SHAPES)
def test_shapes_against_the_oracle(oracle, capi, knob, S, N, B, twin):
    """Every shape, batch size and both twin settings at TOL; a horizon with N / S < 2 keeps the
    sequential kernel (lane_segments says which)."""
    knob("F110QP_LANE_SEG", S)
    knob("F110QP_LANE_TWIN", twin)
    w = batch(B, N)
    out = solve(capi, N, w, B, segs=S if N // S >= 2 else 1)
    parity(capi, out, oracle_ref(oracle, ("box", N, B), N, w))


@pytest.mark.parametrize("frame", ["rot0", "weights"])
@pytest.mark.parametrize("N", [9, 20])
def test_general_frame(oracle, capi, knob, frame, N):
    """The general-frame instantiations: the heading frame switched off, and weights with q0 != q1
    (u_des inside a narrow box: one start)."""
    B = 37
    knob("F110QP_LANE_SEG", "4")
    w = batch(B, N, seed=8900)
    if frame == "rot0":
        knob("F110QP_LANE_ROT", "0")
        w["x0"][:, 2] = np.random.default_rng(N).uniform(-np.pi, np.pi, B).astype(np.float32)
        out = solve(capi, N, w, B, segs=4)
        parity(capi, out, oracle_ref(oracle, ("rot0", N), N, w))
    else:
        out = solve(capi, N, w, B, segs=4, **WEIGHTS)
        parity(capi, out, oracle_ref(oracle, ("weights", N), N, w, **WEIGHTS))


def test_fp32_scratch(oracle, capi, knob):
    """The float-scratch instantiation (F110QP_LANE_SEG_F32=1), S = 4, N = 20."""
    N, B = 20, 37
    knob("F110QP_LANE_SEG", "4")
    knob("F110QP_LANE_SEG_F32", "1")
    w = batch(B, N)
    s = lane(capi, N)
    assert s.lane_segments(B) == 4 and s.backend_info(B)[2] == 2  # LDS fp32
    s.close()
    parity(capi, solve(capi, N, w, B, segs=4), oracle_ref(oracle, ("box", N, B), N, w))


def test_against_the_sequential_kernel(capi, knob):
    """One start, B = 512, N = 20, S = 4 against F110QP_LANE_SEG=1: status equal, solutions within
    1e-6 relative, pass counts different on under 1 % of the QPs (test_segments_agree_with_sequential's
    bound). Measured share of QPs whose pass count differs on this batch, MI355X: parent (the ring)
    0 of 512, this kernel 0 of 512."""
    N, B = 20, 512
    knob("F110QP_LANE_TWIN", "0")
    w = batch(B, N, seed=9000)
    out = {}
    for seg in ("1", "4"):
        knob("F110QP_LANE_SEG", seg)
        out[seg] = solve(capi, N, w, B, segs=int(seg))
    a, b = out["1"], out["4"]
    np.testing.assert_array_equal(a[2], b[2])
    share = (a[3] != b[3]).mean()
    du, dx = rel_err(b[0], a[0].astype(np.float64)).max(), rel_err(b[1], a[1].astype(np.float64)).max()
    print(f"pass counts differ on {int((a[3] != b[3]).sum())} of {B} QPs ({share:.4f}); max rel diff u {du:.3e} x {dx:.3e}")
    assert du <= 1e-6 and dx <= 1e-6
    assert share < 0.01


def test_single_flip_pass_counts(oracle, capi, knob):
    """F110QP_LANE_KMAX=0 (single least-index flips from the first pass on), S = 4, N = 20, B = 300:
    the exact optimum, pass counts within 1 of the sequential kernel's."""
    N, B = 20, 300
    knob("F110QP_LANE_KMAX", "0")
    knob("F110QP_LANE_TWIN", "0")
    w = batch(B, N, seed=9100)
    knob("F110QP_LANE_SEG", "4")
    out = solve(capi, N, w, B, segs=4)
    parity(capi, out, oracle_ref(oracle, ("flip", N, B), N, w))
    knob("F110QP_LANE_SEG", "1")
    seq = solve(capi, N, w, B, segs=1)
    d = np.abs(out[3].astype(int) - seq[3].astype(int)).max()
    print(f"largest pass count difference {d}; passes up to {out[3].max()}")
    assert d <= 1


@pytest.mark.parametrize("B", [1, 37])
def test_route_identity(capi, knob, B):
    """F110QP_SEG_FIXEDQ=0 and 1 run the same segment-end code: status, iters, u and x bit-equal."""
    N = 20
    w = batch(B, N)
    out = {}
    for fq in ("0", "1"):
        knob("F110QP_SEG_FIXEDQ", fq)
        s = lane(capi, N)
        assert s.lane_segments(B) == 4 and s.lane_fixed_q(B) == (5 if fq == "1" else 0)
        out[fq] = s.solve(w["x0"], w["u_lin"], w["x_ref"])
        s.close()
    assert (out["1"][2] == capi.SOLVED).all()
    for k in (2, 3, 0, 1):
        np.testing.assert_array_equal(out["0"][k], out["1"][k])


@pytest.mark.parametrize("twin", ["0", "1"])
def test_non_finite_isolation(capi, knob, twin):
    """In every wave (16 QPs, 8 with twin starts) one QP has a NaN reference in segment 1 and another
    an infinite x0: they come back non-solved with NaN outputs, and every other QP of the batch is
    bit-equal to the batch without the bad values."""
    N, B = 20, 37
    knob("F110QP_LANE_SEG", "4")
    knob("F110QP_LANE_TWIN", twin)
    w = batch(B, N)
    clean = solve(capi, N, w, B, segs=4)
    nan_ref, inf_x0 = [2, 10, 18, 26, 33], [5, 13, 21, 29, 35]
    wb = {k: v.copy() for k, v in w.items()}
    wb["x_ref"][nan_ref, 7, 1] = np.nan  # stage 7: segment 1 of four five-stage segments
    wb["x0"][inf_x0, 0] = np.inf
    out = solve(capi, N, wb, B, segs=4)
    bad = np.array(sorted(nan_ref + inf_x0))
    good = np.setdiff1d(np.arange(B), bad)
    assert (out[2][bad] != capi.SOLVED).all()
    assert np.isnan(out[0][bad]).all() and np.isnan(out[1][bad]).all()
    assert (clean[2] == capi.SOLVED).all()
    for k in range(4):
        np.testing.assert_array_equal(out[k][good], clean[k][good])
