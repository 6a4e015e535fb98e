"""The segmented lane kernel after its per-pass instruction trim (csrc/lane_seg_kernel.h: the stage's
accumulations as FMA chains on the accumulator in every instantiation; in the fixed-length kernels the
PDAS passes collect the re-guessed state codes in a word of their own and test `changed` once per
sweep) against the CPU oracle at test_gpu_seg.py's tolerance, against the sequential lane kernel's
pass counts, and route to route (F110QP_SEG_FIXEDQ=0 / 1: the shared text keeps them bit-identical).

Pass counts: one start against the sequential kernel (F110QP_LANE_SEG=1) runs the same PDAS iterates up
to fp64 rounding (a pass differs by ~1e-15 relative, the flip tolerances are 1e-10), so the counts are
equal; with twin starts a QP finishes with the quicker of the cold start and the twin one, so its count
is at most the sequential kernel's. fp32 scratch rounds the gains to ~1e-7 and settles degenerate bounds
in single flips: within one pass (the bound of test_gpu_seg_ends.test_single_flip_pass_counts).

The oracle's answer for a batch is computed once and shared (test_gpu_seg_ends's cache and batches)."""
import numpy as np
import pytest

from test_gpu_parity import TOL, rel_err
from test_gpu_seg_ends import WEIGHTS, batch, lane, oracle_ref, parity, solve

pytestmark = pytest.mark.gpu

_seq = {}


def sequential(capi, knob, key, N, w, B, **cfg):
    """The sequential lane kernel's answer for a batch (one start), computed once."""
    if key not in _seq:
        knob("F110QP_LANE_SEG", "1")
        _seq[key] = solve(capi, N, w, B, segs=1, **cfg)
    return _seq[key]


def routes(capi, knob, N, w, B, call=None, **cfg):
    """(fixed-length, run-time-length) answers of an N = 20, S = 4 batch; the route asserted."""
    out = {}
    for fq in ("1", "0"):
        knob("F110QP_SEG_FIXEDQ", fq)
        s = lane(capi, N, **cfg)
        assert s.lane_segments(B) == 4 and s.lane_fixed_q(B) == (5 if fq == "1" else 0)
        out[fq] = call(s) if call else s.solve(w["x0"], w["u_lin"], w["x_ref"])
        s.close()
    return out["1"], out["0"]


def bit_equal(a, b):
    for k in (2, 3, 0, 1):
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize("twin", ["1", "0"])
@pytest.mark.parametrize("B", [1, 5, 37])
def test_fixed_length_route(oracle, capi, knob, B, twin):
    N = 20
    w = batch(B, N)
    knob("F110QP_LANE_TWIN", twin)
    new, old = routes(capi, knob, N, w, B)
    bit_equal(new, old)
    parity(capi, new, oracle_ref(oracle, ("box", N, B), N, w))
    seq = sequential(capi, knob, ("box", N, B), N, w, B)
    print(f"passes: segmented up to {new[3].max()}, sequential up to {seq[3].max()}")
    if twin == "0":
        np.testing.assert_array_equal(new[3], seq[3])
    else:
        assert (new[3] <= seq[3]).all()


@pytest.mark.parametrize("S,N", [(4, 8), (2, 10), (4, 22)])
def test_short_and_uneven_segments(oracle, capi, knob, S, N):
    """Two-stage segments, five-stage segments at S = 2, and 22 = 6 + 6 + 5 + 5."""
    B = 5
    knob("F110QP_LANE_TWIN", "0")
    knob("F110QP_LANE_SEG", S)
    w = batch(B, N)
    out = solve(capi, N, w, B, segs=S)
    parity(capi, out, oracle_ref(oracle, ("box", N, B), N, w))
    np.testing.assert_array_equal(out[3], sequential(capi, knob, ("box", N, B), N, w, B)[3])


def test_general_frame(oracle, capi, knob):
    """q0 != q1: the general-frame instantiation (u_des inside its box: one start)."""
    N, B = 20, 5
    knob("F110QP_LANE_SEG", "4")
    w = batch(B, N, seed=8900)
    out = solve(capi, N, w, B, segs=4, **WEIGHTS)
    parity(capi, out, oracle_ref(oracle, ("weights5", N), N, w, **WEIGHTS))
    np.testing.assert_array_equal(out[3], sequential(capi, knob, ("weights5", N), N, w, B, **WEIGHTS)[3])


def test_fp32_scratch(oracle, capi, knob):
    N, B = 20, 5
    knob("F110QP_LANE_TWIN", "0")
    knob("F110QP_LANE_SEG", "4")
    knob("F110QP_LANE_SEG_F32", "1")
    w = batch(B, N)
    s = lane(capi, N)
    assert s.lane_segments(B) == 4 and s.backend_info(B)[2] == 2  # LDS fp32
    s.close()
    out = solve(capi, N, w, B, segs=4)
    parity(capi, out, oracle_ref(oracle, ("box", N, B), N, w))
    seq = sequential(capi, knob, ("box", N, B), N, w, B)
    assert np.abs(out[3].astype(int) - seq[3].astype(int)).max() <= 1


# ---- every input-state code at every stage position of a five-stage segment ----
TIGHT = dict(u_min=[3.9, -0.05], u_max=[4.1, 0.1])  # tight, the steer box asymmetric
CODES = (0, 1, 2, 4, 5, 6, 8, 9, 10)                # input 0's state | input 1's << 2 (0 free, 1 lower, 2 upper)


def pdas_model(oracle, prm, x0, ul, xr, N, kmax=16, max_pass=60):
    """numpy fp64 model of the lane kernels' PDAS on one box QP from the cold start (lane_kernel.h's rule:
    a free input outside its box by 1e-10 (1 + |bound|) goes to that bound, a bound input whose
    multiplier has the wrong sign by 1e-10 (1 + r |bound - u_des|_max) is freed; every violation flips
    in a pass before kmax, then the least index only). Returns (passes, {(stage mod 5, code)} of the
    codes every pass started from)."""
    A, Bm, C = oracle.linearize(x0[2], ul[0], ul[1], float(np.float32(prm.dt)))
    Q, R = np.diag([prm.q[i] for i in range(3)]), np.diag([prm.r[i] for i in range(2)])
    ud = np.array([prm.u_des[0], prm.u_des[1]], float)
    lo = np.array([np.float32(prm.u_min[i]) for i in range(2)], float)
    hi = np.array([np.float32(prm.u_max[i]) for i in range(2)], float)
    ref, x0 = xr[:N].astype(float), x0.astype(float)
    gtol = 1e-10 * (1.0 + np.array([R[a, a] * max(abs(lo[a] - ud[a]), abs(hi[a] - ud[a])) for a in range(2)]))
    st, seen = np.zeros((N, 2), int), set()
    for p in range(max_pass):
        seen |= {(i % 5, int(st[i, 0] | (st[i, 1] << 2))) for i in range(N)}
        P, pv = Q.copy(), -Q @ ref[N - 1]
        Ks, ks = [None] * N, [None] * N
        for i in range(N - 1, -1, -1):  # the masked Riccati sweep
            g = P @ C + pv
            H, X = R + Bm.T @ P @ Bm, Bm.T @ P @ A
            fr, inv = st[i] == 0, np.zeros((2, 2))
            if fr.all():
                inv = np.linalg.inv(H)
            elif fr[0]:
                inv[0, 0] = 1 / H[0, 0]
            elif fr[1]:
                inv[1, 1] = 1 / H[1, 1]
            bA = np.where(st[i] == 1, lo, np.where(st[i] == 2, hi, 0.0))
            Ks[i], ks[i] = -inv @ X, bA - inv @ (-R @ ud + Bm.T @ g + H @ bA)
            P, pv = Q + A.T @ P @ A + X.T @ Ks[i], -Q @ ref[i] + A.T @ g + X.T @ ks[i]
        x, us, xs = x0.copy(), [], [x0.copy()]
        for i in range(N):
            us.append(Ks[i] @ x + ks[i])
            x = A @ x + Bm @ us[i] + C
            xs.append(x)
        lam, new = Q @ (xs[N] - ref[N - 1]), st.copy()
        for i in range(N - 1, -1, -1):  # the re-guess from u and the multipliers
            g = R @ (us[i] - ud) + Bm.T @ lam
            for a in range(2):
                if st[i, a] == 0:
                    new[i, a] = 1 if us[i][a] < lo[a] - 1e-10 * (1 + abs(lo[a])) else (
                        2 if us[i][a] > hi[a] + 1e-10 * (1 + abs(hi[a])) else 0)
                elif st[i, a] == 1:
                    new[i, a] = 1 if g[a] > -gtol[a] else 0
                else:
                    new[i, a] = 2 if g[a] < gtol[a] else 0
            lam = Q @ (xs[i] - ref[i]) + A.T @ lam
        if p >= kmax:
            d, one = np.flatnonzero(new.reshape(-1) != st.reshape(-1)), st.copy().reshape(-1)
            if len(d):
                one[d[0]] = new.reshape(-1)[d[0]]
            new = one.reshape(N, 2)
        if (new == st).all():
            return p + 1, seen
        st = new
    return max_pass, seen


@pytest.mark.parametrize("u_des", [[4.1, 0.02], [4.0, 0.02]], ids=["u_des_on_bound", "u_des_inside"])
def test_every_code_at_every_stage_position(oracle, capi, knob, u_des):
    """48 QPs in a tight, asymmetric box far from their references: by the numpy model every one of the
    nine state codes is the input code of every one of the five stage positions of a segment in some
    pass (asserted, so an easy batch cannot pass), and the kernels take the model's pass counts."""
    N, B = 20, 48
    over = dict(TIGHT, u_des=u_des)
    w = batch(B, N, seed=9300)
    prm = oracle.params(N, **over)
    seen, passes = set(), []
    for b in range(B):
        it, s = pdas_model(oracle, prm, w["x0"][b], w["u_lin"][b], w["x_ref"][b], N)
        seen |= s
        passes.append(it)
    missing = [(t, c) for t in range(5) for c in CODES if (t, c) not in seen]
    assert not missing, missing
    knob("F110QP_LANE_TWIN", "0")  # the model's cold start
    new, old = routes(capi, knob, N, w, B, **over)
    bit_equal(new, old)
    parity(capi, new, oracle_ref(oracle, ("tight", tuple(u_des)), N, w, **over))
    print(f"passes up to {new[3].max()} (model {max(passes)})")
    np.testing.assert_array_equal(new[3], np.array(passes))
    np.testing.assert_array_equal(new[3], sequential(capi, knob, ("tight", tuple(u_des)), N, w, B, **over)[3])


@pytest.mark.parametrize("max_iter", [3, 60])
def test_single_flip_passes_restore_the_state_word(oracle, capi, knob, max_iter):
    """F110QP_LANE_KMAX=1: every pass after the first is a single-flip pass (pass >= kmax), where the
    segments that did not hold the QP's first flip put the replaced code back into the state word.
    max_iter = 3 ends most QPs on the pass budget (MAX_ITER, the state word mid-way), 60 lets all
    finish: both routes bit-equal and the sequential kernel's status and pass counts."""
    N, B = 20, 37
    knob("F110QP_LANE_KMAX", "1")
    knob("F110QP_LANE_TWIN", "0")
    w = batch(B, N)
    new, old = routes(capi, knob, N, w, B, max_iter=max_iter)
    bit_equal(new, old)
    seq = sequential(capi, knob, ("flip", max_iter), N, w, B, max_iter=max_iter)
    np.testing.assert_array_equal(new[2], seq[2])
    np.testing.assert_array_equal(new[3], seq[3])
    ok = new[2] == capi.SOLVED
    assert new[3].max() > 2 and (ok.all() if max_iter == 60 else not ok.all())
    ref = oracle_ref(oracle, ("box", N, B), N, w)
    assert rel_err(new[0][ok], ref[0][ok]).max() <= TOL and rel_err(new[1][ok], ref[1][ok]).max() <= TOL


def test_warm_start_pair(oracle, capi, knob):
    """Two calls on the same inputs with warm_start = 1 at B = 5: the second is seeded from the state
    word the first wrote back on every QP and gives the first call's answer in no more passes."""
    N, B = 20, 5
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
    for k in (2, 0, 1):
        np.testing.assert_array_equal(new[1][k], new[0][k])
    assert (new[1][3] <= new[0][3]).all()
    parity(capi, new[1], oracle_ref(oracle, ("box", N, B), N, w))
