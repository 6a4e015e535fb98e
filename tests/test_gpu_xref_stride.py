"""Every solve route with x_ref_points > horizon (include/f110qp.h: x_ref [B][S][3], S >= N, only
points 0..N-1 of a row read: the layout MPC::Update gets, the planner's 50-point miniPath).

Each kernel that reads x_ref has its own row arithmetic (solve_kernel.h, gi64_kernel.h, the staging
walks of lane_kernel.h and lane_seg_kernel.h with its twin-start rows, the host staging of
f110qp_api.cpp), and with S == N a wrong row stride, a twin row offset off by two or a clamp in the
wrong row all read the right values. Here every route is solved three times with the same knobs:

    compact                      x_ref [B][N][3],  x_ref_points = 0
    strided, NaN padding         x_ref [B][P][3],  x_ref_points = P, rows N..P-1 all NaN
    strided, garbage padding     the same with rows N..P-1 = -7.0e3

and must give
  - bit-identical u, x, status, iters, obj, cost in all three (only the addressing differs; the
    compact call is first shown to reproduce itself bit for bit, NOT_BIT_REPRODUCIBLE lists the
    routes where it does not: none);
  - the oracle's statuses and exact optimum of x_ref[:, :N] (the oracle never sees the padding) at
    the tolerances the suite already uses for the route: 1e-4 relative on u and x (2e-6 where the
    Riccati scratch is fp32), obj at rtol / atol 1e-6, cost within 1e-6 max(1, cost) of
    oracle.tracking_cost;
  - the kernel the case is about: every case asserts the dispatch first (backend_info,
    lane_segments, lane_starts, gap_screen, last_recheck_count), so a case that resolves to another
    kernel fails.
Strides: P = N + 1 (the smallest that differs) and P = 50 (the planner's). Batches: 67 (16 and 8
QPs per wave, 32 without twin starts), 131 (64 per wave), 35 (S = 2 twin: 70 starts), so the last
wave is short and not alone; 1 once per back end. Horizons 7, 20, 25, 40, 47, 48: 3N = 21 .. 144
(64 / 3N = 3, 1, 0 in the staging walks), one and two register rows of the wave kernel, S dividing
N and not.

Routes: wave box PDAS; wave GI with gap rows (infeasible wedges included); the fp64 re-check alone;
the sequential lane kernel at 1 / 8 / 16 / 64 QPs per wave, LDS fp64 / LDS fp32 / HBM fp32 scratch,
both frames, with and without the fp64 reference array; the segmented kernel at S = 2 / 4 / 8, equal
and unequal segments, twin and single start, fp32 scratch, stored and refreshed gains; the gap-row
screen (fused SCR variants, twin and not, and the sequential kernel + gap_screen_kernel) with a QP
that goes on to GI; the grouped entry points; warm-started ticks; the device entry points. The
output canary at the end checks that a short last wave (twin starts double the virtual batch)
stores nothing past QP B - 1.

Knowingly not covered: the HBM-scratch path AUTO takes at 65,536 QPs is the F110QP_LANE_MODE=4
kernel run here, reached by size, not by another address; F110QP_LANE_MODE=2 / 3 and QPs per wave
2 / 4 / 32 share the staging code of the variants above; ROT and DREF have no introspection, the
knob is what selects them.
"""
import hashlib

import numpy as np
import pytest

from f110qp import workload
from test_gpu_parity import TOL, halfspaces_oracle, rel_err

pytestmark = pytest.mark.gpu

OUT = ("u", "x", "status", "iters", "obj", "cost")
PADDINGS = (("nan", np.nan), ("garbage", -7.0e3))
STRIDES = ("next", "planner")
F32_TOL = 2e-6  # fp32 Riccati scratch (test_segments_fp32_scratch, test_lane_backend_scratch_modes)
SEQ_TOL = 1e-6  # routes in NOT_BIT_REPRODUCIBLE only (test_segments_agree_with_sequential)
# routes whose compact call does not reproduce itself bit for bit (a finding, compared at SEQ_TOL)
NOT_BIT_REPRODUCIBLE = frozenset()
SENTINEL32, SENTINEL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def points(N, stride):
    return N + 1 if stride == "next" else 50


def strided(x_ref, P, fill):
    """x_ref [B][N][3] as the first N points of rows of P points, the rest `fill`."""
    B, N, _ = x_ref.shape
    assert P > N
    xs = np.full((B, P, 3), fill, np.float32)
    xs[:, :N] = x_ref
    return xs


def _canon(a):
    return np.nan_to_num(a, nan=7.0) if a.dtype.kind == "f" else a


def bits_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(_canon(p), _canon(q)) for p, q in zip(a, b))


def same_bits(got, want, what=""):
    """Every output of two runs equal element for element (NaN outputs in the same places)."""
    assert len(got) == len(want)
    for name, g, r in zip(OUT, got, want):
        if g.dtype.kind == "f":
            np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=f"{what}: NaNs of {name}")
        np.testing.assert_array_equal(_canon(g), _canon(r), err_msg=f"{what}: {name}")


def close_to(got, want, what=""):
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what}: status")
    ok = want[2] == 1
    for k in (0, 1):
        assert rel_err(got[k][ok], want[k][ok].astype(np.float64)).max() <= SEQ_TOL, (what, OUT[k])


_REF = {}


def oracle_ref(oracle, N, w, hs):
    """(u, x, status, obj, cost) of the oracle for a compact batch, solved once per batch."""
    h = hashlib.sha1()
    for a in (w["x0"], w["u_lin"], w["x_ref"]) + (() if hs is None else (hs,)):
        h.update(np.ascontiguousarray(a).tobytes())
    key = (N, hs is not None, h.hexdigest())
    if key not in _REF:
        prm = oracle.params(N)
        ur, xr, sr, obr = oracle.solve_batch(prm, w["x0"], w["u_lin"], w["x_ref"], hs, gap_active=hs is not None,
                                             objective=True)
        ref = (ur, xr, sr, obr, oracle.tracking_cost(prm, ur, xr, w["x_ref"]))
        for a in ref:
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def oracle_parity(oracle, N, out, ref, tol, what=""):
    ur, xr, sr = ref[:3]
    u, x, st = out[:3]
    assert (sr != oracle.UNCERTIFIED).all(), what
    np.testing.assert_array_equal(st, sr, err_msg=f"{what}: status")
    ok = sr == oracle.SOLVED
    assert ok.any(), what
    eu, ex = rel_err(u[ok], ur[ok]), rel_err(x[ok], xr[ok])
    print(f"{what}: rel err u {eu.max():.3e} x {ex.max():.3e} (tol {tol:g})")
    assert eu.max() <= tol, (what, eu.max(), int(np.argmax(eu)))
    assert ex.max() <= tol, (what, ex.max(), int(np.argmax(ex)))
    assert np.isnan(u[~ok]).all() and np.isnan(x[~ok]).all(), what
    if len(out) == 6 and len(ref) == 5:
        obj, cost = out[4:]
        obr, cr = ref[3:]
        np.testing.assert_allclose(obj[ok], obr[ok], rtol=1e-6, atol=1e-6, err_msg=f"{what}: obj")
        ec = np.abs(cost[ok] - cr[ok])
        assert (ec <= 1e-6 * np.maximum(1.0, cr[ok])).all(), (what, ec.max())
        assert np.isnan(obj[~ok]).all() and np.isnan(cost[~ok]).all(), what


def run_route(oracle, capi, route, N, P, w, hs=None, tol=TOL, proof=None, call=None, **cfg):
    """One route three ways (module docstring). proof(solver): the dispatch assertions, made on every
    solver before it solves; call(solver, x_ref) -> outputs (default: the host entry point with the
    objective outputs)."""
    cfg.setdefault("gap_mode", capi.GAP_ACTIVE if hs is not None else capi.GAP_INACTIVE)
    if call is None:
        def call(s, xr):
            return s.solve(w["x0"], w["u_lin"], xr, hs, objective=True)

    def one(pts, xr, twice=False):
        s = capi.Solver(capi.default_config(N, x_ref_points=pts, **cfg))
        try:
            if proof is not None:
                proof(s)
            out = call(s, xr)
            return (out, call(s, xr)) if twice else out
        finally:
            s.close()

    compact, again = one(0, w["x_ref"], twice=True)
    if route in NOT_BIT_REPRODUCIBLE:
        close_to(again, compact, f"{route}: compact twice")
    else:
        same_bits(again, compact, f"{route}: compact twice")
    runs = {}
    for name, fill in PADDINGS:
        runs[name] = one(P, strided(w["x_ref"], P, fill))
        what = f"{route} N={N} P={P} {name} padding against compact"
        if route in NOT_BIT_REPRODUCIBLE:
            close_to(runs[name], compact, what)
        else:
            same_bits(runs[name], compact, what)
    oracle_parity(oracle, N, runs["nan"], oracle_ref(oracle, N, w, hs), tol, f"{route} N={N} P={P}")
    return runs["nan"]


def box_batch(B, N, seed):
    """Hard references: many active bounds on both faces (test_segments_horizons)."""
    return workload.make_batch(B, N, seed=seed, heading="true", lateral=1.5, steer_range=1.0)


def plant_infeasible(w, hs):
    """Both wedges of test_oracle.infeasible_cases (a wall 0.5 m ahead; x0 outside the wedge)."""
    from test_oracle import infeasible_cases

    for i, (x0, h) in enumerate(infeasible_cases()):
        w["x0"][3 + 10 * i] = x0
        w["u_lin"][3 + 10 * i] = [4.5, 0.0]
        hs[3 + 10 * i] = h


def gap_batch(oracle, B, N, seed, infeasible=True):
    """test_gpu_screen._gap_batch, plus the infeasible wedges at QPs 3 and 13."""
    w = workload.make_batch(B, N, seed=seed)
    ranges, *geom = workload.make_scans(B, seed=seed)
    hs = halfspaces_oracle(oracle, w["x0"], ranges, geom)
    if infeasible:
        plant_infeasible(w, hs)
    return w, hs


def plant_wall(oracle, w, hs, b, N, dt=0.01):
    """QP b gets a wall across its heading at 3.75 N dt: the car covers 3 N dt .. 4.5 N dt along the
    heading (the linearised model advances v_k dt per stage along theta0), so the wall can be
    respected, and the box optimum, which follows a 4.5 m/s reference, runs through it: the screen
    must hand this QP to GI. Both facts are checked on the oracle."""
    x, y, th = (float(v) for v in w["x0"][b])
    c, s = np.cos(th), np.sin(th)
    w["u_lin"][b] = [4.5, 0.0]
    hs[b] = [-c, -s, c * x + s * y + 3.75 * N * dt]
    one = {k: w[k][b:b + 1] for k in ("x0", "u_lin", "x_ref")}
    _, xb, sb = oracle.solve_batch(oracle.params(N), one["x0"], one["u_lin"], one["x_ref"])
    row = hs[b, 0].astype(np.float64)
    assert sb[0] == oracle.SOLVED and (xb[0, :, :2] @ row[:2] + row[2]).min() < -0.05, "box optimum inside the wall"
    _, _, sg = oracle.solve_batch(oracle.params(N), one["x0"], one["u_lin"], one["x_ref"], hs[b:b + 1],
                                  gap_active=True)
    assert sg[0] == oracle.SOLVED, "the wall is reachable"


def is_wave(capi, B, grouped=False):
    def proof(s):
        assert s.backend_info(B, grouped) == (capi.BACKEND_WAVE, 1, 0)
        assert not s.gap_screen(B)
    return proof


def is_sequential(capi, B, qpw, scratch):
    def proof(s):
        assert s.test_build
        assert s.lane_segments(B) == 1 and s.lane_starts(B) == 1
        assert s.backend_info(B) == (capi.BACKEND_LANE, qpw, scratch)
    return proof


def is_segmented(capi, B, S, starts, scratch=1):
    def proof(s):
        assert s.lane_segments(B) == S
        assert s.lane_starts(B) == starts
        assert s.backend_info(B) == (capi.BACKEND_LANE, 64 // S, scratch)
    return proof


def is_screened(capi, B):
    def proof(s):
        assert s.test_build and s.gap_screen(B)
    return proof


# ---- 1. wave kernel, box PDAS -------------------------------------------------------------------

@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("N", [7, 20, 40, 48])
def test_wave_box(oracle, capi, N, stride):
    B = 67
    run_route(oracle, capi, "wave box", N, points(N, stride), box_batch(B, N, 3100 + N),
              proof=is_wave(capi, B), backend=capi.BACKEND_WAVE)


@pytest.mark.parametrize("backend", ["wave", "lane"])
def test_single_qp(oracle, capi, backend):
    """B = 1 (the zero-copy host staging): the wave kernel, and the lane back end's own choice for
    one QP (S = 4 at N = 20 by its instruction model, twin starts: two starts in one wave)."""
    N = 20
    proof = is_wave(capi, 1) if backend == "wave" else is_segmented(capi, 1, 4, 2)
    be = capi.BACKEND_WAVE if backend == "wave" else capi.BACKEND_LANE
    run_route(oracle, capi, f"{backend} B=1", N, 50, box_batch(1, N, 3201), proof=proof, backend=be)


# ---- 2. wave kernel, GI with gap rows -----------------------------------------------------------

@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("N", [20, 40])
def test_wave_gap_rows(oracle, capi, N, stride):
    B = 67
    w, hs = gap_batch(oracle, B, N, 3300 + N)
    out = run_route(oracle, capi, "wave GI", N, points(N, stride), w, hs, proof=is_wave(capi, B),
                    backend=capi.BACKEND_WAVE)
    assert (out[2][[3, 13]] == capi.PRIMAL_INFEASIBLE).all()


# ---- 3. the fp64 re-check alone -----------------------------------------------------------------

@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("N", [20, 40])
def test_recheck_alone(oracle, capi, knob, N, stride):
    knob("F110QP_RECHECK_ALL", 1)
    B = 67
    w, hs = gap_batch(oracle, B, N, 3400 + N)

    def call(s, xr):
        out = s.solve(w["x0"], w["u_lin"], xr, hs, objective=True)
        assert s.last_recheck_count() == B  # every QP answered by gi64_kernel.h
        return out

    def proof(s):
        assert s.test_build and not s.gap_screen(B)

    out = run_route(oracle, capi, "fp64 re-check", N, points(N, stride), w, hs, proof=proof, call=call)
    assert (out[2][[3, 13]] == capi.PRIMAL_INFEASIBLE).all()


# ---- 4. sequential lane kernel ------------------------------------------------------------------

# (QPs per wave, F110QP_LANE_MODE, batch, scratch at N = 20, scratch at N = 40): auto scratch is LDS
# fp64 where one wave's 80 N L bytes fit the CU's 160 KiB, else LDS fp32 (lane_launch.hip)
SEQ_CASES = [(1, 0, 67, 1, 1), (8, 0, 67, 1, 1), (64, 0, 131, 1, 2), (16, 1, 67, 1, 1), (16, 4, 67, 4, 4)]


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("N", [20, 40])
@pytest.mark.parametrize("qpw,mode,B,scr20,scr40", SEQ_CASES)
def test_sequential_lane(oracle, capi, knob, qpw, mode, B, scr20, scr40, N, stride):
    knob("F110QP_LANE_SEG", 1)
    knob("F110QP_LANE_QPW", qpw)
    knob("F110QP_LANE_MODE", mode)
    scratch = scr20 if N == 20 else scr40
    run_route(oracle, capi, f"sequential lane L={qpw} scratch={scratch}", N, points(N, stride),
              box_batch(B, N, 3500 + N + qpw), tol=F32_TOL if scratch in (2, 4) else TOL,
              proof=is_sequential(capi, B, qpw, scratch), backend=capi.BACKEND_LANE)


@pytest.mark.parametrize("name", ["F110QP_LANE_ROT", "F110QP_LANE_DREF"])
def test_sequential_lane_frame_and_references(oracle, capi, knob, name):
    """The general-frame kernel (ROT = 0) and the float references (DREF = 0: the staging is the
    reference array itself); ROT = 1 and DREF = 1 are the defaults of every case above."""
    knob("F110QP_LANE_SEG", 1)
    knob("F110QP_LANE_QPW", 16)
    knob(name, 0)
    N, B = 20, 67
    run_route(oracle, capi, f"sequential lane {name}=0", N, 50, box_batch(B, N, 3600),
              proof=is_sequential(capi, B, 16, 1), backend=capi.BACKEND_LANE)


# ---- 5. segmented lane kernel -------------------------------------------------------------------

SEG_EVEN = [(2, 20), (4, 20), (8, 40)]
SEG_UNEVEN = [(2, 25), (4, 25), (8, 25), (8, 47)]


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("twin", [1, 0])
@pytest.mark.parametrize("S,N", SEG_EVEN + SEG_UNEVEN)
def test_segmented_lane(oracle, capi, knob, S, N, twin, stride):
    """Twin starts stage one row per QP for two adjacent slots (rows from b0 >> 1, 8-element
    chunks); one start stages a row per slot. u_des = 4.5 = u_max: twin where not switched off."""
    knob("F110QP_LANE_SEG", S)
    knob("F110QP_LANE_TWIN", twin)
    B = 35 if (S == 2 and twin) else 67
    run_route(oracle, capi, f"segmented S={S} twin={twin}", N, points(N, stride), box_batch(B, N, 3700 + 10 * S + N),
              proof=is_segmented(capi, B, S, 2 if twin else 1), backend=capi.BACKEND_LANE)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("S,N", [(4, 20), (8, 40)])
def test_segmented_lane_fp32_scratch(oracle, capi, knob, S, N, stride):
    knob("F110QP_LANE_SEG", S)
    knob("F110QP_LANE_SEG_F32", 1)
    B = 67
    run_route(oracle, capi, f"segmented S={S} fp32", N, points(N, stride), box_batch(B, N, 3800 + N), tol=F32_TOL,
              proof=is_segmented(capi, B, S, 1, scratch=2), backend=capi.BACKEND_LANE)


@pytest.mark.parametrize("stride", STRIDES)
def test_segmented_lane_refresh_sweep(oracle, capi, knob, stride):
    """F110QP_LANE_DREF=0: the refresh sweep instead of the stored lam-gains (one start)."""
    knob("F110QP_LANE_SEG", 4)
    knob("F110QP_LANE_DREF", 0)
    N, B = 20, 67
    run_route(oracle, capi, "segmented S=4 refresh", N, points(N, stride), box_batch(B, N, 3900),
              proof=is_segmented(capi, B, 4, 1), backend=capi.BACKEND_LANE)


# ---- 6. gap-row screen --------------------------------------------------------------------------

# (horizon, knobs, segments of the screen's lane solve, its starts): AUTO splits N = 20 over 4 and
# N = 25 over 8 lanes at this batch (lane_segments' instruction model), with twin starts
SCREEN_CASES = [(20, {}, 4, 2), (25, {}, 8, 2), (20, {"F110QP_LANE_TWIN": 0}, 4, 1), (20, {"F110QP_LANE_SEG": 1}, 1, 1)]


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("N,knobs,S,starts", SCREEN_CASES)
def test_gap_screen(oracle, capi, knob, N, knobs, S, starts, stride):
    """The box solve of every QP on the lane kernel with the screen (the SCR variants of the
    segmented kernel; the sequential kernel + gap_screen_kernel with F110QP_LANE_SEG=1), GI on the
    wave kernel for the QPs it does not clear: QP 40's box optimum runs through its gap row, the
    wedges of QPs 3 and 13 are empty. The screen's lane solve takes the kernel a box-only lane
    solver with the same knobs reports."""
    knob("F110QP_GAP_SCREEN", 1)
    for k, v in knobs.items():
        knob(k, v)
    B = 67
    w, hs = gap_batch(oracle, B, N, 4000 + N)
    plant_wall(oracle, w, hs, 40, N)
    box = capi.Solver(capi.default_config(N, backend=capi.BACKEND_LANE))
    assert (box.lane_segments(B), box.lane_starts(B)) == (S, starts)
    box.close()

    out = run_route(oracle, capi, f"screen S={S} starts={starts}", N, points(N, stride), w, hs,
                    proof=is_screened(capi, B))
    assert out[2][40] == capi.SOLVED and (out[2][[3, 13]] == capi.PRIMAL_INFEASIBLE).all()


# ---- 7. grouped entry points --------------------------------------------------------------------

@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("backend,gap,N", [("wave", False, 20), ("wave", False, 40), ("lane", False, 20),
                                           ("lane", False, 40), ("wave", True, 20)])
def test_grouped(oracle, capi, backend, gap, N, stride):
    """Two scenarios of 120 candidates cut to 200 QPs (the second group short). Wave: W built once
    per group; lane: the groups are ignored (S = 4 at N = 20, 8 at N = 40 for 200 QPs); gap rows:
    every candidate sees its scenario's scan."""
    B = 200
    g = workload.make_grouped_batch(2, N, seed=4100 + N, heading="true")
    G = g["group_size"]
    w = {k: np.ascontiguousarray(g[k][:B]) for k in ("x0", "u_lin", "x_ref")}
    gid = (np.arange(B) // G).astype(np.int32)
    hs = None
    if gap:
        ranges, *geom = workload.make_scans(2, seed=4100)
        hs = np.ascontiguousarray(halfspaces_oracle(oracle, w["x0"][[0, G]], ranges, geom)[gid])

    def call(s, xr):
        return s.solve_grouped(w["x0"], w["u_lin"], xr, gid, 2, hs, objective=True)

    if backend == "wave":
        proof, be = is_wave(capi, B, grouped=True), capi.BACKEND_WAVE
    else:
        S = {20: 4, 40: 8}[N]
        be = capi.BACKEND_LANE

        def proof(s):
            assert s.backend_info(B, True)[:2] == (capi.BACKEND_LANE, 64 // S) and s.lane_segments(B) == S

    run_route(oracle, capi, f"grouped {backend}", N, points(N, stride), w, hs, proof=proof, call=call, backend=be)


# ---- 8. warm start ------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("backend", ["wave", "lane"])
def test_warm_start_ticks(oracle, capi, backend, stride):
    """Three ticks of the closed loop, the compact and the two strided solvers each with their own
    warm-start state: bit-identical tick by tick, every tick at the oracle's optimum."""
    N, B, T = 20, 67, 3
    P = points(N, stride)
    prm = oracle.params(N)
    ref = []

    def solve(x0, ul, xr):
        u, x, st = oracle.solve_batch(prm, x0, ul, xr)
        ref.append((u, x, st))
        return u

    ticks = workload.closed_loop_stream(solve, B, N, T, seed=57)
    be = capi.BACKEND_WAVE if backend == "wave" else capi.BACKEND_LANE
    proof = is_wave(capi, B) if backend == "wave" else is_segmented(capi, B, 4, 2)
    solvers = {name: capi.Solver(capi.default_config(N, warm_start=1, backend=be, x_ref_points=pts))
               for name, pts in (("compact", 0), ("nan", P), ("garbage", P))}
    fills = dict(PADDINGS)
    try:
        for s in solvers.values():
            proof(s)
        for t, w in enumerate(ticks):
            out = {name: s.solve(w["x0"], w["u_lin"], w["x_ref"] if name == "compact" else
                                 strided(w["x_ref"], P, fills[name]), objective=True)
                   for name, s in solvers.items()}
            for name in fills:
                same_bits(out[name], out["compact"], f"warm {backend} tick {t} {name} padding")
            oracle_parity(oracle, N, out["nan"], ref[t], TOL, f"warm {backend} tick {t}")
    finally:
        for s in solvers.values():
            s.close()


# ---- 9. device entry points and the output canary -----------------------------------------------

def solve_on_device(cuda, s, w, xr, hs, extra=0, sync=False, objective=True):
    """f110qp_solve_batch[_ex]_dev (sync: the _dev_sync launcher, no objective outputs) on output
    buffers of B + extra QPs pre-filled with a sentinel bit pattern, of which the call gets the
    first-B view. Returns the outputs of the B QPs; asserts the extra QPs' worth of every buffer
    still holds the pattern."""
    import torch

    N, B = s.horizon, w["x0"].shape[0]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(cuda)  # noqa: E731
    x0, ul, xrd, hsd = dev(w["x0"]), dev(w["u_lin"]), dev(xr), dev(hs)
    shapes = dict(u=((N, 2), torch.float32), x=((N + 1, 3), torch.float32), status=((), torch.int32),
                  iters=((), torch.int32), obj=((), torch.float64), cost=((), torch.float64))
    if sync or not objective:
        del shapes["obj"], shapes["cost"]
    full, raw = {}, {}
    for k, (shp, dt) in shapes.items():
        full[k] = torch.empty((B + extra,) + shp, dtype=dt, device=cuda)
        raw[k] = full[k].view(torch.int64 if dt == torch.float64 else torch.int32)
        raw[k].fill_(SENTINEL64 if dt == torch.float64 else SENTINEL32)
    v = {k: t[:B] for k, t in full.items()}
    if sync:
        s.prepare_dev(x0, ul, xrd, hsd, v["u"], v["x"], v["status"], v["iters"], sync=True)()
    else:
        s.solve_dev(x0, ul, xrd, hsd, v["u"], v["x"], v["status"], v["iters"], obj=v.get("obj"), cost=v.get("cost"))
        torch.cuda.synchronize()
    for k, r in raw.items():
        tail = r[B:].cpu().numpy()
        assert (tail == (SENTINEL64 if r.dtype == torch.int64 else SENTINEL32)).all(), f"{k} written past QP {B - 1}"
    return tuple(v[k].cpu().numpy() for k in shapes)


@pytest.mark.parametrize("sync", [False, True])
def test_device_entry_points(oracle, capi, cuda, sync):
    """f110qp_solve_batch_ex_dev and the f110qp_solve_batch_dev_sync launcher, AUTO back end (the
    wave kernel at 67 QPs of N = 20), P = 50."""
    N, B = 20, 67
    w = box_batch(B, N, 4300)

    def call(s, xr):
        return solve_on_device(cuda, s, w, xr, None, sync=sync)

    run_route(oracle, capi, "device sync" if sync else "device async", N, 50, w, proof=is_wave(capi, B), call=call)


# route: (batch, knobs, back end, dispatch assertions)
CANARY = {
    "wave": (67, {}, "wave", is_wave),
    "sequential": (131, {"F110QP_LANE_SEG": 1, "F110QP_LANE_QPW": 64}, "lane", lambda c, B: is_sequential(c, B, 64, 1)),
    "segmented": (67, {"F110QP_LANE_SEG": 4, "F110QP_LANE_TWIN": 0}, "lane", lambda c, B: is_segmented(c, B, 4, 1)),
    "twin": (67, {"F110QP_LANE_SEG": 4, "F110QP_LANE_TWIN": 1}, "lane", lambda c, B: is_segmented(c, B, 4, 2)),
    "screen": (67, {"F110QP_GAP_SCREEN": 1}, "auto", is_screened),
}


@pytest.mark.parametrize("route", sorted(CANARY))
def test_outputs_end_at_the_batch(oracle, capi, cuda, knob, route):
    """A short last wave must not store for its duplicate lanes, and twin starts double the virtual
    batch: 64 QPs' worth of every output buffer behind QP B - 1 keeps its sentinel (checked in
    solve_on_device), and the B QPs in front are the host entry point's, bit for bit."""
    B, knobs, backend, proof = CANARY[route]
    for k, val in knobs.items():
        knob(k, val)
    N = 20
    if route == "screen":
        w, hs = gap_batch(oracle, B, N, 4400)
    else:
        w, hs = box_batch(B, N, 4400), None
    be = {"wave": capi.BACKEND_WAVE, "lane": capi.BACKEND_LANE, "auto": capi.BACKEND_AUTO}[backend]
    s = capi.Solver(capi.default_config(N, backend=be, gap_mode=capi.GAP_INACTIVE if hs is None else capi.GAP_ACTIVE))
    try:
        proof(capi, B)(s)
        got = solve_on_device(cuda, s, w, w["x_ref"], hs, extra=64)
        host = s.solve(w["x0"], w["u_lin"], w["x_ref"], hs, objective=True)
    finally:
        s.close()
    same_bits(got, host, f"canary {route}: device against host entry point")
    oracle_parity(oracle, N, got, oracle_ref(oracle, N, w, hs), TOL, f"canary {route}")
