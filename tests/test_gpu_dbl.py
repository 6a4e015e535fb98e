"""The double-precision input entry points (f110qp_solve_*_dbl) against the CPU oracle on doubles.

Inputs: a workload.make_batch batch as float64, (x, y) of x0 and x_ref shifted by `shift` metres,
then uniform offsets of up to +- half a float32 ulp on every entry of x0, x_ref and u_lin (fixed
seed): doubles that no float32 holds. Expected: a per-QP loop of oracle.solve on those doubles (gap
rows: oracle.find_half_spaces on the double state, stored as float32, as the ABI takes them).

Bounds (set by the feature's specification, not by what the kernels give):
    u: |u - u*|_inf / max(1, |u*|_inf) <= 2e-6   (the project's tightest cross-variant bound)
    x: |x - x*| <= 2e-6 max(1, |x* - x0|_inf) + 1/2 spacing(float32(|x*|)) elementwise (the second
       term is the documented float32 rounding of the absolute x_out)
    status equal to the oracle's for every QP.
Seeds: every (seed, shift, gap) used here was checked on the CPU to hold no QP whose oracle status
differs between the doubles and the doubles moved by one float64 ulp (box rows: 99, 7, 21-29, 31-33,
41-43, 51, 61, 71, 81, 91; gap rows: 17, 18).
"""
import functools

import numpy as np
import pytest
from test_gpu_parity import halfspaces_oracle

from f110qp import workload

pytestmark = pytest.mark.gpu

U_TOL = 2e-6


def dbl_batch(B, N, seed, shift, P=None):
    """float64 (x0, u_lin, x_ref [B][P or N][3]) as described in the module docstring; rows N..P-1 of
    a padded x_ref are NaN (never read)."""
    w = workload.make_batch(B, N, seed=seed)
    x0, ul, xr = (w[k].astype(np.float64) for k in ("x0", "u_lin", "x_ref"))
    x0[:, :2] += shift
    xr[:, :, :2] += shift
    rng = np.random.default_rng(seed + 1)

    def jitter(a):
        ulp = np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
        return a + rng.uniform(-0.5, 0.5, a.shape) * ulp

    x0, xr, ul = jitter(x0), jitter(xr), jitter(ul)
    if P is not None and P > N:
        xr = np.concatenate([xr, np.full((B, P - N, 3), np.nan)], 1)
    return np.ascontiguousarray(x0), np.ascontiguousarray(ul), np.ascontiguousarray(xr)


_cache = {}


def expected(oracle, B, N, seed, shift, gap=False, P=None):
    """(x0, u_lin, x_ref, hs, u*, x*, status*, obj*) of a dbl_batch, computed once per case."""
    key = (B, N, seed, shift, gap, P)
    if key not in _cache:
        x0, ul, xr = dbl_batch(B, N, seed, shift, P)
        hs = None
        if gap:
            ranges, amin, ainc, amax = workload.make_scans(B, seed=seed + 2)
            hs = halfspaces_oracle(oracle, x0, ranges, (amin, ainc, amax))
        prm = oracle.params(N)
        us, xs, st, ob = np.zeros((B, N, 2)), np.zeros((B, N + 1, 3)), np.zeros(B, np.int32), np.zeros(B)
        for b in range(B):
            r = oracle.solve(prm, x0[b], ul[b], xr[b, :N], None if hs is None else hs[b], gap)
            us[b], xs[b], st[b], ob[b] = r["u"], r["x"], r["status"], r["obj"]
        for a in (x0, ul, xr, us, xs, st, ob):
            a.setflags(write=False)
        _cache[key] = (x0, ul, xr, hs, us, xs, st, ob)
    return _cache[key]


def u_err(u, us):
    return np.abs(u.astype(np.float64) - us).max(axis=(1, 2)) / np.maximum(1.0, np.abs(us).max(axis=(1, 2)))


def assert_parity(capi, oracle, out, exp, what=""):
    u, x, st = out[0], out[1], out[2]
    x0, _, _, _, us, xs, sts, _ = exp
    np.testing.assert_array_equal(st, sts, err_msg=what)
    ok = sts == oracle.SOLVED
    assert ok.any()
    eu = u_err(u[ok], us[ok])
    print(f"{what}: max u err {eu.max():.3e} over {int(ok.sum())} QPs")
    assert eu.max() <= U_TOL, (what, eu.max(), int(np.argmax(eu)))
    span = np.maximum(1.0, np.abs(xs[ok] - x0[ok][:, None, :]).max(axis=(1, 2)))[:, None, None]
    bound = U_TOL * span + 0.5 * np.spacing(np.abs(xs[ok]).astype(np.float32)).astype(np.float64)
    ex = np.abs(x[ok].astype(np.float64) - xs[ok])
    assert (ex <= bound).all(), (what, float((ex - bound).max()))
    if (~ok).any():
        assert np.isnan(u[~ok]).all() and np.isnan(x[~ok]).all()


def solver(capi, N, gap=False, **cfg):
    return capi.Solver(capi.default_config(N, gap_mode=capi.GAP_ACTIVE if gap else capi.GAP_INACTIVE, **cfg))


def solve_dbl(capi, N, exp, gap=False, objective=False, proof=None, **cfg):
    s = solver(capi, N, gap, **cfg)
    if proof:
        proof(s)
    out = s.solve_dbl(exp[0], exp[1], exp[2], exp[3], objective=objective)
    s.close()
    return out


# ---- 1. the discriminating test ------------------------------------------------------------------

def test_dbl_meets_the_bound_where_the_float_call_cannot(oracle, capi):
    """256 x N = 20, seed 99, 1 km from the origin, AUTO: the _dbl call meets the bound on all 256
    QPs; the float call on the same inputs rounded to float32 misses the u bound on at least half of
    them (the CPU probe of the rounding alone: 256 of 256)."""
    B, N = 256, 20
    exp = expected(oracle, B, N, 99, 1000.0)
    assert_parity(capi, oracle, solve_dbl(capi, N, exp), exp, "dbl +1000 m")
    s = solver(capi, N)
    u32, _, st32, _ = s.solve(exp[0], exp[1], exp[2])  # (solve() narrows to float32)
    s.close()
    eu = u_err(u32, exp[4])
    print(f"float call on rounded inputs: median {np.median(eu):.3e} max {eu.max():.3e}, over bound {(eu > U_TOL).sum()}")
    assert (eu > U_TOL).sum() >= B // 2


@pytest.mark.parametrize("shift", [50.0, -50.0])
def test_dbl_near_the_origin(oracle, capi, shift):
    exp = expected(oracle, 256, 20, 99, shift)
    assert_parity(capi, oracle, solve_dbl(capi, 20, exp), exp, f"dbl {shift:+} m")


# ---- 2. route matrix at +1000 m ------------------------------------------------------------------

def _is_wave(capi, B):
    return lambda s: s.backend_info(B) == (capi.BACKEND_WAVE, 1, 0) or pytest.fail("not the wave back end")


@pytest.mark.parametrize("N", [5, 20, 33])
def test_route_wave_box(oracle, capi, N):
    B = 7
    exp = expected(oracle, B, N, 20 + N % 10, 1000.0)
    out = solve_dbl(capi, N, exp, backend=capi.BACKEND_WAVE, proof=_is_wave(capi, B))
    assert_parity(capi, oracle, out, exp, f"wave box N={N}")


def test_route_wave_gap_rows(oracle, capi):
    B, N = 16, 20
    exp = expected(oracle, B, N, 17, 1000.0, gap=True)
    out = solve_dbl(capi, N, exp, gap=True, backend=capi.BACKEND_WAVE)
    assert_parity(capi, oracle, out, exp, "wave GI")


@pytest.mark.parametrize("B,N,S,twin,f32", [(5, 20, 4, 0, 0), (5, 20, 4, 1, 0), (3, 40, 8, 1, 0), (5, 20, 4, 0, 1)])
def test_route_segmented_lane(oracle, capi, knob, B, N, S, twin, f32):
    knob("F110QP_LANE_SEG", S)
    knob("F110QP_LANE_TWIN", twin)
    if f32:
        knob("F110QP_LANE_SEG_F32", 1)

    def proof(s):
        assert s.test_build and s.lane_segments(B) == S
        assert s.lane_starts(B) == (2 if twin and not f32 else 1)
        assert s.backend_info(B)[2] == (2 if f32 else 1)

    exp = expected(oracle, B, N, 31 + (S == 8), 1000.0)
    out = solve_dbl(capi, N, exp, backend=capi.BACKEND_LANE, proof=proof)
    assert_parity(capi, oracle, out, exp, f"segmented S={S} twin={twin} f32={f32}")


@pytest.mark.parametrize("dref", [0, 1])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("qpw,B", [(64, 70), (1, 3)])
def test_route_sequential_lane(oracle, capi, knob, qpw, B, mode, dref):
    """lane_kernel.h, every scratch placement x fp64 / float references in LDS; 64 QPs per wave with
    a part-filled second wave, and one QP per wave."""
    N = 20
    knob("F110QP_LANE_SEG", 1)
    knob("F110QP_LANE_QPW", qpw)
    knob("F110QP_LANE_MODE", mode)
    knob("F110QP_LANE_DREF", dref)

    def proof(s):
        assert s.test_build and s.lane_segments(B) == 1
        assert s.backend_info(B) == (capi.BACKEND_LANE, qpw, mode)

    exp = expected(oracle, B, N, 41 + (qpw == 1), 1000.0)
    out = solve_dbl(capi, N, exp, backend=capi.BACKEND_LANE, proof=proof)
    assert_parity(capi, oracle, out, exp, f"sequential L={qpw} mode={mode} dref={dref}")


def test_route_gap_screen_and_recheck(oracle, capi, knob):
    """Gap rows, 64 QPs: the box screen on the lane kernel + GI, and the fp64 re-check alone."""
    B, N = 64, 20
    exp = expected(oracle, B, N, 18, 1000.0, gap=True)
    knob("F110QP_GAP_SCREEN", 1)
    out = solve_dbl(capi, N, exp, gap=True, proof=lambda s: s.gap_screen(B) or pytest.fail("no screen"))
    assert_parity(capi, oracle, out, exp, "gap screen")
    knob("F110QP_GAP_SCREEN", 0)
    knob("F110QP_RECHECK_ALL", 1)
    s = solver(capi, N, True)
    out = s.solve_dbl(exp[0], exp[1], exp[2], exp[3])
    assert s.last_recheck_count() == B
    s.close()
    assert_parity(capi, oracle, out, exp, "fp64 re-check")


# ---- 3. x_ref_points > horizon -------------------------------------------------------------------

@pytest.mark.parametrize("route", ["wave", "lane", "segmented"])
def test_x_ref_points_above_horizon(oracle, capi, knob, route):
    B, N, P = 9, 20, 50
    exp = expected(oracle, B, N, 51, 1000.0, P=P)
    if route == "lane":
        knob("F110QP_LANE_SEG", 1)
    if route == "segmented":
        knob("F110QP_LANE_SEG", 4)
    be = capi.BACKEND_WAVE if route == "wave" else capi.BACKEND_LANE
    out = solve_dbl(capi, N, exp, backend=be, x_ref_points=P,
                    proof=lambda s: route == "wave" or s.lane_segments(B) == (4 if route == "segmented" else 1)
                    or pytest.fail("route"))
    assert_parity(capi, oracle, out, exp, f"P=50 {route}")


# ---- 4. entry points -----------------------------------------------------------------------------

@pytest.mark.parametrize("B", [64, 65])
def test_host_entry_zero_copy_and_staged(oracle, capi, B):
    """B = 64: zero-copy pinned staging with 8-byte input fields; B = 65: staged through device
    memory. obj / cost against the oracle's objective and the tracking cost of its solution, at the
    float *_ex tolerances (test_gpu_parity.py::test_objective_matches_oracle)."""
    N = 20
    exp = expected(oracle, B, N, 61, 1000.0)
    s = solver(capi, N)
    n0 = s.sync_signals()
    u, x, st, it, ob, co = s.solve_dbl(exp[0], exp[1], exp[2], objective=True)
    assert s.sync_signals() - n0 == (1 if B <= 64 else 0)
    s.close()
    assert_parity(capi, oracle, (u, x, st), exp, f"host B={B}")
    np.testing.assert_allclose(ob, exp[7], rtol=1e-6, atol=1e-6)
    cr = oracle.tracking_cost(oracle.params(N), exp[4], exp[5], exp[2])
    assert (np.abs(co - cr) <= 1e-6 * np.maximum(1.0, cr)).all(), np.abs(co - cr).max()


def _dev_buffers(torch, cuda, exp, B, N):
    t = lambda a: torch.from_numpy(a.copy()).to(cuda)  # noqa: E731
    return (t(exp[0]), t(exp[1]), t(exp[2]), torch.empty((B, N, 2), dtype=torch.float32, device=cuda),
            torch.empty((B, N + 1, 3), dtype=torch.float32, device=cuda),
            torch.empty(B, dtype=torch.int32, device=cuda))


def test_dev_entry_on_a_stream_and_dev_sync(oracle, capi, cuda):
    import torch

    B, N = 33, 20
    exp = expected(oracle, B, N, 71, 1000.0)
    x0, ul, xr, uo, xo, st = _dev_buffers(torch, cuda, exp, B, N)
    ob = torch.empty(B, dtype=torch.float64, device=cuda)
    s = solver(capi, N)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    s.solve_dev_dbl(x0, ul, xr, None, uo, xo, st, stream=side, obj=ob)
    side.synchronize()
    assert_parity(capi, oracle, (uo.cpu().numpy(), xo.cpu().numpy(), st.cpu().numpy()), exp, "dev_dbl on a stream")
    np.testing.assert_allclose(ob.cpu().numpy(), exp[7], rtol=1e-6, atol=1e-6)
    uo.zero_(); xo.zero_(); st.zero_()
    torch.cuda.synchronize(cuda)
    n0 = s.sync_signals()
    s.solve_dev_dbl(x0, ul, xr, None, uo, xo, st, sync=True)
    assert s.sync_signals() == n0 + 1
    out = (uo.cpu().numpy(), xo.cpu().numpy(), st.cpu().numpy())
    s.close()
    assert_parity(capi, oracle, out, exp, "dev_sync_dbl")


# ---- 5. grouped ----------------------------------------------------------------------------------

def test_grouped_key_compares_the_full_doubles(oracle, capi, cuda):
    """4 scenarios on the wave back end; scenarios 0 and 1 share every input except theta0, which is
    the same float32 and a different double in the two, and carry the same group id: the group's W
    belongs to scenario 0's members only, and a key that compared narrowed bits would hand it to
    scenario 1's. Every QP must match its own oracle solve; host and device entry points."""
    import torch

    N = 20
    w = workload.make_grouped_batch(4, N, seed=81, lanes=(0.0, 0.25), steers=3)
    G = w["group_size"]
    B = 4 * G
    x0, ul, xr = (w[k].astype(np.float64) for k in ("x0", "u_lin", "x_ref"))
    x0[:, :2] += 1000.0
    xr[:, :, :2] += 1000.0
    x0[G:2 * G], ul[G:2 * G], xr[G:2 * G] = x0[:G], ul[:G], xr[:G]
    th = x0[0, 2]
    x0[G:2 * G, 2] = th + 0.4 * np.spacing(np.float32(abs(th)))
    assert np.float32(x0[G, 2]) == np.float32(th) and x0[G, 2] != th
    group = np.repeat(np.array([0, 0, 2, 3], np.int32), G)
    prm = oracle.params(N)
    us, xs, sts = np.zeros((B, N, 2)), np.zeros((B, N + 1, 3)), np.zeros(B, np.int32)
    for b in range(B):
        r = oracle.solve(prm, x0[b], ul[b], xr[b])
        us[b], xs[b], sts[b] = r["u"], r["x"], r["status"]
    exp = (x0, ul, xr, None, us, xs, sts, None)
    assert np.abs(us[:G] - us[G:2 * G]).max() > 0  # the two scenarios do differ
    s = solver(capi, N, backend=capi.BACKEND_WAVE)
    assert s.backend_info(B, True)[0] == capi.BACKEND_WAVE
    out = s.solve_grouped_dbl(x0, ul, xr, group, 4)
    assert_parity(capi, oracle, out, exp, "grouped host")
    plain = s.solve_dbl(x0, ul, xr)
    for a, b in zip(out[:3], plain[:3]):
        np.testing.assert_array_equal(a, b)  # grouping never changes a result
    d = _dev_buffers(torch, cuda, exp, B, N)
    s.solve_grouped_dev_dbl(d[0], d[1], d[2], None, torch.from_numpy(group).to(cuda), 4, d[3], d[4], d[5])
    torch.cuda.synchronize(cuda)
    for a, b in zip(out[:3], d[3:]):
        np.testing.assert_array_equal(a, b.cpu().numpy())
    s.close()


# ---- 6. same arithmetic --------------------------------------------------------------------------

SAME = [("auto", {}, {}), ("wave", {}, {}), ("segmented", {"F110QP_LANE_SEG": 4}, {}),
        ("sequential dref", {"F110QP_LANE_SEG": 1, "F110QP_LANE_QPW": 16}, {})]


@pytest.mark.parametrize("name,knobs,cfg", SAME, ids=[c[0] for c in SAME])
def test_float_values_give_the_float_call_bit_for_bit(capi, knob, name, knobs, cfg):
    """Doubles that are float32 values: the _dbl outputs equal the float call's bit for bit (u, x,
    status, iterations, obj, cost) on every route but the one DESIGN.md 2h lists."""
    for k, v in knobs.items():
        knob(k, v)
    B, N = 37, 20
    w = workload.make_batch(B, N, seed=91)
    w["x0"][:, :2] += 1000.0
    w["x_ref"][:, :, :2] += 1000.0
    be = {"auto": capi.BACKEND_AUTO, "wave": capi.BACKEND_WAVE}.get(name, capi.BACKEND_LANE)
    s = solver(capi, N, backend=be)
    f = s.solve(w["x0"], w["u_lin"], w["x_ref"], objective=True)
    d = s.solve_dbl(*(w[k].astype(np.float64) for k in ("x0", "u_lin", "x_ref")), objective=True)
    s.close()
    assert (f[2] == capi.SOLVED).all()
    for a, b in zip(f, d):
        np.testing.assert_array_equal(a, b)


def test_float_references_route_stays_within_the_bound(capi, knob):
    """The listed route: lane_kernel.h with float references in LDS (DREF = 0) stages x_ref - x0
    rounded to float32 for double inputs and the absolute float32 for float inputs; the two calls
    agree to the 2e-6 bound on u."""
    knob("F110QP_LANE_SEG", 1)
    knob("F110QP_LANE_QPW", 16)
    knob("F110QP_LANE_DREF", 0)
    B, N = 37, 20
    w = workload.make_batch(B, N, seed=91)
    s = solver(capi, N, backend=capi.BACKEND_LANE)
    f = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    d = s.solve_dbl(*(w[k].astype(np.float64) for k in ("x0", "u_lin", "x_ref")))
    s.close()
    np.testing.assert_array_equal(f[2], d[2])
    assert u_err(d[0], f[0].astype(np.float64)).max() <= U_TOL


# ---- 7. warm context -----------------------------------------------------------------------------

def test_warm_context_dbl_calls_solve_cold_and_leave_the_state(oracle, capi):
    B, N = 256, 20
    exp = expected(oracle, B, N, 99, 1000.0)
    w = workload.make_batch(B, N, seed=5)
    fresh = solve_dbl(capi, N, exp, backend=capi.BACKEND_LANE)
    ref = solver(capi, N, backend=capi.BACKEND_LANE, warm_start=1)  # the float stream alone
    f1 = ref.solve(w["x0"], w["u_lin"], w["x_ref"])
    ref.warm_hits()
    f2 = ref.solve(w["x0"], w["u_lin"], w["x_ref"])
    want = ref.warm_hits()
    ref.close()
    assert want[1] == B  # every slot's key repeats
    s = solver(capi, N, backend=capi.BACKEND_LANE, warm_start=1)
    g1 = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.warm_hits()
    d1 = s.solve_dbl(exp[0], exp[1], exp[2])
    assert s.warm_hits() == (0, 0)  # not moved by a _dbl call
    g2 = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    d2 = s.solve_dbl(exp[0], exp[1], exp[2])
    assert s.warm_hits() == want  # the float stream hits as without the _dbl calls between
    s.close()
    for a, b in zip(g1 + g2, f1 + f2):
        np.testing.assert_array_equal(a, b)
    for d in (d1, d2):
        for a, b in zip(d, fresh):
            np.testing.assert_array_equal(a, b)


# ---- 8. bad data ---------------------------------------------------------------------------------

@pytest.mark.parametrize("be", ["wave", "lane", "segmented"])
def test_non_finite_doubles_are_numerical(oracle, capi, knob, be):
    B, N = 12, 20
    exp = expected(oracle, B, N, 7, 1000.0)
    x0, xr = exp[0].copy(), exp[2].copy()
    x0[2, 1] = np.nan
    x0[5, 0] = np.inf
    xr[7, 3, 0] = np.nan
    xr[9, N - 1, 2] = -np.inf
    bad = np.zeros(B, bool)
    bad[[2, 5, 7, 9]] = True
    knob("F110QP_LANE_SEG", 4 if be == "segmented" else 1)
    s = solver(capi, N, backend=capi.BACKEND_WAVE if be == "wave" else capi.BACKEND_LANE)
    u, x, st, it = s.solve_dbl(x0, exp[1], xr)
    s.close()
    assert (st[bad] == capi.NUMERICAL).all() and np.isnan(u[bad]).all() and np.isnan(x[bad]).all()
    good = tuple(a[~bad] for a in (u, x, st))
    assert_parity(capi, oracle, good, tuple(None if a is None else a[~bad] for a in exp), f"good QPs {be}")
