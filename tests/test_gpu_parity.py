"""Parity of the HIP path (through the C ABI) with the CPU oracle on MI355X.

Tolerance (north star: match the QP's primal solution to 1e-4 rel-tol): for every QP
    ||u_gpu - u*||_inf / max(1, ||u*||_inf) <= 1e-4   and the same for x*,
against the exact optimum u* of the reference QP (oracle/f110_oracle.c, KKT-certified), plus
identical per-QP status. In practice the kernel lands at fp32 output rounding (~1e-7).
"""
import json
import os

import numpy as np
import pytest
from conftest import GOLDEN

from f110qp import workload

pytestmark = pytest.mark.gpu

TOL = 1e-4


def rel_err(a, b):
    axes = tuple(range(1, a.ndim))
    return np.abs(a.astype(np.float64) - b).max(axis=axes) / np.maximum(1.0, np.abs(b).max(axis=axes))


def halfspaces_oracle(oracle, x0, ranges, geom):
    B = x0.shape[0]
    hs = np.zeros((B, 2, 3), np.float32)
    for b in range(B):
        rc, l1, l2, _, _ = oracle.find_half_spaces(x0[b].astype(np.float64), ranges[b], *geom)
        assert rc == 0
        hs[b] = l1, l2
    return hs


def check(oracle, capi, N, w, hs=None, gap=False, tol=TOL, **cfg):
    s = capi.Solver(capi.default_config(N, gap_mode=capi.GAP_ACTIVE if gap else capi.GAP_INACTIVE, **cfg))
    u, x, st, it = s.solve(w["x0"], w["u_lin"], w["x_ref"], hs)
    s.close()
    over = {k: v for k, v in cfg.items() if k in ("q", "r", "u_des", "u_min", "u_max")}
    ur, xr, sr = oracle.solve_batch(oracle.params(N, **over), w["x0"], w["u_lin"], w["x_ref"], hs, gap_active=gap)
    np.testing.assert_array_equal(st, sr)
    ok = sr == oracle.SOLVED
    if ok.any():
        eu, ex = rel_err(u[ok], ur[ok]), rel_err(x[ok], xr[ok])
        assert eu.max() <= tol, (eu.max(), int(np.argmax(eu)))
        assert ex.max() <= tol, (ex.max(), int(np.argmax(ex)))
    if (~ok).any():
        assert np.isnan(u[~ok]).all() and np.isnan(x[~ok]).all()
    return u, x, st, it


# ref_*.npz are the reference-recorded fixtures of test_reference_parity.py / test_gpu_reference.py
GOLDEN_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and not f.startswith("ref_"))


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_fixtures(capi, name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = int(d["horizon"])
    gap = bool(d["gap"])
    over = json.loads(str(d["params"])) if "params" in d.files else {}  # stiff-corner fixtures
    s = capi.Solver(capi.default_config(N, gap_mode=capi.GAP_ACTIVE if gap else capi.GAP_INACTIVE, **over))
    u, x, st, _ = s.solve(d["x0"], d["u_lin"], d["x_ref"], d["halfspace"] if gap else None)
    s.close()
    np.testing.assert_array_equal(st, d["status"])
    assert rel_err(u, d["u"]).max() <= TOL
    assert rel_err(x, d["x"]).max() <= TOL


def test_c2_full_batch(oracle, capi):
    """BASELINE configs[1] at its full size: 1,024 horizon-20 box QPs."""
    w = workload.make_batch(1024, 20, seed=2024)
    u, x, st, it = check(oracle, capi, 20, w)
    assert (st == capi.SOLVED).all()


def test_c3_full_batch_gap_rows(oracle, capi):
    """BASELINE configs[2] at its full size: 4,096 horizon-20 QPs with half-space rows."""
    B = 4096
    w = workload.make_batch(B, 20, seed=2025)
    ranges, *geom = workload.make_scans(B, seed=2025)
    hs = halfspaces_oracle(oracle, w["x0"], ranges, geom)
    u, x, st, it = check(oracle, capi, 20, w, hs, gap=True)
    assert (st == capi.SOLVED).mean() > 0.99


def test_c3_bench_batch_gap_rows(oracle, capi):
    """The bench's own C3 batch (bench.py seeds: make_batch 1000, make_scans 2000): every QP exact
    against the oracle. QP 3008 of it took GI's negative-multiplier re-entry when that was added
    (solve_kernel.h: the refined set held a row with a negative multiplier; the row is dropped and
    GI continues instead of the fp64 re-check)."""
    B = 4096
    w = workload.make_batch(B, 20, seed=1000)
    ranges, *geom = workload.make_scans(B, seed=2000)
    hs = halfspaces_oracle(oracle, w["x0"], ranges, geom)
    u, x, st, it = check(oracle, capi, 20, w, hs, gap=True)
    assert (st == capi.SOLVED).all()


@pytest.mark.parametrize("N", [1, 2, 3, 7, 10, 16, 17, 24, 25, 30, 32, 33, 36, 40, 41, 47, 48])
def test_horizons(oracle, capi, N):
    w = workload.make_batch(200, N, seed=300 + N, lateral=0.6)
    check(oracle, capi, N, w)


@pytest.mark.parametrize("N", [5, 12, 20, 32, 40, 48])
def test_horizons_gap(oracle, capi, N):
    B = 300
    w = workload.make_batch(B, N, seed=400 + N)
    ranges, *geom = workload.make_scans(B, seed=400 + N)
    check(oracle, capi, N, w, halfspaces_oracle(oracle, w["x0"], ranges, geom), gap=True)


@pytest.mark.parametrize("N", [20, 40])
def test_true_heading_and_hard_references(oracle, capi, N):
    """x_ref with the true heading, large lateral offsets and steer beyond the +-0.43 box:
    many active rows (both box faces)."""
    w = workload.make_batch(1024, N, seed=77, heading="true", lateral=2.0, steer_range=1.2)
    u, x, st, it = check(oracle, capi, N, w)
    lo = np.float32([3.0, -0.43])
    hi = np.float32([4.5, 0.43])
    n_active = ((np.abs(u - lo) < 1e-6) | (np.abs(u - hi) < 1e-6)).sum(axis=(1, 2))
    assert n_active.max() >= 10 and ((np.abs(u[..., 1] - lo[1]) < 1e-6).any() and (np.abs(u[..., 1] - hi[1]) < 1e-6).any())


def test_custom_weights(oracle, capi):
    """Non-default params: heading cost q2 > 0, other R, u_des inside the box, narrow bounds."""
    N = 20
    over = dict(q=[3.0, 7.0, 2.0], r=[0.5, 1.5], u_des=[3.7, 0.05], u_min=[3.5, -0.2], u_max=[4.0, 0.2])
    w = workload.make_batch(512, N, seed=88, lateral=0.7)
    s = capi.Solver(capi.default_config(N, **over))
    u, x, st, _ = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    ur, xr, sr = oracle.solve_batch(oracle.params(N, **over), w["x0"], w["u_lin"], w["x_ref"])
    np.testing.assert_array_equal(st, sr)
    assert rel_err(u, ur).max() <= TOL and rel_err(x, xr).max() <= TOL


def test_far_from_origin(oracle, capi):
    """Positions of 1 km: recentring on x0 keeps fp32 exact."""
    w = workload.make_batch(256, 20, seed=99)
    w["x0"][:, :2] += np.float32(1000.0)
    w["x_ref"][:, :, :2] += np.float32(1000.0)
    check(oracle, capi, 20, w)


def test_infeasible_and_mixed_batch(oracle, capi):
    """Infeasible gap wedges inside a feasible batch: identical status, NaN outputs only for
    the infeasible instances (OSQP leaves NaN in its solution on failure)."""
    from test_oracle import infeasible_cases

    N = 20
    B = 64
    w = workload.make_batch(B, N, seed=5)
    ranges, *geom = workload.make_scans(B, seed=5)
    hs = halfspaces_oracle(oracle, w["x0"], ranges, geom)
    for i, (x0, h) in enumerate(infeasible_cases()):
        w["x0"][3 + 10 * i] = x0
        w["u_lin"][3 + 10 * i] = [4.5, 0.0]
        hs[3 + 10 * i] = h
    u, x, st, it = check(oracle, capi, N, w, hs, gap=True)
    assert (st == capi.PRIMAL_INFEASIBLE).sum() == 2


def test_batch_edges(oracle, capi, cuda):
    import torch

    N = 20
    s = capi.Solver(capi.default_config(N))
    # batch 0 is a no-op
    e = torch.empty(0, device=cuda)
    s.solve_dev(e, e, e, None, e, e, torch.empty(0, dtype=torch.int32, device=cuda))
    for B in (1, 63, 65, 1023):
        w = workload.make_batch(B, N, seed=B)
        check(oracle, capi, N, w)
    s.close()


def test_device_path_equals_host_path_and_is_deterministic(capi, cuda):
    import torch

    N, B = 20, 2048
    w = workload.make_batch(B, N, seed=4242)
    s = capi.Solver(capi.default_config(N))
    u_h, x_h, st_h, it_h = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    t = {k: torch.from_numpy(w[k]).to(cuda) for k in ("x0", "u_lin", "x_ref")}
    outs = []
    for _ in range(2):
        uo = torch.empty((B, N, 2), device=cuda)
        xo = torch.empty((B, N + 1, 3), device=cuda)
        st = torch.empty(B, dtype=torch.int32, device=cuda)
        it = torch.empty(B, dtype=torch.int32, device=cuda)
        s.solve_dev(t["x0"], t["u_lin"], t["x_ref"], None, uo, xo, st, it)
        torch.cuda.synchronize()
        outs.append((uo.cpu().numpy(), xo.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()))
    s.close()
    for o in outs:
        np.testing.assert_array_equal(o[0], u_h)
        np.testing.assert_array_equal(o[1], x_h)
        np.testing.assert_array_equal(o[2], st_h)
        np.testing.assert_array_equal(o[3], it_h)


def test_states_are_the_rollout_of_inputs(oracle, capi):
    """x* satisfies the dynamics rows of the reference QP (mpc.cpp:244-248,299,305)."""
    N, B = 20, 256
    w = workload.make_batch(B, N, seed=55)
    s = capi.Solver(capi.default_config(N))
    u, x, st, _ = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    for b in range(0, B, 17):
        A, Bm, Cm = oracle.linearize(float(w["x0"][b, 2]), float(w["u_lin"][b, 0]), float(w["u_lin"][b, 1]))
        np.testing.assert_array_equal(x[b, 0], w["x0"][b])
        for i in range(N):
            pred = A @ x[b, i].astype(np.float64) + Bm @ u[b, i].astype(np.float64) + Cm
            np.testing.assert_allclose(x[b, i + 1], pred, rtol=0, atol=2e-5)
        assert np.all(u[b, :, 0] >= np.float32(3.0) - 1e-6) and np.all(u[b, :, 0] <= np.float32(4.5) + 1e-6)
        assert np.all(np.abs(u[b, :, 1]) <= np.float32(0.43) + 1e-6)


def test_condensed_hessian_and_gradient(oracle, capi, cuda):
    """The kernel's closed-form condensing (A = I + E, E^2 = 0) against the oracle's explicit
    Gamma'Q Gamma (mpc.cpp:208-229 eliminated through the dynamics rows)."""
    import torch

    for N in (1, 7, 20, 32, 40, 48):
        B = 16
        w = workload.make_batch(B, N, seed=600 + N)
        s = capi.Solver(capi.default_config(N))
        t = {k: torch.from_numpy(w[k]).to(cuda) for k in ("x0", "u_lin", "x_ref")}
        H = torch.empty((B, 2 * N, 2 * N), dtype=torch.float64, device=cuda)
        g = torch.empty((B, 2 * N), dtype=torch.float64, device=cuda)
        s.condense_debug_dev(t["x0"], t["u_lin"], t["x_ref"], H, g)
        torch.cuda.synchronize()
        s.close()
        H = H.cpu().numpy()
        g = g.cpu().numpy()
        for b in range(B):
            x0 = w["x0"][b].astype(np.float64)
            # the kernel recentres on (x0, y0): the oracle gets the same shift
            xr = w["x_ref"][b].astype(np.float64) - np.array([x0[0], x0[1], 0.0])
            Hr, gr = oracle.condense(oracle.params(N), np.array([0.0, 0.0, x0[2]]), w["u_lin"][b], xr)
            np.testing.assert_allclose(H[b], Hr, rtol=2e-6, atol=2e-6 * np.abs(Hr).max())
            np.testing.assert_allclose(g[b], gr, rtol=1e-9, atol=1e-9 * np.abs(gr).max())


@pytest.mark.parametrize("nr,seed", [(1080, 11), (1081, 12), (200, 13), (64, 14), (2000, 15)])
def test_half_space_kernel_adversarial(oracle, capi, cuda, nr, seed):
    """The wave-per-scan kernel's parallel gap search on adversarial scans (short runs, single-beam
    gaps, equal longest runs, runs across 64-beam blocks, windows opening on short/long beams,
    NaN/inf/threshold ranges): gap indices identical to the reference state machine; half-space
    coefficients within fp32 rounding (cos/sin from different libms) and mostly bit-equal."""
    import torch
    from halfspace_cases import adversarial_scans, scan_geometry

    B = 512
    amin, ainc, amax = scan_geometry(nr)
    r = adversarial_scans(B, nr, seed)
    rng = np.random.default_rng(seed)
    st = np.column_stack([rng.uniform(-30, 30, B), rng.uniform(-30, 30, B), rng.uniform(-3, 3, B)]).astype(np.float32)
    hs = torch.empty((B, 2, 3), dtype=torch.float32, device=cuda)
    lo = torch.empty(B, dtype=torch.int32, device=cuda)
    hi = torch.empty(B, dtype=torch.int32, device=cuda)
    capi.find_half_spaces_dev(torch.from_numpy(st).to(cuda), torch.from_numpy(r).to(cuda), amin, ainc, amax,
                              hs, lo, hi)
    torch.cuda.synchronize()
    hs, lo, hi = hs.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
    same = total = 0
    for b in range(B):
        rc, l1, l2, rlo, rhi = oracle.find_half_spaces(st[b].astype(np.float64), r[b], amin, ainc, amax)
        assert (lo[b], hi[b]) == (rlo, rhi), b
        if rc != 0:
            assert np.isnan(hs[b]).all()
            continue
        ref = np.float32([l1, l2])
        if not np.isfinite(ref).all():  # an infinite range at an end point: inf/NaN propagate alike
            np.testing.assert_array_equal(np.isnan(hs[b]), np.isnan(ref))
            inf = np.isinf(ref)
            np.testing.assert_array_equal(hs[b][inf], ref[inf])
            continue
        # fp32 rounding of the reference's float arithmetic (constraints.cpp:233-253) from end
        # points whose cos/sin may differ by one double ulp between libms: a, b carry the end
        # point's float ulp, c = px*p1y - py*p1x the ulp of the products (cancellation)
        P = max(abs(float(st[b, 0])), abs(float(st[b, 1]))) + max(float(r[b, rlo]), float(r[b, rhi]))
        eps = float(np.finfo(np.float32).eps)
        tol = np.float64([8 * eps * P, 8 * eps * P, 8 * eps * 2 * P * P])
        for k in range(2):
            if (np.abs(hs[b][k].astype(np.float64) - ref[k]) <= tol).all():
                continue
            # orientation flip (constraints.cpp:236,248): allowed only where the side test
            # a*px + b*py + c of the other end point is zero to rounding (coincident or collinear
            # end points), where a 1-ulp cos/sin difference decides the sign
            flip = np.float32([-ref[k][0], -ref[k][1], 1.0 - ref[k][2]])  # (-a, -b, -c + 0.5)
            assert (np.abs(hs[b][k].astype(np.float64) - flip) <= tol).all(), (b, k, hs[b], ref, tol)
            ang = [np.float32(np.float32(amin + np.float32(np.float32(i) * ainc)) + st[b, 2]) for i in (rlo, rhi)]
            p1 = [np.float64(r[b, rlo]) * np.cos(np.float64(ang[0])) + st[b, 0], np.float64(r[b, rlo]) * np.sin(np.float64(ang[0])) + st[b, 1]]
            p2 = [np.float64(r[b, rhi]) * np.cos(np.float64(ang[1])) + st[b, 0], np.float64(r[b, rhi]) * np.sin(np.float64(ang[1])) + st[b, 1]]
            q = p2 if k == 0 else p1
            a_, b_, c_ = (float(v) for v in ref[k])
            c_ -= 0.5
            side = a_ * q[0] + b_ * q[1] + c_
            assert abs(side) <= 1e-5 * (abs(a_ * q[0]) + abs(b_ * q[1]) + abs(c_)), (b, k, side)
        same += int((hs[b] == ref).all())
        total += 1
    assert total == 0 or same / total >= 0.95, (same, total)


def test_half_space_kernel_long_run_and_empty_window(oracle, capi, cuda):
    """Edge cases of the wave-per-scan gap search: a run of open beams longer than 32,767 (the
    run key (length << 16 | 65535 - end) must not overflow) and an empty field-of-view window
    (angle_max < angle_min: no block is loaded, (lo, hi) = (0, 0) and ranges[0] is read, as the
    reference does). Indices and half-spaces as the reference state machine."""
    import torch

    nr = 40000
    amin = np.float32(-1.0)
    ainc = np.float32(2.0 / (nr - 1))
    amax = np.float32(amin + ainc * np.float32(nr - 1))
    r = np.full((3, nr), 5.0, np.float32)
    r[0, 100] = 1.0          # runs of 99 and 39,899 beams
    r[1, 36000] = 1.0        # the longest run (35,999 beams) first
    r[2, :] = 1.0
    r[2, 5:38000] = 6.0      # one run of 37,995 beams
    st = np.float32([[1.0, -2.0, 0.3], [0.0, 0.0, 0.0], [-5.0, 4.0, -1.2]])
    for amax_use in (amax, np.float32(amin - 5 * ainc)):
        hs = torch.empty((3, 2, 3), dtype=torch.float32, device=cuda)
        lo = torch.empty(3, dtype=torch.int32, device=cuda)
        hi = torch.empty(3, dtype=torch.int32, device=cuda)
        capi.find_half_spaces_dev(torch.from_numpy(st).to(cuda), torch.from_numpy(r).to(cuda), amin, ainc,
                                  amax_use, hs, lo, hi)
        torch.cuda.synchronize()
        hs, lo, hi = hs.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
        for b in range(3):
            rc, l1, l2, rlo, rhi = oracle.find_half_spaces(st[b].astype(np.float64), r[b], amin, ainc, amax_use)
            assert (lo[b], hi[b]) == (rlo, rhi), (b, lo[b], hi[b], rlo, rhi)
            if amax_use == amax:
                assert hi[b] - lo[b] > 32767 - 6, (b, lo[b], hi[b])
            ref = np.float32([l1, l2])
            np.testing.assert_allclose(hs[b], ref, rtol=2e-6, atol=2e-6 * np.abs(ref).max())


def test_half_space_kernel(oracle, capi, cuda):
    """Batched FindHalfSpaces on the device: identical gap indices, coefficients within
    fp32 rounding of the host reference (cos/sin come from different libms)."""
    import torch

    B = 2048
    w = workload.make_batch(B, 20, seed=9)
    ranges, amin, ainc, amax = workload.make_scans(B, seed=9)
    hs = torch.empty((B, 2, 3), dtype=torch.float32, device=cuda)
    lo = torch.empty(B, dtype=torch.int32, device=cuda)
    hi = torch.empty(B, dtype=torch.int32, device=cuda)
    capi.find_half_spaces_dev(torch.from_numpy(w["x0"]).to(cuda), torch.from_numpy(ranges).to(cuda), amin, ainc,
                              amax, hs, lo, hi)
    torch.cuda.synchronize()
    hs, lo, hi = hs.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
    for b in range(B):
        rc, l1, l2, rlo, rhi = oracle.find_half_spaces(w["x0"][b].astype(np.float64), ranges[b], amin, ainc, amax)
        assert (lo[b], hi[b]) == (rlo, rhi)
        ref = np.float32([l1, l2])
        np.testing.assert_allclose(hs[b], ref, rtol=2e-6, atol=2e-6 * np.abs(ref).max())
    # quirk: no gap -> NaN half spaces, indices (-1, -1)
    r = torch.ones((4, 1080), device=cuda)
    capi.find_half_spaces_dev(torch.zeros((4, 3), device=cuda), r, amin, ainc, amax, hs_t := torch.empty((4, 2, 3), device=cuda), lo_t := torch.empty(4, dtype=torch.int32, device=cuda), None)
    torch.cuda.synchronize()
    assert torch.isnan(hs_t).all() and (lo_t == -1).all()


def test_large_batch_throughput_shape(oracle, capi):
    """65,536 QPs in one launch (the C4 batch size at horizon 20): all solved, parity on a
    strided sample."""
    N, B = 20, 65536
    w = workload.make_batch(B, N, seed=65536)
    s = capi.Solver(capi.default_config(N))
    u, x, st, _ = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    assert (st == capi.SOLVED).all()
    idx = np.arange(0, B, 61)
    ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"][idx], w["u_lin"][idx], w["x_ref"][idx])
    assert rel_err(u[idx], ur).max() <= TOL and rel_err(x[idx], xr).max() <= TOL


def test_warm_started_stream(oracle, capi):
    """Config C5: a receding-horizon stream solved with warm_start = 1 (OsqpEigen
    setWarmStart(true), mpc.cpp:98). Slots whose linearisation point is unchanged reuse the
    cached W; a tenth of the cars turn every 3 ticks (cache misses). Every tick must equal the
    exact optimum, and the warm solve must not need more active-set passes than the cold one."""
    N, B, T = 20, 512, 7
    stream = workload.make_stream(B, N, T, seed=11, heading_change_every=3)
    warm = capi.Solver(capi.default_config(N, warm_start=1))
    cold = capi.Solver(capi.default_config(N))
    it_w, it_c = [], []
    for t, w in enumerate(stream):
        uw, xw, sw, iw = warm.solve(w["x0"], w["u_lin"], w["x_ref"])
        uc, xc, sc, ic = cold.solve(w["x0"], w["u_lin"], w["x_ref"])
        ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"], w["u_lin"], w["x_ref"])
        np.testing.assert_array_equal(sw, sr)
        assert rel_err(uw, ur).max() <= TOL and rel_err(xw, xr).max() <= TOL, t
        assert rel_err(uc, ur).max() <= TOL
        if t > 0:
            it_w.append(iw.mean())
            it_c.append(ic.mean())
    assert np.mean(it_w) <= np.mean(it_c)
    # a reset, and a different batch size, both fall back to a cold solve
    warm.warm_reset()
    w = stream[-1]
    uw, xw, sw, _ = warm.solve(w["x0"], w["u_lin"], w["x_ref"])
    ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"], w["u_lin"], w["x_ref"])
    assert rel_err(uw, ur).max() <= TOL
    uw, xw, sw, _ = warm.solve(w["x0"][:100], w["u_lin"][:100], w["x_ref"][:100])
    assert rel_err(uw, ur[:100]).max() <= TOL
    warm.close()
    cold.close()


def test_warm_start_gap_rows(oracle, capi):
    """warm_start with gap rows: W reuse under the GI path."""
    N, B, T = 20, 256, 4
    stream = workload.make_stream(B, N, T, seed=12)
    ranges, *geom = workload.make_scans(B, seed=12)
    s = capi.Solver(capi.default_config(N, warm_start=1, gap_mode=capi.GAP_ACTIVE))
    for w in stream:
        hs = halfspaces_oracle(oracle, w["x0"], ranges, geom)
        u, x, st, _ = s.solve(w["x0"], w["u_lin"], w["x_ref"], hs)
        ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"], w["u_lin"], w["x_ref"], hs, gap_active=True)
        np.testing.assert_array_equal(st, sr)
        ok = sr == oracle.SOLVED
        assert rel_err(u[ok], ur[ok]).max() <= TOL
    s.close()


def test_c4_grouped_candidates_horizon40(oracle, capi):
    """BASELINE configs[3] per GPU: 8,192 horizon-40 QPs (a 1/8 shard of 65,536 = 546
    scenarios x 120 candidates + remainder), two register rows per lane. All solved, parity on
    a strided sample plus every candidate of two whole scenarios."""
    N = 40
    w = workload.make_grouped_batch(69, N, seed=4040)
    B = 8192
    w = {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    s = capi.Solver(capi.default_config(N))
    u, x, st, it = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    assert (st == capi.SOLVED).all()
    idx = np.concatenate([np.arange(0, B, 37), np.arange(120, 360)])
    ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"][idx], w["u_lin"][idx], w["x_ref"][idx])
    assert (sr == oracle.SOLVED).all()
    assert rel_err(u[idx], ur).max() <= TOL and rel_err(x[idx], xr).max() <= TOL


def test_c4_full_single_gpu_batch(oracle, capi):
    """BASELINE configs[3] at its full single-GPU size: 65,536 x N = 40 grouped candidates (546
    scenarios x 120 + 16), the launch the c4 bench line times (AUTO: lane_kernel with fp32
    Riccati-gain scratch in HBM). Every QP solved; parity on a strided sample of 1,024 QPs plus
    every candidate of one whole scenario."""
    N, B = 40, 65536
    g = workload.make_grouped_batch(-(-B // 120), N, seed=4000)
    w = {k: np.ascontiguousarray(g[k][:B]) for k in ("x0", "u_lin", "x_ref")}
    s = capi.Solver(capi.default_config(N))
    be, qpw, scr = s.backend_info(B)
    assert be == capi.BACKEND_LANE and s.lane_segments(B) == 1 and scr == 4  # HBM fp32
    u, x, st, it = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    assert (st == capi.SOLVED).all()
    idx = np.concatenate([np.arange(0, B, 64), np.arange(32760, 32880)])
    ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"][idx], w["u_lin"][idx], w["x_ref"][idx])
    assert (sr == oracle.SOLVED).all()
    assert rel_err(u[idx], ur).max() <= 2e-6 and rel_err(x[idx], xr).max() <= 2e-6


def test_warm_started_stream_horizon40(oracle, capi):
    """warm_start at N = 40: the act masks of both register rows carry across ticks."""
    N, B, T = 40, 256, 4
    stream = workload.make_stream(B, N, T, seed=21, heading_change_every=2)
    warm = capi.Solver(capi.default_config(N, warm_start=1))
    for w in stream:
        uw, xw, sw, iw = warm.solve(w["x0"], w["u_lin"], w["x_ref"])
        ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"], w["u_lin"], w["x_ref"])
        np.testing.assert_array_equal(sw, sr)
        assert rel_err(uw, ur).max() <= TOL and rel_err(xw, xr).max() <= TOL
    warm.close()


# ---- lane-per-QP back end (Riccati/PDAS, fp64) ------------------------------------------------

RICCATI = ["lane"]


def _be(capi, name):
    return {"lane": capi.BACKEND_LANE, "wave": capi.BACKEND_WAVE}[name]


@pytest.mark.parametrize("be", RICCATI)
@pytest.mark.parametrize("N", [1, 2, 5, 17, 20, 30, 32, 33, 40, 48])
def test_lane_backend_horizons(oracle, capi, N, be):
    """The Riccati back end (one QP per lane) against the exact optimum; batch not
    a multiple of 64 so the last wave is partial."""
    w = workload.make_batch(1000, N, seed=700 + N, lateral=0.6)
    u, x, st, it = check(oracle, capi, N, w, backend=_be(capi, be))
    assert (st == capi.SOLVED).all()


@pytest.mark.parametrize("be", RICCATI)
@pytest.mark.parametrize("N", [20, 40])
def test_lane_backend_hard_references(oracle, capi, N, be):
    """True-heading references with big offsets and steer beyond the box: many active bounds
    on both faces, several PDAS passes."""
    w = workload.make_batch(2048, N, seed=770 + N, heading="true", lateral=2.0, steer_range=1.2)
    u, x, st, it = check(oracle, capi, N, w, backend=_be(capi, be))
    assert it.max() >= 2


@pytest.mark.parametrize("be", RICCATI)
def test_lane_backend_custom_weights_and_far_origin(oracle, capi, be):
    N = 20
    over = dict(q=[3.0, 7.0, 2.0], r=[0.5, 1.5], u_des=[3.7, 0.05], u_min=[3.5, -0.2], u_max=[4.0, 0.2])
    w = workload.make_batch(640, N, seed=881, lateral=0.7)
    w["x0"][:, :2] += np.float32(1000.0)
    w["x_ref"][:, :, :2] += np.float32(1000.0)
    s = capi.Solver(capi.default_config(N, backend=_be(capi, be), **over))
    u, x, st, _ = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    ur, xr, sr = oracle.solve_batch(oracle.params(N, **over), w["x0"], w["u_lin"], w["x_ref"])
    np.testing.assert_array_equal(st, sr)
    assert rel_err(u, ur).max() <= TOL and rel_err(x, xr).max() <= TOL


@pytest.mark.parametrize("dref", ["0", "1"])
@pytest.mark.parametrize("rot", ["0", "1"])
@pytest.mark.parametrize("N", [20, 40])
def test_lane_backend_heading_frame(oracle, capi, knob, monkeypatch, rot, dref, N):
    """q0 == q1 (the shipped params.yaml) runs the lane kernel in the frame of the heading
    theta0 (lane_kernel.h ROT: four zero model entries); F110QP_LANE_ROT=0 forces the general
    frame. The references are converted once to fp64 offsets in LDS (DREF) where the resident
    waves fit; F110QP_LANE_DREF=0 keeps the per-stage conversion of the float staging. Every
    combination gives the exact optimum, also 1 km from the origin with headings all round the
    circle."""
    knob("F110QP_LANE_ROT", rot)
    knob("F110QP_LANE_DREF", dref)
    w = workload.make_batch(1500, N, seed=6060 + N, heading="true", lateral=1.5, steer_range=1.0)
    w["x0"][:, 2] = np.random.default_rng(N).uniform(-np.pi, np.pi, 1500).astype(np.float32)
    w["x0"][:, :2] += np.float32(1000.0)
    w["x_ref"][:, :, :2] += np.float32(1000.0)
    u, x, st, it = check(oracle, capi, N, w, backend=capi.BACKEND_LANE)
    assert (st == capi.SOLVED).all()


@pytest.mark.parametrize("be", RICCATI)
@pytest.mark.parametrize("kmax,N", [("0", 20), ("1", 20), ("2", 40), ("0", 40)])
def test_lane_backend_single_flip_fallback(oracle, capi, knob, monkeypatch, be, kmax, N):
    """F110QP_LANE_KMAX caps the multi-flip PDAS passes of the lane kernel; past the cap a QP
    flips one complementarity violation per pass (least index, stage-major), so the QPs with
    many active bounds finish inside the same launch in more passes. kmax = 0: single flips
    from the first pass. Results stay exact, repeated calls on one context agree, and the pass
    counts exceed the PDAS ones."""
    knob("F110QP_LANE_KMAX", kmax)
    w = workload.make_batch(3000, N, seed=991 + N, heading="true", lateral=1.5, steer_range=1.0)
    s = capi.Solver(capi.default_config(N, backend=_be(capi, be)))
    ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"], w["u_lin"], w["x_ref"])
    for _ in range(2):
        u, x, st, it = s.solve(w["x0"], w["u_lin"], w["x_ref"])
        np.testing.assert_array_equal(st, sr)
        assert rel_err(u, ur).max() <= TOL and rel_err(x, xr).max() <= TOL
    s.close()
    monkeypatch.delenv("F110QP_LANE_KMAX")
    s = capi.Solver(capi.default_config(N, backend=_be(capi, be)))
    _, _, _, it_pdas = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    assert it.max() > it_pdas.max()


@pytest.mark.parametrize("qpw", ["1", "2", "8", "64"])
def test_lane_backend_qps_per_wave(oracle, capi, knob, monkeypatch, qpw):
    """Every QPs-per-wave layout of the lane kernel (F110QP_LANE_QPW; auto picks by batch)
    gives the same exact results; the batch is not a multiple of the wave width."""
    knob("F110QP_LANE_QPW", qpw)
    N, B = 40, 700
    w = workload.make_batch(B, N, seed=5150, heading="true", lateral=1.2, steer_range=0.8)
    u, x, st, it = check(oracle, capi, N, w, backend=capi.BACKEND_LANE, tol=2e-6)
    assert (st == capi.SOLVED).all()


@pytest.mark.parametrize("cap", ["0", "1", "2"])
def test_wave_box_pdas_cap_falls_back_to_gi(oracle, capi, knob, monkeypatch, cap):
    """F110QP_PDAS_MAX caps the wave kernel's box PDAS on the swept Hessian (0: the GI loop
    solves from the unconstrained point; 1-2: PDAS stops short on the QPs with many active
    bounds and GI restarts): the results stay exact."""
    knob("F110QP_PDAS_MAX", cap)
    N = 20
    w = workload.make_batch(600, N, seed=4242, heading="true", lateral=1.5, steer_range=1.0)
    check(oracle, capi, N, w, backend=capi.BACKEND_WAVE)


def test_lane_and_wave_backends_agree(capi):
    N, B = 20, 4100
    w = workload.make_batch(B, N, seed=1234, heading="true", lateral=1.0)
    res = []
    for be in (capi.BACKEND_WAVE, capi.BACKEND_LANE, capi.BACKEND_AUTO):
        s = capi.Solver(capi.default_config(N, backend=be))
        res.append(s.solve(w["x0"], w["u_lin"], w["x_ref"]))
        s.close()
    for r in res[1:]:
        np.testing.assert_array_equal(r[2], res[0][2])
        assert rel_err(r[0], res[0][0].astype(np.float64)).max() <= 1e-5
        assert rel_err(r[1], res[0][1].astype(np.float64)).max() <= 1e-5


@pytest.mark.parametrize("be", RICCATI)
def test_lane_backend_warm_stream(oracle, capi, be):
    """Config C5 on the lane back end: the previous tick's active set seeds PDAS."""
    N, B, T = 20, 4096, 5
    stream = workload.make_stream(B, N, T, seed=31, heading_change_every=2)
    warm = capi.Solver(capi.default_config(N, warm_start=1, backend=_be(capi, be)))
    its = []
    for t, w in enumerate(stream):
        u, x, st, it = warm.solve(w["x0"], w["u_lin"], w["x_ref"])
        ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"], w["u_lin"], w["x_ref"])
        np.testing.assert_array_equal(st, sr)
        assert rel_err(u, ur).max() <= TOL and rel_err(x, xr).max() <= TOL, t
        its.append(it.mean())
    assert np.mean(its[1:]) <= its[0]
    warm.close()


@pytest.mark.parametrize("be", RICCATI + ["auto"])
def test_lane_backend_c4_shard(oracle, capi, be):
    """BASELINE configs[3] at N = 40 through the Riccati back ends (and whatever auto picks)."""
    N, B = 40, 8192
    g = workload.make_grouped_batch(69, N, seed=4041)
    w = {k: np.ascontiguousarray(g[k][:B]) for k in ("x0", "u_lin", "x_ref")}
    s = capi.Solver(capi.default_config(N, backend=capi.BACKEND_AUTO if be == "auto" else _be(capi, be)))
    u, x, st, it = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    assert (st == capi.SOLVED).all()
    idx = np.concatenate([np.arange(0, B, 29), np.arange(480, 720)])
    ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"][idx], w["u_lin"][idx], w["x_ref"][idx])
    assert rel_err(u[idx], ur).max() <= TOL and rel_err(x[idx], xr).max() <= TOL


@pytest.mark.parametrize("mode", ["1", "2", "3", "4"])
def test_lane_backend_scratch_modes(oracle, capi, knob, monkeypatch, mode):
    """Every Riccati-scratch placement of the lane back end (LDS fp64 / LDS fp32 / HBM fp64 /
    HBM fp32, F110QP_LANE_MODE) gives the exact optimum within the tolerance; N = 40 covers
    the fall-back of LDS fp64 (too big) to HBM."""
    knob("F110QP_LANE_MODE", mode)
    lo, hi = np.float32([3.0, -0.43]), np.float32([4.5, 0.43])
    for N, seed in ((20, 811), (40, 812)):
        w = workload.make_batch(1500, N, seed=seed, heading="true", lateral=1.2, steer_range=0.8)
        u, x, st, it = check(oracle, capi, N, w, backend=capi.BACKEND_LANE, tol=2e-6)
        assert (st == capi.SOLVED).all()
        # fp32 gains: the output clamps an input the single-flip tolerance left outside its box
        assert (u >= lo).all() and (u <= hi).all()



@pytest.mark.parametrize("be,mode,kmax", [("wave", "0", "16"), ("lane", "1", "16"), ("lane", "4", "16"),
                                           ("lane", "1", "0"), ("lane", "4", "0")])
def test_degenerate_bound_zero_multiplier(oracle, capi, knob, monkeypatch, be, mode, kmax):
    """u_des = (4.5, 0) with des_vel = umax (params.yaml:42,46): with Q = 0 the optimum is
    u = u_des at every stage, so the speed sits exactly on its upper bound with a ZERO multiplier
    (a degenerate complementarity pair), and with a tiny Q it is within rounding of that. The
    PDAS flip tests carry a tolerance, so rounding noise cannot flip such an input free -> bound
    -> free until the pass cap (MAX_ITER): every QP must come back SOLVED at the exact optimum,
    with the multi-flip passes and with single flips from the first pass, fp64 and fp32 gains."""
    knob("F110QP_LANE_MODE", mode)
    knob("F110QP_LANE_KMAX", kmax)
    N = 20
    for q in ([0.0, 0.0, 0.0], [1e-9, 1e-9, 0.0], [1e-3, 1e-3, 0.0]):
        w = workload.make_batch(700, N, seed=4500, heading="true", lateral=0.0, steer_range=0.0)
        # fp32 gain scratch (mode 4): a degenerate QP settles in the single-flip passes with the
        # looser fp32 flip tolerance (lane_kernel.h): exact to ~1e-6, inside the 1e-4 bound
        u, x, st, it = check(oracle, capi, N, w, backend=_be(capi, be), tol=2e-6 if mode != "4" else 1e-5, q=q)
        assert (st == capi.SOLVED).all(), (q, np.unique(st, return_counts=True))
        if q[0] == 0.0:
            np.testing.assert_allclose(u[..., 0], 4.5, atol=1e-5)
            np.testing.assert_allclose(u[..., 1], 0.0, atol=1e-5)


@pytest.mark.parametrize("be", ["wave", "lane"])
def test_non_finite_inputs_are_numerical(oracle, capi, be):
    """NaN / inf in x0, u_lin or x_ref (the planning stage emits a NaN x_ref when no candidate is
    valid) -> status F110QP_NUMERICAL and NaN outputs for those QPs only; the rest exact."""
    N, B = 20, 4160
    w = workload.make_batch(B, N, seed=1313)
    bad = {3: ("x_ref", (3, 5, 0), np.nan), 70: ("x0", (70, 2), np.inf), 130: ("u_lin", (130, 1), np.nan),
           4000: ("x_ref", (4000, 0, 1), -np.inf), 4159: ("x_ref", (4159, N - 1, 2), np.nan)}
    for b, (k, idx, v) in bad.items():
        w[k][idx] = v
    s = capi.Solver(capi.default_config(N, backend=_be(capi, be)))
    u, x, st, it = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    badi = np.array(sorted(bad))
    assert (st[badi] == capi.NUMERICAL).all()
    assert np.isnan(u[badi]).all() and np.isnan(x[badi]).all()
    good = np.setdiff1d(np.arange(B), badi)[::13]
    ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"][good], w["u_lin"][good], w["x_ref"][good])
    assert (st[good] == capi.SOLVED).all()
    assert rel_err(u[good], ur).max() <= TOL and rel_err(x[good], xr).max() <= TOL


@pytest.mark.parametrize("be", ["wave", "lane"])
def test_closed_loop_stream_warm(oracle, capi, be):
    """Config C5 as a closed receding-horizon loop (workload.closed_loop_stream): theta0 and the
    linearisation steer change every tick (the wave back end's W cache never hits), mini paths are
    re-planned every 5 ticks, the plant is simulate_dynamics with u*_0. Each back end solves the
    stream warm (previous active set seeds the solve) and matches the exact optimum on every tick;
    warm passes do not exceed cold ones on average."""
    N, B, T = 20, 4096, 8
    prm = oracle.params(N)
    ref = []

    def solve(x0, ul, xr):
        u, x, st = oracle.solve_batch(prm, x0, ul, xr)
        ref.append((u, x, st))
        return u

    ticks = workload.closed_loop_stream(solve, B, N, T, seed=55)
    assert workload.warm_key_hit_rate(ticks) < 0.01
    warm = capi.Solver(capi.default_config(N, warm_start=1, backend=_be(capi, be)))
    cold = capi.Solver(capi.default_config(N, backend=_be(capi, be)))
    itw, itc = [], []
    for t, w in enumerate(ticks):
        u, x, st, it = warm.solve(w["x0"], w["u_lin"], w["x_ref"])
        ur, xr, sr = ref[t]
        np.testing.assert_array_equal(st, sr)
        assert rel_err(u, ur).max() <= TOL and rel_err(x, xr).max() <= TOL, t
        itw.append(it.mean())
        itc.append(cold.solve(w["x0"], w["u_lin"], w["x_ref"])[3].mean())
    warm.close()
    cold.close()
    assert np.mean(itw[1:]) <= np.mean(itc[1:]) + 1e-9, (np.mean(itw[1:]), np.mean(itc[1:]))


@pytest.mark.parametrize("mode", ["0", "1", "2", "4"])
@pytest.mark.parametrize("N", [30, 32])
def test_lane_backend_reference_horizon_scratch(oracle, capi, knob, monkeypatch, mode, N):
    """The reference default horizon (params.yaml:12, N = 30) and N = 32 at a C5-sized batch on
    every lane scratch placement (auto, LDS fp64, LDS fp32, HBM fp32): the auto policy's LDS
    budget near its cap stays exact. Checked on a sample against the exact optimum."""
    knob("F110QP_LANE_MODE", mode)
    B = 4096
    w = workload.make_batch(B, N, seed=3030 + N, heading="true", lateral=1.0, steer_range=0.6)
    s = capi.Solver(capi.default_config(N, backend=capi.BACKEND_LANE))
    u, x, st, it = s.solve(w["x0"], w["u_lin"], w["x_ref"])
    s.close()
    assert (st == capi.SOLVED).all()
    idx = np.arange(0, B, 7)
    ur, xr, sr = oracle.solve_batch(oracle.params(N), w["x0"][idx], w["u_lin"][idx], w["x_ref"][idx])
    assert rel_err(u[idx], ur).max() <= 2e-6 and rel_err(x[idx], xr).max() <= 2e-6


@pytest.mark.parametrize("gap", [False, True])
@pytest.mark.parametrize("N", [1, 20, 40])
def test_assembly_hook_matches_reference_layout(oracle, capi, N, gap):
    """f110qp_assemble_debug_dev: the product's reading of the reference QP on the
    device equals the oracle's restatement of src/mpc.cpp:208-306 entry by entry: identical CSC
    structure (explicit zeros, the stage-0 all-ones gap block of the shipped code, the C3 rows),
    identical bounds, q with the terminal x_ref[N-1]; values to fp64 rounding (device vs host libm
    sin/cos in Linearize, 1 ulp)."""
    w = workload.make_batch(8, N, seed=600 + N, heading="true")
    hs_all = None
    if gap:
        ranges, *geom = workload.make_scans(8, seed=600 + N)
        hs_all = halfspaces_oracle(oracle, w["x0"], ranges, geom)
    s = capi.Solver(capi.default_config(N, gap_mode=capi.GAP_ACTIVE if gap else capi.GAP_INACTIVE))
    prm = oracle.params(N)
    for b in range(8):
        h = None if hs_all is None else hs_all[b]
        got = s.assemble_debug(w["x0"][b], w["u_lin"][b], w["x_ref"][b], h)
        ref = oracle.assemble(prm, w["x0"][b].astype(np.float64), w["u_lin"][b].astype(np.float64),
                              w["x_ref"][b].astype(np.float64), None if h is None else h.astype(np.float64), gap)
        for k in ("P_colptr", "P_rowind", "A_colptr", "A_rowind"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        for k in ("P_val", "q"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        for k in ("A_val", "l", "u"):  # A, B, C entries carry the device/host sin/cos ulp
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-15, atol=1e-18, err_msg=k)
        assert (got["A_val"] == 0).sum() == (ref["A_val"] == 0).sum()  # explicit zeros kept
    s.close()


@pytest.mark.parametrize("be,gap,N", [("wave", False, 20), ("lane", False, 20), ("lane", False, 40),
                                      ("wave", True, 20), ("wave", False, 40)])
def test_objective_matches_oracle(oracle, capi, be, gap, N):
    """f110qp_solve_batch_ex: obj = OSQP's 1/2 z'Pz + q'z (what osqp_info::obj_val holds after
    mpc.cpp:133) and cost = the tracking cost (obj plus the constant OSQP drops), both fp64 from
    the device, against the exact optimum's objective (oracle, f110_oracle.c:544-554) and the
    tracking cost of the oracle's solution: rel 1e-6 on obj (about |obj| ~ 1e5 in world
    coordinates) and 1e-6 * max(1, cost) on cost. Non-solved QPs give NaN."""
    B = 1500
    w = workload.make_batch(B, N, seed=6060 + N, heading="true", lateral=1.0, steer_range=0.6)
    hs = None
    if gap:
        ranges, amin, ainc, amax = workload.make_scans(B, seed=6061)
        hs = halfspaces_oracle(oracle, w["x0"], ranges, (amin, ainc, amax))
    s = capi.Solver(capi.default_config(N, gap_mode=capi.GAP_ACTIVE if gap else capi.GAP_INACTIVE,
                                        backend=_be(capi, be)))
    u, x, st, it, ob, co = s.solve(w["x0"], w["u_lin"], w["x_ref"], hs, objective=True)
    s.close()
    prm = oracle.params(N)
    ur, xr, sr, obr = oracle.solve_batch(prm, w["x0"], w["u_lin"], w["x_ref"], hs, gap_active=gap, objective=True)
    np.testing.assert_array_equal(st, sr)
    ok = sr == oracle.SOLVED
    assert ok.mean() > 0.9
    np.testing.assert_allclose(ob[ok], obr[ok], rtol=1e-6, atol=1e-6)
    cr = oracle.tracking_cost(prm, ur, xr, w["x_ref"])
    assert (np.abs(co[ok] - cr[ok]) <= 1e-6 * np.maximum(1.0, cr[ok])).all(), np.abs(co[ok] - cr[ok]).max()
    assert (co[ok] >= 0).all()
    assert np.isnan(ob[~ok]).all() and np.isnan(co[~ok]).all()


@pytest.mark.parametrize("be", ["wave", "lane"])
def test_select_per_scenario(oracle, capi, cuda, be):
    """C4 candidate sets (6 lanes x 20 steers per scenario, N = 40) solved grouped with the cost
    output, then f110qp_select_dev: the winner of every scenario is the argmin of the costs
    (smallest index on ties: two identical candidates are planted), equal to the argmin of the
    exact optimum's costs wherever the best two candidates differ by more than the tolerance; a
    scenario whose candidates are all non-finite gets winner -1 / +inf."""
    import torch

    N, S = 40, 12
    g = workload.make_grouped_batch(S, N, seed=7070)
    G = g["group_size"]
    w = {k: np.ascontiguousarray(g[k]) for k in ("x0", "u_lin", "x_ref")}
    B = S * G
    for k in w:
        w[k][5 * G + 7] = w[k][5 * G + 3]     # a tie inside scenario 5
    w["x_ref"][11 * G:12 * G] = np.nan        # scenario 11: no solvable candidate
    gid_np = (np.arange(B) // G).astype(np.int32)
    dev = cuda
    t = {k: torch.from_numpy(v).to(dev) for k, v in w.items()}
    gid = torch.from_numpy(gid_np).to(dev)
    uo = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
    xo = torch.empty((B, N + 1, 3), dtype=torch.float32, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    co = torch.empty(B, dtype=torch.float64, device=dev)
    s = capi.Solver(capi.default_config(N, backend=_be(capi, be)))
    s.solve_grouped_dev(t["x0"], t["u_lin"], t["x_ref"], None, gid, S, uo, xo, st, None, cost=co)
    win = torch.empty(S, dtype=torch.int32, device=dev)
    best = torch.empty(S, dtype=torch.float64, device=dev)
    capi.select_dev(gid, S, co, st, win, best)
    torch.cuda.synchronize()
    s.close()
    stn, con, winn, bestn = st.cpu().numpy(), co.cpu().numpy(), win.cpu().numpy(), best.cpu().numpy()
    w_chk, b_chk = oracle.select(gid_np, S, con, stn)     # the argmin of the device's own costs
    np.testing.assert_array_equal(winn, w_chk)
    np.testing.assert_array_equal(bestn, b_chk)
    assert winn[11] == -1 and np.isinf(bestn[11])
    assert winn[5] != 5 * G + 7 or con[5 * G + 3] > con[5 * G + 7]
    prm = oracle.params(N)
    ur, xr, sr = oracle.solve_batch(prm, w["x0"], w["u_lin"], w["x_ref"])
    cr = oracle.tracking_cost(prm, ur, xr, w["x_ref"])
    w_ref, b_ref = oracle.select(gid_np, S, cr, sr)
    for sc in range(S):
        if w_ref[sc] < 0:
            assert winn[sc] == -1
            continue
        c = np.sort(cr[sc * G:(sc + 1) * G][sr[sc * G:(sc + 1) * G] == oracle.SOLVED])
        if len(c) > 1 and c[1] - c[0] > 1e-6 * max(1.0, c[0]):
            assert winn[sc] == w_ref[sc], (sc, winn[sc], w_ref[sc])
        assert abs(bestn[sc] - b_ref[sc]) <= 1e-6 * max(1.0, b_ref[sc])


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fuzz_configs_against_oracle(oracle, capi, seed):
    """Random corners of the ABI's parameter space, each against the exact oracle: horizon
    1..48, dt 0.005..0.05, unequal / zero state weights (general frame), R, u_des inside or on a
    bound, narrow or wide bounds, random batch sizes, both back ends, gap rows on the wave back
    end. Status parity is exact: every QP's status equals the oracle's. The wave kernel's gap-row
    QPs it does not certify itself (fp32 GI on stiff or near-degenerate wedges: SOLVED_INACCURATE,
    MAX_ITER, or an infeasibility claim) are re-checked in fp64 by the lane interior point in the
    same call (a KKT-checked polished point, or a Farkas certificate of an empty set).
    Only QPs the oracle cannot certify itself (UNCERTIFIED) are left out of the comparison."""
    rng = np.random.default_rng(9000 + seed)
    for case in range(4):
        N = int(rng.choice([1, 2, 5, 13, 20, 27, 33, 40, 48]))
        lo0, lo1 = float(rng.uniform(1.0, 3.5)), float(rng.uniform(-0.6, -0.1))
        hi0, hi1 = lo0 + float(rng.uniform(0.3, 2.0)), -lo1 * float(rng.uniform(0.5, 1.5))
        ud = [float(rng.choice([hi0, lo0, 0.5 * (lo0 + hi0)])), float(rng.choice([0.0, hi1, lo1]))]
        q01 = float(rng.choice([0.0, 1.0, 10.0, 40.0]))
        over = dict(q=[q01, q01 if rng.random() < 0.5 else float(rng.uniform(0.5, 20.0)), float(rng.choice([0.0, 0.5, 3.0]))],
                    r=[float(rng.uniform(0.05, 2.0)), float(rng.uniform(0.5, 10.0))], u_des=ud,
                    u_min=[lo0, lo1], u_max=[hi0, hi1])
        dt = float(np.float32(rng.choice([0.005, 0.01, 0.02, 0.05])))
        B = int(rng.integers(1, 400))
        gap = bool(rng.random() < 0.3)
        be = "wave" if (gap or rng.random() < 0.5) else "lane"
        w = workload.make_batch(B, N, seed=int(rng.integers(1 << 30)), heading="true",
                                lateral=float(rng.uniform(0.0, 1.5)), steer_range=float(rng.uniform(0.0, 0.8)))
        hs = None
        if gap:
            ranges, amin, ainc, amax = workload.make_scans(B, seed=int(rng.integers(1 << 30)))
            hs = halfspaces_oracle(oracle, w["x0"], ranges, (amin, ainc, amax))
        cfg = capi.default_config(N, gap_mode=capi.GAP_ACTIVE if gap else capi.GAP_INACTIVE,
                                  backend=_be(capi, be), dt=dt, **over)
        s = capi.Solver(cfg)
        u, x, st, it, ob, co = s.solve(w["x0"], w["u_lin"], w["x_ref"], hs, objective=True)
        s.close()
        prm = oracle.params(N, dt=dt, **over)
        ur, xr, sr, obr = oracle.solve_batch(prm, w["x0"], w["u_lin"], w["x_ref"], hs, gap_active=gap, objective=True)
        tag = (seed, case, N, dt, be, gap, over)
        # QPs the oracle cannot certify itself (near-infeasible degenerate wedges) have no answer
        cmp = sr != oracle.UNCERTIFIED
        assert (sr == oracle.UNCERTIFIED).sum() <= max(1, 0.02 * B), tag
        np.testing.assert_array_equal(st[cmp], sr[cmp], err_msg=str(tag))
        assert not (st == capi.SOLVED_INACCURATE).any(), tag
        ok = sr == oracle.SOLVED
        assert not (ok & (st != capi.SOLVED)).any(), tag
        if ok.any():
            assert rel_err(u[ok], ur[ok]).max() <= TOL, tag
            assert rel_err(x[ok], xr[ok]).max() <= TOL, tag
            np.testing.assert_allclose(ob[ok], obr[ok], rtol=1e-6, atol=1e-6, err_msg=str(tag))


def test_warm_traffic_switches_off_and_back_on(oracle, capi):
    """The lane back ends' warm write-back (f110qp_kernels.h warm_traffic): on a closed-loop stream
    no key hits, so after kWarmRecent calls the masks and keys are no longer written (solves are
    then cold ones); when the linearisation points start to repeat, a probe call (every
    kWarmProbe = 32) writes them again, the next call hits, and the repeated QP is seeded with its
    own final active set (one pass, bar degenerate bounds). Every answer exact throughout."""
    N, B, T = 20, 1024, 6
    prm = oracle.params(N)
    ref = []

    def solve(x0, ul, xr):
        u, x, st = oracle.solve_batch(prm, x0, ul, xr)
        ref.append((u, x, st))
        return u

    ticks = workload.closed_loop_stream(solve, B, N, T, seed=77)
    warm = capi.Solver(capi.default_config(N, warm_start=1))
    cold = capi.Solver(capi.default_config(N))
    assert warm.backend_info(B)[0] == capi.BACKEND_LANE
    for t, w in enumerate(ticks):
        u, x, st, it = warm.solve(w["x0"], w["u_lin"], w["x_ref"])
        assert rel_err(u, ref[t][0]).max() <= TOL, t
        if t >= 3:  # write-back off: the same passes as a cold solve
            np.testing.assert_array_equal(it, cold.solve(w["x0"], w["u_lin"], w["x_ref"])[3])
    w = ticks[-1]
    its = []
    for k in range(40):  # calls T+1 .. T+40 repeat the last tick: probes at calls 32 and 33
        u, x, st, it = warm.solve(w["x0"], w["u_lin"], w["x_ref"])
        assert rel_err(u, ref[-1][0]).max() <= TOL, k
        its.append(it.mean())
    warm.close()
    cold.close()
    assert its[-1] <= 1.01 and its[-1] < its[0], its


def test_solve_batch_dev_sync_matches_async(capi):
    """f110qp_solve_batch_dev_sync returns with the results in device memory, equal to the
    asynchronous entry point's (one tick and a C2-size batch)."""
    import torch
    N = 20
    for B in (1, 1024):
        w = workload.make_batch(B, N, seed=90 + B)
        d = {k: torch.from_numpy(np.ascontiguousarray(w[k])).cuda() for k in ("x0", "u_lin", "x_ref")}
        s = capi.Solver(capi.default_config(N))
        outs = []
        for sync in (False, True):
            uo = torch.empty((B, N, 2), dtype=torch.float32, device="cuda")
            xo = torch.empty((B, N + 1, 3), dtype=torch.float32, device="cuda")
            st = torch.empty((B,), dtype=torch.int32, device="cuda")
            launch = s.prepare_dev(d["x0"], d["u_lin"], d["x_ref"], None, uo, xo, st, sync=sync)
            launch()
            if not sync:
                torch.cuda.synchronize()
            outs.append((uo.cpu().numpy(), xo.cpu().numpy(), st.cpu().numpy()))
        s.close()
        for a, b in zip(outs[0], outs[1]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("seg", ["auto", "1"])
def test_warm_hits_report_what_a_stream_reuses(capi, knob, seg):
    """f110qp_warm_hits counts what the lane back ends' warm start actually did: a repeated
    linearisation point hits on every QP; a stream whose theta0 moves every tick (the configs[4]
    closed loop) never hits, and its calls move warm traffic only for two calls after the last hit
    and on the two probe calls in every 32 (warm_traffic, f110qp_kernels.h)."""
    if seg == "1":
        knob("F110QP_LANE_SEG", "1")
    N, B = 20, 4096
    w = workload.make_batch(B, N, seed=31)
    s = capi.Solver(capi.default_config(N, warm_start=1, backend=capi.BACKEND_LANE))
    s.solve(w["x0"], w["u_lin"], w["x_ref"])  # call 1: keys written, none valid yet
    s.solve(w["x0"], w["u_lin"], w["x_ref"])  # call 2: every key repeats
    assert s.warm_hits() == (2, B)
    for k in range(40):  # calls 3..42: theta0 moves every call
        w["x0"][:, 2] += np.float32(1e-3)
        u, x, st, it = s.solve(w["x0"], w["u_lin"], w["x_ref"])
        assert (st == capi.SOLVED).all()
    assert s.warm_hits() == (4, 0)  # calls 3, 4 (within 2 of the hit) and the probes 32, 33
    s.close()
