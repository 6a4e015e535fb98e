"""The closed loop with gap rows recomputed at every tick's pose on MI355X: f110qp_find_half_spaces_dev_dbl,
the split of FindHalfSpaces into f110qp_gap_search_dev and f110qp_half_space_rows_dev, the fused plant
step f110qp_advance_scan_dev and f110qp_rollout_scan[_dev].

Bounds. Rows against the oracle: those of test_gpu_parity.py::test_half_space_kernel_adversarial (a, b
within 8 eps32 P, c within 16 eps32 P^2 for P = max(|x|, |y|) + the longer end-point range, a sign flip
only where the side test is zero to rounding, at least 95% of the rows bit-equal). Everything between
two device routes is bit equality. The per-tick solve and plant-step bounds are test_gpu_rollout.py's.
"""
import numpy as np
import pytest
import rollout_cases as rc_
import rollout_scan_cases as sc_
from halfspace_cases import adversarial_scans, scan_geometry
from test_gpu_rollout import KEYS, buffers, check_ticks, same_bits, solver
from test_gpu_rollout import rollout_dev as held_rollout_dev

from f110qp import workload

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


def scan_config(capi, nr, geom, **over):
    return capi.default_scan_config(num_ranges=nr, angle_min=geom[0], angle_increment=geom[1], angle_max=geom[2],
                                    **over)


def dev_rows(capi, cuda, st, r, geom, dbl=True, **kw):
    """find_half_spaces_dev[_dbl] on host arrays: (hs [B,2,3], lo [B], hi [B]) as numpy."""
    import torch

    B = r.shape[0]
    hs = torch.full((B, 2, 3), -7.0, dtype=torch.float32, device=cuda)
    lo = torch.full((B,), -7, dtype=torch.int32, device=cuda)
    hi = torch.full((B,), -7, dtype=torch.int32, device=cuda)
    fn = capi.find_half_spaces_dev_dbl if dbl else capi.find_half_spaces_dev
    fn(torch.from_numpy(np.ascontiguousarray(st)).to(cuda), torch.from_numpy(r).to(cuda), *geom, hs, lo, hi, **kw)
    torch.cuda.synchronize(cuda)
    return hs.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()


def split_rows(capi, cuda, st, r, geom, **kw):
    """gap_search_dev then half_space_rows_dev on host arrays: (hs [B,2,3], records [B]) as numpy."""
    import torch

    B, nr = r.shape
    sc = scan_config(capi, nr, geom, **kw)
    gap = torch.full((B, 4), -7, dtype=torch.int32, device=cuda)
    hs = torch.full((B, 2, 3), -7.0, dtype=torch.float32, device=cuda)
    capi.gap_search_dev(sc, torch.from_numpy(r).to(cuda), gap)
    capi.half_space_rows_dev(sc, gap, torch.from_numpy(np.ascontiguousarray(st)).to(cuda), hs)
    torch.cuda.synchronize(cuda)
    return hs.cpu().numpy(), gap.cpu().numpy().view(capi.GAP_RECORD_DTYPE).reshape(B)


def check_rows_against_oracle(oracle, hs, st, r, geom, lo=None, hi=None, what=""):
    """The row checks of test_half_space_kernel_adversarial on device rows hs [B,2,3] for fp64 states st
    [B,3]. Returns (rows bit-equal to the oracle's, rows compared)."""
    amin, ainc, amax = geom
    same = total = 0
    for b in range(r.shape[0]):
        rc, l1, l2, rlo, rhi = oracle.find_half_spaces(st[b], r[b], amin, ainc, amax)
        if lo is not None:
            assert (lo[b], hi[b]) == (rlo, rhi), (what, b)
        if rc != 0:
            assert np.isnan(hs[b]).all(), (what, b)
            continue
        ref = np.float32([l1, l2])
        if not np.isfinite(ref).all():  # an infinite range at an end point: inf/NaN propagate alike
            np.testing.assert_array_equal(np.isnan(hs[b]), np.isnan(ref))
            inf = np.isinf(ref)
            np.testing.assert_array_equal(hs[b][inf], ref[inf])
            continue
        P = max(abs(float(st[b, 0])), abs(float(st[b, 1]))) + max(float(r[b, rlo]), float(r[b, rhi]))
        tol = np.float64([8 * EPS32 * P, 8 * EPS32 * P, 8 * EPS32 * 2 * P * P])
        for k in range(2):
            if (np.abs(hs[b][k].astype(np.float64) - ref[k]) <= tol).all():
                continue
            flip = np.float32([-ref[k][0], -ref[k][1], 1.0 - ref[k][2]])  # (-a, -b, -c + 0.5)
            assert (np.abs(hs[b][k].astype(np.float64) - flip) <= tol).all(), (what, b, k, hs[b], ref, tol)
            cur = np.float32(st[b, 2])
            ang = [np.float32(np.float32(amin + np.float32(np.float32(i) * ainc)) + cur) for i in (rlo, rhi)]
            p1 = [np.float64(r[b, rlo]) * np.cos(np.float64(ang[0])) + st[b, 0],
                  np.float64(r[b, rlo]) * np.sin(np.float64(ang[0])) + st[b, 1]]
            p2 = [np.float64(r[b, rhi]) * np.cos(np.float64(ang[1])) + st[b, 0],
                  np.float64(r[b, rhi]) * np.sin(np.float64(ang[1])) + st[b, 1]]
            q = p2 if k == 0 else p1
            a_, b_, c_ = (float(v) for v in ref[k])
            c_ -= 0.5
            side = a_ * q[0] + b_ * q[1] + c_
            assert abs(side) <= 1e-5 * (abs(a_ * q[0]) + abs(b_ * q[1]) + abs(c_)), (what, b, k, side)
        same += int((hs[b] == ref).all())
        total += 1
    return same, total


def far_states(B, seed):
    """fp64 states about 1 km from the origin whose x and y no float32 holds (offsets below the float32
    ulp there, 6.1e-5), and the same states rounded to float32."""
    rng = np.random.default_rng(seed)
    f = np.column_stack([1000.0 + rng.uniform(-30, 30, B), -1000.0 + rng.uniform(-30, 30, B),
                         rng.uniform(-3, 3, B)]).astype(np.float32)
    d = f.astype(np.float64)
    d[:, :2] += rng.uniform(-0.45, 0.45, (B, 2)) * np.spacing(np.abs(f[:, :2])).astype(np.float64)
    assert (d.astype(np.float32) == f).all() and (d[:, :2] != f[:, :2]).all()
    return d, f


# ---- 1: the double-state entry against the oracle ------------------------------------------------

@pytest.mark.parametrize("nr,seed", [(64, 21), (200, 22), (1080, 23)])
def test_find_half_spaces_dbl_against_oracle(oracle, capi, cuda, nr, seed):
    """1: 256 adversarial scans, states 1 km out with sub-float32-ulp offsets: gap indices equal to the
    oracle's, rows within the bounds of the module docstring and >= 95% bit-equal. The float call on the
    same states rounded to float32 misses bit equality on most rows (why the double entry exists); on
    doubles that are float32 values the double call returns the float call's bits."""
    B = 256
    geom = scan_geometry(nr)
    r = adversarial_scans(B, nr, seed)
    d, f = far_states(B, seed)
    hs, lo, hi = dev_rows(capi, cuda, d, r, geom)
    same, total = check_rows_against_oracle(oracle, hs, d, r, geom, lo, hi, "double states")
    hs32, lo32, hi32 = dev_rows(capi, cuda, f, r, geom, dbl=False)
    finite = np.array([oracle.find_half_spaces(d[b], r[b], *geom)[0] == 0 for b in range(B)]) & \
        np.isfinite(hs).all(axis=(1, 2))
    ref = np.float32([oracle.find_half_spaces(d[b], r[b], *geom)[1:3] if finite[b] else np.zeros((2, 3))
                      for b in range(B)])
    miss = int((hs32[finite] != ref[finite]).any(axis=(1, 2)).sum())
    print(f"nr {nr}: {same} of {total} rows bit-equal to the oracle; the float call misses {miss} of {int(finite.sum())}")
    assert total >= B // 4 and same / total >= 0.95, (same, total)
    assert miss > finite.sum() / 2, (miss, int(finite.sum()))
    np.testing.assert_array_equal(lo32, lo)
    np.testing.assert_array_equal(hi32, hi)
    back, lo_b, hi_b = dev_rows(capi, cuda, f.astype(np.float64), r, geom)
    same_bits(back, hs32, "float32-valued doubles")
    np.testing.assert_array_equal(lo_b, lo32)
    np.testing.assert_array_equal(hi_b, hi32)


# ---- 2: split equals whole -----------------------------------------------------------------------

def _scans(B, nr, seed):
    if nr >= 8:
        return adversarial_scans(B, nr, seed), scan_geometry(nr)
    rng = np.random.default_rng(seed)  # one beam: open, short, NaN or inf, in a window of its own
    r = rng.choice(np.float32([5.0, 1.0, np.nan, np.inf]), (B, nr)).astype(np.float32)
    return r, (np.float32(-0.1), np.float32(0.2), np.float32(-0.1 + 0.2 * (nr - 1)))


def _split_equals_whole(capi, cuda, st, r, geom, what, **kw):
    hs, lo, hi = dev_rows(capi, cuda, st, r, geom, **kw)
    hs2, rec = split_rows(capi, cuda, st, r, geom, **{{"thresh": "ftg_thresh"}.get(k, k): v for k, v in kw.items()})
    same_bits(hs2, hs, what)
    np.testing.assert_array_equal(rec["lo"], lo, err_msg=what)
    np.testing.assert_array_equal(rec["hi"], hi, err_msg=what)
    nr = r.shape[1]
    nogap = (lo < 0) | (hi < 0) | (lo >= nr) | (hi >= nr)
    assert np.isnan(rec["r_lo"][nogap]).all() and np.isnan(rec["r_hi"][nogap]).all(), what
    assert np.isnan(hs[nogap]).all(), what
    ok = np.flatnonzero(~nogap)
    same_bits(rec["r_lo"][ok], r[ok, lo[ok]], what + " r_lo")
    same_bits(rec["r_hi"][ok], r[ok, hi[ok]], what + " r_hi")
    return hs, lo, hi


@pytest.mark.parametrize("nr", [1, 63, 64, 65, 1080, 1600])
def test_split_equals_whole(capi, cuda, nr):
    """2: gap_search_dev + half_space_rows_dev against find_half_spaces_dev_dbl, bit for bit (NaN rows
    included), at beam counts around the 64-beam block, at 1,080 and past the 1,536-beam register batch
    (the re-read path), for B = 1, 5 and 257 (ragged last workgroup of the 4-scan search and of the
    256-car rows kernel)."""
    for B in (1, 5, 257):
        r, geom = _scans(B, nr, 30 + nr + B)
        d, _ = far_states(B, nr + B)
        _, lo, hi = _split_equals_whole(capi, cuda, d, r, geom, f"nr {nr} B {B}")
        if B == 257 and nr >= 63:
            assert ((lo >= 0) & (hi > lo)).any() and (lo < 0).any(), "the set holds a gap and a scan without one"


def test_split_equals_whole_adversarial(capi, cuda):
    """2, the adversarial set: scans without a gap, the empty window (angle_max < angle_min: (0, 0),
    ranges[0] read, here 5, inf and NaN), inf at an end beam, and a negative buffer that moves lo and
    hi out of the scan."""
    nr = 1080
    geom = scan_geometry(nr)
    r = np.full((6, nr), 1.0, np.float32)  # 0: every beam short, (-1, -1)
    r[1, 500:600] = 5.0                    # 1: one run
    r[2, 500:600] = 5.0
    r[2, 503], r[2, 596] = np.inf, np.inf  # 2: inf at both end beams after the 3-beam inflation
    r[3, 0::2] = 5.0                       # 3: single-beam gaps only: never recorded
    r[4, :] = 5.0                          # 4: all open
    r[5, 0], r[5, 540:] = np.nan, 5.0      # 5: NaN beam 0 outside the window
    d, _ = far_states(6, 5)
    _, lo, hi = _split_equals_whole(capi, cuda, d, r, geom, "hand-built")
    assert (lo[0], hi[0]) == (-1, -1) and (lo[1], hi[1]) == (503, 596) and (lo[2], hi[2]) == (503, 596)
    empty = (geom[0], geom[1], np.float32(geom[0] - 1.0))
    r0 = np.full((3, nr), 5.0, np.float32)
    r0[1, 0], r0[2, 0] = np.inf, np.nan
    hs, lo, hi = _split_equals_whole(capi, cuda, d[:3], r0, empty, "empty window")
    assert (lo == 0).all() and (hi == 0).all() and np.isfinite(hs[0]).all() and not np.isfinite(hs[1:]).any()
    wide = (np.float32(-1.0), np.float32(2.0 / (nr - 1)), np.float32(1.0))
    _, lo, hi = _split_equals_whole(capi, cuda, d[:1], r[4:5], wide, "negative buffer", buffer=-3.0)
    assert lo[0] < 0 or hi[0] >= nr


# ---- 3: fused equals unfused ---------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 5, 20])
def test_advance_scan_is_advance_then_rows(capi, cuda, N):
    """3: advance_scan_dev's x_next, u_lin_next and u_applied have advance_dev's bits and its hs_next
    those of half_space_rows_dev at x_next; N = 1 (no u*_1), 5 (plan rows 8-byte but not 16-byte aligned)
    and 20, B = 1, 5 and 257 (a ragged second workgroup), every status mixed in, scans with and without
    a gap."""
    import torch

    nr = 200
    geom = scan_geometry(nr)
    sc = scan_config(capi, nr, geom)
    rc = capi.default_rollout_config()
    for B in (1, 5, 257):
        rng = np.random.default_rng(40 + N + B)
        x = np.column_stack([rng.uniform(-50, 50, B), rng.uniform(-50, 50, B), rng.uniform(-3, 3, B)])
        up = np.stack([rng.uniform(3.0, 4.5, (B, N)), rng.uniform(-0.43, 0.43, (B, N))], 2).astype(np.float32)
        st = rng.choice(np.int32([capi.SOLVED, capi.SOLVED, capi.SOLVED_INACCURATE, capi.MAX_ITER,
                                  capi.PRIMAL_INFEASIBLE, capi.NUMERICAL]), B).astype(np.int32)
        up[~np.isin(st, (capi.SOLVED, capi.SOLVED_INACCURATE))] = np.nan
        r = adversarial_scans(B, nr, 50 + N + B)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
        xd, upd, std = t(x), t(up), t(st)
        gap = torch.empty((B, 4), dtype=torch.int32, device=cuda)
        capi.gap_search_dev(sc, t(r), gap)
        e = lambda shape, dt: torch.full(shape, -7, dtype=dt, device=cuda)  # noqa: E731
        a = [e((B, 3), torch.float64), e((B, 2), torch.float64), e((B, 2), torch.float32)]
        f = [e((B, 3), torch.float64), e((B, 2), torch.float64), e((B, 2), torch.float32)]
        hs_f, hs_r = e((B, 2, 3), torch.float32), e((B, 2, 3), torch.float32)
        capi.advance_dev(rc, N, xd, upd, std, a[0], a[1], a[2])
        capi.half_space_rows_dev(sc, gap, a[0], hs_r)
        capi.advance_scan_dev(rc, sc, N, xd, upd, std, gap, f[0], f[1], hs_f, f[2])
        torch.cuda.synchronize(cuda)
        for name, p, q in zip(("x_next", "u_lin_next", "u_applied"), a, f):
            same_bits(q.cpu().numpy(), p.cpu().numpy(), f"N {N} B {B} {name}")
        same_bits(hs_f.cpu().numpy(), hs_r.cpu().numpy(), f"N {N} B {B} hs_next")
        assert not (hs_f == -7).any()
        if B == 257:
            nan = torch.isnan(hs_f).all(dim=2).all(dim=1)
            assert nan.any() and (~nan).any()
        # without u_applied
        g = [e((B, 3), torch.float64), e((B, 2), torch.float64)]
        capi.advance_scan_dev(rc, sc, N, xd, upd, std, gap, g[0], g[1], hs_r)
        torch.cuda.synchronize(cuda)
        same_bits(g[0].cpu().numpy(), a[0].cpu().numpy(), "x_next, no u_applied")
        same_bits(hs_r.cpu().numpy(), hs_f.cpu().numpy(), "hs_next, no u_applied")


# ---- 4: the rollout is its parts -----------------------------------------------------------------

SKEYS = KEYS + ("hs_traj",)


def rollout_scan_dev(capi, cuda, s, x0, ul, xr, ranges, geom, T, rows=True, full=True, scan_rows=1):
    """One Solver.rollout_scan_dev call on fresh device arrays; returns the recorded arrays as numpy."""
    import torch

    B, N = x0.shape[0], s.horizon
    d = buffers(torch, cuda, x0, ul, B, N, T, full)
    if rows:
        d["hs_traj"] = torch.full((T, B, 2, 3), -7.0, dtype=torch.float32, device=cuda)
    sc = scan_config(capi, ranges.shape[-1], geom, scan_rows=scan_rows)
    rg = torch.from_numpy(ranges.reshape(scan_rows, B, -1)).to(cuda)
    cfg = capi.default_rollout_config(ticks=T)
    torch.cuda.synchronize(cuda)
    s.rollout_scan_dev(cfg, sc, torch.from_numpy(xr).to(cuda), rg, d["x_traj"], d["u_lin_traj"], d["u_applied"],
                       d["status"], d.get("iters"), d.get("cost"), d.get("u_plan"), d.get("x_plan"), d.get("hs_traj"))
    torch.cuda.synchronize(cuda)
    return {k: v.cpu().numpy() for k, v in d.items()}


def manual_scan_loop(capi, cuda, s, x0, ul, xr, ranges, geom, T, scan_rows=1):
    """The loop a caller enqueues from the public calls: gap_search_dev, half_space_rows_dev for tick
    0, then per tick solve_dev_dbl and advance_scan_dev (the last tick: advance_dev)."""
    import torch

    B, N = x0.shape[0], s.horizon
    gap_on = s.config.gap_mode == capi.GAP_ACTIVE
    d = buffers(torch, cuda, x0, ul, B, N, T)
    d["hs_traj"] = torch.full((T, B, 2, 3), -7.0, dtype=torch.float32, device=cuda)
    sc = scan_config(capi, ranges.shape[-1], geom, scan_rows=scan_rows)
    rg = torch.from_numpy(ranges.reshape(scan_rows, B, -1)).to(cuda)
    xrd = torch.from_numpy(xr).to(cuda)
    gap = torch.empty((scan_rows, B, 4), dtype=torch.int32, device=cuda)
    rc = capi.default_rollout_config()
    capi.gap_search_dev(sc, rg, gap)
    capi.half_space_rows_dev(sc, gap[0], d["x_traj"][0], d["hs_traj"][0])
    for t in range(T):
        s.solve_dev_dbl(d["x_traj"][t], d["u_lin_traj"][t], xrd, d["hs_traj"][t] if gap_on else None, d["u_plan"][t],
                        d["x_plan"][t], d["status"][t], d["iters"][t], cost=d["cost"][t])
        if t + 1 < T:
            capi.advance_scan_dev(rc, sc, N, d["x_traj"][t], d["u_plan"][t], d["status"][t],
                                  gap[0 if scan_rows == 1 else t + 1], d["x_traj"][t + 1], d["u_lin_traj"][t + 1],
                                  d["hs_traj"][t + 1], d["u_applied"][t])
        else:
            capi.advance_dev(rc, N, d["x_traj"][t], d["u_plan"][t], d["status"][t], d["x_traj"][t + 1],
                             d["u_lin_traj"][t + 1], d["u_applied"][t])
    torch.cuda.synchronize(cuda)
    return {k: v.cpu().numpy() for k, v in d.items()}


PARTS = [
    ("64 cars, gap rows", 64, 20, 4, True, 1),
    ("one car, gap rows", 1, 20, 3, True, 1),
    ("one car, partitioned horizon", 1, 20, 3, False, 1),
    ("5 cars, N=5, T=2", 5, 5, 2, True, 1),
    ("one tick", 5, 20, 1, True, 1),
    ("a scan per tick", 64, 20, 4, True, 4),
]


@pytest.mark.parametrize("name,B,N,T,gap,rows", PARTS, ids=[p[0] for p in PARTS])
def test_rollout_scan_is_its_parts(capi, cuda, name, B, N, T, gap, rows):
    """4: rollout_scan_dev equals, bit for bit in every recorded array (hs_traj included), the loop of
    the public calls; without hs_traj the other arrays keep their bits; the host-pointer rollout_scan
    returns the device call's bits. scan_rows = T: a different scan in each row, tick t reads row t."""
    x0, ul, xr = rc_.start(B, N, seed=sc_.SCAN_SEED)
    made = [workload.make_scans(B, seed=sc_.SCAN_SEED + 2 + 10 * k) for k in range(rows)]
    geom = made[0][1:]
    ranges = np.stack([m[0] for m in made]) if rows > 1 else made[0][0]
    s = solver(capi, N, gap=gap)
    if not gap and B == 1:
        assert s.backend_info(B)[0] == capi.BACKEND_LANE and s.lane_segments(B) > 1
    a = rollout_scan_dev(capi, cuda, s, x0, ul, xr, ranges, geom, T, scan_rows=rows)
    m = manual_scan_loop(capi, cuda, s, x0, ul, xr, ranges, geom, T, scan_rows=rows)
    lean = rollout_scan_dev(capi, cuda, s, x0, ul, xr, ranges, geom, T, rows=False, scan_rows=rows)
    sc = scan_config(capi, ranges.shape[-1], geom, scan_rows=rows)
    host = s.rollout_scan(x0, ul, xr, ranges, sc, T, plans=True, objective=True)
    host_lean = s.rollout_scan(x0, ul, xr, ranges, sc, T, rows=False)
    s.close()
    assert set(a) == set(SKEYS) == set(host) and "hs_traj" not in lean and "hs_traj" not in host_lean
    for k in SKEYS:
        same_bits(a[k], m[k], f"{name}: manual loop, {k}")
        same_bits(host[k], a[k], f"{name}: host rollout, {k}")
    for k in KEYS:
        same_bits(lean[k], a[k], f"{name}: no hs_traj, {k}")
    for k in host_lean:
        same_bits(host_lean[k], a[k], f"{name}: lean host rollout, {k}")
    assert np.isfinite(a["hs_traj"]).all()
    if B == 64:
        assert (a["status"] == capi.SOLVED).mean() >= 0.5
    if T > 1:  # the rows moved with the cars
        assert (a["hs_traj"][1:] != a["hs_traj"][:-1]).any(axis=(2, 3)).all()
    if rows > 1:  # ... and tick t read row t: not the rows of row 0's scan at the same pose
        s = solver(capi, N, gap=gap)
        one = rollout_scan_dev(capi, cuda, s, x0, ul, xr, ranges[0], geom, T)
        s.close()
        same_bits(one["x_traj"][:2], a["x_traj"][:2], "tick 0 reads row 0")
        assert (one["hs_traj"][1] != a["hs_traj"][1]).any(axis=(1, 2)).all()


# ---- 5: against the oracle, per tick -------------------------------------------------------------

def test_rollout_scan_against_oracle(oracle, capi, cuda):
    """5: 64 x N=20 x 4 ticks, gap_mode ACTIVE, one workload.make_scans scan per car held over the call,
    seed rollout_scan_cases.SCAN_SEED = 1: the first seed from 1 that met rollout_scan_cases.
    scan_seed_is_robust on the CPU (oracle loop with the rows recomputed from each tick's fp64 pose: no
    pair uncertified; 256 of 256 pairs SOLVED; no pair changes status when its pose moves by +-1e-6 in
    any coordinate, rows recomputed; 90 of the 192 pairs with t >= 1 have a u* more than 1e-3 (relative,
    u_inf) from the same solve with the car's tick-0 rows, the largest 0.111 at tick 3, car 26).
    Per tick, from the recorded arrays: hs_traj[t] against oracle.find_half_spaces(x_traj[t]); the oracle
    solved on (x_traj[t], u_lin_traj[t], hs_traj[t]) gives the status, u within U_TOL and the plant step
    within its bound (test_gpu_rollout.check_ticks); and the pair with the largest difference in the
    oracle loop shows on the device: its rows moved and its u is the per-tick rows', not the tick-0
    rows'."""
    B, N, T = 64, 20, 4
    x0, ul, xr, ranges, geom = sc_.scan_case(sc_.SCAN_SEED, B, N)
    s = solver(capi, N, gap=True)
    out = rollout_scan_dev(capi, cuda, s, x0, ul, xr, ranges, geom, T)
    s.close()
    same = total = 0
    for t in range(T):
        sm, tt = check_rows_against_oracle(oracle, out["hs_traj"][t], out["x_traj"][t], ranges, geom, what=f"tick {t}")
        same, total = same + sm, total + tt
        tick = {k: out[k][t : t + (2 if k in ("x_traj", "u_lin_traj") else 1)] for k in KEYS}
        sts, _, _ = check_ticks(oracle, capi, tick, xr, out["hs_traj"][t], N, gap=True, what=f"scan rows, tick {t}")
        assert (sts == oracle.SOLVED).mean() >= 0.5
    print(f"{same} of {total} recorded rows bit-equal to the oracle's")
    assert total == T * B and same / total >= 0.95, (same, total)
    xs, uls, hss, sts, us = sc_.oracle_scan_loop(oracle, x0, ul, xr, ranges, geom, N, T)
    pairs = sc_.rows_matter(oracle, xs, uls, xr, hss, sts, us, N)
    assert pairs, "the seed no longer holds a pair whose tick-0 rows give another answer"
    d, t, b = pairs[0]
    assert t >= 1 and (out["hs_traj"][t, b] != out["hs_traj"][0, b]).any()
    r0 = oracle.solve(oracle.params(N), out["x_traj"][t, b], out["u_lin_traj"][t, b], xr[b, :N], out["hs_traj"][0, b], True)
    u_dev = out["u_plan"][t, b].astype(np.float64)
    print(f"pair (tick {t}, car {b}): oracle-loop difference {d:.4f}; with the tick-0 rows status {r0['status']}, "
          f"device status {out['status'][t, b]}")
    assert out["status"][t, b] != r0["status"] or sc_.u_differs(u_dev, r0["u"])


# ---- 6: the failure branch -----------------------------------------------------------------------

_failure = {}


def _failure_case(capi, cuda):
    """(dead, reference run, run with every fourth car's scan short everywhere), computed once."""
    if not _failure:
        B, N, T = 64, 20, 3
        x0, ul, xr, ranges, geom = sc_.scan_case(sc_.SCAN_SEED, B, N)
        dead = np.arange(B) % 4 == 0
        bad = ranges.copy()
        bad[dead] = 1.0
        s = solver(capi, N, gap=True)
        ref = rollout_scan_dev(capi, cuda, s, x0, ul, xr, ranges, geom, T)
        out = rollout_scan_dev(capi, cuda, s, x0, ul, xr, bad, geom, T)
        s.close()
        _failure.update(dead=dead, ref=ref, out=out)
    return _failure["dead"], _failure["ref"], _failure["out"]


def test_rollout_scan_failure_status_is_numerical(capi, cuda):
    """6, the status: a car whose scan has no gap (NaN rows) reports F110QP_NUMERICAL at every tick, on
    the host-pointer call as well. The solve calls themselves keep PRIMAL_INFEASIBLE for non-finite rows
    (tests/test_gpu_screen.py::test_screen_infeasible_and_non_finite): solve_dev_dbl on the rows and
    inputs this rollout recorded for tick 0 says so, with every other output bit-equal."""
    import torch

    dead, _, out = _failure_case(capi, cuda)
    print("statuses of the cars without a gap:", np.unique(out["status"][:, dead], return_counts=True))
    assert (out["status"][:, dead] == capi.NUMERICAL).all(), out["status"][:, dead]
    B, N = dead.size, 20
    x0, ul, xr, ranges, geom = sc_.scan_case(sc_.SCAN_SEED, B, N)
    bad = ranges.copy()
    bad[dead] = 1.0
    s = solver(capi, N, gap=True)
    host = s.rollout_scan(x0, ul, xr, bad, scan_config(capi, bad.shape[-1], geom), 3, plans=True, objective=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    uo = torch.empty((B, N, 2), dtype=torch.float32, device=cuda)
    xo = torch.empty((B, N + 1, 3), dtype=torch.float32, device=cuda)
    st = torch.empty(B, dtype=torch.int32, device=cuda)
    s.solve_dev_dbl(t(x0), t(ul), t(xr), t(out["hs_traj"][0]), uo, xo, st)
    torch.cuda.synchronize(cuda)
    s.close()
    for k in SKEYS:
        same_bits(host[k], out[k], f"host rollout, {k}")
    st = st.cpu().numpy()
    assert (st[dead] == capi.PRIMAL_INFEASIBLE).all(), st[dead]
    np.testing.assert_array_equal(st[~dead], out["status"][0, ~dead])
    same_bits(uo.cpu().numpy(), out["u_plan"][0], "tick-0 plan")
    same_bits(xo.cpu().numpy(), out["x_plan"][0], "tick-0 states")


def test_rollout_scan_failure_branch(capi, cuda):
    """6: every fourth car's scan has no gap (every beam short): its rows are NaN at every tick, its
    solve is not usable (NaN plan), it applies fail_u; the other cars are bit-equal to a run in which
    the bad cars keep their scans."""
    T = 3
    dead, ref, out = _failure_case(capi, cuda)
    for k in SKEYS:
        same_bits(out[k][:, ~dead], ref[k][:, ~dead], f"live cars, {k}")
    assert (ref["status"] == capi.SOLVED).all()
    n = int(dead.sum())
    assert np.isnan(out["hs_traj"][:, dead]).all()
    assert not np.isin(out["status"][:, dead], (capi.SOLVED, capi.SOLVED_INACCURATE)).any(), out["status"][:, dead]
    assert np.isnan(out["u_plan"][:, dead]).all() and np.isnan(out["x_plan"][:, dead]).all()
    for t in range(T):
        same_bits(out["u_applied"][t, dead], np.tile(np.float32(rc_.FAIL_U), (n, 1)))
        same_bits(out["u_lin_traj"][t + 1, dead], np.tile([rc_.V_LIN, rc_.FAIL_U[1]], (n, 1)))
        exp = rc_.plant_step(out["x_traj"][t, dead], np.tile(rc_.FAIL_U, (n, 1)))
        err = np.abs(out["x_traj"][t + 1, dead] - exp)
        assert (err <= 2 * np.spacing(np.abs(exp)) + 2e-16).all(), float(err.max())


# ---- 7: gap rows inactive ------------------------------------------------------------------------

def test_rollout_scan_gap_inactive(capi, cuda):
    """7: gap_mode INACTIVE. With hs_traj recorded every other array has rollout_dev's bits and row t of
    hs_traj those of find_half_spaces_dev_dbl at x_traj[t]; without hs_traj (rollout_dev's launches) the
    arrays keep those bits too."""
    B, N, T = 64, 20, 4
    x0, ul, xr, ranges, geom = sc_.scan_case(sc_.SCAN_SEED, B, N)
    s = solver(capi, N)
    held = held_rollout_dev(capi, cuda, s, x0, ul, xr, None, T)
    out = rollout_scan_dev(capi, cuda, s, x0, ul, xr, ranges, geom, T)
    lean = rollout_scan_dev(capi, cuda, s, x0, ul, xr, ranges, geom, T, rows=False, full=False)
    s.close()
    for k in KEYS:
        same_bits(out[k], held[k], k)
    for k in lean:
        same_bits(lean[k], held[k], f"no hs_traj, {k}")
    for t in range(T):
        hs, _, _ = dev_rows(capi, cuda, out["x_traj"][t], ranges, geom)
        same_bits(out["hs_traj"][t], hs, f"rows of tick {t}")
    assert np.isfinite(out["hs_traj"]).all()
