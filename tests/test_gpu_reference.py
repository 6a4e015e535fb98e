"""The device kernels against the reference's own compiled tick (tests/golden/ref_*.npz, recorded by
tests/golden/make_ref_golden.py from the reference's unmodified sources; see
tests/test_reference_parity.py). Only the fixtures are read: no reference checkout, no driver.

Every tolerance is the one the suite already applies to the same comparison against the oracle; the
test it is taken from is named next to it. Tick fixtures hold 4 instances x 2 calls per group;
instances 0 and 1 are float32 values throughout (the float entry points get exactly the recorded
QP), instances 2 and 3 carry positions no float32 holds (double entry points only).
"""
import os

import numpy as np
import pytest
from conftest import GOLDEN
from ref_cases import condense_captured, dense
from test_gpu_parity import TOL, rel_err

pytestmark = pytest.mark.gpu

QP_KEYS = ("P_colptr", "P_rowind", "P_val", "q", "A_colptr", "A_rowind", "A_val", "l", "u")
OVER = {"default": {}, "unequal": dict(q=(3.0, 25.0, 0.0), r=(0.7, 2.0), dt=float(np.float32(0.05)))}


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def groups(d):
    for g in d["groups"]:
        name, N, S, pset = str(g).split(":")
        yield name, int(N), int(S), pset


GROUPS = list(groups(load("ref_tick")))


def config(capi, N, S, pset, **cfg):
    return capi.default_config(N, x_ref_points=S if S != N else 0, **OVER[pset], **cfg)


def qp_of(d, name, b, c):
    return {k: d[f"{name}_{k}"][b, c] for k in QP_KEYS}


def rows_of(qp, N):
    """The half-space rows (a, b) of a captured A (stage 1's gap block), as the float32 [2,3] array
    the entry points take; the third entry is not read with inactive gap rows."""
    ns = 3 * (N + 1)
    A = dense(qp["A_colptr"], qp["A_rowind"], qp["A_val"], 7 * N + 5, 5 * N + 3)
    hs = np.zeros((2, 3), np.float32)
    hs[:, :2] = A[ns + 2:ns + 4, 3:5]
    return hs


@pytest.mark.parametrize("name,N,S,pset", GROUPS)
def test_assembly_hook_equals_captured_qp(capi, name, N, S, pset):
    """f110qp_assemble_debug_dev against what MPC::Update handed to the solver, compared as
    test_assembly_hook_matches_reference_layout compares. Would catch: the terminal gradient on
    x_ref[N] instead of x_ref[N-1], a stage-0 gap block that is overwritten, dropped explicit zeros."""
    d = load("ref_tick")
    s = capi.Solver(config(capi, N, S, pset))
    for b in (0, 1):
        for c in range(2):
            ref = qp_of(d, name, b, c)
            got = s.assemble_debug(d[f"{name}_x0"][b, c], d[f"{name}_u_lin"][b, c], d[f"{name}_x_ref"][b, c], rows_of(ref, N))
            for k in ("P_colptr", "P_rowind", "A_colptr", "A_rowind", "P_val", "q"):
                np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k}, instance {b} call {c}")
            for k in ("A_val", "l", "u"):  # A, B, C entries carry the device/host sin/cos ulp
                np.testing.assert_allclose(got[k], ref[k], rtol=1e-15, atol=1e-18, err_msg=f"{k}, instance {b} call {c}")
            assert (got["A_val"] == 0).sum() == (ref["A_val"] == 0).sum()
            assert (got["P_val"] == 0).sum() == (ref["P_val"] == 0).sum()
    s.close()


@pytest.mark.parametrize("name,N,S,pset", GROUPS)
def test_condensing_matches_captured_qp(capi, cuda, name, N, S, pset):
    """f110qp_condense_debug_dev against the condensation of the captured matrices, at the tolerances of
    test_condensed_hessian_and_gradient. Would catch: a wrong power of A in the closed form, dt or L
    read as double, the terminal weight on the wrong reference point."""
    import torch

    d = load("ref_tick")
    s = capi.Solver(config(capi, N, S, pset))
    for c in range(2):
        t = {k: torch.from_numpy(np.ascontiguousarray(d[f"{name}_{k}"][:2, c], np.float32)).to(cuda) for k in ("x0", "u_lin", "x_ref")}
        H = torch.empty((2, 2 * N, 2 * N), dtype=torch.float64, device=cuda)
        g = torch.empty((2, 2 * N), dtype=torch.float64, device=cuda)
        s.condense_debug_dev(t["x0"], t["u_lin"], t["x_ref"], H, g)
        torch.cuda.synchronize()
        H, g = H.cpu().numpy(), g.cpu().numpy()
        for b in (0, 1):
            cc = condense_captured(qp_of(d, name, b, c), N)  # states eliminated through the captured rows
            Hr, gr = cc["H"], cc["g"]
            np.testing.assert_allclose(H[b], Hr, rtol=2e-6, atol=2e-6 * np.abs(Hr).max())
            np.testing.assert_allclose(g[b], gr, rtol=1e-9, atol=1e-9 * np.abs(gr).max())
    s.close()


# ---- FindHalfSpaces --------------------------------------------------------------------------------

def scan_batches(d):
    """The scans of ref_halfspace.npz grouped by beam count: (indices, ranges [B,R], geometry)."""
    off = np.r_[0, np.cumsum(d["beams"])]
    for nr in np.unique(d["beams"]):
        idx = np.where(d["beams"] == nr)[0]
        yield idx, np.stack([d["ranges"][off[k]:off[k + 1]] for k in idx]), d["geom"][idx[0]]


BIT_EQUAL = {}  # route -> [scans whose six coefficients have the reference's bits, scans]


def close_rows(hs, l1, l2, what, route=None):
    """test_half_space_kernel's rtol = 2e-6, atol = 2e-6 max|ref| per scan; with `route`, also counts the
    scans that are bit-equal to the reference (bit_equal_share)."""
    for b in range(hs.shape[0]):
        ref = np.float32([l1[b], l2[b]])
        np.testing.assert_allclose(hs[b], ref, rtol=2e-6, atol=2e-6 * np.abs(ref).max(), err_msg=f"{what}, scan {b}")
        if route is not None:
            n = BIT_EQUAL.setdefault(route, [0, 0])
            n[0] += int((hs[b].view(np.uint32) == ref.view(np.uint32)).all())
            n[1] += 1


def bit_equal_share(route, total):
    """As test_half_space_kernel_adversarial asks of the kernel against the oracle: at least 95% of
    the rows bit-equal. The tolerance above cannot see a float rounded in another place (half a
    float32 ulp of an angle moves an end point by 1e-6 m), the bits can: device and host differ only
    in the last bits of a double sin / cos, which rarely survive the rounding to float32."""
    same, n = BIT_EQUAL.pop(route)
    assert n == total and same >= 0.95 * n, (route, same, n)


def test_find_half_spaces_kernels_match_reference(capi, cuda):
    """f110qp_find_half_spaces_dev on float32-rounded poses, _dev_dbl on the double poses, and
    f110qp_gap_search_dev + f110qp_half_space_rows_dev, against the reference's l1, l2 (the build whose
    cos(float) is the double function, which the kernels assume). The gap indices are not recorded
    (locals of the reference's function): the three routes must agree on them. Would catch: a
    double current_angle, float products where the reference widens (or the reverse), a side test
    evaluated in another order (the 20 km scans are decided by float32 rounding), the buffer shrink
    off by one, a run at the window edge."""
    import torch

    d = load("ref_halfspace")
    assert (d["params"] == np.float32([3.0, 1.5, 3.0])).all()
    for idx, ranges, geom in scan_batches(d):
        B, R = ranges.shape
        rd = torch.from_numpy(ranges).to(cuda)
        pose64 = np.ascontiguousarray(d["poses"][idx])
        out = {}
        for key, fn, st in (("f32", capi.find_half_spaces_dev, pose64.astype(np.float32)),
                            ("f64", capi.find_half_spaces_dev_dbl, pose64)):
            hs = torch.empty((B, 2, 3), dtype=torch.float32, device=cuda)
            lo = torch.empty(B, dtype=torch.int32, device=cuda)
            hi = torch.empty(B, dtype=torch.int32, device=cuda)
            fn(torch.from_numpy(st).to(cuda), rd, geom[0], geom[1], geom[2], hs, lo, hi)
            torch.cuda.synchronize()
            out[key] = hs.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
        close_rows(out["f32"][0], d["l1_f32pose"][idx], d["l2_f32pose"][idx], f"float poses, {R} beams", "f32")
        close_rows(out["f64"][0], d["l1"][idx], d["l2"][idx], f"double poses, {R} beams", "f64")
        sc = capi.default_scan_config(num_ranges=R, angle_min=geom[0], angle_increment=geom[1], angle_max=geom[2])
        gap = torch.empty((B, 4), dtype=torch.int32, device=cuda)
        hs = torch.empty((B, 2, 3), dtype=torch.float32, device=cuda)
        capi.gap_search_dev(sc, rd, gap)
        capi.half_space_rows_dev(sc, gap, torch.from_numpy(pose64).to(cuda), hs)
        torch.cuda.synchronize()
        close_rows(hs.cpu().numpy(), d["l1"][idx], d["l2"][idx], f"gap search + rows, {R} beams", "split")
        rec = gap.cpu().numpy().view(capi.GAP_RECORD_DTYPE).reshape(B)
        for key in ("f32", "f64"):
            np.testing.assert_array_equal(out[key][1], rec["lo"])
            np.testing.assert_array_equal(out[key][2], rec["hi"])
        assert (rec["hi"] > rec["lo"]).all() and (rec["lo"] > 0).all()  # every recorded scan holds a gap
    for route in ("f32", "f64", "split"):
        bit_equal_share(route, len(d["beams"]))


def test_advance_scan_rows_match_reference(capi, cuda):
    """f110qp_advance_scan_dev's hs_next: for every recorded scan a start state and a two-entry plan are
    constructed (numpy fp64) so that one plant step of the plan's first input lands on the recorded
    pose; hs_next against the recorded l1, l2 at test_half_space_kernel's tolerance, x_next against
    the recorded pose at the plant bound. Would catch: rows taken at the start pose instead of x_next,
    a double current_angle or another rounding of the end points in the fused kernel."""
    import torch

    d = load("ref_halfspace")
    rc = capi.default_rollout_config()
    L, dt, N = float(rc.car_length), float(rc.plant_dt), 2
    for idx, ranges, geom in scan_batches(d):
        B, R = ranges.shape
        pose = np.ascontiguousarray(d["poses"][idx])
        plan = np.zeros((B, N, 2), np.float32)
        plan[:, 0, 0] = np.float32(4.5)
        plan[:, 0, 1] = np.linspace(-0.4, 0.4, B).astype(np.float32)
        plan[:, 1] = np.float32([4.0, 0.1])
        v, st = plan[:, 0, 0].astype(np.float64), plan[:, 0, 1].astype(np.float64)
        th0 = pose[:, 2] - np.tan(st) * v / L * dt
        x = np.stack([pose[:, 0] - v * np.cos(th0) * dt, pose[:, 1] - v * np.sin(th0) * dt, th0], 1)
        sc = capi.default_scan_config(num_ranges=R, angle_min=geom[0], angle_increment=geom[1], angle_max=geom[2])
        gap = torch.empty((B, 4), dtype=torch.int32, device=cuda)
        capi.gap_search_dev(sc, torch.from_numpy(ranges).to(cuda), gap)
        xn = torch.full((B, 3), -7.0, dtype=torch.float64, device=cuda)
        uln = torch.full((B, 2), -7.0, dtype=torch.float64, device=cuda)
        hs = torch.full((B, 2, 3), -7.0, dtype=torch.float32, device=cuda)
        status = torch.full((B,), capi.SOLVED, dtype=torch.int32, device=cuda)
        capi.advance_scan_dev(rc, sc, N, torch.from_numpy(x).to(cuda), torch.from_numpy(plan).to(cuda), status, gap,
                              xn, uln, hs)
        torch.cuda.synchronize()
        # landing: the constructed start adds one subtraction's rounding to the step's own
        err = np.abs(xn.cpu().numpy() - pose)
        assert (err <= plant_bound(pose) + np.spacing(np.abs(pose))).all(), float(err.max())
        close_rows(hs.cpu().numpy(), d["l1"][idx], d["l2"][idx], f"advance_scan hs_next, {R} beams")
        # not counted bit for bit: the constructed step lands within rounding of the recorded pose, not on it


# ---- plant step ------------------------------------------------------------------------------------

def plant_bound(exp):
    """The bound written at the top of tests/test_gpu_rollout.py, unchanged: 2 spacing(|expected|) + 2e-16."""
    return 2 * np.spacing(np.abs(exp)) + 2e-16


def test_plant_step_matches_reference_simulate_dynamics(capi, cuda):
    """f110qp_advance_dev against the recorded Model::simulate_dynamics (inputs rounded to float32 as a
    plan holds them), per recorded dt, every row at the bound of tests/test_gpu_rollout.py although the
    rows reach increments beyond the 0.06 that bound was derived for (v = 7, dt = 0.05f, steer 0.6):
    measured, the device's step equals the host's bit for bit on all of them. u_lin_next = (4.5, steer of the plan's second entry; of its
    first when N == 1). Would catch: car_length 0.3302 in the plant, a fused multiply-add, the
    float dt widened differently, the N == 1 rule."""
    import torch

    d = load("ref_model")
    rows, exp = d["rows"], d["sim_f32u"]
    for N in (1, 3):
        for dt in np.unique(rows[:, 5]):
            sel = np.where(rows[:, 5] == dt)[0]
            B = len(sel)
            plan = np.full((B, N, 2), 0.25, np.float32) + np.arange(N, dtype=np.float32)[None, :, None] / 64
            plan[:, 0] = rows[sel, 3:5].astype(np.float32)
            rc = capi.default_rollout_config(plant_dt=float(dt))
            x = torch.from_numpy(np.ascontiguousarray(rows[sel, :3])).to(cuda)
            xn = torch.full((B, 3), -7.0, dtype=torch.float64, device=cuda)
            uln = torch.full((B, 2), -7.0, dtype=torch.float64, device=cuda)
            ua = torch.full((B, 2), -7.0, dtype=torch.float32, device=cuda)
            st = torch.full((B,), capi.SOLVED, dtype=torch.int32, device=cuda)
            capi.advance_dev(rc, N, x, torch.from_numpy(plan).to(cuda), st, xn, uln, ua)
            torch.cuda.synchronize()
            err = np.abs(xn.cpu().numpy() - exp[sel])
            bound = plant_bound(exp[sel])
            print(f"N {N} dt {dt:.9g}: worst error at {float((err / bound).max()):.3f} of its bound")
            assert (err <= bound).all(), (N, dt, float((err / bound).max()))
            np.testing.assert_array_equal(ua.cpu().numpy(), plan[:, 0])
            want = np.stack([np.full(B, 4.5), plan[:, 1 if N > 1 else 0, 1].astype(np.float64)], 1)
            np.testing.assert_array_equal(uln.cpu().numpy(), want)


def test_plant_step_follows_recorded_loop(capi, cuda):
    """f110qp_advance_dev on the recorded loop's plans (rounded to float32): x_next against the
    recorded next state at the plant bound (unscaled: v <= 4.5, dt = 0.01), u_lin_next against the
    recorded next input (its steer is the double the reference's solve returned; the device holds it
    as float32: half a float32 ulp). Would catch: the next input taken from plan[0] or plan[2], v not
    forced to 4.5."""
    import torch

    d = load("ref_loop")
    N, T = int(d["horizon"]), int(d["ticks"])
    B = d["x"].shape[0]
    rc = capi.default_rollout_config()
    for t in range(T):
        plan = d["plan"][:, t].astype(np.float32)
        xn = torch.empty((B, 3), dtype=torch.float64, device=cuda)
        uln = torch.empty((B, 2), dtype=torch.float64, device=cuda)
        st = torch.full((B,), capi.SOLVED, dtype=torch.int32, device=cuda)
        capi.advance_dev(rc, N, torch.from_numpy(np.ascontiguousarray(d["x"][:, t])).to(cuda),
                         torch.from_numpy(plan).to(cuda), st, xn, uln, None)
        torch.cuda.synchronize()
        err = np.abs(xn.cpu().numpy() - d["x"][:, t + 1])
        assert (err <= plant_bound(d["x"][:, t + 1])).all(), t
        uln = uln.cpu().numpy()
        np.testing.assert_array_equal(uln[:, 0], d["u_lin"][:, t + 1, 0])
        assert (np.abs(uln[:, 1] - d["u_lin"][:, t + 1, 1]) <= 0.5 * np.spacing(np.abs(plan[:, 1, 1])).astype(np.float64)).all()


# ---- solve -----------------------------------------------------------------------------------------

ROUTES = [  # name, knobs, backend
    ("auto", {}, None),
    ("wave", {}, "WAVE"),
    ("sequential lane", {"F110QP_LANE_SEG": 1}, "LANE"),
    ("segmented lane", {"F110QP_LANE_SEG": 4, "F110QP_SEG_FIXEDQ": 1}, "LANE"),  # horizons of 20 and more
]
SOLVE_CASES = [g + r for g in GROUPS for r in ROUTES if r[0] != "segmented lane" or g[1] >= 20]


def check_solutions(capi, out, zs, P, qs, N, what):
    """u and x against z_star at TOL (test_gpu_parity.check), obj against 1/2 z*'Pz* + q'z* of the
    captured matrices at rtol 1e-6, status SOLVED wherever the recorder certified z_star (everywhere)."""
    u, x, st, it, obj, cost = out
    ns = 3 * (N + 1)
    assert len(zs) == len(st)
    for k, (z, q) in enumerate(zip(zs, qs)):
        assert st[k] == capi.SOLVED, (what, k, st[k])
        eu = rel_err(u[k][None], z[ns:].reshape(1, N, 2))[0]
        ex = rel_err(x[k][None], z[:ns].reshape(1, N + 1, 3))[0]
        assert eu <= TOL and ex <= TOL, (what, k, eu, ex)
        np.testing.assert_allclose(obj[k], 0.5 * z @ P @ z + q @ z, rtol=1e-6, err_msg=f"{what} obj {k}")


def route_solver(capi, knob, cfg, N, pset, route, knobs, backend):
    for k, v in knobs.items():
        knob(k, v)
    s = capi.Solver(cfg({} if backend is None else {"backend": getattr(capi, "BACKEND_" + backend)}))
    if route == "segmented lane":
        assert s.test_build and s.lane_segments(8) == 4
        if N == 20 and pset == "default":  # the fixed five-stage segments (default weights and dt only)
            assert s.lane_fixed_q(8) == 5
    return s


def batch_of(d, name, inst, dtype):
    return [np.ascontiguousarray(np.concatenate([d[f"{name}_{k}"][inst, c] for c in range(2)]), dtype)
            for k in ("x0", "u_lin", "x_ref")]


@pytest.mark.parametrize("name,N,S,pset,route,knobs,backend", SOLVE_CASES, ids=[f"{c[0]}-{c[4]}" for c in SOLVE_CASES])
def test_solves_match_captured_optimum(capi, knob, name, N, S, pset, route, knobs, backend):
    """solve_batch (float instances), solve_batch_dbl (all instances) and solve_grouped (one group per
    distinct model) against the optimum of the captured matrices, on every route. Would catch: any
    misreading of P, q, A, l, u shared by the kernels and the oracle: a terminal weight on x_ref[N],
    bounds of 0.43 instead of 0.43f, dt or L as doubles."""
    d = load("ref_tick")
    s = route_solver(capi, knob, lambda c: config(capi, N, S, pset, **c), N, pset, route, knobs, backend)
    n = 5 * N + 3
    P = dense(d[f"{name}_P_colptr"][0, 0], d[f"{name}_P_rowind"][0, 0], d[f"{name}_P_val"][0, 0], n, n)

    def expected(inst):
        order = [(b, c) for c in range(2) for b in inst]
        return [d[f"{name}_z_star"][b, c] for b, c in order], [d[f"{name}_q"][b, c] for b, c in order]

    x0, ul, xr = batch_of(d, name, [0, 1], np.float32)
    zs, qs = expected([0, 1])
    check_solutions(capi, s.solve(x0, ul, xr, objective=True), zs, P, qs, N, f"{route} solve_batch")
    check_solutions(capi, s.solve_grouped(x0, ul, xr, np.arange(4), objective=True), zs, P, qs, N, f"{route} solve_grouped")
    x0, ul, xr = batch_of(d, name, [0, 1, 2, 3], np.float64)
    zs, qs = expected([0, 1, 2, 3])
    check_solutions(capi, s.solve_dbl(x0, ul, xr, objective=True), zs, P, qs, N, f"{route} solve_batch_dbl")
    s.close()


@pytest.mark.parametrize("route,knobs,backend", ROUTES, ids=[r[0] for r in ROUTES])
def test_solves_match_captured_optimum_loop_ticks(capi, knob, route, knobs, backend):
    """Every tick of the recorded loop (4 cars x 8 ticks) through solve_batch_dbl on the recorded
    doubles, and through solve_batch and solve_grouped on their float32 roundings, on every route, u, x
    and obj against z_star of the captured matrices. The recorded positions are doubles no float32
    holds, so the float entry points solve a QP whose start is moved by at most half a float32 ulp of
    50 m (2e-6 m), far inside TOL max(1, |x|). Would catch: what test_solves_match_captured_optimum
    names, on QPs whose start state came out of the reference's own loop (steer bound active on the
    first ticks of two cars)."""
    d = load("ref_loop")
    N, T = int(d["horizon"]), int(d["ticks"])
    B = d["x"].shape[0]
    n = 5 * N + 3
    s = route_solver(capi, knob, lambda c: capi.default_config(N, **c), N, "default", route, knobs, backend)
    P = dense(d["P_colptr"], d["P_rowind"], d["P_val"], n, n)
    x0 = d["x"][:, :T].reshape(B * T, 3).copy()
    ul = d["u_lin"][:, :T].reshape(B * T, 2).copy()
    xr = np.ascontiguousarray(np.repeat(d["x_ref"][:, None], T, 1).reshape(B * T, N, 3))
    zs, qs = d["z_star"].reshape(B * T, n), d["q"].reshape(B * T, n)
    check_solutions(capi, s.solve_dbl(x0, ul, xr, objective=True), zs, P, qs, N, f"{route} solve_batch_dbl")
    f = [np.ascontiguousarray(a, np.float32) for a in (x0, ul, xr)]
    check_solutions(capi, s.solve(*f, objective=True), zs, P, qs, N, f"{route} solve_batch")
    check_solutions(capi, s.solve_grouped(*f, np.arange(B * T), objective=True), zs, P, qs, N, f"{route} solve_grouped")
    s.close()


# ---- closed loop -----------------------------------------------------------------------------------

def one_step_allowance(d, t):
    """What one tick may add to the difference between the device loop and the recorded one, derived as
    rollout_cases / test_gpu_rollout derive theirs: the solve's TOL propagated through the plant step.
    From the same start, tick t's applied input and next steer differ from the recorded ones by at
    most du = TOL max(1, |u*|_inf) per component. One plant step
    x + dt (v cos th, v sin th, tan(d) v / L) then moves by at most dt du in x and y, and by
    dt (du tan|d| + |v| du / cos^2 d) / L = 0.01 (0.459 + 5.45) / 0.35 du = 0.169 du in th
    (|v| <= 4.5, |d| <= 0.43); plus the plant step's own rounding. Returns (du, [dx, dy, dth, dsteer])."""
    du = TOL * max(1.0, float(np.abs(d["plan"][:, t]).max()))
    x1 = np.abs(d["x"][:, t + 1])
    return du, np.concatenate([np.array([0.01 * du, 0.01 * du, 0.169 * du]) + 4 * np.spacing(x1),
                               np.full((x1.shape[0], 1), du)], 1)


def loop_gains(oracle, d, b, t, h=1e-5):
    """First-order sensitivity of tick t's closed-loop map (x, y, th, steer_lin) -> (next state, next
    steer_lin) and -> applied input, at car b's recorded point: central differences of the exact map
    (oracle solve, asserted equal to the reference's QP in test_reference_parity.py, then the numpy
    plant step). Returns (|K| [4,4], |Ku| [2,4])."""
    prm = oracle.params(int(d["horizon"]))
    xr = d["x_ref"][b]

    def F(s):
        r = oracle.solve(prm, s[:3], [4.5, s[3]], xr)
        assert r["status"] == oracle.SOLVED
        ua = r["u"][0]
        x2 = s[:3] + 0.01 * np.array([ua[0] * np.cos(s[2]), ua[0] * np.sin(s[2]), np.tan(ua[1]) * ua[0] / 0.35])
        return np.r_[x2, r["u"][1, 1]], ua

    s0 = np.r_[d["x"][b, t], d["u_lin"][b, t, 1]]
    K, Ku = np.zeros((4, 4)), np.zeros((2, 4))
    for j in range(4):
        e = np.zeros(4)
        e[j] = h
        (fp, up), (fm, um) = F(s0 + e), F(s0 - e)
        K[:, j], Ku[:, j] = (fp - fm) / (2 * h), (up - um) / (2 * h)
    return np.abs(K), np.abs(Ku)


@pytest.mark.parametrize("scan", [False, True], ids=["rollout_dev", "rollout_scan_dev"])
def test_closed_loop_follows_recorded_loop(oracle, capi, cuda, scan):
    """f110qp_rollout_dev and f110qp_rollout_scan_dev (held scan, scan_rows = 1; gap rows inactive as in
    the reference) over the recorded 4 cars x 8 ticks, x_traj, u_lin_traj and u_applied asserted tick by
    tick in order, so that a first divergence is reported at its tick.

    Allowance of the free-running loop. Row 0 is the recorded start exactly: a_0 = 0 for the vector
    (x, y, th, steer_lin). A difference a_t at the start of tick t passes through the tick's map, whose
    first-order gain |K_t| is computed at the recorded point (loop_gains), and the tick adds its own
    one-step term o_t (one_step_allowance):  a_{t+1} = 2 |K_t| a_t + o_t,  and for the applied input
    du + 2 |Ku_t| a_t. The factor 2 stands for what first order leaves out: the map is piecewise smooth
    (a QP solution is piecewise affine in its data, the linearisation is smooth in th and steer_lin)
    and the allowance stays below 0.03 over the 8 ticks, where its second-order terms and the
    finite-difference error are far below the first-order one; a change of the active set inside so small a neighbourhood is
    covered only as far as the factor reaches, which is the one assumption of this bound.

    Then every tick again as a one-tick rollout from the recorded state of that tick, against the
    one-step term alone. Would catch: the plant's car length, the next input's index, half-spaces
    entering an inactive QP, a drive input that is not the plan's first entry, a hand-over of
    x_traj[t+1] / u_lin_traj[t+1] into tick t+1 that drops or swaps a component."""
    import torch

    d = load("ref_loop")
    N, T = int(d["horizon"]), int(d["ticks"])
    B = d["x"].shape[0]
    s = capi.Solver(capi.default_config(N))
    xr = torch.from_numpy(np.ascontiguousarray(d["x_ref"])).to(cuda)
    rd = torch.from_numpy(np.ascontiguousarray(d["ranges"], np.float32)[None]).to(cuda)  # [scan_rows = 1, B, R]
    geom = d["geom"]
    sc = capi.default_scan_config(num_ranges=rd.shape[2], angle_min=geom[0], angle_increment=geom[1], angle_max=geom[2],
                                  scan_rows=1)

    def run(x_start, ul_start, ticks):
        xt = torch.full((ticks + 1, B, 3), -7.0, dtype=torch.float64, device=cuda)
        ult = torch.full((ticks + 1, B, 2), -7.0, dtype=torch.float64, device=cuda)
        ua = torch.full((ticks, B, 2), -7.0, dtype=torch.float32, device=cuda)
        st = torch.full((ticks, B), 77, dtype=torch.int32, device=cuda)
        xt[0] = torch.from_numpy(np.ascontiguousarray(x_start)).to(cuda)
        ult[0] = torch.from_numpy(np.ascontiguousarray(ul_start)).to(cuda)
        rc = capi.default_rollout_config()
        rc.ticks = ticks
        if scan:
            s.rollout_scan_dev(rc, sc, xr, rd, xt, ult, ua, st, None, None, None, None)
        else:
            s.rollout_dev(rc, xr, None, xt, ult, ua, st, None, None, None, None)
        torch.cuda.synchronize()
        return xt.cpu().numpy(), ult.cpu().numpy(), ua.cpu().numpy(), st.cpu().numpy()

    xt, ult, ua, st = run(d["x"][:, 0], d["u_lin"][:, 0], T)
    assert (st == capi.SOLVED).all()
    a = np.zeros((B, 4))
    worst = 0.0
    for t in range(T):
        du, o = one_step_allowance(d, t)
        nxt = np.zeros((B, 4))
        for b in range(B):
            K, Ku = loop_gains(oracle, d, b, t)
            ua_allow = du + 2 * Ku @ a[b]
            eu = np.abs(ua[t, b] - d["u_applied"][b, t])
            assert (eu <= ua_allow).all(), ("u_applied", t, b, eu, ua_allow)
            nxt[b] = 2 * K @ a[b] + o[b]
            worst = max(worst, float((eu / ua_allow).max()))
        a = nxt
        ex = np.abs(xt[t + 1] - d["x"][:, t + 1])
        es = np.abs(ult[t + 1, :, 1] - d["u_lin"][:, t + 1, 1])
        assert (ex <= a[:, :3]).all(), ("x_traj", t + 1, ex, a[:, :3])
        assert (es <= a[:, 3]).all() and (ult[t + 1, :, 0] == 4.5).all(), ("u_lin_traj", t + 1, es, a[:, 3])
        worst = max(worst, float((ex / a[:, :3]).max()), float((es / a[:, 3]).max()))
    print(f"free-running loop: worst deviation at {worst:.3e} of its allowance; allowance at tick {T}: {a.max(axis=0)}")
    for t in range(T):  # tick by tick from the recorded states
        x1, ul1, ua1, st1 = run(d["x"][:, t], d["u_lin"][:, t], 1)
        du, o = one_step_allowance(d, t)
        assert (st1 == capi.SOLVED).all(), t
        assert (np.abs(ua1[0] - d["u_applied"][:, t]) <= du).all(), (t, np.abs(ua1[0] - d["u_applied"][:, t]).max(), du)
        assert (np.abs(x1[1] - d["x"][:, t + 1]) <= o[:, :3]).all(), (t, (np.abs(x1[1] - d["x"][:, t + 1]) / o[:, :3]).max())
        assert (ul1[1][:, 0] == 4.5).all() and (np.abs(ul1[1][:, 1] - d["u_lin"][:, t + 1, 1]) <= du).all(), t
    s.close()
