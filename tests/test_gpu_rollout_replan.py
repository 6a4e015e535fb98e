"""The closed loop with re-planning on MI355X: f110qp_plan_listed_dev, f110qp_replan_start_dev,
f110qp_advance_replan_dev and f110qp_rollout_replan[_dev] (include/f110qp.h, "closed loop with re-planning").

Everything between two device routes is bit equality. The state machine is compared with its numpy
restatement (replan_cases.tick_action / next_kind), which is exact: integers, float32 copies and one float
expression (Transforms::CalcDist) whose double square root is correctly rounded on both sides. The per-tick
solve and plant-step bounds are test_gpu_rollout.py's (U_TOL; 2 spacing + 2e-16), on the inputs the device
itself recorded, so no closed-loop drift enters a tolerance. The pose row's sin / cos are compared with
numpy's within 4 eps64 (two 2-ulp routines).
"""
import numpy as np
import pytest
import replan_cases as rp_
import rollout_cases as rc_
from halfspace_cases import adversarial_scans, scan_geometry
from test_gpu_dbl import U_TOL
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_scan import scan_config

from f110qp import workload

pytestmark = pytest.mark.gpu

P = 50  # traj_discrete of the default plan config
KINDS = {rp_.MPC, rp_.PLAN, rp_.HOLD, rp_.PLAN_FAILED}


def dev(cuda, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def full(cuda, shape, dtype, fill):
    import torch

    return torch.full(shape, fill, dtype=dtype, device=cuda)


# ---- 1: the listed plan equals f110qp_plan_batch_dev ------------------------------------------------

_plans = {}


def plan_reference(capi, cuda, B):
    """(scene, table, f110qp_plan_batch_dev's outputs) of B scenes, every seventh without a valid
    candidate, computed once per B."""
    import torch

    if B not in _plans:
        sc = workload.make_scenes(B, seed=40 + B)
        sc["ranges"][np.arange(B) % 7 == 3] = 0.5
        cfg = capi.default_plan_config()
        table = capi.traj_table(cfg)
        out = dict(x_ref=torch.empty((B, P, 3), dtype=torch.float32, device=cuda),
                   x0=torch.empty((B, 3), dtype=torch.float32, device=cuda),
                   best_traj=torch.empty(B, dtype=torch.int32, device=cuda),
                   best_global=torch.empty(B, dtype=torch.int32, device=cuda),
                   status=torch.empty(B, dtype=torch.int32, device=cuda))
        capi.plan_batch_dev(cfg, dev(cuda, sc["pose"]), dev(cuda, sc["ranges"]), sc["angle_min"], sc["angle_inc"],
                            sc["angle_max"], dev(cuda, table), dev(cuda, sc["waypoints"]), out["x_ref"], out["x0"],
                            out["best_traj"], out["best_global"], out["status"])
        torch.cuda.synchronize(cuda)
        _plans[B] = sc, table, {k: v.cpu().numpy() for k, v in out.items()}
    return _plans[B]


LISTS = [(5, "two", [3, 0]), (300, "none", 0), (300, "one", 1), (300, "257", 257), (300, "all", 300),
         (1100, "all, above the grid cap", 1100)]


@pytest.mark.parametrize("B,name,cars", LISTS, ids=[f"{b}-{n}" for b, n, _ in LISTS])
def test_plan_listed_equals_plan_batch(capi, cuda, B, name, cars):
    """Listed cars (a scrambled list; the entries past the count name cars too and must be ignored): plan
    status and indices equal, x_ref the float32 path widened, bit for bit, on status 0. Unlisted cars and
    listed cars without a valid candidate keep the sentinel in every x_ref word (no NaN is written); unlisted
    cars keep it in the status and index arrays too. Count 0 changes nothing. 1,100 cars: more than the
    768-workgroup grid, every workgroup takes a second car."""
    import torch

    sc, table, ref = plan_reference(capi, cuda, B)
    rng = np.random.default_rng(B + len(name))
    order = rng.permutation(B).astype(np.int32)
    if isinstance(cars, list):
        order = np.array(cars + [c for c in order if c not in cars], np.int32)
        cars = len(cars)
    listed = np.zeros(B, bool)
    listed[order[:cars]] = True
    rp = capi.default_replan_config(num_waypoints=sc["waypoints"].shape[0])
    scn = scan_config(capi, sc["ranges"].shape[1], (sc["angle_min"], sc["angle_inc"], sc["angle_max"]))
    xr = full(cuda, (B, P, 3), torch.float64, -7.0)
    st, bt, bg = (full(cuda, (B,), torch.int32, -7) for _ in range(3))
    capi.plan_listed_dev(rp, scn, dev(cuda, order), dev(cuda, np.int32([cars])), dev(cuda, sc["pose"]),
                         dev(cuda, sc["ranges"]), dev(cuda, table), dev(cuda, sc["waypoints"]), xr, st, bt, bg)
    torch.cuda.synchronize(cuda)
    xr, st, bt, bg = (v.cpu().numpy() for v in (xr, st, bt, bg))
    for got, key in ((st, "status"), (bt, "best_traj"), (bg, "best_global")):
        np.testing.assert_array_equal(got[listed], ref[key][listed], err_msg=key)
        assert (got[~listed] == -7).all(), key
    ok = listed & (ref["status"] == 0)
    same_bits(xr[ok], ref["x_ref"][ok].astype(np.float64), "x_ref of the listed cars")
    assert (xr[~ok] == -7.0).all(), "a car without a new path keeps the one it had"
    if cars >= 257:
        assert ok.any() and (listed & (ref["status"] == 1)).any()
    if cars == 0:
        assert not listed.any()


# ---- 2: the step alone -------------------------------------------------------------------------------

def threshold_neighbours():
    """The two float32 neighbours of replan_dist: the largest below 1.98 (as the reference compares: the
    float widened to double) and the smallest not below."""
    f = np.float32(rp_.REPLAN_DIST)
    hi = f if np.float64(f) >= rp_.REPLAN_DIST else np.nextafter(f, np.float32(np.inf))
    lo = np.nextafter(hi, np.float32(0))
    assert np.float64(lo) < rp_.REPLAN_DIST <= np.float64(hi)
    return lo, hi


def end_at(xp, yp, t, exact):
    """A path end at float32 distance t from (xp, yp) along one axis. exact: CalcDist gives exactly t, i.e. the
    float32 difference of the two float32 coordinates is +-t (the other coordinate equal); None where no
    float32 does that on either axis or side (a half-way case of the subtraction can skip t)."""
    f = np.float32
    xf, yf, t = f(xp), f(yp), f(t)
    if not exact:
        return np.float64(f(xf - t)), np.float64(yf)
    for axis, v in ((0, xf), (1, yf)):
        for side in (-1, 1):
            e = f(v + f(side) * t)
            for c in (e, np.nextafter(e, f(-np.inf)), np.nextafter(e, f(np.inf))):
                if abs(f(v - c)) == t:
                    return (np.float64(c), np.float64(yf)) if axis == 0 else (np.float64(xf), np.float64(c))
    return None


@pytest.mark.parametrize("B,N", [(1, 20), (63, 5), (65, 20), (257, 20)])
def test_advance_replan_step(capi, cuda, B, N):
    """One f110qp_advance_replan_dev launch on hand-built states against replan_cases.tick_action /
    next_kind: every branch (MPC usable and not, HOLD, PLAN ok and failed), every held-plan situation (len 0
    or N, idx from 0 to past the end: the car ran out and drives fail_u), path ends far, near and at the two
    float neighbours of the threshold from the next pose. x_next, u_lin_next, u_applied and hs_next are
    bit-equal to f110qp_advance_scan_dev given the same applied input; the next list is compared as a set
    with its count. B = 1, 63, 65, 257: the ballot's partial and ragged waves."""
    import torch

    rng = np.random.default_rng(70 + B)
    branch = (np.arange(B) + rng.integers(0, 5)) % 5 if B > 1 else np.array([2])
    out = np.arange(B) % 11 == 7  # these plan (ok and failed in turn) with a whole plan held and its index past the end
    branch[out] = 3 + (np.arange(B)[out] // 11) % 2
    kind = np.int32([rp_.MPC, rp_.MPC, rp_.HOLD, rp_.PLAN, rp_.PLAN])[branch]
    status = np.where(branch == 0, rng.choice([capi.SOLVED, capi.SOLVED_INACCURATE], B),
                      rng.choice([capi.MAX_ITER, capi.PRIMAL_INFEASIBLE, capi.NUMERICAL], B)).astype(np.int32)
    plan_status = np.where(branch == 3, 0, rng.choice([1, 2], B)).astype(np.int32)
    up = np.stack([rng.uniform(3.0, 4.5, (B, N)), rng.uniform(-0.43, 0.43, (B, N))], 2).astype(np.float32)
    up[(branch == 1)] = np.nan
    S = rp_.new_state(B, N)
    S["have"][:] = (kind != rp_.PLAN).astype(np.int32)
    S["held"][:] = np.stack([rng.uniform(3.0, 4.5, (B, N)), rng.uniform(-0.43, 0.43, (B, N))], 2)
    S["len"][:] = rng.choice([0, N], B)
    S["idx"][:] = rng.integers(0, N + 2, B)
    S["len"][out], S["idx"][out] = N, N + np.arange(B)[out] % 2
    x = np.column_stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B)])
    # the next pose as numpy predicts it, to place the path ends
    S0 = {k: v.copy() for k, v in S.items()}
    _, _, u_pred, _, _ = rp_.tick_action({k: v.copy() for k, v in S.items()}, kind, plan_status, status, up)
    xp = rc_.plant_step(x, u_pred)
    lo, hi = threshold_neighbours()
    xr = rng.uniform(-5, 5, (B, P, 3))
    where = (np.arange(B) // 5) % 4 if B > 1 else np.array([2])
    for b in range(B):
        t = [np.float32(3.0), np.float32(1.0), lo, hi][where[b]]
        end = end_at(xp[b, 0], xp[b, 1], t, where[b] >= 2) or end_at(xp[b, 0], xp[b, 1], 3.0, False)
        xr[b, -1, 0], xr[b, -1, 1] = end
    nr = 200
    geom = scan_geometry(nr)
    sc = scan_config(capi, nr, geom)
    rc, rpc = capi.default_rollout_config(), capi.default_replan_config()
    gap = torch.empty((B, 4), dtype=torch.int32, device=cuda)
    capi.gap_search_dev(sc, dev(cuda, adversarial_scans(B, nr, 80 + B)), gap)
    d = dict(kind=dev(cuda, kind), status=dev(cuda, status), held=dev(cuda, S["held"]), len=dev(cuda, S["len"]),
             idx=dev(cuda, S["idx"]), have=dev(cuda, S["have"]), x_next=full(cuda, (B, 3), torch.float64, -7.0),
             ul=full(cuda, (B, 2), torch.float64, -7.0), ua=full(cuda, (B, 2), torch.float32, -7.0),
             pose=full(cuda, (B, 4), torch.float64, -7.0), knext=full(cuda, (B,), torch.int32, -7),
             list=full(cuda, (B,), torch.int32, -7), count=full(cuda, (1,), torch.int32, 0),
             hs=full(cuda, (B, 2, 3), torch.float32, -7.0))
    xd, upd, xrd = dev(cuda, x), dev(cuda, up), dev(cuda, xr)
    capi.advance_replan_dev(rc, rpc, sc, N, xd, d["kind"], upd, d["status"], dev(cuda, plan_status), xrd, d["held"],
                            d["len"], d["idx"], d["have"], d["x_next"], d["ul"], d["pose"], u_applied=d["ua"],
                            kind_next=d["knext"], next_list=d["list"], next_count=d["count"], gap=gap, hs_next=d["hs"])
    torch.cuda.synchronize(cuda)
    g = {k: v.cpu().numpy() for k, v in d.items()}
    # the numpy restatement
    k_rep, st_rep, u, u32, nxt = rp_.tick_action(S, kind, plan_status, status, up)
    np.testing.assert_array_equal(g["kind"], k_rep)
    np.testing.assert_array_equal(g["status"], st_rep)
    for key in ("have", "len", "idx"):
        np.testing.assert_array_equal(g[key], S[key], err_msg=key)
    same_bits(g["held"], S["held"], "u_held")
    same_bits(g["ua"], u32, "u_applied")
    same_bits(g["ul"], np.stack([np.full(B, rc_.V_LIN), nxt], 1), "u_lin_next")
    # advance_scan_dev on a plan that applies the same input
    has0 = S["idx"] - 1 < S["len"]  # the index DriveStep read, against the length after the action
    plan2 = np.zeros((B, N, 2), np.float32)
    plan2[:, 0], plan2[:, 1, 1] = u32, nxt.astype(np.float32)
    st2 = np.where(has0, capi.SOLVED, capi.MAX_ITER).astype(np.int32)
    r = [full(cuda, (B, 3), torch.float64, -7.0), full(cuda, (B, 2), torch.float64, -7.0),
         full(cuda, (B, 2, 3), torch.float32, -7.0), full(cuda, (B, 2), torch.float32, -7.0)]
    capi.advance_scan_dev(rc, sc, N, xd, dev(cuda, plan2), dev(cuda, st2), gap, r[0], r[1], r[2], r[3])
    torch.cuda.synchronize(cuda)
    for name, a, b_ in zip(("x_next", "ul", "hs", "ua"), r, (g["x_next"], g["ul"], g["hs"], g["ua"])):
        same_bits(b_, a.cpu().numpy(), f"{name} against advance_scan_dev")
    err = np.abs(g["x_next"] - xp)
    assert (err <= 2 * np.spacing(np.abs(xp)) + 2e-16).all()
    # the pose row and the next tick
    same_bits(g["pose"][:, :2], g["x_next"][:, :2], "pose row x, y")
    want = rp_.pose_row(g["x_next"])
    assert np.abs(g["pose"][:, 2:] - want[:, 2:]).max() <= 4 * np.finfo(np.float64).eps
    k_next = rp_.next_kind(S["have"], g["x_next"], xr)
    np.testing.assert_array_equal(g["knext"], k_next)
    n = int(g["count"][0])
    assert n == int((k_next == rp_.PLAN).sum())
    assert sorted(g["list"][:n].tolist()) == np.flatnonzero(k_next == rp_.PLAN).tolist()
    assert (g["list"][n:] == -7).all()
    if B >= 63:  # what the states covered
        assert set(k_rep.tolist()) == KINDS and set(k_next.tolist()) == {rp_.MPC, rp_.PLAN, rp_.HOLD}
        ran = (S["idx"] - 1 >= S["len"]) & (S["len"] == N) & (k_rep != rp_.MPC)
        assert ran.any() and (g["ua"][ran] == np.float32(rc_.FAIL_U)).all(), "a car past the end of its plan"
        dist = rp_.calc_dist(g["x_next"][:, 0], g["x_next"][:, 1], xr[:, -1, 0], xr[:, -1, 1])
        held = S["have"] == 1
        assert (held & (dist == lo)).any() and (k_next[held & (dist == lo)] == rp_.HOLD).all()
        assert (held & (dist == hi)).any() and (k_next[held & (dist == hi)] == rp_.MPC).all()
    # without the next tick (a call's last tick) and without rows: the state and the step keep their bits
    d2 = dict(kind=dev(cuda, kind), status=dev(cuda, status), held=dev(cuda, S0["held"]), len=dev(cuda, S0["len"]),
              idx=dev(cuda, S0["idx"]), have=dev(cuda, S0["have"]))
    o = [full(cuda, (B, 3), torch.float64, -7.0), full(cuda, (B, 2), torch.float64, -7.0),
         full(cuda, (B, 4), torch.float64, -7.0)]
    capi.advance_replan_dev(rc, rpc, None, N, xd, d2["kind"], upd, d2["status"], dev(cuda, plan_status), xrd,
                            d2["held"], d2["len"], d2["idx"], d2["have"], o[0], o[1], o[2])
    torch.cuda.synchronize(cuda)
    for key in d2:
        same_bits(d2[key].cpu().numpy(), g[key], f"last tick, {key}")
    same_bits(o[0].cpu().numpy(), g["x_next"], "last tick, x_next")
    same_bits(o[2].cpu().numpy(), g["pose"], "last tick, pose")


# ---- 3: the loop is its parts ------------------------------------------------------------------------

RKEYS = ("x_traj", "u_lin_traj", "u_applied", "status", "iters", "cost", "u_plan", "x_plan", "hs_traj", "kind",
         "plan_status", "best_traj", "best_global", "pose_traj")
EVERY = ("x_traj", "u_lin_traj", "u_applied", "status", "hs_traj", "kind", "x_ref", "have_path")
ON_MPC = ("iters", "cost", "u_plan", "x_plan")
ON_PLAN = ("plan_status", "best_traj", "best_global")


def replan_buffers(cuda, x0, ul, B, N, T, lean=False):
    import torch

    f64, f32, i32 = torch.float64, torch.float32, torch.int32
    d = {"x_traj": full(cuda, (T + 1, B, 3), f64, -7.0), "u_lin_traj": full(cuda, (T + 1, B, 2), f64, -7.0),
         "u_applied": full(cuda, (T, B, 2), f32, -7.0), "status": full(cuda, (T, B), i32, 77),
         "x_ref": full(cuda, (B, P, 3), f64, float("nan")), "have_path": full(cuda, (B,), i32, 0)}
    d["x_traj"][0], d["u_lin_traj"][0] = dev(cuda, x0), dev(cuda, ul)
    if not lean:
        d.update(iters=full(cuda, (T, B), i32, -7), cost=full(cuda, (T, B), f64, -7.0),
                 u_plan=full(cuda, (T, B, N, 2), f32, -7.0), x_plan=full(cuda, (T, B, N + 1, 3), f32, -7.0),
                 hs_traj=full(cuda, (T, B, 2, 3), f32, -7.0), kind=full(cuda, (T, B), i32, -7),
                 plan_status=full(cuda, (T, B), i32, -7), best_traj=full(cuda, (T, B), i32, -7),
                 best_global=full(cuda, (T, B), i32, -7), pose_traj=full(cuda, (T + 1, B, 4), f64, -7.0))
    return d


def rollout_replan_dev(capi, cuda, s, case, T, rows=1, lean=False, start=None):
    """One Solver.rollout_replan_dev call on fresh device arrays (start: x0, u_lin, x_ref, have_path of a
    previous call to continue); returns every array as numpy."""
    import torch

    x0, ul, ranges, geom, wp = case
    B, N = x0.shape[0], s.horizon
    if start is not None:
        x0, ul = start["x_traj"][-1], start["u_lin_traj"][-1]
    d = replan_buffers(cuda, x0, ul, B, N, T, lean)
    if start is not None:
        d["x_ref"], d["have_path"] = dev(cuda, start["x_ref"]), dev(cuda, start["have_path"])
    sc = scan_config(capi, ranges.shape[-1], geom, scan_rows=rows)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    table = capi.traj_table(rp.plan)
    cfg = capi.default_rollout_config(ticks=T)
    s.rollout_replan_dev(cfg, sc, rp, dev(cuda, table), dev(cuda, wp), d["x_ref"], d["have_path"],
                         dev(cuda, ranges.reshape(rows, B, -1)), d["x_traj"], d["u_lin_traj"], d["u_applied"],
                         d["status"], d.get("iters"), d.get("cost"), d.get("u_plan"), d.get("x_plan"), d.get("hs_traj"),
                         d.get("kind"), d.get("plan_status"), d.get("best_traj"), d.get("best_global"),
                         d.get("pose_traj"))
    torch.cuda.synchronize(cuda)
    return {k: v.cpu().numpy() for k, v in d.items()}


def manual_replan_loop(capi, cuda, s, case, T, rows=1):
    """The loop written with the public calls, the state machine in numpy on the host between them: per
    tick replan_start_dev (the pose row and the rows at this pose; its kind and list are checked against
    numpy's), plan_listed_dev on numpy's list, solve_dev_dbl, tick_action, and the plant step as
    advance_scan_dev (advance_dev on the last tick) on a plan that applies tick_action's input. Returns the
    recorded arrays and the path ends every tick's kind was decided with."""
    import torch

    x0, ul, ranges, geom, wp = case
    B, N = x0.shape[0], s.horizon
    gap_on = s.config.gap_mode == capi.GAP_ACTIVE
    d = replan_buffers(cuda, x0, ul, B, N, T)
    sc = scan_config(capi, ranges.shape[-1], geom, scan_rows=rows)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    rc = capi.default_rollout_config()
    table, wpd = dev(cuda, capi.traj_table(rp.plan)), dev(cuda, wp)
    rg = dev(cuda, ranges.reshape(rows, B, -1))
    gap = torch.empty((rows, B, 4), dtype=torch.int32, device=cuda)
    capi.gap_search_dev(sc, rg, gap)
    S = rp_.new_state(B, N)
    xr = np.full((B, P, 3), np.nan)
    ends = np.zeros((T, B, 2))
    scratch = [full(cuda, (B,), torch.int32, -7) for _ in range(2)]
    for t in range(T):
        r = 0 if rows == 1 else t
        count = full(cuda, (1,), torch.int32, 0)
        d["have_path"].copy_(dev(cuda, S["have"]))
        capi.replan_start_dev(rp, sc, d["x_traj"][t], d["have_path"], d["x_ref"], gap[r], d["pose_traj"][t],
                              scratch[0], scratch[1], count, hs=d["hs_traj"][t])
        x = d["x_traj"][t].cpu().numpy()
        kind = rp_.next_kind(S["have"], x, xr)
        ends[t] = xr[:, -1, :2]
        cars = np.flatnonzero(kind == rp_.PLAN).astype(np.int32)
        np.testing.assert_array_equal(scratch[0].cpu().numpy(), kind, err_msg=f"kind of tick {t}")
        assert int(count.cpu()[0]) == len(cars) and sorted(scratch[1].cpu().numpy()[:len(cars)].tolist()) == cars.tolist()
        lst = np.zeros(B, np.int32)
        lst[:len(cars)] = cars
        capi.plan_listed_dev(rp, sc, dev(cuda, lst), dev(cuda, np.int32([len(cars)])), d["pose_traj"][t], rg[r], table,
                             wpd, d["x_ref"], d["plan_status"][t], d["best_traj"][t], d["best_global"][t])
        s.solve_dev_dbl(d["x_traj"][t], d["u_lin_traj"][t], d["x_ref"], d["hs_traj"][t] if gap_on else None,
                        d["u_plan"][t], d["x_plan"][t], d["status"][t], d["iters"][t], cost=d["cost"][t])
        torch.cuda.synchronize(cuda)
        xr = d["x_ref"].cpu().numpy()
        k_rep, st_rep, _, u32, nxt = rp_.tick_action(S, kind, d["plan_status"][t].cpu().numpy(),
                                                     d["status"][t].cpu().numpy(), d["u_plan"][t].cpu().numpy())
        d["kind"][t], d["status"][t] = dev(cuda, k_rep), dev(cuda, st_rep)
        has0 = S["idx"] - 1 < S["len"]
        plan2 = np.zeros((B, N, 2), np.float32)
        plan2[:, 0], plan2[:, 1, 1] = u32, nxt.astype(np.float32)
        st2 = dev(cuda, np.where(has0, capi.SOLVED, capi.MAX_ITER).astype(np.int32))
        if t + 1 < T:
            capi.advance_scan_dev(rc, sc, N, d["x_traj"][t], dev(cuda, plan2), st2, gap[0 if rows == 1 else t + 1],
                                  d["x_traj"][t + 1], d["u_lin_traj"][t + 1], d["hs_traj"][t + 1], d["u_applied"][t])
        else:
            capi.advance_dev(rc, N, d["x_traj"][t], dev(cuda, plan2), st2, d["x_traj"][t + 1], d["u_lin_traj"][t + 1],
                             d["u_applied"][t])
    d["have_path"].copy_(dev(cuda, S["have"]))
    count = full(cuda, (1,), torch.int32, 0)
    capi.replan_start_dev(rp, None, d["x_traj"][T], d["have_path"], d["x_ref"], None, d["pose_traj"][T], scratch[0],
                          scratch[1], count)
    torch.cuda.synchronize(cuda)
    return {k: v.cpu().numpy() for k, v in d.items()}, ends


def check_kind_rules(kind):
    """No HOLD tick is followed by anything but PLAN or PLAN_FAILED; a PLAN_FAILED tick by the same two; an
    MPC tick never follows a tick that left the car without a path."""
    after_hold = kind[1:][kind[:-1] == rp_.HOLD]
    assert np.isin(after_hold, (rp_.PLAN, rp_.PLAN_FAILED)).all()
    after_fail = kind[1:][kind[:-1] == rp_.PLAN_FAILED]
    assert np.isin(after_fail, (rp_.PLAN, rp_.PLAN_FAILED)).all()
    assert np.isin(kind[0], (rp_.PLAN, rp_.PLAN_FAILED)).all(), "every car starts without a path"


PARTS = [(B, N, gap, rows) for B in (1, 5, 70) for N in (2, 20) for gap in (False, True) for rows in (1, 20)]


@pytest.mark.parametrize("B,N,gap,rows", PARTS, ids=[f"B{b}-N{n}-{'gap' if g else 'box'}-rows{r}" for b, n, g, r in PARTS])
def test_rollout_replan_is_its_parts(capi, cuda, B, N, gap, rows):
    """rollout_replan_dev against the manual loop, T = 20: every trajectory array, kind_traj, the final
    paths and flags bit-identical for every car and tick; the solve's rows on MPC ticks and the plan's on
    PLAN / PLAN_FAILED ticks (unspecified elsewhere). The case, asserted here: every car that never fails a
    plan shows PLAN, MPC and HOLD and plans at least twice; with more than one car, car 3 has no valid
    candidate on any tick (PLAN_FAILED throughout: its plan stays empty and it drives fail_u), so every kind
    occurs; one car alone cannot both plan and never plan, so B = 1 shows PLAN_FAILED only with a scan per
    tick (ticks 6 to 9 ringed). The invariant: on every MPC tick the float distance to the path end is >=
    replan_dist."""
    T = 20
    case = rp_.loop_case(B, T, rows)
    s = solver(capi, N, gap=gap, x_ref_points=P)
    a = rollout_replan_dev(capi, cuda, s, case, T, rows)
    m, ends = manual_replan_loop(capi, cuda, s, case, T, rows)
    what = f"B {B} N {N} gap {gap} rows {rows}"
    for k in EVERY:
        same_bits(a[k], m[k], f"{what}: {k}")
    same_bits(a["pose_traj"], m["pose_traj"], f"{what}: pose_traj")
    kind = a["kind"]
    mpc, plan = kind == rp_.MPC, np.isin(kind, (rp_.PLAN, rp_.PLAN_FAILED))
    for k in ON_MPC:
        same_bits(a[k][mpc], m[k][mpc], f"{what}: {k} on MPC ticks")
    for k in ON_PLAN:
        same_bits(a[k][plan], m[k][plan], f"{what}: {k} on PLAN ticks")
    assert (a["status"][~mpc] == capi.NO_SOLVE).all() and (a["status"][mpc] != 77).all()
    assert ((a["plan_status"][kind == rp_.PLAN] == 0).all() and (a["plan_status"][kind == rp_.PLAN_FAILED] > 0).all())
    check_kind_rules(kind)
    never_failed = ~(kind == rp_.PLAN_FAILED).any(axis=0)
    assert never_failed.any() or (B == 1 and rows > 1)
    for b in np.flatnonzero(never_failed):
        assert {rp_.PLAN, rp_.MPC, rp_.HOLD} <= set(kind[:, b].tolist()), (b, kind[:, b])
        assert (kind[:, b] == rp_.PLAN).sum() >= 2, (b, kind[:, b])
    if B > 3:
        assert set(np.unique(kind).tolist()) == KINDS
        assert (kind[:, 3] == rp_.PLAN_FAILED).all() and a["have_path"][3] == 0
        same_bits(a["u_applied"][:, 3], np.tile(np.float32(rc_.FAIL_U), (T, 1)), "the car that never plans")
    elif rows > 1:
        assert set(np.unique(kind).tolist()) == KINDS
    dist = rp_.calc_dist(a["x_traj"][:T, :, 0], a["x_traj"][:T, :, 1], ends[:, :, 0], ends[:, :, 1])
    assert (dist[mpc].astype(np.float64) >= rp_.REPLAN_DIST).all()
    assert (dist[kind == rp_.HOLD].astype(np.float64) < rp_.REPLAN_DIST).all()
    if B == 5:  # the optional arrays left out; the host-pointer call
        lean = rollout_replan_dev(capi, cuda, s, case, T, rows, lean=True)
        for k in lean:
            same_bits(lean[k], a[k], f"{what}: no optional array, {k}")
        x0, ul, ranges, geom, wp = case
        rp = capi.default_replan_config(num_waypoints=wp.shape[0])
        host = s.rollout_replan(x0, ul, ranges, scan_config(capi, ranges.shape[-1], geom, scan_rows=rows), rp,
                                capi.traj_table(rp.plan), wp, T, plans=True, objective=True)
        for k in EVERY + ("pose_traj",):
            same_bits(host[k], a[k], f"{what}: host call, {k}")
        for k in ON_MPC:
            same_bits(host[k][mpc], a[k][mpc], f"{what}: host call, {k}")
        for k in ON_PLAN:
            same_bits(host[k][plan], a[k][plan], f"{what}: host call, {k}")
    s.close()


def test_rollout_replan_continues(capi, cuda):
    """Two calls of 10 ticks, the second started from the first's last row, x_ref and have_path, against one
    call of 20. What the contract keeps: the path and the flag, so the first tick of the second call has the
    long call's kind, plan results and pose for every car. The held plan restarts empty: a car whose tick 10
    is an MPC tick publishes a new plan there and is bit-identical to the long call from then on, to its
    final path and flag; a car whose tick 10 is a PLAN or HOLD tick drives fail_u where the long call drives
    its previous plan."""
    B, N, T = 70, 20, 10
    case = rp_.loop_case(B, 2 * T, 1)
    s = solver(capi, N, x_ref_points=P)
    whole = rollout_replan_dev(capi, cuda, s, case, 2 * T)
    first = rollout_replan_dev(capi, cuda, s, case, T)
    second = rollout_replan_dev(capi, cuda, s, case, T, start=first)
    s.close()
    for k in RKEYS:
        n = T + 1 if k in ("x_traj", "u_lin_traj", "pose_traj") else T
        if k in ON_MPC or k in ON_PLAN:
            continue
        same_bits(first[k], whole[k][:n], f"first call, {k}")
    k10 = whole["kind"][T]
    np.testing.assert_array_equal(second["kind"][0], k10)
    same_bits(second["pose_traj"][0], whole["pose_traj"][T], "pose of tick 10")
    plan = np.isin(k10, (rp_.PLAN, rp_.PLAN_FAILED))
    for k in ON_PLAN:
        same_bits(second[k][0][plan], whole[k][T][plan], f"tick 10, {k}")
    mpc = k10 == rp_.MPC
    assert mpc.any() and (~mpc).any()
    for k in ("x_traj", "u_lin_traj", "u_applied", "status", "kind", "hs_traj", "pose_traj"):
        same_bits(second[k][:, mpc], whole[k][T:][:, mpc] if k in ("x_traj", "u_lin_traj", "pose_traj")
                  else whole[k][T:][:, mpc], f"cars on an MPC tick at 10, {k}")
    same_bits(second["x_ref"][mpc], whole["x_ref"][mpc], "their final paths")
    np.testing.assert_array_equal(second["have_path"][mpc], whole["have_path"][mpc])
    held = ~mpc & (whole["u_applied"][T] != np.float32(rc_.FAIL_U)).any(axis=1)
    assert held.any(), "a car that drives its previous plan through tick 10 in the long call"
    same_bits(second["u_applied"][0][~mpc], np.tile(np.float32(rc_.FAIL_U), (int((~mpc).sum()), 1)), "a fresh node")


# ---- 4: against the CPU chain ------------------------------------------------------------------------

def test_rollout_replan_against_cpu_chain(oracle, capi, cuda):
    """64 cars x N = 20 x 20 ticks, box rows, one scan per car, seed replan_cases.REPLAN_SEED: chosen by
    replan_cases.choose_replan_seed on the CPU chain alone (oracle.plan, oracle.solve on doubles,
    rollout_cases.plant_step, the numpy state machine): no tick with |dist - 1.98| or the margin between the
    two best end-point distances below 1e-3, every kind occurs.
    Against the chain: kind_traj, the plan statuses and the chosen candidates and waypoints are equal.
    Per tick, on the arrays the device recorded (the tolerances of test_rollout_scan_against_oracle, every
    car and tick): oracle.plan at pose_traj[t] gives the plan status, indices and, bit for bit, the path;
    oracle.solve on (x_traj[t], u_lin_traj[t], that path) gives the status and u within U_TOL; u_applied and
    u_lin_traj[t + 1] are the state machine's on the recorded plan, bit for bit; the plant step is within 2
    spacing + 2e-16."""
    B, N, T = 64, 20, 20
    ok, chain = rp_.replan_seed_is_robust(oracle, rp_.REPLAN_SEED, B, N, T)
    print(f"seed {rp_.REPLAN_SEED}: min |dist - 1.98| {chain['min_dist_margin']:.3e}, min end-point margin "
          f"{chain['min_end_margin']:.3e}, kinds {np.unique(chain['kind'], return_counts=True)}")
    assert ok, "the recorded seed no longer meets the conditions it was chosen for"
    case = rp_.replan_case(B, rp_.REPLAN_SEED, blocked=(3,))
    x0, ul, ranges, geom, wp = case
    s = solver(capi, N, x_ref_points=P)
    out = rollout_replan_dev(capi, cuda, s, case, T)
    s.close()
    kind = out["kind"]
    np.testing.assert_array_equal(kind, chain["kind"])
    plan = np.isin(kind, (rp_.PLAN, rp_.PLAN_FAILED))
    for k in ON_PLAN:
        np.testing.assert_array_equal(out[k][plan], chain[k][plan], err_msg=k)
    np.testing.assert_array_equal(out["status"], chain["status"])
    np.testing.assert_array_equal(out["have_path"], chain["have_path"])
    # per tick, on the recorded arrays
    pp = oracle.plan_params()
    table = oracle.traj_table(pp)
    prm = oracle.params(N)
    S = rp_.new_state(B, N)
    xr = np.full((B, P, 3), np.nan)
    worst_u = worst_x = 0.0
    for t in range(T):
        x, u_lin = out["x_traj"][t], out["u_lin_traj"][t]
        np.testing.assert_array_equal(rp_.next_kind(S["have"], x, xr), np.where(kind[t] == rp_.PLAN_FAILED, rp_.PLAN, kind[t]))
        for b in np.flatnonzero(plan[t]):
            g, off = oracle.fill_occ_grid(pp, out["pose_traj"][t, b], ranges[b], *geom)
            r = oracle.plan(pp, out["pose_traj"][t, b], g, off, table, wp)
            assert (out["plan_status"][t, b], out["best_traj"][t, b], out["best_global"][t, b]) == \
                (r["status"], r["best_traj"], r["best_global"]), (t, b)
            if r["status"] == 0:
                xr[b] = r["x_ref"].astype(np.float64)
        for b in np.flatnonzero(kind[t] == rp_.MPC):
            r = oracle.solve(prm, x[b], u_lin[b], xr[b, :N], None, False)
            assert r["status"] != oracle.UNCERTIFIED and out["status"][t, b] == r["status"], (t, b)
            if r["status"] == oracle.SOLVED:
                eu = np.abs(out["u_plan"][t, b].astype(np.float64) - r["u"]).max() / max(1.0, np.abs(r["u"]).max())
                worst_u = max(worst_u, float(eu))
                assert eu <= U_TOL, (t, b, eu)
        _, st_rep, u, u32, nxt = rp_.tick_action(S, np.where(kind[t] == rp_.PLAN_FAILED, rp_.PLAN, kind[t]),
                                                 out["plan_status"][t], out["status"][t], out["u_plan"][t])
        same_bits(out["u_applied"][t], u32, f"u_applied, tick {t}")
        same_bits(out["u_lin_traj"][t + 1], np.stack([np.full(B, rc_.V_LIN), nxt], 1), f"u_lin_traj, tick {t + 1}")
        exp = rc_.plant_step(x, u)
        err = np.abs(out["x_traj"][t + 1] - exp)
        bound = 2 * np.spacing(np.abs(exp)) + 2e-16
        worst_x = max(worst_x, float((err / bound).max()))
        assert (err <= bound).all(), (t, float((err / bound).max()))
    same_bits(out["x_ref"], xr, "the final paths are the oracle's at the recorded poses")
    print(f"max u err {worst_u:.3e} (bound {U_TOL:.0e}), plant step at {worst_x:.3f} of its bound")
