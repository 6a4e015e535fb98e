"""The closed loop with a simulated LiDAR on MI355X: f110qp_rollout_world[_dev] (include/f110qp.h, "closed
loop with a simulated LiDAR"). Between two device routes everything is bit equality; the recorded scans are
compared with the numpy oracle under world_cases.py's bound and cap.

The cars start at workload.make_scenes poses on the track of workload.make_world(5, 40) (walls + 40
obstacles), without a path: every car plans on tick 0 from the scan cast at its start pose.
"""
import numpy as np
import pytest
import replan_cases as rp_
import rollout_cases as rc_
import world_cases as wc_
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_replan import P, dev, full, replan_buffers
from test_gpu_rollout_scan import scan_config
from world_loop import GEOM, R, rollout_dev

from f110qp import workload

pytestmark = pytest.mark.gpu

OUT = ("x_traj", "u_lin_traj", "u_applied", "status", "kind", "x_ref", "have_path", "pose_traj")
ON_MPC = ("iters", "cost", "u_plan", "x_plan")
ON_PLAN = ("plan_status", "best_traj", "best_global")


def world_case(B, per_car=False):
    """(x0 [B,3], u_lin [B,2], circles [C,3] or [B,C,3], waypoints): make_scenes(B, seed=3) poses in the
    track world; per_car: every car its own copy of it with the obstacles in another order."""
    x0 = wc_.track_poses(B)
    w = wc_.track_world()
    if per_car:
        w = np.ascontiguousarray(np.stack([np.concatenate([w[:1000], np.roll(w[1000:], b, axis=0)]) for b in range(B)]))
    return x0, np.tile([rc_.V_LIN, 0.0], (B, 1)), w, workload.track_waypoints()


def world_config(capi, circles):
    return capi.default_world_config(num_circles=circles.shape[-2], world_rows=1 if circles.ndim == 2 else circles.shape[0])


def rollout_world_dev(capi, cuda, s, case, T, scans=True, hs=True, start=None):
    """One Solver.rollout_world_dev call on fresh device arrays -> every array as numpy."""
    null = (() if hs else ("hs_traj",)) + (() if scans else ("ranges_traj",))
    return rollout_dev(capi, cuda, s, "world", case, T, null=null, start=start, scan_rows=7)


def manual_world_loop(capi, cuda, s, case, T, scans, hs):
    """The loop written with the public calls, all on the device: the memset, (rows computed) cast_scans_dev
    for all cars at row 0 and gap_search_dev, replan_start_dev; per tick cast_scans_dev (on the tick's list,
    or for all cars into row t), plan_listed_dev, solve_dev_dbl, advance_replan_dev."""
    import torch

    x0, ul, circles, wp = case
    B, N = x0.shape[0], s.horizon
    gap_on = s.config.gap_mode == capi.GAP_ACTIVE
    rows_on = gap_on or hs
    d = replan_buffers(cuda, x0, ul, B, N, T)
    if not hs:
        d["hs_traj"] = full(cuda, (T, B, 2, 3), torch.float32, -7.0) if rows_on else None
    d["ranges_traj"] = full(cuda, (T, B, R), torch.float32, -7.0) if scans else None
    one = full(cuda, (B, R), torch.float32, -7.0)
    row = (lambda t: d["ranges_traj"][t]) if scans else (lambda t: one)
    sc, wc = scan_config(capi, R, GEOM), world_config(capi, circles)
    rp, rc = capi.default_replan_config(num_waypoints=wp.shape[0]), capi.default_rollout_config()
    table, wpd, cid = dev(cuda, capi.traj_table(rp.plan)), dev(cuda, wp), dev(cuda, circles)
    held = full(cuda, (B, N, 2), torch.float32, 0.0)
    hlen, hidx = full(cuda, (B,), torch.int32, 0), full(cuda, (B,), torch.int32, 0)
    count = full(cuda, (T + 1,), torch.int32, 0)
    lst = full(cuda, (B,), torch.int32, -7)
    gap = None
    if rows_on:
        gap = torch.empty((B, 4), dtype=torch.int32, device=cuda)
        capi.cast_scans_dev(sc, wc, d["x_traj"][0], cid, row(0))
        capi.gap_search_dev(sc, row(0), gap)
    capi.replan_start_dev(rp, sc if rows_on else None, d["x_traj"][0], d["have_path"], d["x_ref"], gap, d["pose_traj"][0],
                          d["kind"][0], lst, count[0:1], hs=d["hs_traj"][0] if rows_on else None)
    for t in range(T):
        if scans:
            capi.cast_scans_dev(sc, wc, d["x_traj"][t], cid, row(t))
        else:
            capi.cast_scans_dev(sc, wc, d["x_traj"][t], cid, row(t), list_=lst, count=count[t:t + 1])
        capi.plan_listed_dev(rp, sc, lst, count[t:t + 1], d["pose_traj"][t], row(t), table, wpd, d["x_ref"],
                             d["plan_status"][t], d["best_traj"][t], d["best_global"][t])
        s.solve_dev_dbl(d["x_traj"][t], d["u_lin_traj"][t], d["x_ref"], d["hs_traj"][t] if gap_on else None,
                        d["u_plan"][t], d["x_plan"][t], d["status"][t], d["iters"][t], cost=d["cost"][t])
        last = t + 1 == T
        capi.advance_replan_dev(rc, rp, sc if rows_on and not last else None, N, d["x_traj"][t], d["kind"][t], d["u_plan"][t],
                                d["status"][t], d["plan_status"][t], d["x_ref"], held, hlen, hidx, d["have_path"],
                                d["x_traj"][t + 1], d["u_lin_traj"][t + 1], d["pose_traj"][t + 1], u_applied=d["u_applied"][t],
                                kind_next=None if last else d["kind"][t + 1], next_list=None if last else lst,
                                next_count=None if last else count[t + 1:t + 2],
                                gap=gap if rows_on and not last else None,
                                hs_next=d["hs_traj"][t + 1] if rows_on and not last else None)
    torch.cuda.synchronize(cuda)
    return {k: v.cpu().numpy() for k, v in d.items() if v is not None}


def compare(a, m, what, scans, hs):
    for k in OUT:
        same_bits(a[k], m[k], f"{what}: {k}")
    kind = a["kind"]
    mpc, plan = kind == rp_.MPC, np.isin(kind, (rp_.PLAN, rp_.PLAN_FAILED))
    for k in ON_MPC:
        same_bits(a[k][mpc], m[k][mpc], f"{what}: {k} on MPC ticks")
    for k in ON_PLAN:
        same_bits(a[k][plan], m[k][plan], f"{what}: {k} on PLAN ticks")
    if hs:
        same_bits(a["hs_traj"], m["hs_traj"], f"{what}: hs_traj")
    if scans:
        same_bits(a["ranges_traj"], m["ranges_traj"], f"{what}: ranges_traj")
    assert np.isin(kind[0], (rp_.PLAN, rp_.PLAN_FAILED)).all(), "every car starts without a path"


LOOPS = [(1, 2, 1), (1, 20, 2), (3, 2, 12), (3, 20, 2), (70, 2, 2), (70, 20, 12)]


@pytest.mark.parametrize("B,N,T", LOOPS, ids=[f"B{b}-N{n}-T{t}" for b, n, t in LOOPS])
def test_rollout_world_is_its_parts(capi, cuda, B, N, T):
    """f110qp_rollout_world_dev against the manual loop of public calls (cast_scans_dev -> plan_listed_dev ->
    solve_dev_dbl -> advance_replan_dev), bit-identical in every output: box rows without and with hs_traj,
    gap rows without and with hs_traj, with ranges_traj (all-cars casts) and without (listed casts); one
    world for all cars and, once per shape, one per car. 70 x N = 20 x T = 12 x 1,080 beams is the largest."""
    modes = [(gap, hs, scans) for gap in (False, True) for hs in (False, True) for scans in (True, False)]
    seen = set()
    for i, (gap, hs, scans) in enumerate(modes):
        per_car = i == 3 and B > 1
        case = world_case(B, per_car)
        s = solver(capi, N, gap=gap, x_ref_points=P)
        a = rollout_world_dev(capi, cuda, s, case, T, scans=scans, hs=hs)
        m = manual_world_loop(capi, cuda, s, case, T, scans, hs)
        s.close()
        compare(a, m, f"B {B} N {N} T {T} gap {gap} hs {hs} scans {scans} per-car {per_car}", scans, hs)
        seen |= set(np.unique(a["kind"]).tolist())
    if B == 70 and T == 12:
        assert {rp_.PLAN, rp_.MPC, rp_.HOLD} <= seen, seen


_REC = {}


def recorded(capi, cuda, gap=False):
    """One 70 x N = 20 x T = 12 call with every array recorded, shared by the tests below."""
    if gap not in _REC:
        s = solver(capi, 20, gap=gap, x_ref_points=P)
        _REC[gap] = rollout_world_dev(capi, cuda, s, world_case(70), 12)
        s.close()
    return _REC[gap]


def test_replay_of_the_recorded_scans(capi, cuda):
    """f110qp_rollout_replan_dev at scan_rows = T on the recorded ranges_traj reproduces every other output
    bit for bit. Compared with gap mode inactive and without hs_traj: the world call holds the first scan's
    gap records, the replay would search every row's."""
    import torch

    a = recorded(capi, cuda)
    x0, ul, circles, wp = world_case(70)
    B, N, T = 70, 20, 12
    s = solver(capi, N, x_ref_points=P)
    d = replan_buffers(cuda, x0, ul, B, N, T)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    s.rollout_replan_dev(capi.default_rollout_config(ticks=T), scan_config(capi, R, GEOM, scan_rows=T), rp,
                         dev(cuda, capi.traj_table(rp.plan)), dev(cuda, wp), d["x_ref"], d["have_path"],
                         dev(cuda, a["ranges_traj"]), d["x_traj"], d["u_lin_traj"], d["u_applied"], d["status"], d["iters"],
                         d["cost"], d["u_plan"], d["x_plan"], None, d["kind"], d["plan_status"], d["best_traj"],
                         d["best_global"], d["pose_traj"])
    torch.cuda.synchronize(cuda)
    s.close()
    m = {k: v.cpu().numpy() for k, v in d.items()}
    compare(a, m, "replay", False, False)


def test_recorded_scans_match_the_oracle(capi, cuda):
    """Every row t of ranges_traj against the oracle cast at x_traj row t: world_cases' bound on every
    non-grazing beam, at most 0.1 % of a row's beams grazing. 8 cars x 12 ticks (the oracle takes 15 ms a
    scan); the rows of the 70-car call are the same kernel's, compared with the manual loop's above."""
    s = solver(capi, 20, x_ref_points=P)
    a = rollout_world_dev(capi, cuda, s, world_case(8), 12)
    s.close()
    w = wc_.track_world()
    worst = 0.0
    assert (a["x_traj"][12] != a["x_traj"][0]).any(axis=1).all(), "every car moved"
    for t in range(12):
        _, e = wc_.check_scan(a["ranges_traj"][t], a["x_traj"][t], w, GEOM, R, f"tick {t}")
        worst = max(worst, e)
    print(f"recorded scans: worst error {worst:.3f} of the bound")


@pytest.mark.parametrize("gap", [False, True], ids=["box", "gap"])
def test_listed_casts_equal_all_cars_casts(capi, cuda, gap):
    """ranges_traj NULL (the cast runs on each tick's plan list, into one row set of the context) against
    ranges_traj given (all cars, every tick): bit-identical trajectories, kinds and statuses, and every
    other output where it is specified."""
    a = recorded(capi, cuda, gap)
    s = solver(capi, 20, gap=gap, x_ref_points=P)
    b = rollout_world_dev(capi, cuda, s, world_case(70), 12, scans=False)
    s.close()
    compare(a, b, f"listed casts, gap {gap}", False, True)


def test_rollout_world_continues(capi, cuda):
    """Two calls of 6 ticks through x_ref / have_path against one of 12, under rollout_replan's carry-over
    rule: the first call is the long call's first half; the second call's first tick has the long call's
    kind, pose and scan for every car; a car whose tick 6 is an MPC tick publishes a new plan there and is
    bit-identical from then on (the held plan does not carry over: the others drive fail_u on tick 6)."""
    T = 6
    whole = recorded(capi, cuda)
    case = world_case(70)
    s = solver(capi, 20, x_ref_points=P)
    first = rollout_world_dev(capi, cuda, s, case, T)
    second = rollout_world_dev(capi, cuda, s, case, T, start=first)
    s.close()
    for k in ("x_traj", "u_lin_traj", "u_applied", "status", "kind", "pose_traj", "hs_traj", "ranges_traj"):
        n = T + 1 if k in ("x_traj", "u_lin_traj", "pose_traj") else T
        same_bits(first[k], whole[k][:n], f"first call, {k}")
    k6 = whole["kind"][T]
    np.testing.assert_array_equal(second["kind"][0], k6)
    same_bits(second["pose_traj"][0], whole["pose_traj"][T], "pose of tick 6")
    same_bits(second["ranges_traj"][0], whole["ranges_traj"][T], "scan of tick 6")
    mpc = k6 == rp_.MPC
    assert mpc.any()
    for k in ("x_traj", "u_lin_traj", "u_applied", "status", "kind", "pose_traj", "ranges_traj"):
        same_bits(second[k][:, mpc], whole[k][T:][:, mpc], f"cars on an MPC tick at 6, {k}")
    same_bits(second["x_ref"][mpc], whole["x_ref"][mpc], "their final paths")
    np.testing.assert_array_equal(second["have_path"][mpc], whole["have_path"][mpc])
    same_bits(second["u_applied"][0][~mpc], np.tile(np.float32(rc_.FAIL_U), (int((~mpc).sum()), 1)), "a fresh node")


def test_the_scan_follows_the_car(capi, cuda):
    """One obstacle 1.2 m ahead of the LiDAR and no wall: the planner sees it on tick 0 and the car drives
    on (at fail_u or on its plan, forwards either way), so the obstacle's nearest return shortens from tick
    to tick: the recorded scan of the last tick differs from tick 0's, and each row is the oracle's at that
    row's pose."""
    x0 = wc_.track_poses(1)
    ox, oy = x0[0, 0] + 0.275 * np.cos(x0[0, 2]), x0[0, 1] + 0.275 * np.sin(x0[0, 2])
    ci = np.array([[ox + 1.2 * np.cos(x0[0, 2] + 0.4), oy + 1.2 * np.sin(x0[0, 2] + 0.4), 0.2]])
    case = (x0, np.tile([rc_.V_LIN, 0.0], (1, 1)), ci, workload.track_waypoints())
    T = 8
    s = solver(capi, 20, x_ref_points=P)
    a = rollout_world_dev(capi, cuda, s, case, T)
    s.close()
    rg = a["ranges_traj"][:, 0]
    for t in range(T):
        wc_.check_scan(a["ranges_traj"][t], a["x_traj"][t], ci, GEOM, R, f"tick {t}")
    near = rg.min(axis=1)
    assert near[0] < 1.01 and (np.diff(near) < 0).all(), near
    assert (rg[T - 1] != rg[0]).sum() > 20
    moved = np.hypot(*(a["x_traj"][T, 0, :2] - a["x_traj"][0, 0, :2]))
    assert moved > 0.03, moved
