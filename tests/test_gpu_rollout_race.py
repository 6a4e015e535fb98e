"""Head-to-head races in the closed loop on MI355X: f110qp_rollout_race[_dev] (include/f110qp.h, "head-to-head
races"). Between two device routes everything is bit equality; the recorded scans are compared with the numpy
oracle (world_cases' bound and cap) on per-car circle rows: the static world and, from workload.race_circles at
x_traj row t, the race-mates where they stood at that tick.

The cars start on workload.make_race_grid in the track world of workload.make_world(5, 40), without a path:
every car plans on tick 0 from the scan cast at its start pose, its race-mates in it.
"""
import numpy as np
import pytest
import race_cases as rc_
import replan_cases as rp_
import rollout_cases as roc_
import world_cases as wc_
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_replan import P, dev, full, replan_buffers
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_world import GEOM, R, compare, rollout_world_dev, world_case
from world_loop import rollout_dev

from f110qp import workload

pytestmark = pytest.mark.gpu


def race_case(B, G, seed=41, static="track"):
    """(x0 [B,3], u_lin [B,2], circles [C,3] or None, waypoints): B / G races on the grid of make_race_grid."""
    x0 = workload.make_race_grid(B // G, G, seed)
    return x0, np.tile([roc_.V_LIN, 0.0], (B, 1)), wc_.track_world() if static == "track" else None, workload.track_waypoints()


def configs(capi, circles, G):
    wc = capi.default_world_config(num_circles=0 if circles is None else circles.shape[-2],
                                   world_rows=1 if circles is None or circles.ndim == 2 else circles.shape[0])
    return wc, capi.default_race_config(group_size=G)


def rollout_race_dev(capi, cuda, s, case, G, T, scans=True, hs=True):
    """One Solver.rollout_race_dev call on fresh device arrays -> every array as numpy."""
    null = (() if hs else ("hs_traj",)) + (() if scans else ("ranges_traj",))
    return rollout_dev(capi, cuda, s, "race", case, T, group=G, null=null, scan_rows=7)


def manual_race_loop(capi, cuda, s, case, G, T, scans, hs):
    """The loop written with the public calls, all on the device: the memset, (rows computed)
    cast_scans_race_dev for all cars at row 0 and gap_search_dev, replan_start_dev; per tick
    cast_scans_race_dev (on the tick's list, or for all cars into row t), plan_listed_dev, solve_dev_dbl,
    advance_replan_dev."""
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
    sc = scan_config(capi, R, GEOM)
    wc, race = configs(capi, circles, G)
    rp, rc = capi.default_replan_config(num_waypoints=wp.shape[0]), capi.default_rollout_config()
    table, wpd = dev(cuda, capi.traj_table(rp.plan)), dev(cuda, wp)
    cid = None if circles is None else dev(cuda, circles)
    held = full(cuda, (B, N, 2), torch.float32, 0.0)
    hlen, hidx = full(cuda, (B,), torch.int32, 0), full(cuda, (B,), torch.int32, 0)
    count = full(cuda, (T + 1,), torch.int32, 0)
    lst = full(cuda, (B,), torch.int32, -7)
    gap = None
    if rows_on:
        gap = torch.empty((B, 4), dtype=torch.int32, device=cuda)
        capi.cast_scans_race_dev(sc, wc, race, d["x_traj"][0], cid, row(0))
        capi.gap_search_dev(sc, row(0), gap)
    capi.replan_start_dev(rp, sc if rows_on else None, d["x_traj"][0], d["have_path"], d["x_ref"], gap, d["pose_traj"][0],
                          d["kind"][0], lst, count[0:1], hs=d["hs_traj"][0] if rows_on else None)
    for t in range(T):
        if scans:
            capi.cast_scans_race_dev(sc, wc, race, d["x_traj"][t], cid, row(t))
        else:
            capi.cast_scans_race_dev(sc, wc, race, d["x_traj"][t], cid, row(t), list_=lst, count=count[t:t + 1])
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


LOOPS = [(2, 2, 2, 2), (6, 3, 20, 2), (72, 4, 20, 12)]


@pytest.mark.parametrize("B,G,N,T", LOOPS, ids=[f"B{b}-G{g}-N{n}-T{t}" for b, g, n, t in LOOPS])
def test_rollout_race_is_its_parts(capi, cuda, B, G, N, T):
    """9. f110qp_rollout_race_dev against the manual loop of public calls, bit-identical in every output
    test_gpu_rollout_world.py compares: box and gap rows, without and with hs_traj, with ranges_traj (all-cars
    casts) and without (listed casts)."""
    case = race_case(B, G)
    for gap in (False, True):
        for hs in (False, True):
            for scans in (True, False):
                s = solver(capi, N, gap=gap, x_ref_points=P)
                a = rollout_race_dev(capi, cuda, s, case, G, T, scans=scans, hs=hs)
                m = manual_race_loop(capi, cuda, s, case, G, T, scans, hs)
                s.close()
                compare(a, m, f"B {B} G {G} N {N} T {T} gap {gap} hs {hs} scans {scans}", scans, hs)


def test_group_of_one_is_the_world_rollout(capi, cuda):
    """10. G = 1 through f110qp_rollout_race_dev equals f110qp_rollout_world_dev bit for bit."""
    case = world_case(70)
    for gap in (False, True):
        s = solver(capi, 20, gap=gap, x_ref_points=P)
        a = rollout_race_dev(capi, cuda, s, case, 1, 12)
        w = rollout_world_dev(capi, cuda, s, case, 12)
        s.close()
        compare(a, w, f"G = 1, gap {gap}", True, True)


_REC = {}


def recorded(capi, cuda, B, gap=False):
    """One B x G = 4 x N = 20 x T = 12 call with every array recorded."""
    if (B, gap) not in _REC:
        s = solver(capi, 20, gap=gap, x_ref_points=P)
        _REC[B, gap] = rollout_race_dev(capi, cuda, s, race_case(B, 4), 4, 12)
        s.close()
    return _REC[B, gap]


@pytest.mark.parametrize("gap", [False, True], ids=["box", "gap"])
def test_listed_casts_equal_all_cars_casts(capi, cuda, gap):
    """11. ranges_traj NULL (each tick's cast runs on the plan list; the listed cars read their unlisted
    race-mates' poses from x_traj row t) against ranges_traj given: bit-identical trajectories, kinds and
    statuses, and every other output where it is specified."""
    a = recorded(capi, cuda, 72, gap)
    s = solver(capi, 20, gap=gap, x_ref_points=P)
    b = rollout_race_dev(capi, cuda, s, race_case(72, 4), 4, 12, scans=False)
    s.close()
    compare(a, b, f"listed casts, gap {gap}", False, True)
    assert rp_.MPC in set(np.unique(a["kind"]).tolist()), "ticks on which not every car is listed"


def test_recorded_scans_match_the_oracle(capi, cuda):
    """12. Every row t of ranges_traj against the oracle cast at x_traj row t with the opponents from
    race_circles(x_traj[t]): two races of four, 12 ticks; every car has moved."""
    c = rc_.rollout_race_start()
    case = (c.x, np.tile([roc_.V_LIN, 0.0], (8, 1)), c.static, workload.track_waypoints())
    s = solver(capi, 20, x_ref_points=P)
    a = rollout_race_dev(capi, cuda, s, case, c.G, 12)
    s.close()
    assert (a["x_traj"][12] != a["x_traj"][0]).any(axis=1).all(), "every car moved"
    worst = 0.0
    for t in range(12):
        _, e = c.check(a["ranges_traj"][t], a["x_traj"][t], f"tick {t}")
        worst = max(worst, e)
    alone = wc_.oracle_scan(a["x_traj"][11], c.static, GEOM, R)
    assert ((a["ranges_traj"][11] != alone).sum(axis=1) >= 10).all(), "the race-mates are still in the last scans"
    print(f"recorded race scans: worst error {worst:.3f} of the bound")


def test_the_opponent_is_seen_and_matters(capi, cuda):
    """13. Two cars and no static circle, the follower (car 1) 1.5 m straight behind the leader (car 0) on
    make_race_grid(lateral = 0). Tick 0: the follower's scan holds the leader's return, the leader's forward
    beams are all max_range, and the follower's plan differs from the plan the same car makes alone (G = 1).
    At 1.5 m the planner's grid registers the 0.3 m circle (the CPU planner on the oracle's scan: 47 occupied
    cells, best_traj 22 against 16 alone), so the distance the issue names is the distance used. Every later
    row of both cars matches the oracle at both cars' poses of that tick."""
    c = rc_.follower_start()
    case = (c.x, np.tile([roc_.V_LIN, 0.0], (2, 1)), None, workload.track_waypoints())
    T = 8
    s = solver(capi, 20, x_ref_points=P)
    a = rollout_race_dev(capi, cuda, s, case, 2, T)
    alone = rollout_race_dev(capi, cuda, s, case, 1, T)
    s.close()
    rg = a["ranges_traj"]
    ang = float(GEOM[0]) + float(GEOM[1]) * np.arange(R, dtype=np.float64)
    fwd = np.abs(ang) < np.pi / 2
    near = rc_.GAP + rc_.CENTER_OFFSET - wc_.LIDAR_OFFSET - rc_.CAR_RADIUS  # along the path's chord, a little less
    assert near - 0.02 < rg[0, 1].min() <= near + 1e-6, rg[0, 1].min()
    assert (rg[0, 0][fwd] == np.float32(wc_.MAX_RANGE)).all() and (rg[0, 0] < wc_.MAX_RANGE).any()
    assert (alone["ranges_traj"] == np.float32(wc_.MAX_RANGE)).all()
    assert a["kind"][0, 1] in (rp_.PLAN, rp_.PLAN_FAILED) and alone["kind"][0, 1] == rp_.PLAN
    assert (a["plan_status"][0, 1], a["best_traj"][0, 1]) != (alone["plan_status"][0, 1], alone["best_traj"][0, 1])
    assert (a["x_traj"][T] != a["x_traj"][0]).any(axis=1).all(), "both cars moved"
    for t in range(T):
        c.check(rg[t], a["x_traj"][t], f"tick {t}")


def test_host_call_equals_the_device_call(capi, cuda):
    """14. f110qp_rollout_race on host pointers equals f110qp_rollout_race_dev bit for bit."""
    B, G, N, T = 6, 3, 20, 4
    case = race_case(B, G)
    x0, ul, circles, wp = case
    for gap in (False, True):
        s = solver(capi, N, gap=gap, x_ref_points=P)
        a = rollout_race_dev(capi, cuda, s, case, G, T)
        rp = capi.default_replan_config(num_waypoints=wp.shape[0])
        h = s.rollout_race(x0, ul, circles, capi.default_race_config(group_size=G), scan_config(capi, R, GEOM), rp,
                           capi.traj_table(rp.plan), wp, T, plans=True, objective=True, scans=True)
        s.close()
        compare(a, h, f"host call, gap {gap}", True, True)
