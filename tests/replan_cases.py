"""Inputs and CPU references of the re-planning closed-loop tests (test_gpu_rollout_replan.py): the per-car
state machine of Project::OdomCallback + Project::DriveStep (f110-mpc_amd/host/src/project.cpp:31-100,
include/f110qp.h "closed loop with re-planning") restated in numpy, the scenes, the CPU chain (oracle.plan,
oracle.solve on doubles, rollout_cases.plant_step, the numpy state machine) and the CPU check that chose
the seed of the chain test:
    python tests/replan_cases.py [first_seed [count]]
and the one that chose the cars of the loop cases:
    python tests/replan_cases.py cars
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "f110-mpc_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rollout_cases as rc_  # noqa: E402

from f110qp import workload  # noqa: E402

MPC, PLAN, HOLD, PLAN_FAILED = 0, 1, 2, 3  # F110QP_TICK_*
NO_SOLVE = 0
REPLAN_DIST = 1.98
USABLE = (1, 2)  # F110QP_SOLVED, F110QP_SOLVED_INACCURATE
MARGIN = 1e-3    # the chain seed keeps |dist - 1.98| and the two best end-point distances this far apart
REPLAN_SEED = 11636  # chosen by choose_replan_seed(11054, 1500) below; none of the seeds 1 .. 553 passes


# ---- the specification in numpy --------------------------------------------------------------------

def calc_dist(x, y, ex, ey):
    """Transforms::CalcDist((float)x, (float)y, (float)ex, (float)ey): float differences, squared and
    added in double, the double root narrowed to float32."""
    f = np.float32
    dx = (np.asarray(x, np.float64).astype(f) - np.asarray(ex, np.float64).astype(f)).astype(np.float64)
    dy = (np.asarray(y, np.float64).astype(f) - np.asarray(ey, np.float64).astype(f)).astype(np.float64)
    return np.sqrt(dx * dx + dy * dy).astype(f)


def next_kind(have, x, x_ref, replan_dist=REPLAN_DIST):
    """The kind of the tick at pose x [B,3] for cars holding have [B] and paths x_ref [B,P,3]."""
    with np.errstate(invalid="ignore"):
        d = calc_dist(x[:, 0], x[:, 1], x_ref[:, -1, 0], x_ref[:, -1, 1])
        near = d.astype(np.float64) < replan_dist
    return np.where(have == 0, PLAN, np.where(near, HOLD, MPC)).astype(np.int32)


def new_state(B, N):
    """A fresh node: no path, no published plan."""
    return dict(have=np.zeros(B, np.int32), held=np.zeros((B, N, 2), np.float32), len=np.zeros(B, np.int32),
                idx=np.zeros(B, np.int32))


def tick_action(S, kind, plan_status, status, u_plan, fail_u=rc_.FAIL_U):
    """One tick's action on the state S (in place) and Project::DriveStep. Returns (the kind as reported,
    the status as reported, the applied input [B,2] float64, u_applied [B,2] float32, the steer of the next
    linearisation input [B])."""
    B, N = S["held"].shape[:2]
    kind = kind.copy()
    status = status.copy()
    plan = kind == PLAN
    ok = plan & (plan_status == 0)
    kind[plan & ~ok] = PLAN_FAILED
    S["have"][ok] = 1
    hold = kind == HOLD
    S["have"][hold] = 0
    S["idx"][hold] = 0
    mpc = kind == MPC
    usable = mpc & np.isin(status, USABLE)
    S["held"][usable] = u_plan[usable]
    S["len"][usable] = N
    S["len"][mpc & ~usable] = 0
    S["idx"][mpc] = 0
    status[~mpc] = NO_SOLVE
    cars = np.arange(B)
    has0 = S["idx"] < S["len"]
    a0 = S["held"][cars, np.minimum(S["idx"], N - 1)]
    u32 = np.where(has0[:, None], a0, np.float32(fail_u)[None, :]).astype(np.float32)
    u = np.where(has0[:, None], a0.astype(np.float64), np.float64(fail_u)[None, :])
    S["idx"] += 1
    has1 = S["idx"] < S["len"]
    a1 = S["held"][cars, np.minimum(S["idx"], N - 1), 1].astype(np.float64)
    nxt = np.where(has1, a1, fail_u[1])
    return kind, status, u, u32, nxt


def pose_row(x):
    """(x, y, sin(ori/2), cos(ori/2)) of states x [B,3]."""
    return np.stack([x[:, 0], x[:, 1], np.sin(x[:, 2] * 0.5), np.cos(x[:, 2] * 0.5)], 1)


# ---- scenes ------------------------------------------------------------------------------------------

def replan_case(B, seed, blocked=(), T=None, blocked_rows=None, cars=None):
    """B cars of workload.make_scenes: (x0 [B,3], u_lin [B,2], ranges, (angle_min, inc, max), waypoints
    [W,2]). The cars in `blocked` see a ring of returns at 0.5 m (no valid candidate, and no gap). T: ranges
    [T,B,R], the scan repeated for every tick, with the cars of blocked_rows = {tick: cars} ringed on those
    rows only. cars: the scenes of make_scenes(B) to keep, in this order."""
    sc = workload.make_scenes(B, seed=seed)
    if cars is not None:
        sc = dict(sc, pose=sc["pose"][list(cars)], ranges=sc["ranges"][list(cars)])
        B = len(cars)
    pose = sc["pose"]
    yaw = 2.0 * np.arctan2(pose[:, 2], pose[:, 3])
    x0 = np.ascontiguousarray(np.stack([pose[:, 0], pose[:, 1], yaw], 1))
    ul = np.tile([rc_.V_LIN, 0.0], (B, 1))
    ranges = sc["ranges"].copy()
    for b in blocked:
        ranges[b] = 0.5
    if T is not None:
        ranges = np.ascontiguousarray(np.tile(ranges[None], (T, 1, 1)))
        for t, cars in (blocked_rows or {}).items():
            ranges[t, list(cars)] = 0.5
    return x0, ul, ranges, (sc["angle_min"], sc["angle_inc"], sc["angle_max"]), sc["waypoints"]


# The cars of the loop-is-its-parts cases: scenes of make_scenes(LOOP_POOL, LOOP_SEED) chosen by
# choose_loop_cars() on the CPU chain alone. Each shows PLAN, MPC and HOLD and plans at least twice within
# 20 ticks at N = 2 and N = 20, with box rows and with gap rows (a car that picks one of the sharp candidates
# whose end lies within 1.98 m alternates PLAN and HOLD; one whose gap-row solves fail crawls at fail_u and
# never reaches its path's end: neither is in the list); the first one plans again on one of the ticks 6 to 9.
LOOP_SEED, LOOP_POOL = 7, 300
LOOP_CARS = (0, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 16, 17, 18, 20, 21, 25, 26, 27, 28, 31, 32, 33, 38, 39, 40, 41, 42, 45,
             46, 47, 49, 50, 52, 53, 54, 56, 57, 58, 59, 60, 62, 63, 64, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 77, 79,
             80, 82, 83, 84, 85, 86, 87, 88, 89, 90, 91, 93, 94)


def loop_case(B, T, rows):
    """The scene of a parts case: the first B of LOOP_CARS; car 3 (of 5 and 70) sits behind a ring of returns
    and never plans. With a scan per tick, car 0's scan is ringed on ticks 6 to 9: the plan it makes there
    fails until tick 10."""
    assert len(LOOP_CARS) >= B
    blocked = (3,) if B > 3 else ()
    kw = dict(T=T, blocked_rows={t: (0,) for t in range(6, 10)}) if rows > 1 else {}
    return replan_case(LOOP_POOL, LOOP_SEED, blocked, cars=LOOP_CARS[:B], **kw)


def shows_every_kind(kind):
    """Per car of kind [T,B]: PLAN, MPC and HOLD occur, at least two PLAN ticks, no failed plan."""
    return ((kind == PLAN).sum(0) >= 2) & (kind == MPC).any(0) & (kind == HOLD).any(0) & ~(kind == PLAN_FAILED).any(0)


def choose_loop_cars(count=70, T=20):
    import oracle

    oracle.build()
    x0, ul, ranges, geom, wp = replan_case(LOOP_POOL, LOOP_SEED)
    good = np.ones(LOOP_POOL, bool)
    first = np.ones(LOOP_POOL, bool)
    for N in (2, 20):
        for gap in (False, True):
            kind = cpu_chain(oracle, x0, ul, ranges, geom, wp, N, T, gap=gap)["kind"]
            good &= shows_every_kind(kind)
            first &= (kind[6:10] == PLAN).any(0)
    lead = int(np.flatnonzero(good & first)[0])
    cars = [lead] + [int(b) for b in np.flatnonzero(good) if b != lead][:count - 1]
    return tuple(cars)


# ---- the CPU chain -----------------------------------------------------------------------------------

def end_point_margin(pose, r, table):
    """The margin between the two smallest end-point distances of the valid candidates of an oracle plan
    r (project.cpp:122-141), recomputed in numpy; inf with fewer than two."""
    valid = np.flatnonzero(r["valid"])
    if len(valid) < 2 or r["status"] != 0:
        return np.inf
    x, y, qz, qw = pose
    c, s = 1 - 2 * qz * qz / (qz * qz + qw * qw), 2 * qw * qz / (qz * qz + qw * qw)
    e = table[valid, -1, :2]
    ex, ey = c * e[:, 0] - s * e[:, 1] + x, s * e[:, 0] + c * e[:, 1] + y
    d = np.sort(np.hypot(ex - r["goal"][0], ey - r["goal"][1]))
    return float(d[1] - d[0])


def cpu_chain(oracle, x0, ul, ranges, geom, wp, N, T, gap=False, stop_below=None):
    """T ticks of the loop on the CPU: oracle.fill_occ_grid + oracle.plan at the pose row on PLAN ticks,
    oracle.solve on the fp64 state on MPC ticks (oracle.solve_batch narrows its inputs to float32; the
    per-car entry takes the doubles), rollout_cases.plant_step, the numpy state machine. ranges [B,R], one
    scan per car, or [T,B,R], one per tick. stop_below: give up (None) at the first tick on which a margin
    falls below it (the seed search). Returns the per-tick arrays and the smallest margins met: `dist` = min |dist - 1.98|
    over (tick, car) with a path, `ends` = min end-point margin over the plans."""
    import rollout_scan_cases as sc_

    pp = oracle.plan_params()
    table = oracle.traj_table(pp)
    prm = oracle.params(N)
    B, P = x0.shape[0], table.shape[1]
    S = new_state(B, N)
    xr = np.full((B, P, 3), np.nan)
    out = dict(x_traj=np.zeros((T + 1, B, 3)), u_lin_traj=np.zeros((T + 1, B, 2)), u_applied=np.zeros((T, B, 2), np.float32),
               kind=np.zeros((T, B), np.int32), status=np.zeros((T, B), np.int32), plan_status=np.full((T, B), -9, np.int32),
               best_traj=np.full((T, B), -9, np.int32), best_global=np.full((T, B), -9, np.int32))
    out["x_traj"][0], out["u_lin_traj"][0] = x0, ul
    m_dist = m_ends = np.inf
    for t in range(T):
        x, u_lin = out["x_traj"][t], out["u_lin_traj"][t]
        kind = next_kind(S["have"], x, xr)
        with np.errstate(invalid="ignore"):
            d = calc_dist(x[:, 0], x[:, 1], xr[:, -1, 0], xr[:, -1, 1]).astype(np.float64)
        if (S["have"] == 1).any():
            m_dist = min(m_dist, float(np.abs(d[S["have"] == 1] - REPLAN_DIST).min()))
        if stop_below is not None and min(m_dist, m_ends) < stop_below:
            return None
        pose = pose_row(x)
        rg = ranges[t] if ranges.ndim == 3 else ranges
        ps = np.full(B, -9, np.int32)
        for b in np.flatnonzero(kind == PLAN):
            g, off = oracle.fill_occ_grid(pp, pose[b], rg[b], *geom)
            r = oracle.plan(pp, pose[b], g, off, table, wp)
            ps[b], out["best_traj"][t, b], out["best_global"][t, b] = r["status"], r["best_traj"], r["best_global"]
            if r["status"] == 0:
                xr[b] = r["x_ref"].astype(np.float64)
                if r["best_global"] >= 0:
                    m_ends = min(m_ends, end_point_margin(pose[b], dict(r, goal=wp[r["best_global"]]), table))
        st = np.zeros(B, np.int32)
        up = np.full((B, N, 2), np.nan, np.float32)
        hs = sc_.rows_at(oracle, x, rg, geom) if gap else None
        for b in np.flatnonzero(kind == MPC):
            r = oracle.solve(prm, x[b], u_lin[b], xr[b, :N], None if hs is None else hs[b], gap)
            st[b] = r["status"]
            if r["status"] == oracle.SOLVED:
                up[b] = r["u"].astype(np.float32)
        out["plan_status"][t] = ps
        out["kind"][t], out["status"][t], u, out["u_applied"][t], nxt = tick_action(S, kind, ps, st, up)
        out["x_traj"][t + 1] = rc_.plant_step(x, u)
        out["u_lin_traj"][t + 1] = np.stack([np.full(B, rc_.V_LIN), nxt], 1)
    out.update(x_ref=xr, have_path=S["have"].copy(), min_dist_margin=m_dist, min_end_margin=m_ends)
    return out


def replan_seed_is_robust(oracle, seed, B=64, N=20, T=20, search=False):
    """The conditions on the chain seed, from the CPU chain alone: no tick with |dist - 1.98| or the margin
    between the two best end-point distances below MARGIN, no uncertified solve, every kind occurs."""
    x0, ul, ranges, geom, wp = replan_case(B, seed, blocked=(3,))
    out = cpu_chain(oracle, x0, ul, ranges, geom, wp, N, T, stop_below=MARGIN if search else None)
    if out is None:
        return False, None
    kinds = set(np.unique(out["kind"]).tolist())
    ok = (out["min_dist_margin"] >= MARGIN and out["min_end_margin"] >= MARGIN and kinds == {MPC, PLAN, HOLD, PLAN_FAILED}
          and not (out["status"] == oracle.UNCERTIFIED).any())
    return ok, out


def choose_replan_seed(first=1, count=20):
    import oracle

    oracle.build()
    for seed in range(first, first + count):
        ok, out = replan_seed_is_robust(oracle, seed, search=True)
        if out is None:
            continue
        vals, n = np.unique(out["kind"], return_counts=True)
        print(f"seed {seed}: ok={ok} kinds {dict(zip(vals.tolist(), n.tolist()))} min |dist - 1.98| "
              f"{out['min_dist_margin']:.2e}, min end-point margin {out['min_end_margin']:.2e}", flush=True)
        if ok:
            return seed
    return None


if __name__ == "__main__":
    if sys.argv[1:2] == ["cars"]:
        print("LOOP_CARS =", choose_loop_cars())
        sys.exit(0)
    a = [int(v) for v in sys.argv[1:]]
    print("chosen:", choose_replan_seed(*a))
