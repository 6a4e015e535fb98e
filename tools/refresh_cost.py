"""Cost and effect of a refreshed MPC scan in the closed loop, the set-up of tools/walls_cost.py: 4,096 cars x
N = 20, T = 50 ticks, 1,080 beams (product library, AUTO back end), by HIP events on the stream, one process, in
workload.make_wall_world(5, 40) (250 segments + 40 circles); the cars start on workload.make_race_grid(256, 16,
seed=91) as races of G = 16 and as G = 1, every car without a path, stop_on_contact = 0.
  (a) us per tick of f110qp_rollout_walls_dev, gap rows INACTIVE: the control;
  (b) f110qp_rollout_refresh_dev at every = 0, the same configuration: the same launches;
  (c) f110qp_rollout_refresh_dev with gap rows ACTIVE at every = 0, 1 and 5, ranges_traj NULL;
  (d) one f110qp_gap_refresh_dev launch for all cars next to f110qp_gap_search_dev + f110qp_half_space_rows_dev
      back to back, on the scans cast at row 0;
  (e) per G and every, gap rows ACTIVE: the shares of F110QP_PRIMAL_INFEASIBLE and F110QP_NUMERICAL among the
      50 x 4,096 statuses, of PLAN_FAILED among the kinds, and of cars crashed by row 50 (margin 0).
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`.

usage: python tools/refresh_cost.py [rounds [out.json]]   (default profiles/r18/refresh_cost.json)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contact_cost import BEAMS, B, N, P, T, shares  # noqa: E402
from f110qp import capi, workload  # noqa: E402
from world_cost import stat, timed  # noqa: E402

GROUPS = (16, 1)
PERIODS = (0, 1, 5)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r18", "refresh_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    x0 = workload.make_race_grid(B // 16, 16, seed=91)
    ul = np.tile([4.5, 0.0], (B, 1))
    wp = workload.track_waypoints()
    segs, obst = workload.make_wall_world(5, 40)
    amin, ainc, amax = workload.scan_geometry(BEAMS)
    solvers = {gap: capi.Solver(capi.default_config(N, x_ref_points=P, gap_mode=capi.GAP_ACTIVE if gap else
                                                    capi.GAP_INACTIVE)) for gap in (False, True)}
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=amin, angle_increment=ainc, angle_max=amax)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    wc = capi.default_world_config(num_circles=obst.shape[0])
    wl = capi.default_walls_config(num_segments=segs.shape[0])
    body, cc = capi.default_body_config(), capi.default_contact_config(stop_on_contact=0)
    races = {G: capi.default_race_config(group_size=G) for G in GROUPS}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, obd, sgd = t(capi.traj_table(rp.plan)), t(wp), t(obst), t(segs)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt, kt = z((T, B, 2), torch.float32), z((T, B), torch.int32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    clt, crash = z((T + 1, B), torch.float64), z((B,), torch.int32)
    rg, gap_rec, hs = z((B, BEAMS), torch.float32), z((B, 4), torch.int32), z((B, 2, 3), torch.float32)

    def rollout(gap, G, every, kind=None):
        have.zero_()  # every call replays the same ticks: no car holds a path
        s = solvers[gap]
        if every is None:
            s.rollout_walls_dev(rc, sc, rp, wc, races[G], cc, body, wl, table, wpd, xr, have, obd, sgd, xt, ult, ua, stt,
                                clt, crash, kind_traj=kind)
        else:
            s.rollout_refresh_dev(rc, sc, rp, wc, races[G], cc, body, wl, capi.default_refresh_config(every=every), table,
                                  wpd, xr, have, obd, sgd, xt, ult, ua, stt, clt, crash, kind_traj=kind)

    effect = {}
    for G in GROUPS:
        for every in PERIODS:
            rollout(True, G, every, kt)
            torch.cuda.synchronize()
            st = stt.cpu().numpy()
            effect[f"G{G}_every{every}"] = {
                "primal_infeasible_share": round(float((st == capi.PRIMAL_INFEASIBLE).mean()), 4),
                "numerical_share": round(float((st == capi.NUMERICAL).mean()), 4),
                "solved_share": round(float((st == capi.SOLVED).mean()), 4),
                "plan_failed_share": shares(kt.cpu().numpy()).get("PLAN_FAILED", 0.0),
                "crashed_share_by_row_50": round(float((crash.cpu().numpy() >= 0).mean()), 4)}
    xt[0] = t(x0)
    capi.cast_scans_walls_dev(sc, wc, races[16], body, wl, xt[0], obd, sgd, rg)

    def two_launches():
        capi.gap_search_dev(sc, rg, gap_rec)
        capi.half_space_rows_dev(sc, gap_rec, xt[0], hs)

    variants = {"gap_search_then_half_space_rows": (two_launches, 1),
                "gap_refresh": (lambda: capi.gap_refresh_dev(sc, rg, xt[0], gap_rec, hs), 1)}
    for G in GROUPS:
        variants[f"rollout_walls_dev_G{G}_inactive"] = (lambda G=G: rollout(False, G, None), T)
        variants[f"rollout_refresh_dev_G{G}_inactive_every0"] = (lambda G=G: rollout(False, G, 0), T)
        for every in PERIODS:
            variants[f"rollout_refresh_dev_G{G}_active_every{every}"] = (lambda G=G, every=every: rollout(True, G, every), T)
    for fn, _ in variants.values():  # warm-up: code objects, workspaces
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, per) in variants.items():
            ev[k].append(timed(stream, fn) / per)
    res = {"B": B, "N": N, "T": T, "beams": BEAMS, "segments": int(segs.shape[0]), "circles": int(obst.shape[0]),
           "rounds": rounds, "start": "make_race_grid(256, 16, seed=91)", "stop_on_contact": 0,
           "backend_info": {("active" if g else "inactive"): list(s.backend_info(B)) for g, s in solvers.items()},
           "unit": "us by HIP events: median, [min, max]; the rollouts per tick, the single launches per call",
           "note": "the rollout times include one have_path memset per call",
           **{k: stat(v) for k, v in ev.items()}, "effect": effect}
    for s in solvers.values():
        s.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
