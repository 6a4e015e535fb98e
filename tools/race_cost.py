"""Cost of head-to-head races in the closed loop, 4,096 cars x N = 20, T = 50 ticks, 1,080 beams (product
library, AUTO back end, gap_mode INACTIVE), by HIP events on the stream, one process: the cars start on
workload.make_race_grid (races of 16; the same poses for every group size) in the track world of
workload.make_world(5, 40) (1,040 circles), every car without a path.
  (a) us per tick of the yardstick, f110qp_rollout_world_dev, and of f110qp_rollout_race_dev at G = 1, 4 and
      16, each with the casts on each tick's plan list (no ranges_traj) and with ranges_traj (every car cast
      every tick);
  (b) one cast launch for all 4,096 cars: f110qp_cast_scans_dev, and f110qp_cast_scans_race_dev at G = 1, 4
      and 16 (the kernel alone: the tick-kind mix of (a) changes with the opponents, this does not);
  (c) the share of the 50 x 4,096 ticks by kind for the world call and for every G.
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`. Every call of
(a) starts from the same cars without a path, so each replays the same 50 ticks.

usage: python tools/race_cost.py [rounds [out.json]]   (default profiles/r11/race_cost.json)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from f110qp import capi, workload  # noqa: E402
from world_cost import shares, stat, timed  # noqa: E402

B, N, T, BEAMS, P = 4096, 20, 50, 1080, 50
GROUPS = (1, 4, 16)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r11", "race_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    x0 = workload.make_race_grid(B // 16, 16, seed=91)
    ul = np.tile([4.5, 0.0], (B, 1))
    wp = workload.track_waypoints()
    world = workload.make_world(5, 40)
    amin, ainc, amax = workload.scan_geometry(BEAMS)
    s = capi.Solver(capi.default_config(N, x_ref_points=P))
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=amin, angle_increment=ainc, angle_max=amax)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    wc = capi.default_world_config(num_circles=world.shape[0])
    races = {G: capi.default_race_config(group_size=G) for G in GROUPS}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, cid = t(capi.traj_table(rp.plan)), t(wp), t(world)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt, kt = z((T, B, 2), torch.float32), z((T, B), torch.int32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    rgt = z((T, B, BEAMS), torch.float32)
    one = z((B, BEAMS), torch.float32)

    def rollout(G=None, kind=None, scans=None):
        have.zero_()  # every call replays the same ticks: no car holds a path
        if G is None:
            s.rollout_world_dev(rc, sc, rp, wc, table, wpd, xr, have, cid, xt, ult, ua, stt, kind_traj=kind,
                                ranges_traj=scans)
        else:
            s.rollout_race_dev(rc, sc, rp, wc, races[G], table, wpd, xr, have, cid, xt, ult, ua, stt, kind_traj=kind,
                               ranges_traj=scans)

    kinds = {}
    for G in (None,) + GROUPS:
        rollout(G, kt)
        torch.cuda.synchronize()
        kinds["world" if G is None else f"race_G{G}"] = shares(kt.cpu().numpy())

    variants = {"rollout_world_dev_listed": (lambda: rollout(), T),
                "rollout_world_dev_ranges_traj": (lambda: rollout(scans=rgt), T),
                "cast_all_cars": (lambda: capi.cast_scans_dev(sc, wc, xt[0], cid, one), 1)}
    for G in GROUPS:
        variants[f"rollout_race_dev_G{G}_listed"] = (lambda G=G: rollout(G), T)
        variants[f"rollout_race_dev_G{G}_ranges_traj"] = (lambda G=G: rollout(G, scans=rgt), T)
        variants[f"cast_race_all_cars_G{G}"] = (lambda G=G: capi.cast_scans_race_dev(sc, wc, races[G], xt[0], cid, one), 1)
    for fn, _ in variants.values():  # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, per) in variants.items():
            ev[k].append(timed(stream, fn) / per)
    res = {"B": B, "N": N, "T": T, "beams": BEAMS, "circles": int(world.shape[0]), "rounds": rounds,
           "start": "make_race_grid(256, 16, seed=91)", "backend_info": list(s.backend_info(B)),
           "unit": "us by HIP events: median, [min, max]; the rollouts per tick, the casts per launch",
           "note": "the rollout times include one have_path memset per call",
           **{k: stat(v) for k, v in ev.items()}, "kind_share": kinds}
    s.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
