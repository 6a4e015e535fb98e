"""Cost and effect of straight walls in the closed loop, the set-up of tools/body_cost.py: 4,096 cars x N = 20,
T = 50 ticks, 1,080 beams (product library, AUTO back end, gap_mode INACTIVE), by HIP events on the stream, one
process: the cars start on workload.make_race_grid(256, 16, seed=91), every car without a path, in two worlds of
the same track: workload.make_world(5, 40) (1,040 circles, f110qp_rollout_body_dev's world) and
workload.make_wall_world(5, 40) (250 segments + 40 circles).
  (a) one all-cars cast launch and one clearance launch at x_traj row 0, G = 16: f110qp_cast_scans_walls_dev and
      f110qp_clearance_walls_dev in the walls world next to their body twins in the circle world;
  (b) us per tick of f110qp_rollout_walls_dev next to the yardstick f110qp_rollout_body_dev, G = 1, 4 and 16,
      stop_on_contact = 0 and 1;
  (c) per G and stop, for both worlds: the share of cars crashed by row 50 (margin 0), the share of the
      50 x 4,096 ticks by kind, and from f110qp_race_standings at row 50 the share of cars whose rank differs
      from the grid rank.
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`.

usage: python tools/walls_cost.py [rounds [out.json]]   (default profiles/r17/walls_cost.json)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contact_cost import BEAMS, GROUPS, B, N, P, T, shares  # noqa: E402
from f110qp import capi, workload  # noqa: E402
from world_cost import stat, timed  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r17", "walls_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    x0 = workload.make_race_grid(B // 16, 16, seed=91)
    ul = np.tile([4.5, 0.0], (B, 1))
    wp = workload.track_waypoints()
    world = workload.make_world(5, 40)
    segs, obst = workload.make_wall_world(5, 40)
    amin, ainc, amax = workload.scan_geometry(BEAMS)
    s = capi.Solver(capi.default_config(N, x_ref_points=P))
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=amin, angle_increment=ainc, angle_max=amax)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    wc = capi.default_world_config(num_circles=world.shape[0])
    wcw = capi.default_world_config(num_circles=obst.shape[0])
    wl = capi.default_walls_config(num_segments=segs.shape[0])
    body = capi.default_body_config()
    races = {G: capi.default_race_config(group_size=G) for G in GROUPS}
    ccs = {stop: capi.default_contact_config(stop_on_contact=stop) for stop in (0, 1)}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, cid, obd, sgd = t(capi.traj_table(rp.plan)), t(wp), t(world), t(obst), t(segs)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt, kt = z((T, B, 2), torch.float32), z((T, B), torch.int32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    clt, crash = z((T + 1, B), torch.float64), z((B,), torch.int32)
    rg = z((B, BEAMS), torch.float32)

    def rollout(walls, G, stop, kind=None):
        have.zero_()  # every call replays the same ticks: no car holds a path
        if walls:
            s.rollout_walls_dev(rc, sc, rp, wcw, races[G], ccs[stop], body, wl, table, wpd, xr, have, obd, sgd, xt, ult, ua,
                                stt, clt, crash, kind_traj=kind)
        else:
            s.rollout_body_dev(rc, sc, rp, wc, races[G], ccs[stop], body, table, wpd, xr, have, cid, xt, ult, ua, stt, clt,
                               crash, kind_traj=kind)

    effect = {}
    for G in GROUPS:
        for stop in (0, 1):
            for walls in (False, True):
                rollout(walls, G, stop, kt)
                torch.cuda.synchronize()
                ct = crash.cpu().numpy()
                st = capi.race_standings(races[G], xt.cpu().numpy()[[0, T]], wp, seg=False, lateral=False, lap=False)
                effect[f"{'walls' if walls else 'discs'}_G{G}_stop{stop}"] = {
                    "crashed_share_by_row_50": round(float((ct >= 0).mean()), 4), "kind_share": shares(kt.cpu().numpy()),
                    "rank_differs_from_grid": round(float((st["rank"][1] != st["rank"][0]).mean()), 4)}
    xt[0] = t(x0)
    variants = {"clearance_body_rows1_G16": (lambda: capi.clearance_body_dev(wc, races[16], body, xt[0], cid, clt[0]), 1),
                "clearance_walls_rows1_G16": (lambda: capi.clearance_walls_dev(wcw, races[16], body, wl, xt[0], obd, sgd,
                                                                                 clt[0]), 1),
                "cast_body_G16": (lambda: capi.cast_scans_body_dev(sc, wc, races[16], body, xt[0], cid, rg), 1),
                "cast_walls_G16": (lambda: capi.cast_scans_walls_dev(sc, wcw, races[16], body, wl, xt[0], obd, sgd, rg), 1)}
    for G in GROUPS:
        for stop in (0, 1):
            variants[f"rollout_body_dev_G{G}_stop{stop}"] = (lambda G=G, stop=stop: rollout(False, G, stop), T)
            variants[f"rollout_walls_dev_G{G}_stop{stop}"] = (lambda G=G, stop=stop: rollout(True, G, stop), T)
    for fn, _ in variants.values():  # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, per) in variants.items():
            ev[k].append(timed(stream, fn) / per)
    res = {"B": B, "N": N, "T": T, "beams": BEAMS, "circles": int(world.shape[0]), "segments": int(segs.shape[0]),
           "circles_next_to_segments": int(obst.shape[0]), "rounds": rounds, "start": "make_race_grid(256, 16, seed=91)",
           "backend_info": list(s.backend_info(B)),
           "unit": "us by HIP events: median, [min, max]; the rollouts per tick, the single launches per launch",
           "note": "the rollout times include one have_path memset per call",
           **{k: stat(v) for k, v in ev.items()}, "effect": effect}
    s.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
