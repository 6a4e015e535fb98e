"""Cost of contact in the closed loop, 4,096 cars x N = 20, T = 50 ticks, 1,080 beams (product library, AUTO
back end, gap_mode INACTIVE), by HIP events on the stream, one process: the cars start on
workload.make_race_grid(256, 16, seed=91) (the same poses for every group size) in the track world of
workload.make_world(5, 40) (1,040 circles), every car without a path.
  (a) one clearance launch, f110qp_clearance_dev, at rows = 1 (x_traj row 0) and at rows = 51 (a whole x_traj),
      G = 16;
  (b) us per tick of f110qp_rollout_contact_dev at stop_on_contact = 0 and 1, G = 1, 4 and 16, and of the
      yardstick f110qp_rollout_race_dev at the same G (casts on each tick's plan list);
  (c) per G: the share of cars crashed by row 50 (margin 0), and the share of the 50 x 4,096 ticks by kind
      without and with parking.
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`. Every call of (b)
starts from the same cars without a path, so each replays the same 50 ticks.

usage: python tools/contact_cost.py [rounds [out.json]]   (default profiles/r13/contact_cost.json)
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
from world_cost import stat, timed  # noqa: E402

B, N, T, BEAMS, P = 4096, 20, 50, 1080, 50
GROUPS = (1, 4, 16)
KINDS = {capi.TICK_MPC: "MPC", capi.TICK_PLAN: "PLAN", capi.TICK_HOLD: "HOLD", capi.TICK_PLAN_FAILED: "PLAN_FAILED",
         capi.TICK_CRASHED: "CRASHED"}


def shares(kinds):
    vals, n = np.unique(kinds, return_counts=True)
    return {KINDS[int(k)]: round(float(c) / kinds.size, 4) for k, c in zip(vals, n)}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r13", "contact_cost.json")
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
    ccs = {stop: capi.default_contact_config(stop_on_contact=stop) for stop in (0, 1)}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, cid = t(capi.traj_table(rp.plan)), t(wp), t(world)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt, kt = z((T, B, 2), torch.float32), z((T, B), torch.int32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    clt, crash = z((T + 1, B), torch.float64), z((B,), torch.int32)

    def race(G):
        have.zero_()  # every call replays the same ticks: no car holds a path
        s.rollout_race_dev(rc, sc, rp, wc, races[G], table, wpd, xr, have, cid, xt, ult, ua, stt)

    def contact(G, stop, kind=None):
        have.zero_()
        s.rollout_contact_dev(rc, sc, rp, wc, races[G], ccs[stop], table, wpd, xr, have, cid, xt, ult, ua, stt, clt, crash,
                              kind_traj=kind)

    crashed, kinds = {}, {}
    for G in GROUPS:
        for stop in (0, 1):
            contact(G, stop, kt)
            torch.cuda.synchronize()
            kinds[f"G{G}_stop{stop}"] = shares(kt.cpu().numpy())
            crashed[f"G{G}_stop{stop}"] = round(float((crash.cpu().numpy() >= 0).mean()), 4)
    race(16)  # x_traj of the G = 16 race rollout: the poses of the rows = 51 launch
    torch.cuda.synchronize()
    variants = {"clearance_rows1_G16": (lambda: capi.clearance_dev(wc, races[16], xt[0], cid, clt[0]), 1),
                "clearance_rows51_G16": (lambda: capi.clearance_dev(wc, races[16], xt, cid, clt), 1)}
    for G in GROUPS:
        variants[f"rollout_race_dev_G{G}"] = (lambda G=G: race(G), T)
        variants[f"rollout_contact_dev_G{G}_stop0"] = (lambda G=G: contact(G, 0), T)
        variants[f"rollout_contact_dev_G{G}_stop1"] = (lambda G=G: contact(G, 1), T)
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
           "unit": "us by HIP events: median, [min, max]; the rollouts per tick, the clearance launches per launch",
           "note": "the rollout times include one have_path memset per call; the rows = 51 launch reads the x_traj of "
                   "the G = 16 race rollout",
           **{k: stat(v) for k, v in ev.items()}, "crashed_share_by_row_50": crashed, "kind_share": kinds}
    s.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
