"""Cost of the closed loop with a simulated LiDAR, 4,096 cars x N = 20, T = 50 ticks, 1,080 beams (product
library, AUTO back end, gap_mode INACTIVE), by HIP events on the stream, one process: workload.make_scenes
poses on the track of workload.make_world(5, 40) (1,040 circles), every car without a path.
  (a) us per tick of f110qp_rollout_world_dev with the casts on each tick's plan list (no ranges_traj), of
      the same with ranges_traj (every car cast every tick), and of the yardstick, f110qp_rollout_replan_dev
      at scan_rows = 1 on the scans of the same world cast at the start poses: the difference is the price
      of the scan;
  (b) one f110qp_cast_scans_dev launch for all 4,096 cars and one on an empty list;
  (c) the share of the 50 x 4,096 ticks by kind, for the world call and for the yardstick (scans held).
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`. Every call of
(a) starts from the same cars without a path, so each replays the same 50 ticks.

usage: python tools/world_cost.py [rounds [out.json]]   (default profiles/r10/world_cost.json)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
from f110qp import capi, workload  # noqa: E402

B, N, T, BEAMS, P = 4096, 20, 50, 1080, 50
KIND_NAMES = {capi.TICK_MPC: "MPC", capi.TICK_PLAN: "PLAN", capi.TICK_HOLD: "HOLD", capi.TICK_PLAN_FAILED: "PLAN_FAILED"}


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def stat(v):
    return {"median": round(float(np.median(v)), 2), "min_max": [round(min(v), 2), round(max(v), 2)]}


def shares(kinds):
    vals, n = np.unique(kinds, return_counts=True)
    return {KIND_NAMES[int(k)]: round(float(c) / kinds.size, 4) for k, c in zip(vals, n)}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r10", "world_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    pose = np.concatenate([workload.make_scenes(256, seed=91 + i, beams=8, obstacles=0)["pose"] for i in range(B // 256)])
    x0 = np.ascontiguousarray(np.stack([pose[:, 0], pose[:, 1], 2.0 * np.arctan2(pose[:, 2], pose[:, 3])], 1))
    ul = np.tile([4.5, 0.0], (B, 1))
    wp = workload.track_waypoints()
    world = workload.make_world(5, 40)
    amin, ainc, amax = workload.scan_geometry(BEAMS)
    s = capi.Solver(capi.default_config(N, x_ref_points=P))
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=amin, angle_increment=ainc, angle_max=amax)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    wc = capi.default_world_config(num_circles=world.shape[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, cid = t(capi.traj_table(rp.plan)), t(wp), t(world)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt, kt = z((T, B, 2), torch.float32), z((T, B), torch.int32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    rgt = z((T, B, BEAMS), torch.float32)
    rg0 = z((1, B, BEAMS), torch.float32)
    capi.cast_scans_dev(sc, wc, xt[0], cid, rg0[0])  # the yardstick's held scans: this world at the start poses

    def world_call(kind=None, scans=None):
        have.zero_()  # every call replays the same ticks: no car holds a path
        s.rollout_world_dev(rc, sc, rp, wc, table, wpd, xr, have, cid, xt, ult, ua, stt, kind_traj=kind,
                            ranges_traj=scans)

    def replan(kind=None):
        have.zero_()
        s.rollout_replan_dev(rc, sc, rp, table, wpd, xr, have, rg0, xt, ult, ua, stt, kind_traj=kind)

    world_call(kt)
    torch.cuda.synchronize()
    kinds_world = kt.cpu().numpy()
    replan(kt)
    torch.cuda.synchronize()
    kinds_held = kt.cpu().numpy()

    lst = t(np.random.default_rng(5).permutation(B).astype(np.int32))
    empty = z((1,), torch.int32)
    one = z((B, BEAMS), torch.float32)
    variants = {"rollout_world_dev_listed": (lambda: world_call(), T),
                "rollout_world_dev_ranges_traj": (lambda: world_call(scans=rgt), T),
                "rollout_replan_dev": (lambda: replan(), T),
                "cast_all_cars": (lambda: capi.cast_scans_dev(sc, wc, xt[0], cid, one), 1),
                "cast_empty_list": (lambda: capi.cast_scans_dev(sc, wc, xt[0], cid, one, list_=lst, count=empty), 1)}
    for fn, _ in variants.values():  # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, per) in variants.items():
            ev[k].append(timed(stream, fn) / per)
    res = {"B": B, "N": N, "T": T, "beams": BEAMS, "circles": int(world.shape[0]), "rounds": rounds,
           "backend_info": list(s.backend_info(B)),
           "unit": "us by HIP events: median, [min, max]; the rollouts per tick, the casts per launch",
           "note": "the rollout times include one have_path memset per call",
           **{k: stat(v) for k, v in ev.items()},
           "kind_share_world": shares(kinds_world), "kind_share_scans_held": shares(kinds_held)}
    base = res["rollout_replan_dev"]["median"]
    res["scan_price_per_tick_listed"] = round(res["rollout_world_dev_listed"]["median"] - base, 2)
    res["scan_price_per_tick_ranges_traj"] = round(res["rollout_world_dev_ranges_traj"]["median"] - base, 2)
    s.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
