"""Cost of the closed loop with re-planning, 4,096 cars x N = 20, T = 50 ticks, 1,080 beams (product
library, AUTO back end, gap_mode INACTIVE, no optional array), by HIP events on the stream, one process:
  (a) us per tick of f110qp_rollout_replan_dev against f110qp_rollout_scan_dev on the same cars (with rows
      nobody reads left out, the latter makes f110qp_rollout_dev's launches): the price of the listed-plan
      launch, the state traffic of the plant step and the plans themselves;
  (b) one f110qp_plan_listed_dev launch on an empty list and on a full list of the 4,096 cars;
  (c) the share of the 50 x 4,096 ticks by kind.
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`. Every call of
(a) starts from the same cars without a path, so each replays the same 50 ticks.

usage: python tools/replan_cost.py [rounds [out.json]]   (default profiles/r09/replan_cost.json)
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


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r09", "replan_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    parts = [workload.make_scenes(256, seed=91 + i, beams=BEAMS) for i in range(B // 256)]  # in slices: the ray casts
    sc_ = dict(parts[0], pose=np.concatenate([p["pose"] for p in parts]),
               ranges=np.concatenate([p["ranges"] for p in parts]))
    pose = sc_["pose"]
    x0 = np.ascontiguousarray(np.stack([pose[:, 0], pose[:, 1], 2.0 * np.arctan2(pose[:, 2], pose[:, 3])], 1))
    ul = np.tile([4.5, 0.0], (B, 1))
    wp = sc_["waypoints"]
    s = capi.Solver(capi.default_config(N, x_ref_points=P))
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=sc_["angle_min"], angle_increment=sc_["angle_inc"],
                                  angle_max=sc_["angle_max"])
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, rg = t(capi.traj_table(rp.plan)), t(wp), t(sc_["ranges"].reshape(1, B, BEAMS))
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt, kt = z((T, B, 2), torch.float32), z((T, B), torch.int32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)

    def replan(kind=None):
        have.zero_()  # every call replays the same ticks: no car holds a path
        s.rollout_replan_dev(rc, sc, rp, table, wpd, xr, have, rg, xt, ult, ua, stt, kind_traj=kind)

    # the held-path loop on the paths the cars hold after a re-planning call
    replan(kt)
    torch.cuda.synchronize()
    kinds = kt.cpu().numpy()
    xr_held = xr.clone()
    xr_held[torch.isnan(xr_held)] = 0.0  # a car that never planned: any finite path, the solve costs the same

    def scan():
        s.rollout_scan_dev(rc, sc, xr_held, rg, xt, ult, ua, stt)

    poses = z((B, 4), torch.float64)
    poses.copy_(t(pose))
    lst = t(np.random.default_rng(5).permutation(B).astype(np.int32))
    counts = {"empty": z((1,), torch.int32), "full": t(np.int32([B]))}
    ps, bt, bg = (z((B,), torch.int32) for _ in range(3))
    xr_plan = z((B, P, 3), torch.float64)

    def listed(which):
        return lambda: capi.plan_listed_dev(rp, sc, lst, counts[which], poses, rg[0], table, wpd, xr_plan, ps, bt, bg)

    variants = {"rollout_replan_dev": (replan, T), "rollout_scan_dev": (scan, T),
                "plan_listed_empty": (listed("empty"), 1), "plan_listed_full": (listed("full"), 1)}
    for fn, _ in variants.values():  # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, per) in variants.items():
            ev[k].append(timed(stream, fn) / per)
    vals, n = np.unique(kinds, return_counts=True)
    res = {"B": B, "N": N, "T": T, "beams": BEAMS, "rounds": rounds, "backend_info": list(s.backend_info(B)),
           "unit": "us by HIP events: median, [min, max]; the two rollouts per tick, the listed plan per launch",
           "note": "rollout_replan_dev times include one have_path memset per call",
           **{k: stat(v) for k, v in ev.items()},
           "kind_share": {KIND_NAMES[int(k)]: round(float(c) / kinds.size, 4) for k, c in zip(vals, n)}}
    res["replan_minus_scan_per_tick"] = round(res["rollout_replan_dev"]["median"] - res["rollout_scan_dev"]["median"], 2)
    s.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
