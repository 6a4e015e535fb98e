"""Cost of the noisy LiDAR's epilogue, the set-up of tools/walls_cost.py: 4,096 cars, G = 16, 1,080 beams,
workload.make_wall_world(5, 40) (250 segments + 40 circles), the cars on workload.make_race_grid(256, 16, seed=91),
by HIP events on the stream, one process:
  (a) one all-cars launch of f110qp_cast_scans_walls_dev (`cast_walls_G16`, the launch of tools/walls_cost.py) next
      to one of f110qp_cast_scans_noisy_dev at sigma_abs 0.01, dropout 0.01, and at the all-zero config;
  (b) us per tick of f110qp_rollout_refresh_dev next to f110qp_rollout_noisy_dev with that noise, N = 20, T = 50,
      every = 1, stop 0, gap rows ACTIVE and INACTIVE (hs_traj given, so the rows are computed); the noisy call drives
      other ticks than the quiet one (its planner and its gap rows read other scans), so (b) is the tick a user pays,
      not the epilogue alone;
  (c) the share of beams the noisy cast changed and dropped at row 0.
A library without the noisy family (the parent of this tool) gives the quiet rows alone, so the same file times
`cast_walls_G16` on both sides of the change. Warm-up first, the routes alternating within a round; medians and
[min, max] over `rounds`.

usage: python tools/noise_cost.py [rounds [out.json]]   (default profiles/noise/noise_cost.json)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contact_cost import BEAMS, B, N, P, T  # noqa: E402
from f110qp import capi, workload  # noqa: E402
from world_cost import stat, timed  # noqa: E402

G = 16
SIGMA_ABS, DROPOUT, SEED = 0.01, 0.01, 7


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "noise", "noise_cost.json")
    noisy = hasattr(capi, "cast_scans_noisy_dev")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    x0 = workload.make_race_grid(B // G, G, seed=91)
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
    body, race, cc = capi.default_body_config(), capi.default_race_config(group_size=G), capi.default_contact_config()
    rf = capi.default_refresh_config(every=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, obd, sgd = t(capi.traj_table(rp.plan)), t(wp), t(obst), t(segs)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt = z((T, B, 2), torch.float32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    clt, crash = z((T + 1, B), torch.float64), z((B,), torch.int32)
    hst = z((T, B, 2, 3), torch.float32)
    rg, rgn = z((B, BEAMS), torch.float32), z((B, BEAMS), torch.float32)
    if noisy:
        loud = capi.default_noise_config(seed=SEED, sigma_abs=SIGMA_ABS, dropout=DROPOUT)
        quiet = capi.default_noise_config()

    def rollout(gap, noise):
        have.zero_()  # every call replays the same ticks: no car holds a path
        s = solvers[gap]
        if noise is None:
            s.rollout_refresh_dev(rc, sc, rp, wc, race, cc, body, wl, rf, table, wpd, xr, have, obd, sgd, xt, ult, ua, stt,
                                  clt, crash, hs_traj=hst)
        else:
            s.rollout_noisy_dev(rc, sc, rp, wc, race, cc, body, wl, rf, noise, table, wpd, xr, have, obd, sgd, xt, ult, ua,
                                stt, clt, crash, hs_traj=hst)

    variants = {"cast_walls_G16": (lambda: capi.cast_scans_walls_dev(sc, wc, race, body, wl, xt[0], obd, sgd, rg), 1)}
    if noisy:
        variants["cast_noisy_G16"] = (lambda: capi.cast_scans_noisy_dev(sc, wc, race, body, wl, loud, 0, xt[0], obd, sgd,
                                                                         rgn), 1)
        variants["cast_noisy_zero_config_G16"] = (lambda: capi.cast_scans_noisy_dev(sc, wc, race, body, wl, quiet, 0, xt[0],
                                                                                     obd, sgd, rgn), 1)
    for gap in (False, True):
        name = "active" if gap else "inactive"
        variants[f"rollout_refresh_dev_G16_{name}_every1"] = (lambda gap=gap: rollout(gap, None), T)
        if noisy:
            variants[f"rollout_noisy_dev_G16_{name}_every1"] = (lambda gap=gap: rollout(gap, loud), T)
    for fn, _ in variants.values():  # warm-up: code objects, workspaces
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, per) in variants.items():
            ev[k].append(timed(stream, fn) / per)
    effect = {}
    if noisy:
        xt[0] = t(x0)
        variants["cast_walls_G16"][0]()
        variants["cast_noisy_G16"][0]()
        torch.cuda.synchronize()
        a, b = rg.cpu().numpy(), rgn.cpu().numpy()
        hit = a != np.float32(wc.max_range)
        effect = {"beams_with_a_return": round(float(hit.mean()), 4),
                  "changed_share_of_returns": round(float((a != b)[hit].mean()), 4),
                  "dropped_share_of_returns": round(float((b[hit] == np.float32(wc.max_range)).mean()), 4),
                  "max_abs_change_m_of_kept_returns": round(float(np.abs(b - a)[hit & (b != np.float32(wc.max_range))].max()), 5)}
    res = {"B": B, "N": N, "T": T, "G": G, "beams": BEAMS, "segments": int(segs.shape[0]), "circles": int(obst.shape[0]),
           "rounds": rounds, "start": "make_race_grid(256, 16, seed=91)", "noisy_family": noisy,
           "noise": {"seed": SEED, "sigma_abs": SIGMA_ABS, "sigma_rel": 0.0, "dropout": DROPOUT},
           "backend_info": list(solvers[False].backend_info(B)),
           "unit": "us by HIP events: median, [min, max]; the rollouts per tick, the single launches per launch",
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
