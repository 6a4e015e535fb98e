"""Cost of the raster map, the set-up of tools/noise_cost.py: 4,096 cars, G = 16, 1,080 beams, the cars on
workload.make_race_grid(256, 16, seed=91), by HIP events on the stream, one process:
  (a) one all-cars launch of f110qp_cast_scans_walls_dev and of f110qp_cast_scans_noisy_dev on
      workload.make_wall_world(5, 40) (250 segments + 40 circles) next to one of f110qp_cast_scans_grid_dev on
      workload.make_grid_world(5, 40, 0.05), the same track rasterised, with no segment and no circle beside the
      map: at max_range 10 m (the LDS square of 405 cells) and at 10.5 m (a square of 425 cells, which does not
      fit: the map is read from global memory); the two walk the same cells up to 10 m;
  (b) one launch of f110qp_clearance_walls_dev on the segments next to one of f110qp_clearance_grid_dev on the map
      (reach 1.0);
  (c) us per tick of f110qp_rollout_noisy_dev on the segments next to f110qp_rollout_grid_dev on the map, N = 20,
      T = 50, every = 1, stop 0, gap rows ACTIVE; the two drive in different worlds (a raster wall stands up to a
      cell nearer), so (c) is the tick a user pays.
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`.

usage: python tools/grid_cost.py [rounds [out.json]]   (default profiles/grid/grid_cost.json)
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
RES, FAR = 0.05, 10.5


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "grid", "grid_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    x0 = workload.make_race_grid(B // G, G, seed=91)
    ul = np.tile([4.5, 0.0], (B, 1))
    wp = workload.track_waypoints()
    segs, obst = workload.make_wall_world(5, 40)
    grid, spec = workload.make_grid_world(5, 40, RES)
    amin, ainc, amax = workload.scan_geometry(BEAMS)
    solver = capi.Solver(capi.default_config(N, x_ref_points=P, gap_mode=capi.GAP_ACTIVE))
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=amin, angle_increment=ainc, angle_max=amax)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    wc, wc0 = capi.default_world_config(num_circles=obst.shape[0]), capi.default_world_config()
    wc_far = capi.default_world_config(max_range=FAR)
    wl, wl0 = capi.default_walls_config(num_segments=segs.shape[0]), capi.default_walls_config()
    body, race, cc = capi.default_body_config(), capi.default_race_config(group_size=G), capi.default_contact_config()
    rf = capi.default_refresh_config(every=1)
    gc = capi.grid_config_of(spec)
    loud = capi.default_noise_config(seed=SEED, sigma_abs=SIGMA_ABS, dropout=DROPOUT)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, obd, sgd, gd = t(capi.traj_table(rp.plan)), t(wp), t(obst), t(segs), t(grid)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt = z((T, B, 2), torch.float32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    clt, crash = z((T + 1, B), torch.float64), z((B,), torch.int32)
    hst = z((T, B, 2, 3), torch.float32)
    rg, rgg, rgf = (z((B, BEAMS), torch.float32) for _ in range(3))
    cl = z((B,), torch.float64)

    def rollout(on_map):
        have.zero_()  # every call replays the same ticks: no car holds a path
        if on_map:
            solver.rollout_grid_dev(rc, sc, rp, wc0, race, cc, body, wl0, rf, loud, gc, table, wpd, xr, have, None, None,
                                    gd, xt, ult, ua, stt, clt, crash, hs_traj=hst)
        else:
            solver.rollout_noisy_dev(rc, sc, rp, wc, race, cc, body, wl, rf, loud, table, wpd, xr, have, obd, sgd, xt, ult,
                                     ua, stt, clt, crash, hs_traj=hst)

    x = xt[0]
    variants = {
        "cast_walls_G16": (lambda: capi.cast_scans_walls_dev(sc, wc, race, body, wl, x, obd, sgd, rg), 1),
        "cast_noisy_G16": (lambda: capi.cast_scans_noisy_dev(sc, wc, race, body, wl, loud, 0, x, obd, sgd, rg), 1),
        "cast_grid_lds_G16": (lambda: capi.cast_scans_grid_dev(sc, wc0, race, body, wl0, loud, gc, 0, x, None, None, gd,
                                                              rgg), 1),
        "cast_grid_global_G16_max_range_10p5": (lambda: capi.cast_scans_grid_dev(sc, wc_far, race, body, wl0, loud, gc, 0,
                                                                                 x, None, None, gd, rgf), 1),
        "clearance_walls_G16": (lambda: capi.clearance_walls_dev(wc, race, body, wl, x, obd, sgd, cl), 1),
        "clearance_grid_G16": (lambda: capi.clearance_grid_dev(wc0, race, body, wl0, gc, x, None, None, gd, cl), 1),
        "rollout_noisy_dev_G16_active_every1": (lambda: rollout(False), T),
        "rollout_grid_dev_G16_active_every1": (lambda: rollout(True), T),
    }
    for fn, _ in variants.values():  # warm-up: code objects, workspaces
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, per) in variants.items():
            xt[0] = t(x0)
            ev[k].append(timed(stream, fn) / per)
    xt[0] = t(x0)
    variants["cast_grid_lds_G16"][0]()
    variants["cast_grid_global_G16_max_range_10p5"][0]()
    torch.cuda.synchronize()
    a, b = rgg.cpu().numpy(), rgf.cpu().numpy()
    hit = a < np.float32(10.0)
    res = {"B": B, "N": N, "T": T, "G": G, "beams": BEAMS, "segments": int(segs.shape[0]), "circles": int(obst.shape[0]),
           "map": {"width": spec.width, "height": spec.height, "resolution": spec.resolution,
                   "occupied_cells": int(grid.sum())},
           "rounds": rounds, "start": "make_race_grid(256, 16, seed=91)",
           "noise": {"seed": SEED, "sigma_abs": SIGMA_ABS, "sigma_rel": 0.0, "dropout": DROPOUT},
           "unit": "us by HIP events: median, [min, max]; the rollouts per tick, the single launches per launch",
           "note": "the rollout times include one have_path memset per call",
           **{k: stat(v) for k, v in ev.items()},
           "effect": {"beams_with_a_return_below_10m": round(float(hit.mean()), 4),
                      "lds_and_global_returns_bit_equal": bool((a[hit].view(np.uint32) == b[hit].view(np.uint32)).all())}}
    solver.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
