"""Cost of the raster LiDAR through the distance field, the set-up of tools/grid_cost.py: 4,096 cars, G = 16, 1,080
beams, the cars on workload.make_race_grid(256, 16, seed=91), the map workload.make_grid_world(5, 40, 0.05) with no
segment and no circle beside it, by HIP events on the stream, one process, the product library:
  (a) one all-cars launch of f110qp_cast_scans_grid_dev (rule G1, the cell walk) next to one of f110qp_grid_cast_dev
      (rule F1, the jumps), with and without the visits array;
  (b) f110qp_grid_distance_dev, the once-per-map cost of the field;
  (c) us per tick of f110qp_rollout_grid_dev next to f110qp_rollout_field_dev, N = 20, T = 50, every = 1, stop 0, gap
      rows ACTIVE: the same world, the same bits;
  (d) the mean of visits a beam, and whether the two casts' ranges are bit equal.
Warm-up first, the variants alternating within a round; medians and [min, max] over `rounds`.

usage: python tools/field_cast_cost.py [rounds [out.json]]   (default profiles/field_cast/field_cast_cost.json)
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
from grid_cost import DROPOUT, G, RES, SEED, SIGMA_ABS  # noqa: E402
from world_cost import stat, timed  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "field_cast", "field_cast_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    x0 = workload.make_race_grid(B // G, G, seed=91)
    ul = np.tile([4.5, 0.0], (B, 1))
    wp = workload.track_waypoints()
    grid, spec = workload.make_grid_world(5, 40, RES)
    amin, ainc, amax = workload.scan_geometry(BEAMS)
    solver = capi.Solver(capi.default_config(N, x_ref_points=P, gap_mode=capi.GAP_ACTIVE))
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=amin, angle_increment=ainc, angle_max=amax)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    wc0, wl0 = capi.default_world_config(), capi.default_walls_config()
    body, race, cc = capi.default_body_config(), capi.default_race_config(group_size=G), capi.default_contact_config()
    rf = capi.default_refresh_config(every=1)
    gc = capi.grid_config_of(spec)
    loud = capi.default_noise_config(seed=SEED, sigma_abs=SIGMA_ABS, dropout=DROPOUT)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, gd = t(capi.traj_table(rp.plan)), t(wp), t(grid)
    d2, work = z(grid.shape, torch.int32), z(grid.shape, torch.int32)
    capi.grid_distance_dev(gc, gd, d2, work)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt = z((T, B, 2), torch.float32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    clt, crash = z((T + 1, B), torch.float64), z((B,), torch.int32)
    hst = z((T, B, 2, 3), torch.float32)
    rgw, rgf = (z((B, BEAMS), torch.float32) for _ in range(2))
    vis = z((B, BEAMS), torch.int32)

    def rollout(field):
        have.zero_()  # every call replays the same ticks: no car holds a path
        if field:
            solver.rollout_field_dev(rc, sc, rp, wc0, race, cc, body, wl0, rf, loud, gc, table, wpd, xr, have, None, None,
                                     gd, d2, xt, ult, ua, stt, clt, crash, hs_traj=hst)
        else:
            solver.rollout_grid_dev(rc, sc, rp, wc0, race, cc, body, wl0, rf, loud, gc, table, wpd, xr, have, None, None,
                                    gd, xt, ult, ua, stt, clt, crash, hs_traj=hst)

    x = xt[0]
    variants = {
        "cast_scans_grid_dev_G16": (lambda: capi.cast_scans_grid_dev(sc, wc0, race, body, wl0, loud, gc, 0, x, None, None,
                                                                     gd, rgw), 1),
        "grid_cast_dev_G16": (lambda: capi.grid_cast_dev(sc, wc0, race, body, wl0, loud, gc, 0, x, None, None, gd, d2,
                                                         rgf), 1),
        "grid_cast_dev_G16_with_visits": (lambda: capi.grid_cast_dev(sc, wc0, race, body, wl0, loud, gc, 0, x, None, None,
                                                                     gd, d2, rgf, vis), 1),
        "grid_distance_dev": (lambda: capi.grid_distance_dev(gc, gd, d2, work), 1),
        "rollout_grid_dev_G16_active_every1": (lambda: rollout(False), T),
        "rollout_field_dev_G16_active_every1": (lambda: rollout(True), T),
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
    variants["cast_scans_grid_dev_G16"][0]()
    variants["grid_cast_dev_G16_with_visits"][0]()
    torch.cuda.synchronize()
    a, b, v = rgw.cpu().numpy(), rgf.cpu().numpy(), vis.cpu().numpy()
    res = {"B": B, "N": N, "T": T, "G": G, "beams": BEAMS,
           "map": {"width": spec.width, "height": spec.height, "resolution": spec.resolution,
                   "occupied_cells": int(grid.sum())},
           "rounds": rounds, "start": "make_race_grid(256, 16, seed=91)",
           "noise": {"seed": SEED, "sigma_abs": SIGMA_ABS, "sigma_rel": 0.0, "dropout": DROPOUT},
           "unit": "us by HIP events: median, [min, max]; the rollouts per tick, the single launches per launch",
           "note": "the rollout times include one have_path memset per call",
           **{k: stat(v_) for k, v_ in ev.items()},
           "effect": {"mean_visits_a_beam": round(float(v.mean()), 3), "max_visits_a_beam": int(v.max()),
                      "beams_with_a_return_below_10m": round(float((a < np.float32(10.0)).mean()), 4),
                      "walk_and_field_ranges_bit_equal": bool((a.view(np.uint32) == b.view(np.uint32)).all())}}
    solver.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
