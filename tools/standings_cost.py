"""Cost of the race standings, and the standings of the documented contact runs: 4,096 cars, T = 50 ticks
(rows = 51), workload.track_waypoints() (W = 500), the cars on workload.make_race_grid(256, 16, seed=91) in the
track world of workload.make_world(5, 40); product library, one process, HIP events on the stream.
  (a) f110qp_progress_dev and f110qp_standings_dev (G = 16) alone, at rows = 1 (x_traj row 0) and rows = 51 (the
      x_traj of the G = 16 contact rollout, stop_on_contact = 0), and the yardstick f110qp_clearance_dev (G = 16,
      1,040 circles) at the same rows in the same rounds;
  (b) wall clock of the synchronous f110qp_race_standings on host arrays against numpy's workload.progress +
      workload.standings on the same arrays (rows = 51; `wall_rounds` rounds);
  (c) per G in (4, 16) and stop_on_contact in (0, 1): the share of cars whose rank at row 50 differs from their
      rank at row 0 (the grid order), the mean dist gained over the 50 ticks by crashed and by uncrashed cars, and
      the laps.
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`.

usage: python tools/standings_cost.py [rounds [out.json]]   (default profiles/r14/standings_cost.json)
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from f110qp import capi, workload  # noqa: E402
from world_cost import stat, timed  # noqa: E402

B, N, T, BEAMS, P = 4096, 20, 50, 1080, 50
WALL_ROUNDS = 3


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r14", "standings_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    x0 = workload.make_race_grid(B // 16, 16, seed=91)
    ul = np.tile([4.5, 0.0], (B, 1))
    wp = workload.track_waypoints()
    cum = capi.path_lengths(wp)
    L = float(cum[-1])
    world = workload.make_world(5, 40)
    amin, ainc, amax = workload.scan_geometry(BEAMS)
    s = capi.Solver(capi.default_config(N, x_ref_points=P))
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=amin, angle_increment=ainc, angle_max=amax)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    wc = capi.default_world_config(num_circles=world.shape[0])
    races = {G: capi.default_race_config(group_size=G) for G in (4, 16)}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table, wpd, cumd, cid = t(capi.traj_table(rp.plan)), t(wp), t(cum), t(world)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    xt[0], ult[0] = t(x0), t(ul)
    ua, stt = z((T, B, 2), torch.float32), z((T, B), torch.int32)
    xr, have = z((B, P, 3), torch.float64), z((B,), torch.int32)
    clt, crash = z((T + 1, B), torch.float64), z((B,), torch.int32)
    seg, lap, rank = (z((T + 1, B), torch.int32) for _ in range(3))
    sv, lat, dist = (z((T + 1, B), torch.float64) for _ in range(3))

    # (c) the standings of the contact runs; the last run (G = 16, stop 0) leaves the x_traj that (a) reads
    runs = {}
    for G, stop in ((4, 0), (4, 1), (16, 1), (16, 0)):
        have.zero_()
        s.rollout_contact_dev(rc, sc, rp, wc, races[G], capi.default_contact_config(stop_on_contact=stop), table, wpd,
                              xr, have, cid, xt, ult, ua, stt, clt, crash)
        capi.progress_dev(xt, wpd, cumd, sv, seg, lat)
        capi.standings_dev(races[G], sv, L, dist, rank, lap)
        torch.cuda.synchronize()
        d, r, lp, hit = dist.cpu().numpy(), rank.cpu().numpy(), lap.cpu().numpy(), crash.cpu().numpy() >= 0
        assert (r[0] == np.arange(B) % G).all(), "row 0 ranks in grid order"
        gain = d[T] - d[0]
        mean = lambda v: round(float(v.mean()), 3) if v.size else None  # noqa: E731
        runs[f"G{G}_stop{stop}"] = {
            "crashed_share": round(float(hit.mean()), 4),
            "final_rank_differs_from_grid_share": round(float((r[T] != r[0]).mean()), 4),
            "mean_dist_gained_m_crashed": mean(gain[hit]), "mean_dist_gained_m_uncrashed": mean(gain[~hit]),
            "min_max_dist_gained_m": [round(float(gain.min()), 3), round(float(gain.max()), 3)],
            "laps_at_row_50": sorted(int(v) for v in np.unique(lp[T])),
            "max_abs_lateral_m": round(float(np.abs(lat.cpu().numpy()).max()), 3)}
    x_host = xt.cpu().numpy()

    variants = {"progress_rows1": lambda: capi.progress_dev(xt[0], wpd, cumd, sv[0], seg[0], lat[0]),
                "progress_rows51": lambda: capi.progress_dev(xt, wpd, cumd, sv, seg, lat),
                "standings_rows1_G16": lambda: capi.standings_dev(races[16], sv[0], L, dist[0], rank[0], lap[0]),
                "standings_rows51_G16": lambda: capi.standings_dev(races[16], sv, L, dist, rank, lap),
                "clearance_rows1_G16": lambda: capi.clearance_dev(wc, races[16], xt[0], cid, clt[0]),
                "clearance_rows51_G16": lambda: capi.clearance_dev(wc, races[16], xt, cid, clt)}
    for fn in variants.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ev[k].append(timed(stream, fn))

    wall = {"race_standings_host_ms": [], "numpy_oracle_ms": []}
    for _ in range(WALL_ROUNDS):
        t0 = time.perf_counter()
        got = capi.race_standings(races[16], x_host, wp)
        t1 = time.perf_counter()
        _, so, _ = workload.progress(x_host, wp)
        want = workload.standings(so, L, 16)
        t2 = time.perf_counter()
        wall["race_standings_host_ms"].append((t1 - t0) * 1e3)
        wall["numpy_oracle_ms"].append((t2 - t1) * 1e3)
    same = bool((got["rank"] == want[2]).all() and (got["dist"].view(np.int64) == want[0].view(np.int64)).all())

    res = {"B": B, "T": T, "rows": T + 1, "W": int(wp.shape[0]), "circles": int(world.shape[0]), "rounds": rounds,
           "wall_rounds": WALL_ROUNDS, "start": "make_race_grid(256, 16, seed=91)", "path_length_m": L,
           "unit": "us by HIP events per call: median, [min, max]; the wall clocks in ms",
           "note": "rows = 51 is the x_traj of the G = 16 contact rollout at stop_on_contact = 0; standings_dev is two "
                   "launches; the yardstick clearance_dev is timed in the same rounds",
           **{k: stat(v) for k, v in ev.items()}, **{k: stat(v) for k, v in wall.items()},
           "host_call_equals_numpy_bits": same, "contact_runs": runs}
    s.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
