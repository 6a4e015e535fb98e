"""Cost of the raster map's distance field on one MI355X; product library, one process, HIP events on the stream.
Two maps: workload.make_grid_world(5, 40, 0.05), 584 x 344 (a track: walls and discs), and a seeded 4,096 x 4,096 map
with 1 % of its cells occupied.
  (a) f110qp_grid_distance_dev (with nearest) and f110qp_grid_inflate_dev (radius 0.3 m) on both maps;
      f110qp_grid_lookup_dev (with cell) on [201][4,096] poses spread over the small map;
  (b) for scale, f110qp_clearance_grid_dev at reach 1.0 on the 4,096 poses of one row of the same array, the map
      alone (no circles, no segments). Not the same quantity: it is the rectangle's signed distance, exact up to
      reach, where the lookup is the centre-to-centre cell distance, exact everywhere;
  (c) the host alternative, wall clock: the device-to-host copy of the map and the numpy separable transform of
      tests/field_cases.py (the small map alone: it costs H x H x W), and scipy.ndimage.distance_transform_edt on
      both maps where scipy imports (it gives float distances, not d2 and nearest);
  (d) the device results on the small map against the oracle's bits.
The two launches of the transform are not separable through the C ABI; `phases MAP ROUNDS` runs the transform alone
on one map (world or big), for a kernel trace taken from outside to split.
Warm-up first, the variants alternating within a round; medians and [min, max] over `rounds`. No figure is fixed in
advance: they are reported as measured.

usage: python tools/field_cost.py [rounds [out.json]]   (default profiles/field/field_cost.json)
       python tools/field_cost.py phases world|big [rounds]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from f110qp import capi, workload  # noqa: E402
from world_cost import stat, timed  # noqa: E402

ROWS, B = 201, 4096
BIG, DENSITY = 4096, 0.01
RADIUS = 0.3
WALL_ROUNDS = 3


class Field:
    """A map on the device with the transform's arrays."""

    def __init__(self, dev, grid, cfg):
        self.grid, self.cfg, self.gc = grid, cfg, capi.grid_config_of(cfg)
        z = lambda dt: torch.zeros(grid.shape, dtype=dt, device=dev)  # noqa: E731
        self.dgrid = torch.from_numpy(grid).to(dev)
        self.d2, self.near, self.work, self.fat = z(torch.int32), z(torch.int32), z(torch.int32), z(torch.uint8)

    def transform(self):
        capi.grid_distance_dev(self.gc, self.dgrid, self.d2, self.work, self.near)

    def inflate(self):
        capi.grid_inflate_dev(self.gc, self.d2, RADIUS, self.fat)


def maps(dev, which=("world", "big")):
    out = {}
    if "world" in which:
        out["world"] = Field(dev, *workload.make_grid_world(5, 40, 0.05))
    if "big" in which:
        g = (np.random.default_rng(4096).random((BIG, BIG)) < DENSITY).astype(np.uint8)
        out["big"] = Field(dev, g, workload.GridSpec(BIG, BIG, 0.0, 0.0, 0.05, 1.0))
    return out


def phases(which, rounds):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    f = maps(dev, (which,))[which]
    for _ in range(rounds):
        f.transform()
    torch.cuda.synchronize()
    print(json.dumps({"map": which, "shape": list(f.grid.shape), "transforms": rounds}))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "phases":
        return phases(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "field", "field_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    m = maps(dev)
    world = m["world"]
    rng = np.random.default_rng(2025)
    cfg = world.cfg
    x = np.stack([cfg.origin_x + rng.uniform(0.0, cfg.width, (ROWS, B)) * cfg.resolution,
                  cfg.origin_y + rng.uniform(0.0, cfg.height, (ROWS, B)) * cfg.resolution,
                  rng.uniform(-np.pi, np.pi, (ROWS, B))], axis=2)
    dx = torch.from_numpy(x).to(dev)
    dist = torch.zeros((ROWS, B), dtype=torch.float64, device=dev)
    cell = torch.zeros((ROWS, B), dtype=torch.int32, device=dev)
    clear = torch.zeros((1, B), dtype=torch.float64, device=dev)
    cnear = torch.zeros((1, B), dtype=torch.int32, device=dev)
    wc, race = capi.default_world_config(num_circles=0), capi.default_race_config(group_size=1)
    body, walls = capi.default_body_config(), capi.default_walls_config(num_segments=0, wall_rows=1)

    variants = {}
    for name, f in m.items():
        variants[f"transform_{name}"] = f.transform
        variants[f"inflate_{name}"] = f.inflate
    variants["lookup_201x4096"] = lambda: capi.grid_lookup_dev(world.gc, world.d2, dx, dist, world.near, cell)
    variants["clearance_grid_reach1_1x4096"] = lambda: capi.clearance_grid_dev(wc, race, body, walls, world.gc, dx[:1], None,
                                                                             None, world.dgrid, clear, cnear)
    for fn in variants.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ev[k].append(timed(stream, fn))

    import field_cases as fc  # the separable numpy transform and the comparison

    try:
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        distance_transform_edt = None
    wall = {"copy_map_world_ms": [], "copy_map_big_ms": [], "numpy_separable_world_ms": []}
    if distance_transform_edt is not None:
        wall.update({"scipy_edt_world_ms": [], "scipy_edt_big_ms": []})
    same = True
    for _ in range(WALL_ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hw = world.dgrid.cpu().numpy()
        t1 = time.perf_counter()
        hb = m["big"].dgrid.cpu().numpy()
        t2 = time.perf_counter()
        d2, near = fc.separable(hw)
        t3 = time.perf_counter()
        wall["copy_map_world_ms"].append((t1 - t0) * 1e3)
        wall["copy_map_big_ms"].append((t2 - t1) * 1e3)
        wall["numpy_separable_world_ms"].append((t3 - t2) * 1e3)
        if distance_transform_edt is not None:
            t0 = time.perf_counter()
            distance_transform_edt(hw == 0)
            t1 = time.perf_counter()
            distance_transform_edt(hb == 0)
            t2 = time.perf_counter()
            wall["scipy_edt_world_ms"].append((t1 - t0) * 1e3)
            wall["scipy_edt_big_ms"].append((t2 - t1) * 1e3)
        same &= fc.same(world.d2.cpu().numpy(), d2) and fc.same(world.near.cpu().numpy(), near)
        same &= fc.same(world.fat.cpu().numpy(), workload.grid_inflate(d2, cfg, RADIUS))
        wd, wcell = workload.grid_lookup(x, d2, near, cfg)
        same &= fc.same(dist.cpu().numpy(), wd) and fc.same(cell.cpu().numpy(), wcell)

    big_d2 = m["big"].d2.cpu().numpy()
    res = {"world": list(world.grid.shape), "big": [BIG, BIG], "big_density": DENSITY, "rows": ROWS, "B": B,
           "radius": RADIUS, "rounds": rounds, "wall_rounds": WALL_ROUNDS,
           "occupied": {"world": int(world.grid.sum()), "big": int(m["big"].grid.sum())},
           "largest_d2": {"world": int(world.d2.max().item()), "big": int(big_d2.max())},
           "unit": "us by HIP events per call: median, [min, max]; the wall clocks (copies, numpy, scipy) in ms",
           "note": "transform = two launches (rows, columns) with nearest; clearance_grid is one row of 4,096 poses at "
                   "reach 1.0 on the small map, not the lookup's quantity; the copies are pageable device-to-host "
                   "copies through torch's .cpu(); scipy's transform gives float distances only",
           "scipy": distance_transform_edt is not None,
           **{k: stat(v) for k, v in ev.items()}, **{k: stat(v) for k, v in wall.items()},
           "device_equals_numpy_bits_world": bool(same)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
