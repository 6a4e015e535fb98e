"""The raster LiDAR through the distance field on MI355X (f110qp_grid_cast_dev, f110qp_rollout_field[_dev];
include/f110qp.h rule F1). On every case of field_cast_cases.py, with d2 from f110qp_grid_distance_dev on the device:
ranges equal f110qp_cast_scans_grid_dev's on the same arguments bit for bit and the oracle's (workload.ray_field as
float32), and with the map alone visits equal the oracle's exactly. With circles, segments, race-mates, a list, noise
and a batch past the grid cap the ranges are still the grid cast's bits and no beam reads more cells than with the map
alone. One rollout of 8 cars: every array of f110qp_rollout_field_dev and of f110qp_rollout_field equals
f110qp_rollout_grid_dev's.

The oracle's beams come from numpy's sincos, which differs from the device's in the last place on some beams; that
moves a range by some 1e-15 m against float32's 1e-7 and a visit count only for a beam within that of a lattice
corner, which the cases given to the device do not hold (the exact ties are the CPU test's raw beams)."""
import field_cast_cases as fcc
import grid_cases as gc_
import noise_cases as nz
import numpy as np
import pytest
import world_cases as wc_
from test_gpu_grid import QUIET, SEED, grid_cast
from test_gpu_grid import _world as world_of
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_replan import P, dev, full, replan_buffers
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_walls import scene as walls_scene
from test_gpu_walls import walls_of
from test_gpu_world_scan import SENTINEL
from world_loop import GEOM, OPTIONAL, R, rollout_dev

from f110qp import workload

pytestmark = pytest.mark.gpu

CASES = fcc.cases()


def device_field(capi, cuda, grid, cfg):
    """d2 of the map from f110qp_grid_distance_dev, left on the device (None for an empty map)."""
    import torch

    if not grid.size:
        return None
    H, W = grid.shape
    d2 = torch.full((H, W), -7, dtype=torch.int32, device=cuda)
    work = torch.empty((H, W), dtype=torch.int32, device=cuda)
    capi.grid_distance_dev(capi.grid_config_of(cfg), dev(cuda, grid), d2, work)
    return d2


def field_cast(capi, cuda, x, grid, cfg, geom, beams, static=None, segments=None, G=1, setting=QUIET, tick=0, base=0,
               max_range=gc_.MAX_RANGE, listed=None, count=None, visits=True):
    """f110qp_grid_cast_dev on host arrays, test_gpu_grid.grid_cast's arguments -> (ranges [B, R], visits [B, R] or
    None), rows pre-filled with the sentinel and -7."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    nb = x.shape[0]
    C, w, race = world_of(capi, static, x, G, max_range)
    wl = walls_of(capi, segments, nb)
    out = torch.full((nb, beams), float(SENTINEL), dtype=torch.float32, device=cuda)
    vis = torch.full((nb, beams), -7, dtype=torch.int32, device=cuda) if visits else None
    capi.grid_cast_dev(scan_config(capi, beams, geom), w, race, capi.default_body_config(), wl,
                       nz.noise_config(capi, SEED, base, setting), capi.grid_config_of(cfg), tick, dev(cuda, x),
                       dev(cuda, static) if C else None, dev(cuda, segments) if wl.num_segments else None,
                       dev(cuda, grid) if grid.size else None, device_field(capi, cuda, grid, cfg), out, vis,
                       list_=None if listed is None else dev(cuda, np.asarray(listed, np.int32)),
                       count=None if listed is None else dev(cuda, np.int32([count])))
    torch.cuda.synchronize(cuda)
    return out.cpu().numpy(), vis.cpu().numpy() if visits else None


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_cases(capi, cuda, c):
    got, vis = field_cast(capi, cuda, c.x, c.grid, c.cfg, c.geom, c.beams, max_range=c.max_range)
    walk = grid_cast(capi, cuda, c.x, c.grid, c.cfg, c.geom, c.beams, max_range=c.max_range)
    same_bits(got, walk, f"{c.name}: f110qp_cast_scans_grid_dev")
    want, count = workload.ray_field(*fcc.case_beams(c), fcc.field_of(c.grid), c.cfg, c.max_range)
    same_bits(got, want.astype(np.float32), f"{c.name}: workload.ray_field")
    assert (vis == count).all(), (c.name, np.argwhere(vis != count)[:5])
    if c.name == "1x32768":
        assert got[0, 0] == np.float32((32767 - 0.5) * fcc.QUARTER) and vis[0, 0] == 3


def scene():
    """test_gpu_grid's scene as races of four: a 64 x 48 room, circles, segments and mates nearer and farther than
    the raster walls."""
    grid, cfg = gc_.room(64, 48, 0.1, (-3.2, -2.4), seed=4, blocks=5)
    x = np.array([[-0.6, -0.2, 0.1], [0.5, 0.1, 2.9], [-0.3, 0.6, -1.2], [0.4, -0.7, 1.7]])
    circles = np.array([[1.2, 0.9, 0.2], [-1.5, -0.8, 0.15], [5.0, 1.0, 0.5], [-4.5, -3.0, 0.8], [0.0, 1.6, 0.1]])
    sg = np.array([[-1.0, 1.2, 0.2, 1.4], [1.5, -1.5, 1.6, 0.5], [-6.0, -4.0, 6.0, -4.0], [3.5, -1.0, 3.5, 1.0]])
    return x, grid, cfg, circles, sg


def test_other_obstacles_a_list_and_noise(capi, cuda):
    x, grid, cfg, circles, sg = scene()
    beams, geom = 1080, wc_.geometry(1080)
    _, alone = field_cast(capi, cuda, x, grid, cfg, geom, beams)
    assert (alone >= 2).all(), "a closed room from free cells: every beam reads the start cell and a landing"
    kw = dict(static=circles, segments=sg, G=4)
    for tick, base, setting in ((0, 0, QUIET), (5, 1000, nz.SETTINGS[2])):
        got, vis = field_cast(capi, cuda, x, grid, cfg, geom, beams, setting=setting, tick=tick, base=base, **kw)
        same_bits(got, grid_cast(capi, cuda, x, grid, cfg, geom, beams, setting=setting, tick=tick, base=base, **kw),
                  f"circles, segments, mates, tick {tick}")
        assert (vis <= alone).all() and (vis >= 1).all() and (vis < alone).any(), "a nearer obstacle ends the jumps"
    # a list and its count: the cars not listed keep their rows, of ranges and of visits
    got, vis = field_cast(capi, cuda, x, grid, cfg, geom, beams, listed=[2, 0, 3, 1], count=2, **kw)
    same_bits(got, grid_cast(capi, cuda, x, grid, cfg, geom, beams, listed=[2, 0, 3, 1], count=2, **kw), "listed")
    assert (got[[1, 3]] == SENTINEL).all() and (vis[[1, 3]] == -7).all() and (vis[[0, 2]] >= 1).all()
    # visits may be NULL
    got, none = field_cast(capi, cuda, x, grid, cfg, geom, beams, visits=False, **kw)
    assert none is None
    same_bits(got, grid_cast(capi, cuda, x, grid, cfg, geom, beams, **kw), "visits NULL")


def test_a_batch_past_the_grid_cap(capi, cuda):
    """520 cars with 33 beams: past the cap of 512 workgroups. 3 cars with 1,200 beams: two beam tiles."""
    grid, cfg = gc_.room(64, 48, 0.1, (-3.0, -2.0), seed=8, blocks=12)
    for nb, beams, seed in ((520, 33, 6), (3, 1200, 7)):
        x = gc_.free_poses(grid, cfg, nb, seed)
        geom = wc_.geometry(beams)
        got, vis = field_cast(capi, cuda, x, grid, cfg, geom, beams)
        same_bits(got, grid_cast(capi, cuda, x, grid, cfg, geom, beams), f"{nb} cars, {beams} beams")
        want, count = workload.ray_field(*gc_.beams_of(x, geom, beams), fcc.field_of(grid), cfg, gc_.MAX_RANGE)
        same_bits(got, want.astype(np.float32), f"{nb} cars: workload.ray_field")
        assert (vis == count).all()


def test_empty_map_is_the_noisy_cast_and_reads_nothing(capi, cuda):
    x, _, cfg, circles, sg = scene()
    geom = wc_.geometry(1080)
    empty, ecfg = gc_.spec(np.zeros((0, 0), np.uint8), (cfg.origin_x, cfg.origin_y), cfg.resolution)
    kw = dict(static=circles, segments=sg, G=4, setting=nz.SETTINGS[2], tick=3)
    got, vis = field_cast(capi, cuda, x, empty, ecfg, geom, 1080, **kw)
    same_bits(got, grid_cast(capi, cuda, x, empty, ecfg, geom, 1080, **kw), "W * H == 0")
    assert (vis == 0).all()


T, B, G, N = 6, 8, 4, 5
NOISE = (0.01, 0.005, 0.02)
KEYS = ("x_traj", "u_lin_traj", "u_applied", "status", "hs_traj", "kind", "clear_traj", "nearest_traj", "crash_tick",
        "ranges_traj")


def rollout_scene():
    """The walls rollout's eight cars as two races of four on make_grid_world at 0.1 m cropped to 120 x 90 cells
    around four of them."""
    x0, ul, circles, sg, wp = walls_scene()
    assert x0.shape[0] == B
    world, wcfg = workload.make_grid_world(0, 40, 0.1)
    mid = x0[[0, 1, 6, 7], :2].mean(0)  # four cars stand together, two of each race; the others see free space
    i0 = int(np.clip(np.floor((mid[0] - wcfg.origin_x) / 0.1) - 60, 0, world.shape[1] - 120))
    j0 = int(np.clip(np.floor((mid[1] - wcfg.origin_y) / 0.1) - 45, 0, world.shape[0] - 90))
    grid, cfg = workload.crop_map(world, wcfg, i0, j0, 120, 90)
    assert grid.shape == (90, 120) and grid.any()
    return (x0, ul, circles, np.ascontiguousarray(sg[:-1]), wp), np.ascontiguousarray(grid), cfg


def rollout_field_dev(capi, cuda, s, case, grid, cfg, noise):
    """One Solver.rollout_field_dev call on fresh device arrays, built as world_loop.rollout_dev builds the grid
    family's -> every array as numpy."""
    import torch

    x0, ul, circles, sg, wp = case
    d = replan_buffers(cuda, x0, ul, B, s.horizon, T)
    d["ranges_traj"] = full(cuda, (T, B, R), torch.float32, -7.0)
    d["clear_traj"] = full(cuda, (T + 1, B), torch.float64, -7.0)
    d["nearest_traj"] = full(cuda, (T + 1, B), torch.int32, -7)
    d["crash_tick"] = full(cuda, (B,), torch.int32, -7)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    s.rollout_field_dev(
        capi.default_rollout_config(ticks=T), scan_config(capi, R, GEOM), rp,
        capi.default_world_config(num_circles=circles.shape[0]), capi.default_race_config(group_size=G),
        capi.default_contact_config(stop_on_contact=1), capi.default_body_config(),
        capi.default_walls_config(num_segments=sg.shape[0]), capi.default_refresh_config(every=1), noise,
        capi.grid_config_of(cfg), dev(cuda, capi.traj_table(rp.plan)), dev(cuda, wp), d["x_ref"], d["have_path"],
        dev(cuda, circles), dev(cuda, sg), dev(cuda, grid), device_field(capi, cuda, grid, cfg), d["x_traj"],
        d["u_lin_traj"], d["u_applied"], d["status"],
        *(d.get(k) for k in ("clear_traj", "crash_tick", "nearest_traj") + OPTIONAL))
    torch.cuda.synchronize(cuda)
    return {k: v.cpu().numpy() for k, v in d.items()}


def test_rollout_field_equals_rollout_grid(capi, cuda):
    case, grid, cfg = rollout_scene()
    x0, ul, circles, sg, wp = case
    noise = nz.noise_config(capi, SEED, 0, NOISE)
    s = solver(capi, N, gap=True, x_ref_points=P)
    a = rollout_dev(capi, cuda, s, "grid", case, T, G, 1, every=1, noise=noise, grid=grid, cfg=cfg)
    b = rollout_field_dev(capi, cuda, s, case, grid, cfg, noise)
    assert set(a) == set(b)
    for k in a:
        same_bits(b[k], a[k], f"f110qp_rollout_field_dev: {k}")
    own = workload.ray_map(a["x_traj"][0], GEOM, R, grid, cfg).astype(np.float32)
    assert (own < np.float32(10.0)).mean() > 0.2, "the raster walls are in the scans"
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    h = s.rollout_field(x0, ul, circles, sg, grid, capi.grid_config_of(cfg), capi.default_race_config(group_size=G),
                        capi.default_contact_config(stop_on_contact=1), capi.default_body_config(),
                        capi.default_refresh_config(every=1), noise, scan_config(capi, R, GEOM), rp,
                        capi.traj_table(rp.plan), wp, T, scans=True)
    s.close()
    for k in KEYS:
        same_bits(np.asarray(h[k]).reshape(a[k].shape), a[k], f"f110qp_rollout_field: {k}")
