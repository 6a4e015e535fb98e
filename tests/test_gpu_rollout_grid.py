"""The rollout on a raster map on MI355X (f110qp_rollout_grid[_dev]) at T = 12, B = 8, G = 2, N = 5 on the track of
test_gpu_rollout_walls.py with workload.make_grid_world cropped to 64 x 48 cells around the cars and a raster wall in
front of car 0: an empty map is f110qp_rollout_noisy_dev bit for bit; every row of ranges_traj is
f110qp_cast_scans_grid_dev at that row's poses with that tick's noise and every row of clear_traj
f110qp_clearance_grid_dev there; the car facing the raster wall gets a crash_tick whose nearest obstacle is a cell, and
parks; the host call equals the device call; and two halves with car_base equal the whole. All bit equality."""
import noise_cases as nz
import numpy as np
import pytest
import walls_cases as wl_
from test_gpu_grid import SEED, grid_cast, grid_clearance
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_contact import check_parked
from test_gpu_rollout_noisy import rollout_noisy_dev
from test_gpu_rollout_replan import P
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_walls import B, G, N
from test_gpu_rollout_walls import scene as walls_scene
from test_gpu_rollout_world import GEOM, R
from world_loop import rollout_dev

from f110qp import workload

pytestmark = pytest.mark.gpu

T = 12
NOISE = (0.01, 0.005, 0.02)
RES = 0.1


def scene():
    """The walls scene without its extra segment; the map: make_grid_world at 0.1 m cropped to 64 x 48 cells around
    the cars, and the cells of a 0.6 m wall across the path of car 0, as near as leaves row 0 between 5 and 40 mm of
    clearance (found with the oracle)."""
    x0, ul, circles, sg, wp = walls_scene()
    sg = np.ascontiguousarray(sg[:-1])
    world, wcfg = workload.make_grid_world(0, 40, RES)
    mid = x0[[0, 1, 6, 7], :2].mean(0)  # the first and the last race stand together; the others see free space
    i0 = int(np.floor((mid[0] - wcfg.origin_x) / RES)) - 32
    j0 = int(np.floor((mid[1] - wcfg.origin_y) / RES)) - 24
    grid, cfg = workload.crop_map(world, wcfg, i0, j0, 64, 48)
    assert grid.shape == (48, 64) and grid.any()
    c, s = np.cos(x0[0, 2]), np.sin(x0[0, 2])
    for ahead in np.arange(0.02, 0.4, 0.005):
        m = x0[0, :2] + (wl_.CENTER_OFFSET + wl_.HL + ahead) * np.array([c, s])
        across = 0.3 * np.array([-s, c])
        g = grid | workload.rasterize_walls(np.concatenate([m - across, m + across])[None], None, cfg)
        v = workload.clearance_grid(x0[:G], None, None, g, cfg, G, wl_.CENTER_OFFSET)[0][0]
        if 0.005 < v <= 0.04:
            return (x0, ul, circles, sg, wp), np.ascontiguousarray(g), cfg
    raise AssertionError("no wall distance leaves car 0 a clearance in (5, 40] mm")


def rollout_grid_dev(capi, cuda, s, case, grid, cfg, stop, noise, ticks=T, null=(), every=1):
    """One Solver.rollout_grid_dev call on fresh device arrays -> every array as numpy."""
    return rollout_dev(capi, cuda, s, "grid", case, ticks, G, stop, every=every, noise=noise, grid=grid, cfg=cfg, null=null)


def noise_of(capi, car_base=0, setting=NOISE):
    return nz.noise_config(capi, SEED, car_base, setting)


_RUNS = {}


def run(capi, cuda, stop):
    """The run of the scene at every = 1, gap rows on, computed once per stop."""
    if stop not in _RUNS:
        case, grid, cfg = scene()
        s = solver(capi, N, gap=True, x_ref_points=P)
        _RUNS[stop] = rollout_grid_dev(capi, cuda, s, case, grid, cfg, stop, noise_of(capi))
        s.close()
    return _RUNS[stop]


@pytest.mark.parametrize("stop", [0, 1])
def test_empty_map_is_the_noisy_call(capi, cuda, stop):
    case, _, cfg = scene()
    empty = np.zeros((0, 0), np.uint8)
    ecfg = workload.GridSpec(0, 0, cfg.origin_x, cfg.origin_y, cfg.resolution, cfg.reach)
    s = solver(capi, N, gap=True, x_ref_points=P)
    a = rollout_grid_dev(capi, cuda, s, case, empty, ecfg, stop, noise_of(capi))
    b = rollout_noisy_dev(capi, cuda, s, case, stop, 1, noise_of(capi), ticks=T)
    s.close()
    assert set(a) == set(b)
    for k in a:
        same_bits(a[k], b[k], f"stop {stop}: {k}")


def test_rows_are_the_grid_cast_and_the_grid_clearance(capi, cuda):
    a = run(capi, cuda, 0)
    (_, _, circles, sg, _), grid, cfg = scene()
    seen = 0
    for t in range(T + 1):
        x = a["x_traj"][t]
        if t < T:
            want = grid_cast(capi, cuda, x, grid, cfg, GEOM, R, static=circles, segments=sg, G=G, setting=NOISE, tick=t)
            same_bits(a["ranges_traj"][t], want, f"scan of tick {t}: f110qp_cast_scans_grid_dev with tick {t}")
            quiet = grid_cast(capi, cuda, x, grid, cfg, GEOM, R, static=circles, segments=sg, G=G)
            own = workload.ray_map(x, GEOM, R, grid, cfg).astype(np.float32)
            seen += int(((quiet == own) & (own < np.float32(10.0))).sum())
        clear, near = grid_clearance(capi, cuda, x, grid, cfg, circles, sg, G)
        same_bits(a["clear_traj"][t], clear[0], f"clearance of row {t}")
        assert (a["nearest_traj"][t] == near[0]).all(), t
    assert seen > T * B * 50, "the raster walls are in the scans"


def test_a_car_facing_a_raster_wall_crashes_and_parks(capi, cuda):
    free, parked = run(capi, cuda, 0), run(capi, cuda, 1)
    (_, _, circles, sg, _), grid, cfg = scene()
    first_cell = circles.shape[0] + G + sg.shape[0]
    for a in (free, parked):
        k = int(a["crash_tick"][0])
        assert 1 <= k <= T, a["crash_tick"]
        assert a["clear_traj"][k, 0] <= 0.0 < a["clear_traj"][k - 1, 0]
        assert a["nearest_traj"][k, 0] >= first_cell, "the nearest obstacle at the crash is a cell of the map"
        j, i = divmod(int(a["nearest_traj"][k, 0]) - first_cell, grid.shape[1])
        assert grid[j, i]
    check_parked(capi, {k: v for k, v in parked.items() if k != "hs_traj"}, "grid stop 1")
    k = int(parked["crash_tick"][0])
    assert (parked["kind"][k:, 0] == capi.TICK_CRASHED).all()
    assert (parked["crash_tick"][1] < 0) or parked["crash_tick"][1] >= k, "its race-mate drove on at least as long"


@pytest.mark.parametrize("stop", [0, 1])
def test_host_call_equals_the_device_call(capi, cuda, stop):
    (x0, ul, circles, sg, wp), grid, cfg = scene()
    s = solver(capi, N, gap=True, x_ref_points=P)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    h = s.rollout_grid(x0, ul, circles, sg, grid, capi.grid_config_of(cfg), capi.default_race_config(group_size=G),
                       capi.default_contact_config(stop_on_contact=stop), capi.default_body_config(),
                       capi.default_refresh_config(every=1), noise_of(capi), scan_config(capi, R, GEOM), rp,
                       capi.traj_table(rp.plan), wp, T, scans=True)
    s.close()
    a = run(capi, cuda, stop)
    for k in ("x_traj", "u_lin_traj", "u_applied", "status", "hs_traj", "kind", "clear_traj", "nearest_traj", "crash_tick",
              "ranges_traj"):
        same_bits(np.asarray(h[k]).reshape(a[k].shape), a[k], k)


def test_two_halves_with_car_base_equal_the_whole(capi, cuda):
    (x0, ul, circles, sg, wp), grid, cfg = scene()
    whole = run(capi, cuda, 1)
    s = solver(capi, N, gap=True, x_ref_points=P)
    for lo in (0, B // 2):
        cars = slice(lo, lo + B // 2)
        half = rollout_grid_dev(capi, cuda, s, (x0[cars], ul[cars], circles, sg, wp), grid, cfg, 1, noise_of(capi, lo))
        for k in ("x_traj", "u_lin_traj", "u_applied", "status", "hs_traj", "kind", "clear_traj", "nearest_traj",
                  "ranges_traj"):
            same_bits(half[k], whole[k][:, cars], f"cars {lo} to {lo + B // 2 - 1}: {k}")
        same_bits(half["crash_tick"], whole["crash_tick"][cars], "crash_tick")
    s.close()
