"""The raster-map oracles of f110qp/workload.py without a GPU (include/f110qp.h rules G1 and G2): ray_grid against a
slab test over every occupied cell, the cells it walks, clearance_grid against a brute force over the whole map,
rasterize_walls' closed polylines, and load_map on maps written here."""
import grid_cases as gc_
import numpy as np
import pytest
import world_cases as wc_

from f110qp import workload

BEAMS = 360
GEOM = wc_.geometry(BEAMS)
# the beams the corner rule leaves out for (map seed, pose seed) below: counted once, asserted since
SKIPPED = {(0, 1): 0, (3, 2): 0, (5, 4): 0}


@pytest.mark.parametrize("seeds", sorted(SKIPPED))
@pytest.mark.parametrize("resolution,origin", [(0.1, (0.0, 0.0)), (0.05, (-1.3, -0.7))])
def test_walk_against_the_slab_test(seeds, resolution, origin):
    grid, cfg = gc_.room(40, 30, resolution, origin, seed=seeds[0])
    x = gc_.free_poses(grid, cfg, 6, seeds[1])
    ox, oy, dx, dy = gc_.beams_of(x, GEOM, BEAMS)
    got = workload.ray_grid(ox, oy, dx, dy, grid, cfg, gc_.MAX_RANGE)
    want, near = gc_.slab_scan(ox, oy, dx, dy, grid, cfg)
    keep = near > gc_.CORNER
    skipped = int((~keep).sum())
    print(f"seeds {seeds} resolution {resolution}: {skipped} of {keep.size} beams within {gc_.CORNER} cells of a corner, "
          f"worst disagreement {np.abs(got - want)[keep].max():.3e} m")
    assert skipped <= gc_.SKIP_CAP * keep.size and skipped == SKIPPED[seeds]
    assert np.abs(got - want)[keep].max() <= gc_.AGREE
    assert (got < gc_.MAX_RANGE).all(), "a closed room: every beam returns"


def test_cells_before_the_hit_are_free_and_the_hit_is_occupied():
    grid, cfg = gc_.room(40, 30, 0.1, seed=3)
    x = gc_.free_poses(grid, cfg, 4, 9)
    ox, oy, dx, dy = (np.broadcast_to(v, (4, BEAMS)) for v in gc_.beams_of(x, GEOM, BEAMS))
    th = workload.ray_grid(ox, oy, dx, dy, grid, cfg, gc_.MAX_RANGE)
    res = cfg.resolution
    for frac in np.linspace(0.0, 1.0, 400, endpoint=False):  # points strictly before the hit
        i, j = gc_.visited_cells(ox, oy, dx, dy, th * frac - 1e-9 * (frac > 0), cfg)
        assert (grid[j, i] == 0).all(), frac
    i, j = gc_.visited_cells(ox, oy, dx, dy, th + 1e-9 * res, cfg)  # just behind the entry: the hit cell
    assert (grid[j, i] != 0).all()


def test_start_rules():
    g = np.zeros((3, 4), np.uint8)
    g[1, 2] = 1
    grid, cfg = gc_.spec(g, (1.0, -1.0), 0.5)
    ray = lambda ox, oy, dx, dy, mr=10.0: float(workload.ray_grid(ox, oy, dx, dy, grid, cfg, mr))  # noqa: E731
    assert ray(2.2, -0.3, 1.0, 0.0) == 0.0, "inside the occupied cell"
    assert ray(1.25, -0.25, 1.0, 0.0) == 0.75, "along x to the cell's face at x = 2"
    assert ray(1.25, -0.25, 1.0, 0.0, 0.7) == 0.7, "a hit beyond max_range"
    assert ray(1.25, -0.75, 1.0, 0.0) == 10.0, "the row below: leaves the map"
    assert ray(0.9, -0.25, 1.0, 0.0) == 10.0, "a start outside the map sees nothing"
    assert ray(float("nan"), -0.25, 1.0, 0.0) == 10.0 and ray(float("inf"), -0.25, 1.0, 0.0) == 10.0
    assert ray(2.5, -0.25, -1.0, 0.0) == 0.0 and np.signbit(workload.ray_grid(2.5, -0.25, -1.0, 0.0, grid, cfg)) == 0, \
        "on the boundary x = 2.5, looking down the axis into the occupied cell: +0"
    assert ray(2.5, -0.25, 1.0, 0.0) == 10.0, "the same start looking away"
    # the tie: through the lattice corner (2, -0.5) on the diagonal the beam steps in x first, into the occupied cell
    assert ray(1.75, -0.75, np.sqrt(0.5), np.sqrt(0.5)) == pytest.approx(0.25 * np.sqrt(2.0), abs=1e-15)
    empty, ecfg = gc_.spec(np.zeros((0, 0), np.uint8))
    assert float(workload.ray_grid(0.0, 0.0, 1.0, 0.0, empty, ecfg)) == 10.0


def test_a_wall_of_cells_that_touch_at_corners_only_does_not_leak():
    """The walk moves along one axis a step: between two free cells that touch at a corner it visits one of the two
    cells beside it, on the exact tie the x-side one."""
    g = np.zeros((4, 4), np.uint8)
    g[1, 2] = g[2, 1] = 1                       # cells (2, 1) and (1, 2): they touch at the corner (2, 2) only
    grid, cfg = gc_.spec(g, (0.0, 0.0), 1.0)
    d = np.sqrt(0.5)
    for o, sgn in (((1.5, 1.5), 1.0), ((2.5, 2.5), -1.0)):      # through the corner exactly, from either side
        assert float(workload.ray_grid(o[0], o[1], sgn * d, sgn * d, grid, cfg)) == pytest.approx(d, abs=1e-15)
    ang = np.pi / 4 + np.linspace(-1e-6, 1e-6, 2001)            # and a fan of beams around it
    assert (workload.ray_grid(1.5, 1.5, np.cos(ang), np.sin(ang), grid, cfg) < 1.0).all()
    g = np.zeros((6, 6), np.uint8)              # a diamond of corner-touching cells around (2.5, 2.5)
    for i, j in ((2, 0), (3, 1), (4, 2), (3, 3), (2, 4), (1, 3), (0, 2), (1, 1)):
        g[j, i] = 1
    grid, cfg = gc_.spec(g, (0.0, 0.0), 1.0)
    ang = np.linspace(-np.pi, np.pi, 100001)
    assert (workload.ray_grid(2.5, 2.5, np.cos(ang), np.sin(ang), grid, cfg) < 10.0).all()


@pytest.mark.parametrize("reach", [0.0, 0.4, 1.0])
def test_clearance_against_the_brute_force(reach):
    grid, cfg = gc_.room(40, 30, 0.1, (-1.0, -1.0), seed=5, reach=reach)
    rng = np.random.default_rng(11)
    x = np.stack([rng.uniform(-3.5, 5.5, 150), rng.uniform(-3.5, 4.5, 150), rng.uniform(-np.pi, np.pi, 150)], 1)
    clear, near = workload.clearance_grid(x, None, None, grid, cfg)
    want, idx = gc_.brute_clearance(x, grid, cfg)
    close = want <= reach
    assert close.sum() >= (3 if reach == 0.0 else 10) and (want <= 0.0).any() and (~close).any()
    assert (clear[close] == want[close]).all() and (near[close] == 1 + idx[close]).all()  # C = 0, G = 1, S = 0
    assert ((clear[~close] > reach) | np.isinf(clear[~close])).all(), "farther says only: more than reach"
    assert (clear >= want).all()
    nan = workload.clearance_grid(np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]]), None, None, grid, cfg)
    assert np.isinf(nan[0]).all() and (nan[1] == -1).all(), "a non-finite pose visits no cell"


def test_centre_in_cell_clause():
    g = np.zeros((8, 8), np.uint8)
    g[4, 4] = 1
    grid, cfg = gc_.spec(g, (0.0, 0.0), 1.0)    # a cell larger than the body: all four edges can lie outside it
    x = np.array([[4.5 - gc_.CENTER_OFFSET, 4.5, 0.0]])
    assert workload.clearance_grid(x, None, None, grid, cfg)[0][0] <= 0.0
    small = np.array([[4.5 - gc_.CENTER_OFFSET, 4.5, 0.0]])
    v = workload.clearance_grid(small, None, None, grid, cfg, half_length=0.1, half_width=0.1)[0][0]
    assert v == 0.0, "a body wholly inside the cell touches no edge: the centre clause gives 0"


def test_rasterized_closed_polyline_leaks_no_beam():
    import walls_cases as wl_
    sg = wl_.star_polygon(37, seed=2, r=(1.0, 2.2), centre=(0.3, -0.2))
    cfg = workload.GridSpec(64, 48, -2.9, -2.6, 0.1)
    assert np.abs(sg).max() < 2.5
    grid = workload.rasterize_walls(sg, None, cfg)
    assert grid.shape == (48, 64) and 0 < grid.sum() < grid.size // 3
    ang = np.linspace(-np.pi, np.pi, 4001)
    for o in ((0.3, -0.2), (0.31, -0.15), (0.05, 0.0)):
        i, j = int((o[0] - cfg.origin_x) / cfg.resolution), int((o[1] - cfg.origin_y) / cfg.resolution)
        assert not grid[j, i]
        got = workload.ray_grid(o[0], o[1], np.cos(ang), np.sin(ang), grid, cfg)
        seg = workload.ray_segments(o[0], o[1], np.cos(ang), np.sin(ang), sg)
        assert (got < 10.0).all(), "no beam leaves the polygon"
        assert (got <= seg + 1e-12).all(), "the cell of the true hit is occupied: the raster wall is never behind it"
        assert np.median(seg - got) < 0.1, "and mostly less than a cell in front"
    circles = np.array([[0.0, 0.0, 0.5]])
    disc = workload.rasterize_walls(None, circles, cfg)
    jj, ii = np.nonzero(disc)
    cx, cy = cfg.origin_x + (ii + 0.5) * 0.1, cfg.origin_y + (jj + 0.5) * 0.1
    assert np.hypot(cx, cy).max() <= 0.5 + 0.1 and disc.sum() >= np.pi * 0.25 / 0.01


def test_make_grid_world():
    grid, cfg = workload.make_grid_world(0, 40, 0.1)
    assert grid.shape == (cfg.height, cfg.width) and grid.dtype == np.uint8
    wp = workload.track_waypoints()
    i = np.floor((wp[:, 0] - cfg.origin_x) / cfg.resolution).astype(int)
    j = np.floor((wp[:, 1] - cfg.origin_y) / cfg.resolution).astype(int)
    assert grid[j, i].mean() < 0.05, "the race line is (almost) free: obstacles stand beside it"
    ang = np.linspace(-np.pi, np.pi, 721)
    got = workload.ray_grid(wp[0, 0], wp[0, 1], np.cos(ang), np.sin(ang), grid, cfg, 100.0)
    assert (got < 100.0).all(), "between the two closed walls no beam escapes"
    small, scfg = workload.crop_map(grid, cfg, 10, 20, 64, 48)
    assert small.shape == (48, 64) and (small == grid[20:68, 10:74]).all()


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("negate", [0, 1])
def test_load_map_round_trip(tmp_path, binary, negate):
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (7, 11))
    px[0, :3] = (0, 255, 89)                     # the top row: black, white, and just above the threshold's pixel
    gc_.write_pgm(tmp_path / "m.pgm", px, binary)
    (tmp_path / "m.yaml").write_text(
        f"image: m.pgm\nresolution: 0.05  # metres\norigin: [-1.5, 2.25, 0.0]\nnegate: {negate}\n"
        "occupied_thresh: 0.65\nfree_thresh: 0.196\n")
    grid, cfg = workload.load_map(tmp_path / "m.pgm", tmp_path / "m.yaml")
    assert grid.shape == (7, 11) and grid.dtype == np.uint8
    assert (cfg.width, cfg.height, cfg.origin_x, cfg.origin_y, cfg.resolution) == (11, 7, -1.5, 2.25, 0.05)
    occ = (px if negate else 255 - px) / 255.0
    assert (grid == (occ > 0.65)[::-1]).all(), "map_server's rule, the image's top row is the grid's last"
    assert list(grid[-1, :3]) == ([0, 1, 0] if negate else [1, 0, 1])  # 89: (255 - 89) / 255 = 0.651 > 0.65
    (tmp_path / "t.yaml").write_text("resolution: 0.1\norigin: [0, 0, 0]\noccupied_thresh: 0.9\n")
    strict, _ = workload.load_map(tmp_path / "m.pgm", tmp_path / "t.yaml")
    assert (strict == ((255 - px) / 255.0 > 0.9)[::-1]).all(), "the threshold is read; negate defaults to 0"
    (tmp_path / "r.yaml").write_text("resolution: 0.1\norigin: [0, 0, 0.5]\n")
    with pytest.raises(ValueError):
        workload.load_map(tmp_path / "m.pgm", tmp_path / "r.yaml")


def test_load_map_16_bit(tmp_path):
    px = np.array([[0, 65535, 30000], [65535, 0, 100]])
    gc_.write_pgm(tmp_path / "w.pgm", px, True, maxval=65535, comment=False)
    (tmp_path / "w.yaml").write_text("resolution: 1.0\norigin: [0.0, 0.0, 0.0]\n")
    grid, _ = workload.load_map(tmp_path / "w.pgm", tmp_path / "w.yaml")
    assert grid.tolist() == [[0, 1, 1], [1, 0, 0]]
