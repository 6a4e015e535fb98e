"""The distance field's oracle held to its model on the CPU (include/f110qp.h, rules D1 to D4): the definition
(workload.grid_distance) against a separable two-pass transform and, on the small maps, a Python loop, ties included;
the values each case is about; and the stated consequences of rule D3 and of the inflation against
workload.clearance_grid. No GPU."""
import field_cases as fc
import numpy as np
import pytest

from f110qp import workload

CASES = fc.map_cases()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_oracle_equals_the_second_formulation(c):
    o = c.oracle()  # also asserts the case's own expected values
    assert o["d2"].dtype == np.int32 and o["nearest"].dtype == np.int32
    cells = c.W * c.H
    if c.H <= 350:  # the separable pass costs H x H x W
        other = workload.grid_distance(c.grid) if c.how == "separable" and cells <= fc.SMALL else fc.separable(c.grid)
        assert fc.same(other[0], o["d2"]) and fc.same(other[1], o["nearest"]), c.name
    if cells <= 300:
        d2, near = fc.loop(c.grid)
        assert fc.same(d2, o["d2"]) and fc.same(near, o["nearest"]), c.name
    occ = c.grid != 0
    assert (o["d2"][occ] == 0).all() and (o["nearest"][occ] == np.flatnonzero(occ.reshape(-1))).all()
    assert ((o["nearest"] < 0) == (o["d2"] == fc.INT_MAX)).all()
    if occ.any():  # nearest names an occupied cell at exactly d2
        j, i = np.mgrid[0:c.H, 0:c.W]
        q, p = np.divmod(o["nearest"].astype(np.int64), c.W)
        assert occ[q, p].all() and ((i - p) ** 2 + (j - q) ** 2 == o["d2"]).all()


def test_the_world_map_on_a_crop_against_the_definition():
    """The 584 x 344 case's oracle is the separable pass; the definition on a 70 x 60 crop of the same map agrees
    with the separable pass there."""
    world = CASES[-1].grid
    occ = np.argwhere(world)
    j0, i0 = np.clip(occ[len(occ) // 2] - (30, 35), 0, (world.shape[0] - 60, world.shape[1] - 70))
    g = np.ascontiguousarray(world[j0:j0 + 60, i0:i0 + 70])
    assert g.shape == (60, 70) and g.any() and not g.all()
    a, b = workload.grid_distance(g), fc.separable(g)
    assert fc.same(a[0], b[0]) and fc.same(a[1], b[1])


def test_metres_and_inflation():
    c, counts = fc.inflate_case()
    o = c.oracle()
    assert [int(o[f"inflated_{k}"].sum()) for k in range(4)] == list(counts)
    assert fc.same(o["inflated_0"], c.grid), "radius 0 gives the map back as 0 / 1"
    m = workload.grid_dist_metres(np.array([0, 1, 2, fc.INT_MAX], np.int32), c.cfg)
    assert m[0] == 0.0 and m[1] == 0.05 and m[2] == 0.05 * np.sqrt(2.0) and m[3] == np.inf
    e = next(x for x in CASES if x.name.startswith("empty")).oracle()
    assert not e["inflated_3"].any() and (e["d2"] == fc.INT_MAX).all(), "+inf is above every radius"


def test_lookup_oracle():
    for c in fc.lookup_cases():
        o, f = c.oracle(), c.map.oracle()
        x, cfg = c.x[0], c.map.cfg
        inside = ~np.isnan(o["dist"][0])
        assert inside.any() and (~inside).any()
        assert (o["dist"].view(np.uint64)[0][~inside] == fc.NAN_BITS).all() and (o["cell"][0][~inside] == -1).all()
        ix =np.floor((x[inside, 0] - cfg.origin_x) / cfg.resolution).astype(int)
        iy = np.floor((x[inside, 1] - cfg.origin_y) / cfg.resolution).astype(int)
        assert (ix >= 0).all() and (ix < c.map.W).all() and (iy >= 0).all() and (iy < c.map.H).all()
        assert (o["cell"][0][inside] == f["nearest"][iy, ix]).all()
        assert np.isfinite(x[inside, :2]).all(), "a non-finite point is outside"
    only, none = workload.grid_lookup(c.x, f["d2"], None, cfg)
    assert none is None and fc.same(only, o["dist"])
    ecfg = workload.GridSpec(0, 0, 0.0, 0.0, 0.1, 1.0)
    d, cell = workload.grid_lookup(c.x, np.zeros((0, 0), np.int32), np.zeros((0, 0), np.int32), ecfg)
    assert (d.view(np.uint64) == fc.NAN_BITS).all() and (cell == -1).all(), "no map: every point is outside"


# ---- the stated consequences of rule D3 and of the inflation -----------------------------------------------------

SLACK = 1e-9      # metres, for the oracle's own rounding
SEED, POSES = 11, 200
BODIES = ((workload.HALF_LENGTH, workload.HALF_WIDTH), (0.05, 0.03))


def consequence_scene():
    """A 60 x 60 map at 5 % and 0.05 m a cell; 200 body centres in free cells with headings, (x, y) uniform over
    the cell."""
    rng = np.random.default_rng(SEED)
    grid = (rng.random((60, 60)) < 0.05).astype(np.uint8)
    cfg = workload.GridSpec(60, 60, -0.7, 0.3, 0.05, 100.0)  # reach larger than the map: rule G2 sees every cell
    free = np.argwhere(grid == 0)
    pick = free[rng.choice(len(free), POSES, replace=False)]
    u = rng.random((POSES, 2))
    x = np.stack([cfg.origin_x + (pick[:, 1] + u[:, 0]) * cfg.resolution,
                  cfg.origin_y + (pick[:, 0] + u[:, 1]) * cfg.resolution, rng.uniform(-np.pi, np.pi, POSES)], axis=1)
    return grid, cfg, x


def point_to_occupied(grid, cfg, x):
    """The distance from each point to the occupied area (the union of the occupied cells' closed squares)."""
    q, p = np.nonzero(grid)
    x0, y0 = cfg.origin_x + p * cfg.resolution, cfg.origin_y + q * cfg.resolution
    dx = np.maximum(np.maximum(x0[None] - x[:, :1], x[:, :1] - (x0[None] + cfg.resolution)), 0.0)
    dy = np.maximum(np.maximum(y0[None] - x[:, 1:2], x[:, 1:2] - (y0[None] + cfg.resolution)), 0.0)
    return np.hypot(dx, dy).min(axis=1)


def test_distance_bounds_points_and_bodies():
    grid, cfg, x = consequence_scene()
    d2, near = workload.grid_distance(grid)
    dist, cell = workload.grid_lookup(x, d2, near, cfg)
    assert np.isfinite(dist).all() and (dist > 0).all(), "every pose is in a free cell of the map"
    share = float((dist <= 1.0).mean())
    print(f"poses within 1 m of an occupied cell's centre: {share:.3f}; dist {dist.min():.3f} .. {dist.max():.3f} m")
    assert share >= 0.5, "the bound is not tested on empty space only"
    r2 = cfg.resolution * np.sqrt(2.0)
    assert (point_to_occupied(grid, cfg, x) >= dist - r2 - SLACK).all()
    for hl, hw in BODIES:
        clear, _ = workload.clearance_grid(x, None, None, grid, cfg, 1, 0.0, hl, hw)  # the pose is the body's centre
        bound = dist - r2 - np.sqrt(hl * hl + hw * hw)
        print(f"body {hl} x {hw}: least clearance - bound = {(clear - bound).min():.4f} m, bound > 0 at {(bound > 0).sum()}")
        assert (clear >= bound - SLACK).all()


def test_inflated_map_leaves_bodies_clear():
    grid, cfg, _ = consequence_scene()
    d2, _ = workload.grid_distance(grid)
    rng = np.random.default_rng(SEED + 1)
    for (hl, hw), least in zip(BODIES, (0, 20)):
        radius = np.sqrt(hl * hl + hw * hw) + cfg.resolution * np.sqrt(2.0)
        fat = workload.grid_inflate(d2, cfg, radius)
        assert fat[grid != 0].all(), "the inflated map holds the map"
        free = np.argwhere(fat == 0)
        assert len(free) >= least, (hl, hw, len(free))
        if not len(free):
            continue
        pick = free[rng.choice(len(free), min(POSES, len(free)), replace=False)]
        u = rng.random((len(pick), 2))
        x = np.stack([cfg.origin_x + (pick[:, 1] + u[:, 0]) * cfg.resolution,
                      cfg.origin_y + (pick[:, 0] + u[:, 1]) * cfg.resolution,
                      rng.uniform(-np.pi, np.pi, len(pick))], axis=1)
        clear, _ = workload.clearance_grid(x, None, None, grid, cfg, 1, 0.0, hl, hw)
        print(f"body {hl} x {hw}: {len(pick)} poses in cells the inflated map leaves free, least clearance {clear.min():.4f} m")
        assert (clear > -SLACK).all()
