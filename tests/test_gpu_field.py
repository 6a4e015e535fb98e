"""The distance-field kernels on MI355X (f110qp_grid_distance_dev, f110qp_grid_inflate_dev, f110qp_grid_lookup_dev,
f110qp_grid_field, f110qp_wall_distance; include/f110qp.h, rules D1 to D4) against the numpy oracle, bit for bit on
every output: every map of field_cases.py (test_field_cases.py holds the oracle to the model on the CPU) with and
without nearest, the inflation at four radii, the lookups on boundaries, special values and past the grid cap, the
host calls, the inflated map under f110qp_clearance_grid_dev, and one closed loop through the lookup and the fan."""
import field_cases as fc
import numpy as np
import pytest
from test_gpu_rollout_replan import dev

from f110qp import workload

pytestmark = pytest.mark.gpu

CASES = fc.map_cases()


def field(capi, cuda, c, nearest=True, inflate=True):
    """f110qp_grid_distance_dev and f110qp_grid_inflate_dev at the case's radii on outputs pre-filled with -7 ->
    (dict of d2, nearest (None when left out) and inflated_k, the device's d2, the device's nearest)."""
    import torch

    gc = capi.grid_config_of(c.cfg)
    d2 = torch.full((c.H, c.W), -7, dtype=torch.int32, device=cuda)
    near = torch.full((c.H, c.W), -7, dtype=torch.int32, device=cuda) if nearest else None
    work = torch.full((c.H, c.W), -7, dtype=torch.int32, device=cuda)
    capi.grid_distance_dev(gc, dev(cuda, c.grid), d2, work, near)
    got = {}
    for k, r in enumerate(c.radii() if inflate else ()):
        out = torch.full((c.H, c.W), 249, dtype=torch.uint8, device=cuda)
        capi.grid_inflate_dev(gc, d2, r, out)
        got[f"inflated_{k}"] = out
    torch.cuda.synchronize(cuda)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got.update(d2=d2.cpu().numpy(), nearest=near.cpu().numpy() if nearest else None)
    return got, d2, near


def lookup(capi, cuda, c, d2, near, cell=True, x=None):
    import torch

    x = c.x if x is None else x
    shape = x.shape[:-1]
    dist = torch.full(shape, -7.0, dtype=torch.float64, device=cuda)
    out = torch.full(shape, -7, dtype=torch.int32, device=cuda) if cell else None
    capi.grid_lookup_dev(capi.grid_config_of(c.map.cfg), d2, dev(cuda, x), dist, near if cell else None, out)
    torch.cuda.synchronize(cuda)
    return dict(dist=dist.cpu().numpy().reshape(c.x.shape[:2]),
                cell=out.cpu().numpy().reshape(c.x.shape[:2]) if cell else None)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_maps(capi, cuda, c):
    got, _, _ = field(capi, cuda, c)
    c.check(got)
    part, _, _ = field(capi, cuda, c, nearest=False, inflate=False)
    assert part["nearest"] is None
    c.check(part, "nearest left out")


def test_inflation_radii(capi, cuda):
    c, counts = fc.inflate_case()
    got, _, _ = field(capi, cuda, c)
    c.check(got)
    assert [int(got[f"inflated_{k}"].sum()) for k in range(4)] == list(counts)
    assert fc.same(got["inflated_0"], c.grid)


@pytest.mark.parametrize("i", range(3))
def test_lookup_edges(capi, cuda, i):
    c = fc.lookup_cases()[i]
    _, d2, near = field(capi, cuda, c.map, inflate=False)
    got = lookup(capi, cuda, c, d2, near)
    c.check(got)
    alone = lookup(capi, cuda, c, d2, near, cell=False)
    assert alone["cell"] is None
    c.check(alone, "cell left out")
    c.check(lookup(capi, cuda, c, d2, near, x=c.x[0]), "one row given as [B, 3]")


def test_lookup_past_the_grid_cap(capi, cuda):
    c = fc.stride_case()
    _, d2, near = field(capi, cuda, c.map, inflate=False)
    c.check(lookup(capi, cuda, c, d2, near))


def test_lookup_without_a_map(capi, cuda):
    c = fc.lookup_cases()[1]
    import torch

    gc = capi.default_grid_config(width=0, height=0, resolution=0.07)
    dist = torch.full((c.B,), -7.0, dtype=torch.float64, device=cuda)
    capi.grid_lookup_dev(gc, None, dev(cuda, c.x[0]), dist)
    capi.grid_distance_dev(gc, None, None, None)  # launches nothing
    torch.cuda.synchronize(cuda)
    assert (dist.cpu().numpy().view(np.uint64) == fc.NAN_BITS).all()


def test_host_calls_equal_the_device_calls(capi, cuda):
    for c in (CASES[-1], next(x for x in CASES if x.name == "random 129x200 at 0.05"),
              next(x for x in CASES if x.name.startswith("empty"))):
        want, _, _ = field(capi, cuda, c)
        gc = capi.grid_config_of(c.cfg)
        for k, r in enumerate(c.radii()):
            got = capi.grid_field(gc, c.grid, radius=r)
            for name in ("d2", "nearest"):
                assert fc.same(got[name], want[name]), (c.name, name)
            assert fc.same(got["inflated"], want[f"inflated_{k}"]), (c.name, k)
        part = capi.grid_field(gc, c.grid, nearest=False)
        assert part["nearest"] is None and part["inflated"] is None and fc.same(part["d2"], want["d2"])
    for c in fc.lookup_cases():
        _, d2, near = field(capi, cuda, c.map, inflate=False)
        want = lookup(capi, cuda, c, d2, near)
        gc = capi.grid_config_of(c.map.cfg)
        dist, cell = capi.wall_distance(gc, c.map.grid, c.x)
        assert fc.same(dist, want["dist"]) and fc.same(cell, want["cell"]), c.name
        c.check(dict(dist=dist, cell=cell), "host call")
        dist, cell = capi.wall_distance(gc, c.map.grid, c.x, cell=False)
        assert cell is None and fc.same(dist, want["dist"])


def test_inflated_map_under_the_grid_clearance(capi, cuda):
    """The inflated map is a map: f110qp_clearance_grid_dev takes it and gives workload.clearance_grid's bits on it."""
    import grid_cases as gc_
    from test_gpu_grid import grid_clearance

    c = fc.lookup_map(0.07, (-1.234, 0.517))
    got, _, _ = field(capi, cuda, c)
    fat = got["inflated_2"]
    assert fat.sum() > c.grid.sum() and not fat.all()
    rng = np.random.default_rng(9)
    x = np.stack([c.cfg.origin_x + rng.uniform(0, c.W, 24) * c.cfg.resolution,
                  c.cfg.origin_y + rng.uniform(0, c.H, 24) * c.cfg.resolution, rng.uniform(-3, 3, 24)], axis=1)
    clear, near = grid_clearance(capi, cuda, x, fat, c.cfg)
    want, wnear = workload.clearance_grid(x, None, None, fat, c.cfg, 1, gc_.CENTER_OFFSET)
    assert fc.same(clear[0], want) and (near[0] == wnear).all()
    assert np.isfinite(want).any()


def test_closed_loop(capi, cuda):
    """f110qp_rollout_grid_dev on the scene of test_gpu_rollout_grid.py (T = 12, B = 8): the (x, y) of its x_traj
    through the lookup on the scene's own map, the result through f110qp_mc_fan_dev as M = 4 hypotheses of G = 2:
    every value equal to the numpy chain grid_lookup -> mc_fan."""
    import torch
    from test_gpu_rollout_grid import B, T, run, scene

    a = run(capi, cuda, 0)
    _, grid, cfg = scene()
    m = fc.MapCase("rollout map", grid, resolution=cfg.resolution, origin=(cfg.origin_x, cfg.origin_y))
    got, d2, near = field(capi, cuda, m, inflate=False)
    m.check(got)
    lc = fc.LookupCase("x_traj", m, a["x_traj"])
    assert lc.x.shape == (T + 1, B, 3)
    dist = torch.full((T + 1, B), -7.0, dtype=torch.float64, device=cuda)
    cell = torch.full((T + 1, B), -7, dtype=torch.int32, device=cuda)
    capi.grid_lookup_dev(capi.grid_config_of(cfg), d2, dev(cuda, lc.x), dist, near, cell)
    M, G, prob = 4, 2, (0.0, 0.5, 1.0)
    fan = torch.full((T + 1, B // M, len(prob)), -7.0, dtype=torch.float64, device=cuda)
    count = torch.full((T + 1, B // M), -7, dtype=torch.int32, device=cuda)
    capi.mc_fan_dev(capi.default_mc_config(hypotheses=M, group_size=G, prob=prob), dist, fan, count)
    torch.cuda.synchronize(cuda)
    lc.check(dict(dist=dist.cpu().numpy(), cell=cell.cpu().numpy()))
    wfan, wcount = workload.mc_fan(lc.oracle()["dist"], M, G, prob)
    assert fc.same(fan.cpu().numpy(), wfan) and fc.same(count.cpu().numpy(), wcount)
    d = lc.oracle()["dist"]
    print(f"wall distance along x_traj: {np.nanmin(d):.3f} .. {np.nanmax(d):.3f} m, outside the map {int(np.isnan(d).sum())}")
    assert np.isfinite(d).any()
