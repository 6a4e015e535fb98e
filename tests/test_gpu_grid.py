"""The raster-map kernels on MI355X (f110qp_cast_scans_grid_dev, f110qp_clearance_grid_dev; include/f110qp.h rules G1
and G2), bit for bit against the numpy oracles workload.ray_grid and workload.clearance_grid.

The cast. A float32 range is (float)min(...), and rounding to float32 is monotone, so the expected scan is the
device's own noise-free walls cast (circles, mates and segments; a row of max_range without them) folded with
(float32)workload.ray_map by np.minimum, then workload.noisy_scan: the noise tests' construction. The map's share is
computed from numpy's sincos, which differs from the device's in the last place on some beams; that moves a range
by some 1e-15 m against float32's 1e-7, and every scan here was seen to agree in every bit.

The clearance. Its float64 values carry the heading's sincos in every bit, so the bit-for-bit cases stand at
heading 0 (where both give (1, 0)); rotated poses are compared to 1e-12 m (sincos to an ulp on coordinates of a
few metres gives some 1e-15)."""
import grid_cases as gc_
import noise_cases as nz
import numpy as np
import pytest
import world_cases as wc_
from test_gpu_noise import noisy_cast
from test_gpu_rollout import same_bits
from test_gpu_rollout_replan import dev
from test_gpu_rollout_scan import scan_config
from test_gpu_walls import clearance as walls_clearance
from test_gpu_walls import walls_of
from test_gpu_world_scan import SENTINEL

from f110qp import workload

pytestmark = pytest.mark.gpu

SEED = 7
QUIET = (0.0, 0.0, 0.0)


def _world(capi, static, x, G, max_range):
    C = 0 if static is None else static.shape[-2]
    w = capi.default_world_config(num_circles=C, max_range=max_range,
                                  world_rows=1 if static is None or static.ndim == 2 else static.shape[0])
    return C, w, capi.default_race_config(group_size=G, center_offset=gc_.CENTER_OFFSET)


def grid_cast(capi, cuda, x, grid, cfg, geom, beams, static=None, segments=None, G=1, setting=QUIET, tick=0, base=0,
              max_range=gc_.MAX_RANGE, listed=None, count=None):
    """f110qp_cast_scans_grid_dev on host arrays into rows pre-filled with the sentinel -> ranges [B, R]."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    nb = x.shape[0]
    C, w, race = _world(capi, static, x, G, max_range)
    wl = walls_of(capi, segments, nb)
    out = torch.full((nb, beams), float(SENTINEL), dtype=torch.float32, device=cuda)
    gcfg = capi.grid_config_of(cfg)
    capi.cast_scans_grid_dev(scan_config(capi, beams, geom), w, race, capi.default_body_config(), wl,
                             nz.noise_config(capi, SEED, base, setting), gcfg, tick, dev(cuda, x),
                             dev(cuda, static) if C else None, dev(cuda, segments) if wl.num_segments else None,
                             dev(cuda, grid) if grid.size else None, out,
                             list_=None if listed is None else dev(cuda, np.asarray(listed, np.int32)),
                             count=None if listed is None else dev(cuda, np.int32([count])))
    torch.cuda.synchronize(cuda)
    return out.cpu().numpy()


def walls_cast(capi, cuda, x, geom, beams, static, segments, G, max_range):
    """The device's noise-free cast of everything but the map."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    nb = x.shape[0]
    C, w, race = _world(capi, static, x, G, max_range)
    wl = walls_of(capi, segments, nb)
    out = torch.full((nb, beams), float(SENTINEL), dtype=torch.float32, device=cuda)
    capi.cast_scans_walls_dev(scan_config(capi, beams, geom), w, race, capi.default_body_config(), wl, dev(cuda, x),
                              dev(cuda, static) if C else None, dev(cuda, segments) if wl.num_segments else None, out)
    torch.cuda.synchronize(cuda)
    return out.cpu().numpy()


def expected(capi, cuda, x, grid, cfg, geom, beams, static=None, segments=None, G=1, setting=QUIET, tick=0, base=0,
             max_range=gc_.MAX_RANGE):
    """(the expected scan, the noise-free one, the map's share alone as float32)."""
    rest = walls_cast(capi, cuda, x, geom, beams, static, segments, G, max_range)
    own = workload.ray_map(x, geom, beams, grid, cfg, gc_.LIDAR_OFFSET, max_range).astype(np.float32)
    clean = np.minimum(rest, own)
    return nz.oracle(clean, SEED, base, tick, setting, max_range), clean, own


def check(capi, cuda, what, x, grid, cfg, geom, beams, **kw):
    got = grid_cast(capi, cuda, x, grid, cfg, geom, beams, **kw)
    want, clean, own = expected(capi, cuda, x, grid, cfg, geom, beams, **kw)
    same_bits(got, want, what)
    return got, clean, own


@pytest.mark.parametrize("resolution,origin", [(0.1, (0.0, 0.0)), (0.05, (-1.3, -0.7))])
def test_rooms(capi, cuda, resolution, origin):
    """40 x 30 cells; 0.05 is inexact in binary and the origin negative. 1,080 beams, six cars."""
    grid, cfg = gc_.room(40, 30, resolution, origin, seed=3)
    x = gc_.free_poses(grid, cfg, 6, 5)
    got, _, own = check(capi, cuda, f"room at {resolution}", x, grid, cfg, wc_.geometry(1080), 1080)
    assert (got < np.float32(gc_.MAX_RANGE)).all() and (got > 0).all(), "a closed room: every beam returns"


def test_grid_stride_and_beam_tiles(capi, cuda):
    """520 cars with 33 beams: past the cap of 512 workgroups. 3 cars with 1,200 beams: two beam tiles."""
    grid, cfg = gc_.room(64, 48, 0.1, (-3.0, -2.0), seed=8, blocks=12)
    check(capi, cuda, "520 cars", gc_.free_poses(grid, cfg, 520, 6), grid, cfg, wc_.geometry(33), 33)
    got, _, _ = check(capi, cuda, "1,200 beams", gc_.free_poses(grid, cfg, 3, 7), grid, cfg, wc_.geometry(1200), 1200)
    assert (got[:, 1152:] < np.float32(gc_.MAX_RANGE)).all(), "the second tile's beams walk too"


def _lidar_at(lx, ly, yaw=0.0, exact=True):
    """The pose whose LiDAR origin is (lx, ly), with `exact` in the cast's own arithmetic (a few ulps are tried)."""
    c, s = np.cos(yaw), np.sin(yaw)
    x, y = lx - gc_.LIDAR_OFFSET * c, ly - gc_.LIDAR_OFFSET * s
    if exact:
        for _ in range(4):
            x = x if x + gc_.LIDAR_OFFSET * c == lx else np.nextafter(x, x + (lx - (x + gc_.LIDAR_OFFSET * c)))
            y = y if y + gc_.LIDAR_OFFSET * s == ly else np.nextafter(y, y + (ly - (y + gc_.LIDAR_OFFSET * s)))
        assert x + gc_.LIDAR_OFFSET * c == lx and y + gc_.LIDAR_OFFSET * s == ly
    return np.array([x, y, yaw])


def test_starts(capi, cuda):
    """A quarter-metre lattice (exact in binary), heading 0 and angle_min 0: beam 0 is d = (1, 0), d.y == 0."""
    g = np.zeros((12, 16), np.uint8)
    g[4, 8] = g[9, 3] = 1
    grid, cfg = gc_.spec(g, (0.0, 0.0), 0.25)
    beams = 64
    geom = wc_._geom(0.0, 2.0 * np.pi / beams, beams)
    x = np.stack([_lidar_at(1.125, 1.125),    # 0: beam 0 along the row of cell (8, 4): hits its face at x = 2
                  _lidar_at(1.0, 1.125),      # 1: exactly on the boundary x = 1, the same beam
                  _lidar_at(2.125, 1.125),    # 2: inside the occupied cell: every beam reads 0
                  _lidar_at(-0.5, 1.125),     # 3: outside the map: sees nothing
                  _lidar_at(2.25, 1.125),     # 4: on the occupied cell's far face x = 2.25: in the free cell 9
                  _lidar_at(1.125, 2.625),    # 5: a free row: beam 0 leaves the map
                  _lidar_at(2.0, 1.125)])     # 6: on the boundary x = 2 = the occupied cell's near face: inside
    got, _, own = check(capi, cuda, "starts", x, grid, cfg, geom, beams)
    assert got[0, 0] == np.float32(0.875) and got[1, 0] == np.float32(1.0)
    assert (got[2] == 0).all() and (got[6] == 0).all() and not np.signbit(got[2]).any()
    assert (got[3] == np.float32(gc_.MAX_RANGE)).all()
    assert got[5, 0] == np.float32(gc_.MAX_RANGE), "beam 0 leaves the map"
    assert got[4, 0] == np.float32(gc_.MAX_RANGE), "from the far face looking away"
    half = beams // 2                          # beam 32 is d ~ (-1, 1e-16): back into the occupied cell at once
    assert got[4, half] == 0 and not np.signbit(got[4, half]), "0 / g on the boundary is +0"
    # a hit beyond max_range, and max_range itself on the boundary's parameter
    got, _, _ = check(capi, cuda, "max_range 0.5", x[:2], grid, cfg, geom, beams, max_range=0.5)
    assert (got == np.float32(0.5)).all()
    got, _, _ = check(capi, cuda, "max_range 0.875", x[:1], grid, cfg, geom, beams, max_range=0.875)
    assert got[0, 0] == np.float32(0.875), "t == max_range is a hit of that value either way"


def test_tiny_maps(capi, cuda):
    beams = 90
    geom = wc_.geometry(beams)
    x = np.stack([_lidar_at(0.05, 0.05, exact=False), _lidar_at(0.35, 0.45, 0.3, False), _lidar_at(-1.0, 0.05, 0.1, False)])
    one, cfg1 = gc_.spec(np.ones((1, 1), np.uint8), (0.0, 0.0), 0.1)
    got, _, _ = check(capi, cuda, "1 x 1 occupied", x, one, cfg1, geom, beams)
    assert (got[0] == 0).all() and (got[1:] == np.float32(gc_.MAX_RANGE)).all()
    free1, _ = gc_.spec(np.zeros((1, 1), np.uint8), (0.0, 0.0), 0.1)
    assert (check(capi, cuda, "1 x 1 free", x, free1, cfg1, geom, beams)[0] == np.float32(gc_.MAX_RANGE)).all()
    free, cfg = gc_.spec(np.zeros((30, 40), np.uint8), (-1.0, -1.0), 0.1)
    assert (check(capi, cuda, "all free", x, free, cfg, geom, beams)[0] == np.float32(gc_.MAX_RANGE)).all()


def scene():
    """Two races of two in a 64 x 48 room at 0.1 m with circles, segments and mates nearer and farther than the
    raster walls."""
    grid, cfg = gc_.room(64, 48, 0.1, (-3.2, -2.4), seed=4, blocks=5)
    x = np.array([[-0.6, -0.2, 0.1], [0.5, 0.1, 2.9], [-0.3, 0.6, -1.2], [0.4, -0.7, 1.7]])
    for p in x:
        i, j = int((p[0] + 3.2) / 0.1), int((p[1] + 2.4) / 0.1)
        assert not grid[j - 4:j + 5, i - 4:i + 5].any(), "the cars stand clear of the cells"
    circles = np.array([[1.2, 0.9, 0.2], [-1.5, -0.8, 0.15], [5.0, 1.0, 0.5], [-4.5, -3.0, 0.8], [0.0, 1.6, 0.1]])
    sg = np.array([[-1.0, 1.2, 0.2, 1.4], [1.5, -1.5, 1.6, 0.5], [-6.0, -4.0, 6.0, -4.0], [3.5, -1.0, 3.5, 1.0]])
    return x, grid, cfg, circles, sg


def test_other_obstacles_nearer_and_farther_with_noise(capi, cuda):
    x, grid, cfg, circles, sg = scene()
    geom = wc_.geometry(1080)
    kw = dict(static=circles, segments=sg, G=2)
    got, clean, own = check(capi, cuda, "noise-free", x, grid, cfg, geom, 1080, **kw)
    rest = walls_cast(capi, cuda, x, geom, 1080, circles, sg, 2, gc_.MAX_RANGE)
    assert (rest < own).mean() > 0.05 and (own < rest).mean() > 0.3, "both kinds win beams"
    for tick, base, setting in ((0, 0, nz.SETTINGS[0]), (5, 1000, nz.SETTINGS[2]), (1, 0, nz.SETTINGS[3])):
        noisy, _, _ = check(capi, cuda, f"tick {tick} car_base {base} {setting}", x, grid, cfg, geom, 1080,
                            setting=setting, tick=tick, base=base, **kw)
        assert (noisy != clean).mean() > 0.5, "rule Z2 runs on the new float"


def test_empty_map_is_the_noisy_cast(capi, cuda):
    x, _, cfg, circles, sg = scene()
    geom = wc_.geometry(1080)
    empty, ecfg = gc_.spec(np.zeros((0, 0), np.uint8), (cfg.origin_x, cfg.origin_y), cfg.resolution)
    for tick, setting in ((0, QUIET), (3, nz.SETTINGS[2])):
        got = grid_cast(capi, cuda, x, empty, ecfg, geom, 1080, static=circles, segments=sg, G=2, setting=setting,
                        tick=tick)
        want = noisy_cast(capi, cuda, x, circles, sg, 2, geom, 1080, nz.noise_config(capi, SEED, 0, setting), tick,
                          off=gc_.CENTER_OFFSET)
        same_bits(got, want, f"W * H == 0, tick {tick}")


def test_lds_window_and_global_fallback_agree(capi, cuda):
    """max_range 10 m at 0.1 m a cell is a square of 203 cells (1,421 words of LDS); 40 m is one of 803 (20,878
    words, above the kernel's 5,280): the map is read from global memory. In the closed room every beam returns
    below 10 m, so both scans hold the same values; and so does the fallback at 0.05 m a cell with hits beyond."""
    x, grid, cfg, circles, sg = scene()
    geom = wc_.geometry(1080)
    kw = dict(static=circles[:2], segments=sg[:2], G=2, setting=nz.SETTINGS[0], tick=2)
    lds, clean, _ = check(capi, cuda, "LDS window", x, grid, cfg, geom, 1080, **kw)
    assert (clean < np.float32(gc_.MAX_RANGE)).all()
    far, _, _ = check(capi, cuda, "global fallback", x, grid, cfg, geom, 1080, max_range=40.0, **kw)
    same_bits(far, lds, "the path taken does not show in the bits")
    fine, fcfg = gc_.room(64, 48, 0.05, (-1.6, -1.2), seed=4, blocks=5)
    fine[0, 20:30] = 0                              # a door: some beams leave and read max_range
    xf = gc_.free_poses(fine, fcfg, 4, 3)
    a, _, _ = check(capi, cuda, "0.05 m, LDS", xf, fine, fcfg, geom, 1080, max_range=10.0)
    b, _, _ = check(capi, cuda, "0.05 m, fallback", xf, fine, fcfg, geom, 1080, max_range=10.6)
    hit = a < np.float32(10.0)
    assert hit.any() and (~hit).any()
    same_bits(a[hit], b[hit], "returns")
    assert (b[~hit] == np.float32(10.6)).all()


def test_listed_mode(capi, cuda):
    grid, cfg = gc_.room(40, 30, 0.1, seed=3)
    x = gc_.free_poses(grid, cfg, 8, 12)
    geom = wc_.geometry(200)
    full, _, _ = check(capi, cuda, "all cars", x, grid, cfg, geom, 200, setting=nz.SETTINGS[2], tick=1)
    got = grid_cast(capi, cuda, x, grid, cfg, geom, 200, setting=nz.SETTINGS[2], tick=1, listed=[5, 2, 7, 0, 0, 0, 0, 0],
                    count=2)
    same_bits(got[[5, 2]], full[[5, 2]], "listed rows")
    assert (np.delete(got, [5, 2], axis=0) == SENTINEL).all(), "unlisted rows stay"


# ---- the clearance ----------------------------------------------------------------------------------------------

def grid_clearance(capi, cuda, x, grid, cfg, circles=None, segments=None, G=1, nearest=True):
    """f110qp_clearance_grid_dev on x [rows,B,3] between two guard rows -> (clearance [rows,B], nearest or None)."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    x = x[None] if x.ndim == 2 else x
    rows, B = x.shape[:2]
    Cn = 0 if circles is None else circles.shape[-2]
    wc = capi.default_world_config(num_circles=Cn)
    race = capi.default_race_config(group_size=G, center_offset=gc_.CENTER_OFFSET)
    wl = walls_of(capi, segments, B)
    out = torch.full((rows + 2, B), -7.0, dtype=torch.float64, device=cuda)
    near = torch.full((rows + 2, B), -7, dtype=torch.int32, device=cuda) if nearest else None
    capi.clearance_grid_dev(wc, race, capi.default_body_config(), wl, capi.grid_config_of(cfg), dev(cuda, x),
                            dev(cuda, circles) if Cn else None, dev(cuda, segments) if wl.num_segments else None,
                            dev(cuda, grid) if grid.size else None, out[1:rows + 1],
                            None if near is None else near[1:rows + 1])
    torch.cuda.synchronize(cuda)
    o = out.cpu().numpy()
    assert (o[0] == -7.0).all() and (o[-1] == -7.0).all(), "the guard rows stay"
    if near is None:
        return o[1:-1], None
    n = near.cpu().numpy()
    assert (n[0] == -7).all() and (n[-1] == -7).all()
    return o[1:-1], n[1:-1]


def check_clearance(capi, cuda, what, x, grid, cfg, circles=None, segments=None, G=1):
    got, near = grid_clearance(capi, cuda, x, grid, cfg, circles, segments, G)
    want, idx = workload.clearance_grid(x, circles, segments, grid, cfg, G, gc_.CENTER_OFFSET)
    same_bits(got, np.asarray(want).reshape(got.shape), what)
    assert (near == np.asarray(idx).reshape(near.shape)).all(), what
    return got, near


def _heading0(rng, n, lo, hi):
    return np.stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), np.zeros(n)], 1)


@pytest.mark.parametrize("reach", [0.0, 1.0])
def test_clearance_windows_at_every_border(capi, cuda, reach):
    """Heading 0. Poses over the whole room and a metre beyond each border: windows clipped at the left, right,
    lower and upper edge, windows beside the map (no cell), bodies over cells. G = 2, circles and segments too."""
    grid, cfg = gc_.room(40, 30, 0.1, (-1.0, -1.0), seed=5, reach=reach)
    rng = np.random.default_rng(3)
    x = _heading0(rng, 64, (-2.5, -2.5), (4.5, 3.5))
    circles, sg = np.array([[1.0, 0.5, 0.2], [9.0, 9.0, 1.0]]), np.array([[0.0, 0.0, 0.5, 0.5]])
    got, near = check_clearance(capi, cuda, f"reach {reach}", x, grid, cfg, circles, sg, 2)
    cell = near >= 2 + 2 + 1
    assert cell.sum() >= 8 and (got[cell] <= 0.0).any() and (~cell).any()
    for name, edge in (("left", x[:, 0] < -0.5), ("right", x[:, 0] > 2.5), ("lower", x[:, 1] < -0.5), ("upper", x[:, 1] > 1.5)):
        assert (cell[0] & edge).any() or reach == 0.0, name
    alone, an = check_clearance(capi, cuda, f"reach {reach}, the map alone", x, grid, cfg)
    assert ((an >= 1) | (an == -1)).all() and (alone[an >= 0] <= reach + 1e-12).mean() > 0.5


def test_clearance_centre_in_cell(capi, cuda):
    g = np.zeros((8, 8), np.uint8)
    g[4, 4] = 1
    grid, cfg = gc_.spec(g, (0.0, 0.0), 1.0, reach=0.5)   # a cell that holds the whole body
    x = np.array([[4.5 - gc_.CENTER_OFFSET, 4.5, 0.0], [4.05 - gc_.CENTER_OFFSET, 4.5, 0.0], [2.0, 4.5, 0.0]])
    got, near = check_clearance(capi, cuda, "centre in cell", x, grid, cfg)
    assert got[0, 0] == 0.0 and near[0, 0] == 1 + 4 * 8 + 4, "no edge is touched: the centre clause gives 0"
    assert got[0, 1] == 0.0, "over the cell's edge x = 4 with the centre inside: an edge passes through, 0 as well"
    assert np.isinf(got[0, 2]) and near[0, 2] == -1, "beyond reach: the window holds no occupied cell"


@pytest.mark.parametrize("rows", [3, 11])
def test_clearance_rows(capi, cuda, rows):
    """rows > 1: one pass of eight poses and a second of three."""
    grid, cfg = gc_.room(40, 30, 0.1, (-1.0, -1.0), seed=6)
    x = _heading0(np.random.default_rng(rows), rows * 6, (-1.0, -1.0), (3.0, 2.0)).reshape(rows, 6, 3)
    check_clearance(capi, cuda, f"{rows} rows", x, grid, cfg, None, None, 2)


def test_clearance_grid_stride(capi, cuda):
    grid, cfg = gc_.room(64, 48, 0.1, (-3.0, -2.0), seed=8, blocks=12, reach=0.5)
    x = _heading0(np.random.default_rng(1), 520, (-3.5, -2.5), (4.0, 3.3))
    got, near = check_clearance(capi, cuda, "520 cars", x, grid, cfg)
    assert (near >= 0).mean() > 0.3


def test_clearance_rotated_poses(capi, cuda):
    grid, cfg = gc_.room(40, 30, 0.1, (-1.0, -1.0), seed=5)
    rng = np.random.default_rng(9)
    x = np.stack([rng.uniform(-1.5, 3.5, 64), rng.uniform(-1.5, 2.5, 64), rng.uniform(-np.pi, np.pi, 64)], 1)
    got, _ = grid_clearance(capi, cuda, x, grid, cfg)
    want, _ = workload.clearance_grid(x, None, None, grid, cfg, 1, gc_.CENTER_OFFSET)
    both = np.isfinite(want)
    assert (np.isfinite(got[0]) == both).all() and both.sum() > 40
    err = np.abs(got[0][both] - want[both]).max()
    print(f"rotated poses: worst difference {err:.3e} m")
    assert err <= 1e-12


def test_empty_map_is_the_walls_clearance(capi, cuda):
    x, _, cfg, circles, sg = scene()
    empty, ecfg = gc_.spec(np.zeros((0, 0), np.uint8), (cfg.origin_x, cfg.origin_y), cfg.resolution)
    got, near = grid_clearance(capi, cuda, x, empty, ecfg, circles, sg, 2)
    want, wn = walls_clearance(capi, cuda, x, circles, sg, 2, off=gc_.CENTER_OFFSET)
    same_bits(got, want, "W * H == 0")
    assert (near == wn).all()
