"""Cases and second formulations for the raster LiDAR through the distance field (include/f110qp.h rule F1;
test_field_cast_cases.py on the CPU, test_gpu_field_cast.py on the device).

A case is a map and the cars that scan it: poses, a scan geometry and a max_range, so that the device runs exactly
what the CPU oracle ran. Beam directions come from sincos of a double, which never gives an exact (0, 1), (-1, 0) or
(s, s): the beams with gx == 0, with gy == 0 of either sign and the exact diagonals through lattice corners are RAW
beams, (origin, direction) pairs for the oracle alone. Beam 0 of a car at heading 0 with angle_min 0 is the exact
(1, 0), the one such beam the device can be given.

Second formulations kept here, each one beam at a time in plain Python floats:
  walk_field   rule F1 as it is worded: m single applications of rule G1's step 1 between two reads of d2;
  walk_reads   rule G1's walk with a counter on its reads of the map, the start cell's included.
"""
import functools
import math
from typing import NamedTuple

import field_cases as fc
import grid_cases as gc_
import numpy as np
import world_cases as wc_

from f110qp import workload

INT_MAX = fc.INT_MAX
OFF = gc_.LIDAR_OFFSET
QUARTER = 0.25          # a resolution that is exact in binary: cell boundaries are exact doubles
JUMP_VALUES = (1, 2, 4, 5, 9, 10, 16, 17)   # d2 at the start around which m = max(1, isqrt(d2 - 1)) changes
_OFFSETS = {1: (1, 0), 2: (1, 1), 4: (2, 0), 5: (2, 1), 9: (3, 0), 10: (3, 1), 16: (4, 0), 17: (4, 1)}


class Case(NamedTuple):
    name: str
    grid: np.ndarray      # [H, W] uint8
    cfg: object           # workload.GridSpec
    x: np.ndarray         # [B, 3] poses
    geom: tuple           # (angle_min, angle_increment, angle_max) float32
    beams: int
    max_range: float = gc_.MAX_RANGE


def lidar_at(lx, ly, yaw=0.0):
    """The pose whose LiDAR origin is exactly (lx, ly) in the cast's own arithmetic (a few ulps are tried)."""
    c, s = np.cos(yaw), np.sin(yaw)
    x, y = lx - OFF * c, ly - OFF * s
    for _ in range(4):
        x = x if x + OFF * c == lx else np.nextafter(x, x + (lx - (x + OFF * c)))
        y = y if y + OFF * s == ly else np.nextafter(y, y + (ly - (y + OFF * s)))
    assert x + OFF * c == lx and y + OFF * s == ly
    return np.array([x, y, yaw])


def turn(beams):
    """A full turn from angle 0: with heading 0, beam 0 is the exact (1, 0)."""
    return wc_._geom(0.0, 2.0 * np.pi / beams, beams)


def random_map(W, H, density, seed, keep=()):
    rng = np.random.default_rng(seed)
    g = (rng.random((H, W)) < density).astype(np.uint8)
    for i, j in keep:
        g[j, i] = 0
    return g


def field_of(grid):
    """d2 [H, W] int32 of a map: the definition on small maps, the separable pass on the others (test_field_cases.py
    holds the two to each other)."""
    g = np.asarray(grid)
    if g.size == 0:
        return np.zeros(g.shape, np.int32)
    if g.size <= fc.SMALL or g.shape[0] == 1:
        return workload.grid_distance(g)[0]
    return fc.separable(g)[0]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # 1 x 1, free and occupied; 1 x 9 and 9 x 1 with a cell at the end
    for name, g in (("1x1 free", np.zeros((1, 1))), ("1x1 occupied", np.ones((1, 1)))):
        grid, cfg = gc_.spec(g, (0.0, 0.0), QUARTER)
        out.append(Case(name, grid, cfg, np.stack([lidar_at(0.125, 0.125), lidar_at(0.0, 0.0)]), turn(16), 16))
    row = np.zeros((1, 9))
    row[0, 8] = 1
    grid, cfg = gc_.spec(row, (0.0, 0.0), QUARTER)
    out.append(Case("1x9", grid, cfg, np.stack([lidar_at(0.125, 0.125), lidar_at(0.25, 0.0), lidar_at(1.0, 0.2)]),
                    turn(16), 16))
    grid, cfg = gc_.spec(row.T, (0.0, 0.0), QUARTER)
    out.append(Case("9x1", grid, cfg, np.stack([lidar_at(0.125, 0.125, 0.5 * np.pi), lidar_at(0.2, 1.0)]), turn(16), 16))
    # 33 x 40 at three densities, 0.05 m (inexact in binary), a negative origin
    for density in (0.0, 0.01, 0.30):
        g = random_map(33, 40, density, 11, keep=((16, 20), (3, 3)))
        grid, cfg = gc_.spec(g, (-1.3, -0.7), 0.05)
        x = np.concatenate([gc_.free_poses(grid, cfg, 4, 5), [lidar_at(-1.3 + 16.5 * 0.05, -0.7 + 20.5 * 0.05)]])
        out.append(Case(f"33x40 at {int(density * 100)}%", grid, cfg, x, wc_.geometry(120), 120))
    # one cell placed so that d2 at the start is each value around which m changes
    for d in JUMP_VALUES:
        g = np.zeros((24, 24))
        a, b = _OFFSETS[d]
        g[8 + b, 8 + a] = 1
        grid, cfg = gc_.spec(g, (0.0, 0.0), QUARTER)
        x = np.stack([lidar_at(8.5 * QUARTER, 8.5 * QUARTER), lidar_at(8.0 * QUARTER, 8.5 * QUARTER),
                      lidar_at(8.0 * QUARTER, 8.0 * QUARTER), lidar_at(8.3 * QUARTER, 8.9 * QUARTER, 0.7)])
        out.append(Case(f"d2 {d} at the start", grid, cfg, x, turn(64), 64))
    # no occupied cell: d2 is INT_MAX, one jump takes the whole budget and leaves the map inside it
    grid, cfg = gc_.spec(np.zeros((30, 40)), (-1.0, -1.0), 0.1)
    out.append(Case("empty map", grid, cfg, np.stack([lidar_at(0.0, 0.0), lidar_at(2.95, 1.95, 2.0)]), turn(48), 48))
    # a wall of cells that touch at corners only
    g = np.zeros((20, 20))
    g[np.arange(2, 18), np.arange(2, 18)] = 1
    grid, cfg = gc_.spec(g, (0.0, 0.0), QUARTER)
    x = np.stack([lidar_at(1.125, 3.625), lidar_at(3.625, 1.125, 1.0), lidar_at(1.0, 3.5), lidar_at(4.9, 0.1, 2.5)])
    out.append(Case("corner wall", grid, cfg, x, turn(180), 180))
    # 65 x 67 with a cell in each corner
    g = np.zeros((67, 65))
    g[0, 0] = g[0, -1] = g[-1, 0] = g[-1, -1] = 1
    grid, cfg = gc_.spec(g, (-1.0, 2.0), 0.1)
    x = np.stack([lidar_at(-1.0 + 3.25, 2.0 + 3.35), lidar_at(-1.0 + 0.15, 2.0 + 0.05), lidar_at(-1.0 + 6.3, 2.0 + 6.6, 3.0)])
    out.append(Case("65x67 corners", grid, cfg, x, wc_.geometry(360), 360))
    # a quarter-metre lattice: starts on a boundary and on a lattice corner, a max_range that ends inside the first
    # jump (d2 = 16 at the start: three cells, t = 0.625) and one that equals the hit boundary's parameter (0.875)
    g = np.zeros((12, 16))
    g[4, 8] = g[9, 3] = 1
    grid, cfg = gc_.spec(g, (0.0, 0.0), QUARTER)
    x = np.stack([lidar_at(1.125, 1.125), lidar_at(1.0, 1.125), lidar_at(1.0, 1.0), lidar_at(2.125, 1.125),
                  lidar_at(2.25, 1.125), lidar_at(2.0, 1.125)])
    for mr in (gc_.MAX_RANGE, 0.5, 0.875):
        out.append(Case(f"lattice, max_range {mr}", grid, cfg, x, turn(64), 64, mr))
    # starts that see nothing: outside the map, NaN, +inf and -inf
    bad = np.array([[-0.5 - OFF, 1.125, 0.0], [np.nan, 1.0, 0.0], [1.0, np.nan, 0.0], [np.inf, 1.0, 0.0],
                    [1.0, -np.inf, 0.0], [1.0, 1.0, np.nan], [100.0, 1.0, 0.0]])
    out.append(Case("starts without a map", grid, cfg, bad, turn(16), 16))
    # 1 x 32,768 with one cell at the far end: one jump of 32,766 cells, then a step; the budget is W + H + 2
    row = np.zeros((1, 32768))
    row[0, -1] = 1
    grid, cfg = gc_.spec(row, (0.0, 0.0), QUARTER)
    out.append(Case("1x32768", grid, cfg, np.stack([lidar_at(0.125, 0.125), lidar_at(4000.0, 0.0625)]), turn(8), 8, 9000.0))
    return tuple(out)


def case_beams(c):
    """(ox, oy [B, 1], dx, dy [B, R]) of a case as the cast builds them (numpy's sincos)."""
    with np.errstate(invalid="ignore"):
        return gc_.beams_of(c.x, c.geom, c.beams, OFF)


class Raw(NamedTuple):
    name: str
    grid: np.ndarray
    cfg: object
    ox: np.ndarray
    oy: np.ndarray
    dx: np.ndarray
    dy: np.ndarray
    max_range: float = gc_.MAX_RANGE


@functools.lru_cache(maxsize=None)
def raw_cases():
    """Beams no sincos gives: the four axis directions (gx == 0, gy == 0, both signs) and the four exact diagonals,
    from cell centres, cell boundaries and lattice corners, where every step of a diagonal is the x-first tie."""
    s = math.sqrt(0.5)
    dirs = np.array([(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (1.0, -0.0), (-0.0, -1.0),
                     (s, s), (-s, s), (s, -s), (-s, -s)])
    out = []
    maps = {c.name: c for c in cases()}
    for name, starts in (("corner wall", ((1.0, 3.5), (1.125, 3.625), (3.5, 1.0), (4.0, 0.25), (0.25, 4.0), (2.5, 2.75))),
                         ("d2 17 at the start", ((2.0, 2.0), (2.125, 2.125), (2.0, 2.125), (3.5, 1.75))),
                         ("lattice, max_range 10.0", ((1.0, 1.0), (1.125, 1.125), (2.25, 1.25), (0.0, 0.0))),
                         ("1x9", ((0.0, 0.0), (0.125, 0.125), (1.0, 0.25)))):
        c = maps[name]
        st = np.array(starts)
        out.append(Raw(f"{name}, exact beams", c.grid, c.cfg, st[:, :1], st[:, 1:], dirs[None, :, 0], dirs[None, :, 1]))
    g = random_map(33, 40, 0.30, 11, keep=((16, 20), (3, 3)))
    grid, cfg = gc_.spec(g, (0.0, 0.0), QUARTER)
    free = np.argwhere(g == 0)[::37]
    st = np.concatenate([free[:, ::-1] * QUARTER, (free[:, ::-1] + 0.5) * QUARTER])
    out.append(Raw("33x40 at 30%, exact beams", grid, cfg, st[:, :1], st[:, 1:], dirs[None, :, 0], dirs[None, :, 1]))
    c = maps["empty map"]   # leaves the map in the middle of the one jump, along an axis and a diagonal
    st = np.array([(0.05, 0.05), (0.0, 0.0)])
    out.append(Raw("empty map, exact beams", c.grid, c.cfg, st[:, :1], st[:, 1:], dirs[None, :, 0], dirs[None, :, 1]))
    c = maps["1x32768"]
    out.append(Raw("1x32768, exact beams", c.grid, c.cfg, np.array([[0.125], [8191.75]]), np.array([[0.125], [0.0]]),
                   dirs[None, :, 0], dirs[None, :, 1], 9000.0))
    return tuple(out)


def _start(ox, oy, cfg, W, H):
    px, py = (ox - cfg.origin_x) / cfg.resolution, (oy - cfg.origin_y) / cfg.resolution
    if not (px >= 0.0 and px < W and py >= 0.0 and py < H):
        return None
    return px, py, int(math.floor(px)), int(math.floor(py))


class _Walk:
    """Rule G1's state and its step 1 (the move alone) for one beam."""

    def __init__(self, px, py, ix, iy, dx, dy, res):
        self.px, self.py, self.ix, self.iy, self.dx, self.dy = px, py, ix, iy, dx, dy
        self.gx, self.gy = dx / res, dy / res
        self.sx, self.sy = (1 if dx > 0.0 else -1), (1 if dy > 0.0 else -1)
        self.tx = self._bound(ix, px, dx, self.gx) if (dx > 0.0 or dx < 0.0) else math.inf
        self.ty = self._bound(iy, py, dy, self.gy) if (dy > 0.0 or dy < 0.0) else math.inf

    @staticmethod
    def _bound(i, p, d, g):
        # g == 0 is met only behind a move whose t = +inf has already ended the walk
        return (float(i + 1 if d > 0.0 else i) - p) / g if g != 0.0 else math.nan

    def move(self):
        if self.tx <= self.ty:
            t = self.tx
            self.ix += self.sx
            self.tx = self._bound(self.ix, self.px, self.dx, self.gx)
        else:
            t = self.ty
            self.iy += self.sy
            self.ty = self._bound(self.iy, self.py, self.dy, self.gy)
        return t


def walk_field(ox, oy, dx, dy, d2, cfg, limit):
    """Rule F1 for one beam, the m moves taken singly -> (range, visits)."""
    H, W = d2.shape
    st = _start(ox, oy, cfg, W, H)
    if st is None:
        return limit, 0
    D, visits = int(d2[st[3], st[2]]), 1
    if D <= 0:
        return 0.0, visits
    w = _Walk(*st, dx, dy, cfg.resolution)
    left = W + H + 2
    while left > 0:
        m = min(max(1, math.isqrt(D - 1)), left)
        left -= m
        for _ in range(m):
            t = w.move()
        if not t <= limit:
            break
        if w.ix < 0 or w.ix >= W or w.iy < 0 or w.iy >= H:
            break
        D = int(d2[w.iy, w.ix])
        visits += 1
        if D <= 0:
            return t + 0.0, visits
    return limit, visits


def walk_reads(ox, oy, dx, dy, grid, cfg, limit):
    """Rule G1 for one beam with a counter on the cells it reads, the start cell included -> (range, reads)."""
    H, W = grid.shape
    st = _start(ox, oy, cfg, W, H)
    if st is None:
        return limit, 0
    reads = 1
    if grid[st[3], st[2]]:
        return 0.0, reads
    w = _Walk(*st, dx, dy, cfg.resolution)
    for _ in range(W + H + 2):
        t = w.move()
        if not t <= limit:
            break
        if w.ix < 0 or w.ix >= W or w.iy < 0 or w.iy >= H:
            break
        reads += 1
        if grid[w.iy, w.ix]:
            return t + 0.0, reads
    return limit, reads


def each_beam(fn, ox, oy, dx, dy, *rest):
    """fn over the broadcast beams -> (ranges float64, counts int64) of the broadcast shape."""
    ox, oy, dx, dy = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (ox, oy, dx, dy)))
    r, n = np.empty(dx.shape), np.empty(dx.shape, np.int64)
    for k in np.ndindex(dx.shape):
        r[k], n[k] = fn(float(ox[k]), float(oy[k]), float(dx[k]), float(dy[k]), *rest)
    return r, n


TRACK_POSES, TRACK_BEAMS, TRACK_EVERY = 24, 1080, 4


@functools.lru_cache(maxsize=None)
def track():
    """make_grid_world(5, 40, 0.05), its field, 24 seeded free poses and every fourth beam of the 1,080."""
    grid, cfg = workload.make_grid_world(5, 40, 0.05)
    x = gc_.free_poses(grid, cfg, TRACK_POSES, 2024)
    ox, oy, dx, dy = gc_.beams_of(x, wc_.geometry(TRACK_BEAMS), TRACK_BEAMS, OFF)
    return grid, cfg, fc.separable(grid)[0], x, (ox, oy, dx[:, ::TRACK_EVERY], dy[:, ::TRACK_EVERY])
