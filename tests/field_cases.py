"""The distance field's CPU side (test_field_cases.py, test_gpu_field.py): the maps and the poses whose device
results are compared with the numpy oracle (workload.grid_distance, grid_inflate, grid_lookup), a second
formulation of the transform (separable, two passes), and the comparison.

Comparison: bit for bit on every output. d2, nearest and the inflated map are integers; a distance is one correctly
rounded root times the resolution, or +inf, or the one NaN 0x7ff8000000000000, compared by its bits. There is no
tolerance and no skip rule.
"""
import functools

import numpy as np
from mc_cases import check, frozen, same  # noqa: F401  (the comparison is the Monte Carlo outcomes')

from f110qp import workload

INT_MAX = int(np.iinfo(np.int32).max)
LOOKUP_GRID = 2048   # field_lookup_grid's cap: workgroups of 256 poses
RES = 0.05
SIZES = (1, 2, 63, 64, 65, 257)


def separable(grid):
    """Rules D1 and D2 by their stated consequence: along a row the nearer occupied row-neighbour, the smaller p on a
    tie; down a column the least q among the rows that reach the minimum. -> (d2, nearest) int32. H x H x W work."""
    g = np.asarray(grid) != 0
    H, W = g.shape
    big = np.int64(1) << 40
    i = np.broadcast_to(np.arange(W, dtype=np.int64), (H, W))
    left = np.maximum.accumulate(np.where(g, i, -1), axis=1)
    right = np.minimum.accumulate(np.where(g, i, big)[:, ::-1], axis=1)[:, ::-1]
    p = np.where(left < 0, np.where(right == big, -1, right),
                 np.where((right == big) | (i - left <= right - i), left, right))
    dx2 = np.where(p < 0, big, (i - p) ** 2)                       # [q, i]
    q = np.arange(H, dtype=np.int64)
    d2 = np.empty((H, W), np.int64)
    bq = np.empty((H, W), np.int64)
    for j in range(H):
        v = dx2 + ((j - q) ** 2)[:, None]
        bq[j] = np.argmin(v, axis=0)                               # the first minimum: the least q
        d2[j] = v[bq[j], np.arange(W)]
    none = d2 >= big
    bp = p[bq, i]
    return (np.where(none, INT_MAX, d2).astype(np.int32), np.where(none, -1, bq * W + bp).astype(np.int32))


def loop(grid):
    """The definition as a Python loop (small maps): the occupied cells in linear-index order, a strict less."""
    g = np.asarray(grid)
    H, W = g.shape
    d2, near = np.full((H, W), INT_MAX, np.int32), np.full((H, W), -1, np.int32)
    occ = [(q, p) for q in range(H) for p in range(W) if g[q, p]]
    for j in range(H):
        for i in range(W):
            for q, p in occ:
                v = (i - p) ** 2 + (j - q) ** 2
                if v < d2[j, i]:
                    d2[j, i], near[j, i] = v, q * W + p
    return d2, near


class MapCase:
    """grid [H, W] uint8 with its config; expect: {(i, j): (d2, nearest)} values that the case is about."""

    def __init__(self, name, grid, expect=None, oracle="definition", resolution=RES, origin=(0.0, 0.0)):
        self.name, self.how = name, oracle
        self.grid = np.ascontiguousarray(grid, np.uint8)
        self.grid.setflags(write=False)
        self.expect = dict(expect or {})
        self.cfg = workload.GridSpec(self.W, self.H, origin[0], origin[1], resolution, 1.0)
        self._oracle = None

    H = property(lambda self: self.grid.shape[0])
    W = property(lambda self: self.grid.shape[1])

    def radii(self):
        """0, the resolution exactly, resolution sqrt(2) as rule D3 computes it, and a large one."""
        r = np.float64(self.cfg.resolution)
        return (0.0, float(r), float(r * np.sqrt(np.float64(2))), 1e9)

    def oracle(self):
        """dict of d2, nearest, and inflated_k for the radii: computed once, not to be written to."""
        if self._oracle is None:
            d2, near = (separable if self.how == "separable" else workload.grid_distance)(self.grid)
            o = dict(d2=d2, nearest=near)
            for k, r in enumerate(self.radii()):
                o[f"inflated_{k}"] = workload.grid_inflate(d2, self.cfg, r)
            for (i, j), (v, n) in self.expect.items():
                assert (int(d2[j, i]), int(near[j, i])) == (v, n), (self.name, i, j, d2[j, i], near[j, i], v, n)
            self._oracle = frozen(o)
        return self._oracle

    def check(self, got, what=""):
        check(self.name, got, self.oracle(), what)


def cells(W, H, occupied):
    g = np.zeros((H, W), np.uint8)
    for i, j in occupied:
        g[j, i] = 1
    return g


def random_map(seed, W, H, density):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


def tiny_cases():
    return [MapCase("1x1 occupied", np.ones((1, 1)), {(0, 0): (0, 0)}),
            MapCase("1x1 free", np.zeros((1, 1)), {(0, 0): (INT_MAX, -1)})]


def line_cases():
    """Single rows and single columns, so that one phase is degenerate; about one cell in seven occupied, and for
    the longer ones a free stretch at each end so that both carries travel."""
    out = []
    for n in SIZES:
        v = (np.random.default_rng(100 + n).random(n) < 0.15).astype(np.uint8)
        if n >= 63:
            v[:5], v[-9:], v[7], v[n // 2] = 0, 0, 1, 1
        out += [MapCase(f"1x{n} row", v[None, :]), MapCase(f"{n}x1 column", v[:, None])]
    return out


def uniform_cases():
    W, H = 65, 67
    full = MapCase("full 65x67", np.ones((H, W)), {(i, j): (0, j * W + i) for i, j in ((0, 0), (64, 66), (13, 40))})
    return [MapCase("empty 65x67", np.zeros((H, W)), {(0, 0): (INT_MAX, -1), (64, 66): (INT_MAX, -1)}), full]


def corner_cases():
    W, H = 65, 67
    out = []
    for ci, cj in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        far = (W - 1 - ci, H - 1 - cj)
        out.append(MapCase(f"corner ({ci}, {cj})", cells(W, H, [(ci, cj)]),
                           {far: (64 * 64 + 66 * 66, cj * W + ci), (ci, cj): (0, cj * W + ci)}))
    return out


def tie_cases():
    """Each tie by its value in nearest: the least linear index q W + p of the minimisers."""
    return [MapCase("tie along x", cells(5, 5, [(0, 2), (4, 2)]), {(2, 2): (4, 2 * 5 + 0)}),
            MapCase("tie along y", cells(5, 5, [(2, 0), (2, 4)]), {(2, 2): (4, 0 * 5 + 2)}),
            MapCase("tie on the diagonal", cells(5, 5, [(0, 0), (4, 4)]), {(2, 2): (8, 0)}),
            MapCase("tie on the other diagonal", cells(5, 5, [(4, 0), (0, 4)]), {(2, 2): (8, 4)}),
            MapCase("four equidistant", cells(5, 5, [(2, 0), (0, 2), (4, 2), (2, 4)]), {(2, 2): (4, 2)}),
            # the same distance above and below, five to seven rows away: past the first steps of an outward walk
            MapCase("tie along y, far", cells(7, 13, [(3, 0), (3, 12)]), {(3, 6): (36, 3)}),
            MapCase("tie along y, far, off the column", cells(9, 15, [(6, 2), (2, 12)]),
                    {(4, 7): (4 + 25, 2 * 9 + 6)}),
            # a row tie inside a column tie: rows 1 and 5 both reach 4 + 4 through either of their two cells
            MapCase("row ties inside a column tie", cells(5, 7, [(0, 1), (4, 1), (0, 5), (4, 5)]), {(2, 3): (8, 5)})]


def early_stop_cases():
    """The row-nearest is close but a cell straight above is closer; and the only occupied cell is 300 rows away in
    another column."""
    return [MapCase("above beats the row", cells(9, 9, [(1, 4), (4, 2)]), {(4, 4): (4, 2 * 9 + 4), (2, 4): (1, 37)}),
            MapCase("below beats the row", cells(9, 9, [(1, 4), (4, 6)]), {(4, 4): (4, 6 * 9 + 4)}),
            MapCase("300 rows away", cells(5, 301, [(3, 300)]), {(1, 0): (4 + 90000, 300 * 5 + 3)}),
            MapCase("300 rows up", cells(5, 301, [(3, 0)]), {(1, 300): (4 + 90000, 3)})]


def checker_cases():
    j, i = np.mgrid[0:17, 0:70]
    return [MapCase("checkerboard", (i + j) % 2 == 0), MapCase("checkerboard, odd", (i + j) % 2 == 1),
            MapCase("checkerboard of 3x3 blocks", ((i // 3) + (j // 3)) % 2 == 0)]


def random_cases():
    return [MapCase(f"random 129x200 at {d}", random_map(300 + k, 200, 129, d))
            for k, d in enumerate((0.001, 0.05, 0.5))]


def long_cases():
    """The largest single-axis value, 32,767^2: one occupied cell at an end of the longest row and column."""
    n, out = 32768, []
    for end in (0, n - 1):
        v = np.zeros(n, np.uint8)
        v[end] = 1
        far = n - 1 - end
        out += [MapCase(f"1x{n}, cell {end}", v[None, :], {(far, 0): (32767 ** 2, end)}),
                MapCase(f"{n}x1, cell {end}", v[:, None], {(0, far): (32767 ** 2, end)})]
    return out


def world_case():
    """workload.make_grid_world(5, 40, 0.05): 584 x 344. The definition costs cells x occupied cells here, so this
    case's oracle is the separable formulation (test_field_cases.py holds the two together on the small maps)."""
    grid, cfg = workload.make_grid_world(5, 40, 0.05)
    assert grid.shape == (344, 584), grid.shape
    return MapCase("grid world 584x344", grid, oracle="separable", resolution=cfg.resolution,
                   origin=(cfg.origin_x, cfg.origin_y))


@functools.lru_cache(maxsize=None)
def map_cases():
    return tuple(tiny_cases() + line_cases() + uniform_cases() + corner_cases() + tie_cases() + early_stop_cases()
                 + checker_cases() + random_cases() + long_cases() + [world_case()])


SMALL = 5000  # cells: what the Python loop and the H x H x W pass are run on in test_field_cases.py


def inflate_case():
    """One occupied cell in the middle of 7 x 7: radius 0 gives the cell, the resolution its four neighbours too,
    resolution sqrt(2) the diagonals too, a large radius everything."""
    return MapCase("one cell of 7x7", cells(7, 7, [(3, 3)])), (1, 5, 9, 49)


# ---- lookups ---------------------------------------------------------------------------------------------------

class LookupCase:
    """Poses x [rows, B, 3] on a map with its field."""

    def __init__(self, name, m, x):
        self.name, self.map = name, m
        self.x = np.ascontiguousarray(x, np.float64)
        self.x.setflags(write=False)
        self._oracle = None

    rows = property(lambda self: self.x.shape[0])
    B = property(lambda self: self.x.shape[1])

    def oracle(self):
        if self._oracle is None:
            f = self.map.oracle()
            dist, cell = workload.grid_lookup(self.x, f["d2"], f["nearest"], self.map.cfg)
            self._oracle = frozen(dict(dist=dist, cell=cell))
        return self._oracle

    def check(self, got, what=""):
        check(self.name, got, self.oracle(), what)


NAN_BITS = np.uint64(0x7FF8000000000000)


def lookup_map(resolution, origin):
    return MapCase(f"lookup map at {resolution} from {origin}", random_map(400, 65, 67, 0.05), resolution=resolution,
                   origin=origin)


def edge_points(cfg):
    """Points on cell boundaries and on the map's outer edges, and the doubles next to them on either side; -0.0,
    NaN and the infinities in either coordinate; headings of every sort (rule D4 does not read them)."""
    W, H, r = cfg.width, cfg.height, cfg.resolution
    xs = [cfg.origin_x + k * r for k in (0, 1, 2, 31.5, W - 1, W)]
    ys = [cfg.origin_y + k * r for k in (0, 1, 33, H - 1, H)]
    xs = [v for a in xs for v in (np.nextafter(a, -np.inf), a, np.nextafter(a, np.inf))]
    ys = [v for a in ys for v in (np.nextafter(a, -np.inf), a, np.nextafter(a, np.inf))]
    odd = [-0.0, 0.0, np.nan, np.inf, -np.inf, -5e-324, 1e300, -1e300]
    mid = (cfg.origin_x + 10.5 * r, cfg.origin_y + 20.5 * r)
    pts = [(a, b) for a in xs for b in ys] + [(a, mid[1]) for a in odd] + [(mid[0], b) for b in odd]
    pts += [(a, b) for a in odd[:5] for b in odd[:5]]
    head = np.resize(np.array([0.0, 1.0, np.nan, np.inf, -3.0]), len(pts))
    return np.concatenate([np.array(pts, np.float64), head[:, None]], axis=1)


def lookup_cases():
    """An exact lattice (quarter-metre cells from an origin that is no multiple of the cell: x = origin + k / 4 is
    exact, so px is the integer k and the boundary points sit on their boundaries); 0.07 m cells from an inexact
    origin; and the origin (0, 0), where -0.0 is a coordinate of the map's own corner (px = -0.0 is inside)."""
    out = []
    for res, origin in ((0.25, (-2.125, 1.0625)), (0.07, (-1.234, 0.517)), (0.1, (0.0, 0.0))):
        m = lookup_map(res, origin)
        x = edge_points(m.cfg)
        out.append(LookupCase(f"edges at {res}", m, x[None]))
    m = out[0].map
    px = (out[0].x[0, :, 0] - m.cfg.origin_x) / m.cfg.resolution
    assert (px == 0.0).any() and (px == m.W).any() and (px == 1.0).any(), "the lattice points sit on the boundaries"
    got = out[2].oracle()
    on = (out[2].x[0, :, 0] == 0.0) & np.signbit(out[2].x[0, :, 0]) & (out[2].x[0, :, 1] == 0.0)
    assert on.any() and not np.isnan(got["dist"][0][on]).any(), "-0.0 is inside the map whose origin is 0"
    return out


def stride_case():
    """rows x B past the lookup's grid cap of 2,048 workgroups x 256 poses: the first threads take a second pose."""
    m = lookup_map(0.07, (-1.234, 0.517))
    rows, B = 9, 58300
    assert rows * B > LOOKUP_GRID * 256
    rng = np.random.default_rng(500)
    x = np.stack([m.cfg.origin_x + rng.uniform(-1.0, m.W + 1.0, (rows, B)) * m.cfg.resolution,
                  m.cfg.origin_y + rng.uniform(-1.0, m.H + 1.0, (rows, B)) * m.cfg.resolution,
                  rng.uniform(-3.0, 3.0, (rows, B))], axis=2)
    return LookupCase("past the grid cap", m, x)
