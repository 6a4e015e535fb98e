"""The race standings' CPU side (test_standings_cases.py, test_gpu_standings.py): the cases whose device results
are compared with the numpy oracle (workload.path_lengths, progress, standings), and the comparison.

Comparison: bit for bit on every output. Both sides run the same sequence of IEEE fp64 + - x / sqrt, every one
correctly rounded and none fused, on the same input bits (the path's lengths are the caller's, so the device
reads the oracle's cum); no sincos is involved. A NaN compares equal to a NaN whatever its payload, everything
else by its bits, so a zero's sign counts. There is no tolerance and no skip rule.

Paths with exactly representable coordinates (rectangle) make the ties exact: a pose midway between two
opposite sides is at the same d2 from both, and the lowest index must win.
"""
import numpy as np

from f110qp import workload

INT_MIN = np.iinfo(np.int32).min


def same(got, want):
    """Equal bits, or NaN on both sides."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool((got == want).all())
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.int64)[~nan] == want.view(np.int64)[~nan]).all())


class StandingsCase:
    """Poses x [rows, B, 3] in races of G on the closed path wp [W, 2]. ranked False: the path's length is not a
    positive number (a non-finite waypoint), so only the projection is defined."""

    def __init__(self, name, x, wp, G=1, ranked=True):
        self.name, self.G, self.ranked = name, int(G), ranked
        self.x = np.ascontiguousarray(x, np.float64)
        if self.x.ndim == 2:
            self.x = self.x[None]
        self.wp = np.ascontiguousarray(wp, np.float64)
        self._oracle = None

    rows = property(lambda self: self.x.shape[0])
    B = property(lambda self: self.x.shape[1])
    W = property(lambda self: self.wp.shape[0])

    @property
    def cum(self):
        return workload.path_lengths(self.wp)

    def oracle(self):
        """dict of seg, s, lateral and, when ranked, dist, lap, rank: computed once, not to be written to."""
        if self._oracle is None:
            seg, s, lat = workload.progress(self.x, self.wp)
            o = dict(seg=seg, s=s, lateral=lat)
            if self.ranked:
                o["dist"], o["lap"], o["rank"] = workload.standings(s, self.cum[-1], self.G)
            for v in o.values():
                v.setflags(write=False)
            self._oracle = o
        return self._oracle

    def check(self, got, what=""):
        """got: a dict of device results (an absent or None entry is an optional output left out)."""
        want = self.oracle()
        for k, w in want.items():
            g = got.get(k)
            if g is None:
                continue
            g = np.asarray(g).reshape(w.shape)
            if not same(g, w):
                bad = np.argwhere(~((g == w) | (np.isnan(g.astype(float)) & np.isnan(w.astype(float)))))
                r, b = bad[0] if len(bad) else (0, 0)
                raise AssertionError(f"{self.name} {what}: {k} differs at {len(bad)} of {w.size} (signed zeros apart), "
                                     f"first [{r},{b}] got {g[r, b]!r} want {w[r, b]!r}, pose {self.x[r, b]}")


# ---- paths ---------------------------------------------------------------------------------------------------

def ellipse(W):
    """W >= 3 waypoints of the shipped ellipse; W = 2 a there-and-back path whose two segments tie everywhere."""
    if W == 2:
        return np.array([[0.0, 0.0], [3.0, 1.0]])
    return workload.track_waypoints(n=W)


def rectangle(w=100, h=60):
    """The w x h rectangle in unit steps from (0, 0), counter-clockwise: 2 (w + h) integer waypoints. Segment k
    of the bottom side runs from (k, 0); the top side's segment from (k + 1, h) to (k, h) is w + h + (w - 1 - k)."""
    pts = [(k, 0) for k in range(w)] + [(w, k) for k in range(h)] + [(w - k, h) for k in range(w)]
    pts += [(0, h - k) for k in range(h)]
    return np.array(pts, np.float64)


def poses(wp, rows, B, seed, spread=1.0):
    """rows x B poses scattered `spread` metres (normal) around seeded finite waypoints, any heading."""
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero(np.isfinite(wp).all(axis=1))
    at = wp[rng.choice(ok, (rows, B))]
    return np.concatenate([at + rng.normal(0.0, spread, (rows, B, 2)), rng.uniform(-np.pi, np.pi, (rows, B, 1))], 2)


# ---- cases ---------------------------------------------------------------------------------------------------

TILE = 256   # segments per tile step of progress_kernel (one per thread)
PASS = 8     # poses per pass
GRID = 1024  # progress_grid's cap: a larger batch strides

TILE_W = (2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
PASS_ROWS = (1, PASS, PASS + 1, 2 * PASS + 1)
BATCHES = (1, 7, 300, GRID + 6)
GROUPS = (1, 2, TILE + 2)


def tile_case(W, rows=3):
    wp = ellipse(W)
    return StandingsCase(f"W={W}", poses(wp, rows, 6, 100 + W), wp, 2)


def rows_case(rows):
    wp = ellipse(37)
    return StandingsCase(f"rows={rows}", poses(wp, rows, 5, 200 + rows), wp, 5)


def batch_case(B):
    wp = ellipse(5 if B > GRID else 37)
    return StandingsCase(f"B={B}", poses(wp, 2 if B > GRID else 3, B, 300 + B), wp, 1)


def group_case(G):
    """Two races of G; in each, cars 3 and G - 1 stand on car 0's pose all along: equal dist, ranked by index."""
    wp = ellipse(37)
    x = poses(wp, 3, 2 * G, 400 + G, spread=0.5)
    for g in (0, G):
        for twin in {min(3, G - 1), G - 1}:
            x[:, g + twin] = x[:, g]
    return StandingsCase(f"G={G}", x, wp, G)


def vertex_case():
    """Poses exactly on every vertex of a 12-point ellipse and of the rectangle, and exactly on segments of the
    rectangle (d2 == 0 at quarter points, which are exact)."""
    e, r = ellipse(12), rectangle(20, 12)
    on = np.concatenate([r, r[:40] + (np.roll(r, -1, 0) - r)[:40] * 0.25])
    z = lambda p: np.concatenate([p, np.zeros((len(p), 1))], 1)  # noqa: E731
    return [StandingsCase("on the ellipse's vertices", z(e), e, 1),
            StandingsCase("on the rectangle's vertices and segments", z(on), r, 1)]


def tie_case():
    """Midway between the rectangle's long sides: (k + 0.5, 30) ties bottom segment k with the top segment above
    it (another wave of the tile), (k, 30) ties four segments; both squares are exact. With the path's list
    rotated the pairs fall into different tiles."""
    r = rectangle()
    k = np.arange(35, 65, 3, dtype=np.float64)  # nearer to the long sides than to the short ones
    p = np.concatenate([np.stack([k + 0.5, np.full_like(k, 30.0)], 1), np.stack([k[1:], np.full_like(k[1:], 30.0)], 1)])
    x = np.concatenate([p, np.zeros((len(p), 1))], 1)
    return [StandingsCase("ties on the rectangle", x, r, 1), StandingsCase("ties, list rotated", x, np.roll(r, 130, 0), 1)]


def duplicate_case():
    """Waypoint 10 twice (segment 10 has ee == 0), poses around it and one exactly on it."""
    wp = ellipse(40)
    wp = np.concatenate([wp[:11], wp[10:]])
    x = poses(wp[8:14], 2, 9, 51, spread=0.6)
    x[0, 0, :2] = wp[10]
    return StandingsCase("duplicated waypoint", x, wp, 3)


def bad_waypoint_cases():
    """One coordinate of waypoint 7 NaN, +inf or -inf: segments 6 and 7 can never be chosen."""
    out = []
    for k, v in ((0, np.nan), (1, np.nan), (0, np.inf), (1, -np.inf)):
        wp = ellipse(40)
        x = poses(wp[3:12], 2, 12, 61 + k, spread=0.4)
        wp[7, k] = v
        out.append(StandingsCase(f"waypoint 7 [{k}] = {v}", x, wp, 1, ranked=False))
    return out


def bad_pose_case(G):
    """G = 1: every kind of non-finite pose alone. G = 4: one inside each race (never the race's first car), and a
    NaN heading, which is not read."""
    wp = ellipse(40)
    bad = [(0, np.nan), (1, np.nan), (0, np.inf), (1, -np.inf), (0, -np.inf), (1, np.inf)]
    B = len(bad) * G
    x = poses(wp, 3, B, 70 + G, spread=0.5)
    for i, (k, v) in enumerate(bad):
        car = i * G + (0 if G == 1 else 1 + i % (G - 1))
        x[i % 2 if G > 1 else 0, car, k] = v  # in a race: from row 0 on, or from row 1 on
    x[:, 0, 2] = np.nan
    return StandingsCase(f"non-finite poses, G={G}", x, wp, G)


def far_case():
    wp = ellipse(40)
    x = poses(wp, 2, 8, 81)
    x[..., :2] += np.array([[1000.0, 0.0], [0.0, -1000.0], [1000.0, 1000.0], [-1000.0, 1e6]] * 2)
    return StandingsCase("1 km off the track", x, wp, 4)


def grid_case(races, G, seed):
    return StandingsCase(f"grid {races}x{G} seed {seed}", workload.make_race_grid(races, G, seed=seed),
                         workload.track_waypoints(), G)


GRIDS = ((256, 16, 91), (64, 4, 91), (8, 4, 11), (2, 8, 5))


def synthetic_s(rows=9, races=6, G=5, L=70.0, seed=90):
    """s for f110qp_standings_dev alone: steps that cross s = 0 both ways, repeated values, NaN from a row on, a
    NaN first car of a race at row 0, and a NaN that comes back as a number (dist stays NaN)."""
    rng = np.random.default_rng(seed)
    B = races * G
    s = (rng.uniform(0, L, B)[None, :] + np.cumsum(rng.uniform(-9.0, 12.0, (rows, B)), 0)) % L
    s[:, 1] = s[:, 0]
    s[3:, 2] = np.nan
    s[0, G] = np.nan
    s[4, 2 * G + 3] = np.nan
    s[2:, 3 * G:3 * G + 2] = np.nan
    return np.ascontiguousarray(s), L, G


def all_cases():
    c = [tile_case(W) for W in TILE_W] + [rows_case(r) for r in PASS_ROWS] + [batch_case(B) for B in BATCHES]
    c += [group_case(G) for G in GROUPS] + vertex_case() + tie_case() + [duplicate_case()] + bad_waypoint_cases()
    return c + [bad_pose_case(1), bad_pose_case(4), far_case()] + [grid_case(*g) for g in GRIDS[2:]]
