"""The straight-wall model's CPU side (test_walls_cases.py, test_gpu_walls.py, test_gpu_rollout_walls.py): the
cases whose device scans and clearances are compared with the numpy oracles workload.ray_segments and
workload.clearance_walls, and the bounds. No measured number enters either bound.

Beam bound (rule W1). With u = pmax 2^-52, pmax the largest coordinate magnitude of a pose or segment end: the
device's sincos and numpy's may differ by one ulp, everything else is the same correctly rounded operation on
inputs that differ. The LiDAR origin carries off cos + x (two roundings and the cosine's ulp) and A = a - o one
more: each coordinate of A and B is off by at most 4 u. ca = d.x A.y - d.y A.x takes that twice (8 u), the ulp of d
on |A| (2 u) and three roundings (3 u): 13 u; cb likewise, den = ca - cb 27 u. With q = ca / den in [0, 1],
dq <= (13 u + 27 u) / |den| = 40 u / (|e| |sin phi|), phi the angle between beam and wall, and |tb - ta| <= |e|, so
the product moves by 40 u / |sin phi|; ta and tb carry 13 u each and the last sum and product five roundings: at
most 45 u more. Together 85 u / |sin phi|. With GRAZE_SIN = 1e-4 that is 3.8e-9 m at pmax = 20 m, inside
world_cases.ABS_TOL = 4e-9 m, which is the absolute term used next to one float32 ulp. A beam is grazing when
  |sin phi| < GRAZE_SIN on a segment whose ends it straddles or comes within GRAZE_V of straddling, or
  it passes within GRAZE_V = 1e-8 m (above twice ABS_TOL) of a vertex ahead of it that is a free end (no other
  segment ends on the same bits), or a joint whose two outer ends lie on the same side of the beam (there both
  neighbours flip together; with the outer ends on opposite sides one of the two always straddles), or
  0 < |th| < GRAZE_V on any segment it straddles (the LiDAR on the wall: th > 0 can flip).
The circles and mates keep body_cases' rules. Where every heading and beam angle makes sincos exact (heading 0,
beam angles 0 or exact multiples handled by both libraries alike) the scan is compared bit for bit.

Clearance bound (rule W2), derived as body_cases.abs_tol is. Centre: 2^-52 (4 |off| + 4 pmax). Frame: both ends
read it through d.f and d.l with |d| <= D = 2 pmax: 6 pmax 2^-52. Operations on values of at most D: an end into
the frame (a difference, two products, a sum: 4), e (1), g (1), the root's sum and squares (3, halved by the
root), the signed distance's difference (1): 16 with both ends, 32 pmax 2^-52. The corner parameter s = (g.e) /
(e.e) is conditioned by |g| / |e|, but it enters only through s e, which an error ds moves by ds |e| <=
k 2^-52 |g| whatever |e| is (the clamp holds s e within |e|): 8 roundings on values up to D, 16 pmax 2^-52.
Together abs_tol = 2^-52 (4 |off| + 58 pmax): 2.6e-13 m at 20 m. A crossing verdict that flips at a touch moves
the value between 0 and a distance inside this bound. nearest is compared except where the oracle's runner-up
lies within 2 abs_tol.

    python tests/walls_cases.py      # the skip counts of every case
"""
import body_cases as bc_
import numpy as np
import world_cases as wc_

from f110qp import workload

EPS = 2.0 ** -52
GRAZE_SIN, GRAZE_V = 1e-4, 1e-8
CENTER_OFFSET, HL, HW = bc_.CENTER_OFFSET, bc_.HL, bc_.HW
CLEAR_GRID = 512  # clearance_grid's cap for the walls family
CAST_GRID = 512   # cast_scans_grid's cap for the walls family
TILE = wc_.TILE


def beam_tol(pmax):
    """The absolute beam bound of the module docstring at |sin phi| = GRAZE_SIN."""
    return 85.0 * pmax * EPS / GRAZE_SIN


assert beam_tol(wc_.P_ENVELOPE) <= wc_.ABS_TOL


def abs_tol(pmax, off=CENTER_OFFSET):
    """The clearance bound of the module docstring for coordinates up to pmax metres."""
    return EPS * (4.0 * abs(off) + 58.0 * pmax)


# ---- worlds --------------------------------------------------------------------------------------------------

def star_polygon(n=37, seed=0, r=(2.0, 6.0), centre=(0.0, 0.0)):
    """A closed star-shaped polygon of n vertices around `centre` as segments [n, 4]: consecutive segments share
    the vertex's bits and the last closes on the first."""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
    rad = rng.uniform(r[0], r[1], n)
    v = np.stack([centre[0] + rad * np.cos(ang), centre[1] + rad * np.sin(ang)], 1)
    return np.ascontiguousarray(np.concatenate([v, np.roll(v, -1, 0)], 1))


def random_segments(S, seed, spread=9.0, B=None, length=(0.2, 3.0)):
    """S segments of length[0] .. length[1] metres scattered within `spread` metres of the origin, [S, 4] or [B, S, 4]."""
    rng = np.random.default_rng(seed)
    shape = (S,) if B is None else (B, S)
    a = rng.uniform(-spread, spread, shape + (2,))
    ang, ln = rng.uniform(0, 2 * np.pi, shape), rng.uniform(length[0], length[1], shape)
    return np.ascontiguousarray(np.concatenate([a, a + np.stack([ln * np.cos(ang), ln * np.sin(ang)], -1)], -1))


def track():
    """The issue's track: make_wall_world(5, 40) -> (segments [250, 4], circles [40, 3])."""
    return workload.make_wall_world(seed=5, obstacles=40)


# ---- scans ---------------------------------------------------------------------------------------------------

def _beams(x, geom, beams):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        ox = x[:, 0] + wc_.LIDAR_OFFSET * np.cos(x[:, 2])
        oy = x[:, 1] + wc_.LIDAR_OFFSET * np.sin(x[:, 2])
        ang = x[:, 2:3] + (np.float64(geom[0]) + np.float64(geom[1]) * np.arange(beams, dtype=np.float64))[None, :]
    return ox, oy, np.cos(ang), np.sin(ang)


def oracle_scan(x, static, segments, G, geom, beams, off=CENTER_OFFSET):
    """float32 [B, beams]: body_cases.oracle_scan (circles and mates) and the segments' ranges."""
    base = bc_.oracle_scan(x, static, G, geom, beams, off)
    if segments is None or segments.shape[-2] == 0:
        return base
    w = workload.ray_walls(x, geom, beams, segments, wc_.LIDAR_OFFSET, wc_.MAX_RANGE).astype(np.float32)
    return np.minimum(base, w)


def _joints(sg):
    """Per segment end (2S: all a's, then all b's): the vertex, its own other end, and the other end of the one
    other segment end with the same bits (NaN where the vertex is free or shared by more than two)."""
    S = sg.shape[0]
    v = np.concatenate([sg[:, 0:2], sg[:, 2:4]])
    own = np.concatenate([sg[:, 2:4], sg[:, 0:2]])
    key = [r.tobytes() for r in np.ascontiguousarray(v)]
    where = {}
    for i, k in enumerate(key):
        where.setdefault(k, []).append(i)
    other = np.full((2 * S, 2), np.nan)
    for i, k in enumerate(key):
        m = [j for j in where[k] if j != i]
        if len(m) == 1:
            other[i] = own[m[0]]
    return v, own, other


def grazing_walls(x, segments, geom, beams):
    """[B, beams] bool: the module docstring's rule on the segments, car by car."""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    out = np.zeros((B, beams), bool)
    if segments is None or segments.shape[-2] == 0:
        return out
    ox, oy, dx, dy = _beams(x, geom, beams)
    for b in range(B):
        sg = segments if segments.ndim == 2 else segments[b]
        sg = sg[np.isfinite(sg).all(axis=1)]
        if not len(sg) or not np.isfinite(x[b]).all():
            continue
        d_x, d_y = dx[b][:, None], dy[b][:, None]
        ax, ay, bx, by = sg[:, 0] - ox[b], sg[:, 1] - oy[b], sg[:, 2] - ox[b], sg[:, 3] - oy[b]
        ca, cb = d_x * ay - d_y * ax, d_x * by - d_y * bx
        ta, tb = ax * d_x + ay * d_y, bx * d_x + by * d_y
        den = ca - cb
        ln = np.hypot(bx - ax, by - ay)
        near = (np.minimum(ca, cb) <= GRAZE_V) & (np.maximum(ca, cb) >= -GRAZE_V) & (np.maximum(ta, tb) > -GRAZE_V)
        with np.errstate(invalid="ignore", divide="ignore"):
            flat = near & (ln > 0) & (np.abs(den) < GRAZE_SIN * ln) & (den != 0)
            th = ta + (tb - ta) * (ca / np.where(den != 0, den, 1.0))
        on = near & (den != 0) & (np.abs(th) < GRAZE_V)
        v, own, other = _joints(sg)
        vx, vy = v[:, 0] - ox[b], v[:, 1] - oy[b]
        cv, tv = d_x * vy - d_y * vx, vx * d_x + vy * d_y
        cp = d_x * (own[:, 1] - oy[b]) - d_y * (own[:, 0] - ox[b])
        with np.errstate(invalid="ignore"):
            cq = d_x * (other[:, 1] - oy[b]) - d_y * (other[:, 0] - ox[b])
            safe = cp * cq < 0.0  # the outer ends on opposite sides (a free end: NaN, never safe)
        at = (np.abs(cv) <= GRAZE_V) & (tv > -GRAZE_V) & ~safe
        out[b] = flat.any(axis=1) | on.any(axis=1) | at.any(axis=1)
    return out


class WallScan:
    """Poses x [B, 3] in races of G, static circles (or None), segments [S, 4] or [B, S, 4], and the scan."""

    def __init__(self, name, x, G, static, segments, geom=None, beams=64, off=CENTER_OFFSET):
        self.name, self.x, self.G, self.static = name, np.ascontiguousarray(x, np.float64), G, static
        self.segments, self.beams, self.off = np.ascontiguousarray(segments, np.float64), beams, off
        self.geom = wc_.geometry(beams) if geom is None else geom
        ends = self.segments[np.isfinite(self.segments)]
        self.pmax = float(max(np.abs(self.x[..., :2][np.isfinite(self.x[..., :2])]).max(), np.abs(ends).max() if ends.size else 0.0))
        assert self.pmax <= wc_.P_ENVELOPE, (name, self.pmax)

    def oracle(self):
        return oracle_scan(self.x, self.static, self.segments, self.G, self.geom, self.beams, self.off)

    def grazing(self):
        g = bc_.grazing(self.x, self.static, self.G, self.geom, self.beams, self.off)
        return g | grazing_walls(self.x, self.segments, self.geom, self.beams)

    def check(self, got, what=""):
        want = self.oracle()
        name = f"{self.name} {what}"
        assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape)
        skip = self.grazing()
        print(f"{name}: {int(skip.sum())} of {skip.size} beams skipped")
        assert skip.sum() <= wc_.SKIP_CAP * skip.size, f"{name}: {int(skip.sum())} of {skip.size} beams are grazing"
        bound = np.spacing(want).astype(np.float64) + wc_.ABS_TOL
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        bad = (err > bound) & ~skip
        print(f"{name}: worst error {float((err / bound)[~skip].max()):.3f} of the bound")
        assert not bad.any(), (name, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])
        return int(skip.sum())


def track_scan(B=64, beams=1080, seed=3):
    """make_wall_world at B poses along the track, every car alone."""
    sg, ci = track()
    return WallScan(f"walls track {B} poses {beams} beams", wc_.track_poses(B, seed), 1, ci, sg, beams=beams)


def tile_scan(S, C=0, G=1, seed=61, B=6):
    """S random segments behind C circles and G - 1 mates, cars within 0.4 m of the origin."""
    x = wc_.poses_near_origin(B, seed)
    if G > 1:
        x[:, :2] *= 4.0
    st = wc_.random_world(C, seed + 1) if C else None
    return WallScan(f"walls tile S {S} C {C} G {G}", x, G, st, random_segments(S, seed + 2))


def rows_scan(B=6, S=9, seed=71):
    """wall_rows = B: a segment set per car."""
    x = wc_.poses_near_origin(B, seed)
    return WallScan(f"walls rows B {B}", x, 1, wc_.random_world(5, seed + 1), random_segments(S, seed + 2, B=B))


def stride_scan(seed=53, beams=16):
    """B = 2 x 512 + 6 cars in races of 2, a segment set per car: six workgroups take a third car."""
    B = 2 * CAST_GRID + 6
    x = wc_.poses_near_origin(B, seed)
    x[:, :2] *= 4.0
    return WallScan(f"walls stride B {B}", x, 2, wc_.random_world(3, seed + 1), random_segments(5, seed + 2, spread=6.0, B=B),
                    beams=beams)


def scan_cases():
    """Every scan the GPU tests hold against the oracle."""
    return [track_scan(), tile_scan(255), tile_scan(256), tile_scan(257), tile_scan(3, C=TILE - 3, G=3), tile_scan(3, C=TILE - 2, G=3),
            tile_scan(40, C=0, G=1), rows_scan(), stride_scan()]


# ---- clearance -----------------------------------------------------------------------------------------------

class WallCase(bc_.BodyCase):
    """body_cases.BodyCase with segments [S, 4] or [B, S, 4] behind the circles and the mates."""

    def __init__(self, name, x, G, circles, segments, off=CENTER_OFFSET):
        super().__init__(name, x, G, circles, off)
        self.segments = None if segments is None else np.ascontiguousarray(segments, np.float64)
        S = 0 if self.segments is None else self.segments.shape[-2]
        self.S = S
        ends = self.segments[np.isfinite(self.segments)] if S else np.zeros(0)
        self.pmax = float(max(self.pmax, np.abs(ends).max() if ends.size else 0.0))
        self.tol = abs_tol(self.pmax, self.off)

    def oracle(self):
        return workload.clearance_walls(self.x, self.circles, self.segments, self.G, self.off, self.hl, self.hw)

    def wall_values(self):
        """[rows, B, S] (NaN -> +inf)."""
        if not self.S:
            return np.zeros((self.rows, self.B, 0))
        qx, qy, c, s = self._frames()
        sw = self.segments if self.segments.ndim == 3 else self.segments[None]
        v = workload.segment_body(sw[None, :, :, 0], sw[None, :, :, 1], sw[None, :, :, 2], sw[None, :, :, 3], qx[..., None],
                                  qy[..., None], c[..., None], s[..., None], self.hl, self.hw)
        return np.where(np.isnan(v), np.inf, v)

    def index_of(self):
        """The nearest index of every candidate of all_values() + wall_values()."""
        n_body = self.C + self.G - 1
        return n_body, self.C + self.G + np.arange(self.S)

    def skip(self):
        body = self.all_values()
        v = np.sort(np.concatenate([body, self.wall_values()], 2), axis=2)
        near_zero = (np.abs(body[..., self.C:]) <= self.tol).any(axis=2) if self.G > 1 else np.zeros(v.shape[:2], bool)
        if v.shape[2] < 2:
            return near_zero
        with np.errstate(invalid="ignore"):
            return near_zero | (np.isfinite(v[..., 1]) & (v[..., 1] - v[..., 0] <= 2.0 * self.tol))

    def check(self, clear, near, what=""):
        want, wnear = self.oracle()
        clear, near = np.asarray(clear).reshape(want.shape), np.asarray(near).reshape(want.shape)
        name = f"{self.name} {what}"
        if self.exact:
            assert (clear.view(np.int64) == want.view(np.int64)).all(), (name, np.argwhere(clear != want)[:5].tolist())
            assert (near == wnear).all(), (name, np.argwhere(near != wnear)[:5].tolist())
            return 0.0
        assert (np.isinf(want) == np.isinf(clear)).all() and (near[np.isinf(want)] == -1).all(), name
        sk = self.skip()
        print(f"{name}: {int(sk.sum())} of {sk.size} poses skipped")
        assert sk.sum() <= wc_.SKIP_CAP * sk.size, (name, int(sk.sum()))
        v = self.all_values()
        touch = (np.abs(v[..., self.C:]) <= self.tol).any(axis=2) if self.G > 1 else np.zeros(sk.shape, bool)
        fin = np.isfinite(want) & ~touch
        err = np.abs(clear[fin] - want[fin])
        print(f"{name}: worst error {float(err.max()) if err.size else 0.0:.3e} of the bound {self.tol:.3e}")
        assert (err <= self.tol).all(), (name, float(err.max()), self.tol)
        assert (near == wnear)[~sk].all(), (name, np.argwhere((near != wnear) & ~sk)[:5].tolist())
        return float(err.max() / self.tol) if err.size else 0.0


ROWS = bc_.ROWS


def rows_case(rows, seed=91):
    """rows x 8 poses in races of 4 within 3 m, 12 circles and 30 segments."""
    c = bc_.rows_case(rows)
    return WallCase(f"walls rows {rows}", c.x, c.G, c.circles, random_segments(30, seed, spread=3.0, length=(0.1, 0.7)))


def heading0_case(seed=131):
    """body_cases.heading0_case with 40 segments: every heading exactly 0, bit equality."""
    c = bc_.heading0_case(seed)
    return WallCase("walls heading 0", c.x, c.G, c.circles, random_segments(40, seed + 5, spread=6.0, length=(0.1, 0.7)))


def ranges_case(seed=17):
    """One row whose nearest obstacles are a circle, a mate and a segment: car 0 next to circle 0, cars 1 and 2
    next to each other, car 3 next to segment 1."""
    x = np.array([[0.0, 0.0, 0.3], [4.0, 0.0, 0.2], [4.0, 0.45, 0.1], [-4.0, 0.0, -0.4]])
    ci = np.array([[0.3, 0.4, 0.1], [8.0, 8.0, 0.3]])
    sg = np.array([[9.0, -9.0, 9.0, 9.0], [-4.5, 0.5, -3.0, 0.6], [-9.0, -9.0, 9.0, -9.0]])
    return WallCase("walls three index ranges", x[None], 4, ci, sg)


def track_case(B=64, seed=3):
    sg, ci = track()
    return WallCase("walls track", wc_.track_poses(B, seed)[None], 1, ci, sg)


def per_car_case(B=6, seed=37):
    """wall_rows = B with world_rows = 1."""
    x = bc_.cc_.poses(2, B, seed) * [3.0, 3.0, 1.0]
    return WallCase("walls per car", x, 2, wc_.random_world(6, seed + 1), random_segments(7, seed + 2, spread=3.0, B=B, length=(0.1, 0.7)))


def stride_case(seed=43):
    """B = 2 x 512 + 6 in races of 2, a segment set per car."""
    B = 2 * CLEAR_GRID + 6
    x = bc_.cc_.poses(1, B, seed) * [3.0, 3.0, 1.0]
    return WallCase(f"walls stride B {B}", x, 2, wc_.random_world(3, seed + 1), random_segments(4, seed + 2, spread=3.0, B=B, length=(0.1, 0.7)))


def sign_cases():
    """name -> (segment [4], the exact value or None, what holds) for a body at the origin (centre offset 0),
    heading 0: the sign cases of rule W2."""
    return {
        "end inside": ([0.1, 0.05, 2.0, 1.0], max(0.1 - HL, 0.05 - HW), "< 0"),
        "through, both ends out": ([-1.0, 0.02, 1.0, -0.03], 0.0, "== 0"),
        "wholly inside": ([-0.1, 0.0, 0.2, 0.05], min(max(0.1 - HL, 0.0 - HW), max(0.2 - HL, 0.05 - HW)), "< 0"),
        "touching a side": ([-1.0, HW, 1.0, HW], 0.0, "== 0"),
        "touching a corner": ([HL, HW, HL + 0.5, HW + 0.5], 0.0, "== 0"),
        "zero length outside": ([HL + 0.5, 0.0, HL + 0.5, 0.0], 0.5, "> 0"),
        "zero length inside": ([0.0, 0.0, 0.0, 0.0], -HW, "< 0"),
        "apart, beside": ([-1.0, HW + 0.25, 1.0, HW + 0.25], 0.25, "> 0"),
    }


def sign_case(name):
    sg, want, _ = sign_cases()[name]
    return WallCase("walls sign " + name, np.zeros((1, 1, 3)), 1, None, np.array([sg]), off=0.0), want


def oracle_cases():
    """Every clearance case the GPU tests hold against the oracle."""
    return [rows_case(r) for r in ROWS] + [heading0_case(), ranges_case(), track_case(), per_car_case(), stride_case()] + \
        [sign_case(n)[0] for n in sign_cases()]


if __name__ == "__main__":
    for c in oracle_cases():
        print(f"{c.name:60s} tol {c.tol:.2e} skipped {int(c.skip().sum())} of {c.skip().size}")
    for c in scan_cases():
        g = c.grazing()
        print(f"{c.name:60s} grazing {int(g.sum())} of {g.size}")
