"""The rectangular-body model's CPU side (test_body_cases.py, test_gpu_body.py, test_gpu_rollout_body.py): the
cases whose device clearances and scans are compared with the numpy oracles workload.clearance_body and
workload.ray_bodies, and the bounds.

Clearance bound, derived as contact_cases.abs_tol is (abs_tol(pmax), pmax the largest coordinate magnitude of a
pose or circle of the case). Every heading exactly 0: sincos(0) is exact on both sides and every later operation
is the same correctly rounded one: bit equality. Otherwise the device's sincos and numpy's may differ by one
double ulp (2^-52 on a value of at most 1). (a) Centres: each coordinate differs by at most dc = |off| 2^-52 +
ulp(pmax) as in contact_cases, and the distance of two rectangles is 1-Lipschitz in either centre: 2 sqrt(2) dc <
4 dc = 2^-52 (4 |off| + 4 pmax) for both. (b) Frames: the value reads a frame only through d.f and d.l with |d|
at most D = 2 pmax, so one ulp in cos and in sin moves it by at most sqrt(2) D 2^-52 < 3 pmax 2^-52 per frame;
there are now two frames per pair: 6 pmax 2^-52. (c) What follows is the same sequence of rounded operations on
both sides, on inputs that differ, so each may round the other way by an ulp of a value of at most D: the longest
path is a corner distance (two sums that build the corner, dx or dy, two products and their sum, |u| - hl, two
squares and their sum through the root, which halves them: at most 12 operations), 12 D 2^-52 = 24 pmax 2^-52.
Together: abs_tol = 2^-52 (4 |off| + 34 pmax): 1.5e-13 m at 20 m. No measured number enters.

The pair value switches from the separating-axis gap g to the corner distance at g = 0; both vanish there, but the
corner distance of a corner-to-corner approach is up to sqrt(2) g and more for rotated cars, so a pair whose |g|
is within abs_tol may take the other branch on the device. Such a pose is skipped like a nearest tie below
(it needs two cars within 1e-13 m of touching: none of the random cases has one).

nearest: compared except where the oracle's runner-up lies within 2 abs_tol. At most world_cases.SKIP_CAP of a
case's poses may skip; check() asserts the cap and test_body_cases.py asserts it from the oracle alone.

Beams. The static circles keep world_cases' grazing rule and bound (one float32 ulp + ABS_TOL). For a mate's
rectangle the entry parameter is t = (+-h - o'_a) / d'_a on the deciding axis a: o' carries the rounding of the
centres and the frame, at most 2 |p| 2^-52 (3 + 2) < 5e-14 m at |p| = 20 m, so t moves by at most 5e-14 / |d'_a|
(+ t 2^-52 / |d'_a| from d' itself, 2e-15 at t = 10 m). GRAZE_D = 1e-4 keeps that under 7e-10 m, inside ABS_TOL =
4e-9 m. A beam is grazing against a mate when it passes within the mate's circumscribed circle (+ 1 mm) and
  0 < |d'_a| < GRAZE_D on either axis (a beam within 1e-4 rad of a side, not exactly parallel to it), or
  |th_hi - th_lo| < GRAZE_T (the entry and the exit within GRAZE_T: the verdict can flip), or |th| < GRAZE_T
  (the LiDAR on the boundary: th > 0 can flip),
with GRAZE_T = 1e-8 m, above twice the 4e-9 m either end can move by off the first rule. An exactly parallel
beam (d'_a == 0, heading 0 and beam angle 0 on both sides) takes the exact in-slab test and is compared.

    python tests/body_cases.py      # the skip counts of every case
"""
import contact_cases as cc_
import numpy as np
import world_cases as wc_

from f110qp import workload

CENTER_OFFSET = cc_.CENTER_OFFSET
HL, HW = workload.HALF_LENGTH, workload.HALF_WIDTH
RC = float(np.hypot(HL, HW))  # the circumscribed circle
EPS = 2.0 ** -52
GRAZE_D, GRAZE_T = 1e-4, 1e-8
CLEAR_GRID = 512  # clearance_grid's cap for the body family
CAST_GRID = 512   # cast_scans_grid's cap for the body family
PASS = cc_.PASS


def abs_tol(pmax, off=CENTER_OFFSET):
    """The clearance bound of the module docstring for coordinates up to pmax metres."""
    return EPS * (4.0 * abs(off) + 34.0 * pmax)


class BodyCase(cc_.ContactCase):
    """contact_cases.ContactCase with rectangular bodies: the same poses, races and circles."""

    def __init__(self, name, x, G, circles, off=CENTER_OFFSET, hl=HL, hw=HW):
        super().__init__(name, x, G, circles, off)
        self.hl, self.hw = float(hl), float(hw)
        self.tol = abs_tol(self.pmax, self.off)
        self.exact = bool((self.x[..., 2][np.isfinite(self.x[..., 2])] == 0.0).all())

    def oracle(self):
        return workload.clearance_body(self.x, self.circles, self.G, self.off, self.hl, self.hw)

    def _frames(self):
        x = self.x
        c, s = np.cos(x[..., 2]), np.sin(x[..., 2])
        return x[..., 0] + self.off * c, x[..., 1] + self.off * s, c, s

    def all_values(self):
        """Every candidate value [rows, B, C + G - 1] in index order (NaN -> +inf), the oracle's expressions."""
        with np.errstate(invalid="ignore", over="ignore"):
            qx, qy, c, s = self._frames()
            out = []
            if self.C:
                ci = self.circles if self.circles.ndim == 3 else self.circles[None]
                out.append(workload.body_sd(ci[None, :, :, 0], ci[None, :, :, 1], qx[..., None], qy[..., None], c[..., None],
                                            s[..., None], self.hl, self.hw) - np.abs(ci[None, :, :, 2]))
            if self.G > 1:
                m = workload._mates(self.B, self.G)
                out.append(workload.body_pair(qx[..., None], qy[..., None], c[..., None], s[..., None], qx[:, m], qy[:, m],
                                              c[:, m], s[:, m], self.hl, self.hw))
            v = np.concatenate(out, 2) if out else np.zeros((self.rows, self.B, 0))
        return np.where(np.isnan(v), np.inf, v)

    def skip(self):
        """[rows, B] bool: the runner-up within 2 tol of the minimum, or a mate within tol of touching."""
        v = self.all_values()
        near_zero = (np.abs(v[..., self.C:]) <= self.tol).any(axis=2) if self.G > 1 else np.zeros(v.shape[:2], bool)
        v = np.sort(v, axis=2)
        if v.shape[2] < 2:
            return near_zero
        with np.errstate(invalid="ignore"):
            return near_zero | (np.isfinite(v[..., 1]) & (v[..., 1] - v[..., 0] <= 2.0 * self.tol))

    def check(self, clear, near, what=""):
        """The device's clearance and nearest against the oracle: bits when every heading is 0, else tol and the
        skip rule (a skipped pose keeps the clearance comparison unless a mate is within tol of touching)."""
        want, wnear = self.oracle()
        clear, near = np.asarray(clear).reshape(want.shape), np.asarray(near).reshape(want.shape)
        name = f"{self.name} {what}"
        if self.exact:
            assert (clear.view(np.int64) == want.view(np.int64)).all(), (name, np.argwhere(clear != want)[:5].tolist())
            assert (near == wnear).all(), (name, np.argwhere(near != wnear)[:5].tolist())
            return 0.0
        assert (np.isinf(want) == np.isinf(clear)).all() and (near[np.isinf(want)] == -1).all(), name
        sk = self.skip()
        assert sk.sum() <= wc_.SKIP_CAP * sk.size, (name, int(sk.sum()))
        v = self.all_values()
        touch = (np.abs(v[..., self.C:]) <= self.tol).any(axis=2) if self.G > 1 else np.zeros(sk.shape, bool)
        fin = np.isfinite(want) & ~touch
        err = np.abs(clear[fin] - want[fin])
        print(f"{name}: worst error {float(err.max()) if err.size else 0.0:.3e} of the bound {self.tol:.3e}")
        assert (err <= self.tol).all(), (name, float(err.max()), self.tol)
        assert (near == wnear)[~sk].all(), (name, np.argwhere((near != wnear) & ~sk)[:5].tolist())
        return float(err.max() / self.tol) if err.size else 0.0


def of(c, **kw):
    """A contact case's poses, races and circles with rectangular bodies."""
    return BodyCase("body " + c.name, c.x, c.G, c.circles, c.off, **kw)


ROWS = (1, PASS, PASS + 1, 2 * PASS + 1)


def rows_case(rows):
    return of(cc_.rows_case(rows))


def stride_case():
    """B = 2 CLEAR_GRID + 6 = 1030 in races of 5, a world per car: workgroups 0 .. 5 take a third car."""
    c = of(cc_.stride_case(True))
    assert c.B == 2 * CLEAR_GRID + 6 and c.world_rows == c.B
    return c


def crowd_case(seed=83):
    """One race of 258 cars within 8 m and 255 circles: the mates are indices 255 .. 511, across the tile edge."""
    c = cc_.crowd_case(seed)
    return BodyCase("body crowd G 258 C 255", c.x, c.G, wc_.random_world(255, seed + 2))


def heading0_case(seed=131):
    """Two races of 4 within 2.4 m, 40 circles, every heading exactly 0: bit equality."""
    x = cc_.poses(3, 8, seed) * [6.0, 6.0, 0.0]
    return BodyCase("body heading 0", x, 4, wc_.random_world(40, seed + 1))


def oracle_cases():
    return [rows_case(r) for r in ROWS] + [stride_case(), crowd_case(), heading0_case(), of(cc_.edge_case(0, 5)),
                                           of(cc_.batch_case(65, 1)), of(cc_.random_case(True)), of(cc_.track_case())]


# ---- scans -------------------------------------------------------------------------------------------------

def oracle_scan(x, static, G, geom, beams, off=CENTER_OFFSET, hl=HL, hw=HW):
    """float32 [B, beams]: the static circles' ranges (world_cases.oracle_scan) and the opponents' (ray_bodies)."""
    x = np.asarray(x, np.float64)
    opp = workload.ray_bodies(x, geom, beams, G, off, hl, hw, wc_.LIDAR_OFFSET, wc_.MAX_RANGE).astype(np.float32)
    if static is None or static.shape[-2] == 0:
        return opp
    return np.minimum(wc_.oracle_scan(x, static, geom, beams), opp)


def grazing(x, static, G, geom, beams, off=CENTER_OFFSET, hl=HL, hw=HW):
    """[B, beams] bool: world_cases' rule on the static circles, the module docstring's on the mates."""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    g = np.zeros((B, beams), bool)
    if static is not None and static.shape[-2]:
        g |= wc_.grazing(x, static, geom, beams)
    if G == 1:
        return g
    rc = float(np.hypot(hl, hw))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c, s = np.cos(x[:, 2]), np.sin(x[:, 2])
        ox, oy = x[:, 0] + wc_.LIDAR_OFFSET * c, x[:, 1] + wc_.LIDAR_OFFSET * s
        qx, qy = x[:, 0] + off * c, x[:, 1] + off * s
        ang = x[:, 2:3] + (np.float64(geom[0]) + np.float64(geom[1]) * np.arange(beams, dtype=np.float64))[None, :]
        dx, dy = np.cos(ang)[:, :, None], np.sin(ang)[:, :, None]
        m = workload._mates(B, G)
        px, py = (qx[m] - ox[:, None])[:, None, :], (qy[m] - oy[:, None])[:, None, :]
        cm, sm = c[m][:, None, :], s[m][:, None, :]
        t = px * dx + py * dy
        close = (px * px + py * py - t * t <= (rc + 1e-3) ** 2) & (t > -rc)
        df, dl = dx * cm + dy * sm, dy * cm - dx * sm
        flat = ((df != 0) & (np.abs(df) < GRAZE_D)) | ((dl != 0) & (np.abs(dl) < GRAZE_D))
        of_, ol = -(px * cm + py * sm), -(py * cm - px * sm)

        def ends(o, d, h):
            dd = np.where(d == 0, 1.0, d)
            t1, t2 = (-h - o) / dd, (h - o) / dd
            ins = np.abs(o) <= h
            return (np.where(d == 0, np.where(ins, -np.inf, np.inf), np.fmin(t1, t2)),
                    np.where(d == 0, np.where(ins, np.inf, -np.inf), np.fmax(t1, t2)))
        lf, hf = ends(of_, df, hl)
        ll, hl_ = ends(ol, dl, hw)
        th, ex = np.fmax(lf, ll), np.fmin(hf, hl_)
        edge = (np.abs(ex - th) < GRAZE_T) | (np.abs(th) < GRAZE_T)
        return g | (close & (flat | edge)).any(axis=2)


class ScanCase:
    """Poses x [B, 3] in races of G, the static world and the scan; `cars`: the cars compared (all when None)."""

    def __init__(self, name, x, G, static, geom=None, beams=1080, cars=None, off=CENTER_OFFSET):
        self.name, self.x, self.G, self.static, self.beams, self.off = name, np.ascontiguousarray(x, np.float64), G, static, beams, off
        self.geom = wc_.geometry(beams) if geom is None else geom
        self.cars = np.arange(len(self.x)) if cars is None else np.asarray(cars)

    def _sub(self, x):
        """The compared cars' rows: the oracle runs on whole races, so the cars' races are kept whole."""
        races = np.unique(self.cars // self.G)
        keep = (races[:, None] * self.G + np.arange(self.G)[None, :]).ravel()
        st = self.static if self.static is None or self.static.ndim == 2 else self.static[keep]
        return keep, x[keep], st, np.searchsorted(keep, self.cars)

    def grazing(self, x=None):
        keep, xs, st, at = self._sub(self.x if x is None else np.asarray(x, np.float64))
        return grazing(xs, st, self.G, self.geom, self.beams, self.off)[at]

    def check(self, got, x=None, what=""):
        x = self.x if x is None else np.asarray(x, np.float64)
        keep, xs, st, at = self._sub(x)
        want = oracle_scan(xs, st, self.G, self.geom, self.beams, self.off)[at]
        got = np.ascontiguousarray(got[self.cars])
        name = f"{self.name} {what}"
        assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape)
        skip = self.grazing(x)
        assert skip.sum() <= wc_.SKIP_CAP * skip.size, f"{name}: {int(skip.sum())} of {skip.size} beams are grazing"
        bound = np.spacing(want).astype(np.float64) + wc_.ABS_TOL
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        bad = (err > bound) & ~skip
        print(f"{name}: worst error {float((err / bound)[~skip].max()):.3f} of the bound, {int(skip.sum())} beams skipped")
        assert not bad.any(), (name, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])
        return int(skip.sum())


def track_scan(beams=1080, races=2, G=4, seed=11):
    return ScanCase(f"body track {races}x{G} {beams} beams", workload.make_race_grid(races, G, seed), G, wc_.track_world(),
                    beams=beams)


def crowd_scan(C=250, seed=21, G=258):
    """One race of 258 cars within 8 m, 64 beams, C static circles: the opponents span two circle tiles."""
    c = __import__("race_cases").crowd(C, seed, G)
    return ScanCase(f"body crowd C {C}", c.x, G, c.static, c.geom, c.beams, cars=c.cars)


def stride_scan(B=CAST_GRID + 268, G=4, seed=53, beams=64):
    """B = 780 cars within 1.6 m in races of 4, a world of three circles per car: above the cap of 512, 268
    workgroups take a second car. The first and the last two races meet the oracle."""
    x = wc_.poses_near_origin(B, seed)
    x[:, :2] *= 4.0
    cars = np.concatenate([np.arange(8), np.arange(CAST_GRID - 4, CAST_GRID + 4), np.arange(B - 8, B)])
    return ScanCase(f"body stride B {B}", x, G, wc_.random_world(3, seed + 1, B, spread=3.0), beams=beams, cars=cars)


def seam_scan(beams=64):
    """Three cars, no static circle, car 0 heading 0 at the origin: car 1 straight behind it (its rectangle
    straddles the atan2 seam of p and, the scan running from -pi, the first and the last beam), car 2 ahead."""
    x = np.array([[0.0, 0.0, 0.0], [-1.5, 0.004, 0.4], [1.7, 0.3, -1.1]])
    return ScanCase("body seam", x, 3, None, beams=beams)


def inside_scan(beams=64):
    """Car 1's rectangle covers car 0's LiDAR (it sees through it to car 2); car 2 stands 2 m ahead."""
    x = np.array([[0.0, 0.0, 0.1], [0.2, 0.02, 0.5], [2.2, 0.1, 1.3]])
    return ScanCase("body inside", x, 3, None, beams=beams)


def parallel_scan():
    """Heading 0 and beam 2 of 5 at angle 0 exactly (-0.5 + 2 x 0.25): car 1 is 2 m straight ahead at heading 0, so
    the beam is exactly parallel to its long sides (d'_l == 0) and returns its rear face."""
    g = (np.float32(-0.5), np.float32(0.25), np.float32(0.5))
    x = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    return ScanCase("body parallel", x, 2, None, geom=g, beams=5)


def scan_cases():
    return [track_scan(64), track_scan(1080), track_scan(1200, races=1), crowd_scan(), stride_scan(), seam_scan(),
            inside_scan(), parallel_scan()]


if __name__ == "__main__":
    for c in oracle_cases():
        print(f"{c.name:60s} tol {c.tol:.2e} skipped {int(c.skip().sum())} of {c.skip().size}")
    for c in scan_cases():
        g = c.grazing()
        print(f"{c.name:60s} grazing {int(g.sum())} of {g.size}")
