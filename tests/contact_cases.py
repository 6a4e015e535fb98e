"""The contact model's CPU side (test_contact_cases.py, test_gpu_contact.py, test_gpu_rollout_contact.py): the
cases whose device clearances are compared with the numpy oracle workload.clearance, and the bound.

Bound, derived (abs_tol(pmax), pmax the largest coordinate magnitude of a pose or a circle centre of the case,
radii included): at center_offset = 0 there is none, the centres are the poses' bits and every later operation
is a correctly rounded one on both sides: bit equality. With an offset the device's sincos and numpy's may
differ by one double ulp (2^-52 relative on a value of at most 1), so off * cos differs by at most
|off| 2^-52 before its own rounding, and each centre coordinate by at most dc = |off| 2^-52 + ulp(pmax) (one
rounding of the product, one of the sum, each half an ulp of a value below pmax). The distance is 1-Lipschitz
in either centre: moving q (and, for a mate, q_m as well) changes the exact distance by at most
2 sqrt(2) dc < 4 dc. What follows the centres is the same sequence of at most eight rounded operations on
both sides (dx, dy, two squares, their sum, the root, - |r| or - R, - R; the last three are the three
roundings behind the distance), but on inputs that differ, so each may round the other way: every one of
them is within half an ulp of a value of at most D = 2 pmax (a difference of two coordinates, a distance or a
clearance; the squares and their sum enter through the root, which halves their relative error), on either
side. Together: abs_tol = 2^-52 (4 (|off| + pmax) + 8 D) = 2^-52 (4 |off| + 20 pmax): 9.0e-14 m at 20 m.
No measured number enters.

nearest: the device may pick another obstacle only when the oracle's two smallest values lie within
2 abs_tol of each other; such a pose skips the nearest comparison (never the clearance one). At most
world_cases.SKIP_CAP of a case's poses may; test_contact_cases.py asserts from the oracle alone that every case
here stays inside the cap.

    python tests/contact_cases.py      # the closest pair of candidates of every case
"""
import numpy as np
import world_cases as wc_

from f110qp import workload

CAR_RADIUS, CENTER_OFFSET = 0.3, 0.1651  # f110qp_default_race_config
TILE = wc_.TILE
EPS = 2.0 ** -52


def abs_tol(pmax, off=CENTER_OFFSET):
    """The bound of the module docstring for coordinates up to pmax metres."""
    return EPS * (4.0 * abs(off) + 20.0 * pmax)


class ContactCase:
    """Poses x [rows, B, 3] in races of G, circles [C, 3], [B, C, 3] or None, the body (R, off)."""

    def __init__(self, name, x, G, circles, off=CENTER_OFFSET, R=CAR_RADIUS):
        self.name, self.G, self.circles, self.off, self.R = name, int(G), circles, float(off), float(R)
        self.x = np.ascontiguousarray(x, np.float64)
        if self.x.ndim == 2:
            self.x = self.x[None]
        fin = [np.abs(self.x[..., :2][np.isfinite(self.x[..., :2])])]
        if circles is not None and circles.size:
            fin.append(np.abs(circles[np.isfinite(circles)]))
        self.pmax = float(max([v.max() for v in fin if v.size] + [1.0])) + abs(self.off)
        self.tol = abs_tol(self.pmax, self.off)

    @property
    def rows(self):
        return self.x.shape[0]

    @property
    def B(self):
        return self.x.shape[1]

    @property
    def C(self):
        return 0 if self.circles is None else self.circles.shape[-2]

    @property
    def world_rows(self):
        return 1 if self.circles is None or self.circles.ndim == 2 else self.circles.shape[0]

    def oracle(self):
        return workload.clearance(self.x, self.circles, self.G, self.R, self.off)

    def all_values(self):
        """Every candidate value [rows, B, C + G - 1] in index order (NaN -> +inf), the oracle's expressions."""
        out = np.full((self.rows, self.B, self.C + self.G - 1), np.inf)
        for c in range(out.shape[2]):
            out[:, :, c] = self._single(c)
        return out

    def _single(self, c):
        """The value of candidate c alone for every pose."""
        x, off, R = self.x, self.off, self.R
        with np.errstate(invalid="ignore", over="ignore"):
            qx, qy = x[..., 0] + off * np.cos(x[..., 2]), x[..., 1] + off * np.sin(x[..., 2])
            if c < self.C:
                ci = self.circles if self.circles.ndim == 2 else self.circles[None]
                dx, dy = ci[..., c, 0] - qx, ci[..., c, 1] - qy
                v = (np.sqrt(dx * dx + dy * dy) - np.abs(ci[..., c, 2])) - R
            else:
                i = c - self.C
                b = np.arange(self.B)
                m = b - b % self.G + i + (i >= b % self.G)   # mate with stepped index i
                dx, dy = qx[:, m] - qx, qy[:, m] - qy
                v = (np.sqrt(dx * dx + dy * dy) - R) - R
        return np.where(np.isnan(v), np.inf, v)

    def skip(self):
        """[rows, B] bool: the poses whose two smallest candidates lie within 2 tol (nearest may differ)."""
        v = np.sort(self.all_values(), axis=2)
        if v.shape[2] < 2:
            return np.zeros(v.shape[:2], bool)
        with np.errstate(invalid="ignore"):
            return np.isfinite(v[..., 1]) & (v[..., 1] - v[..., 0] <= 2.0 * self.tol)

    def check(self, clear, near, what=""):
        """The device's clearance and nearest against the oracle: bits at off = 0, else tol and the skip rule."""
        want, wnear = self.oracle()
        clear, near = np.asarray(clear).reshape(want.shape), np.asarray(near).reshape(want.shape)
        name = f"{self.name} {what}"
        if self.off == 0.0:
            assert (clear.view(np.int64) == want.view(np.int64)).all(), (name, np.argwhere(clear != want)[:5].tolist())
            assert (near == wnear).all(), (name, np.argwhere(near != wnear)[:5].tolist())
            return 0.0
        assert (np.isinf(want) == np.isinf(clear)).all() and (near[np.isinf(want)] == -1).all(), name
        fin = np.isfinite(want)
        err = np.abs(clear[fin] - want[fin])
        assert (err <= self.tol).all(), (name, float(err.max()), self.tol)
        sk = self.skip()
        assert sk.sum() <= wc_.SKIP_CAP * sk.size, (name, int(sk.sum()))
        assert (near == wnear)[~sk].all(), (name, np.argwhere((near != wnear) & ~sk)[:5].tolist())
        return float(err.max() / self.tol) if err.size else 0.0


def poses(rows, B, seed):
    return wc_.poses_near_origin(rows * B, seed).reshape(rows, B, 3)


def random_case(per_car, off=CENTER_OFFSET, seed=61):
    """B = 8 in races of 4 within 3.2 m of the origin, rows = 3, C = 300 random circles (the list crosses the
    256-circle tile): some cars in contact, some clear."""
    B = 8
    return ContactCase(f"random world_rows {B if per_car else 1} off {off}", poses(3, B, seed) * [8.0, 8.0, 1.0], 4,
                       wc_.random_world(300, seed + 1, B if per_car else None), off)


def edge_case(C, rows, seed=71):
    """C circles with the nearest placed last (so that a tile or a tail cut short loses it), G = 2; C = 0: the
    circles are None and the race-mate is the only obstacle."""
    x = poses(rows, 4, seed + C)
    if C == 0:
        return ContactCase(f"edge C 0 rows {rows}", x, 2, None)
    ci = wc_.random_world(C, seed + C + 1)
    ci[:, :2] *= 3.0  # far: the race-mates and the last circle are the near ones
    ci[-1] = [x[0, 0, 0], x[0, 0, 1], 0.5]  # over car 0 of row 0: (0.1651 - 0.5) - 0.3, below any mate's -0.6
    return ContactCase(f"edge C {C} rows {rows}", x, 2, ci)


def crowd_case(seed=81):
    """One race of 258 cars scattered within 8 m and 3 circles: the mates span two tiles."""
    rng = np.random.default_rng(seed)
    G = 258
    rad, phi = 8.0 * np.sqrt(rng.uniform(0, 1, G)), rng.uniform(-np.pi, np.pi, G)
    x = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(-np.pi, np.pi, G)], 1)
    return ContactCase("crowd G 258", x, G, wc_.random_world(3, seed + 1) * [3.0, 3.0, 1.0])


def batch_case(B, rows, seed=91):
    """B cars alone (G = 1) or in pairs in 40 circles: B = 1, 63, 65, 257 (under and over a wave, over a
    workgroup's 256 threads)."""
    G = 1 if B % 2 else 2
    x = np.stack([wc_.track_poses(B, seed + r) for r in range(rows)])
    x[..., :2] *= 0.5
    return ContactCase(f"batch B {B} rows {rows}", x, G, wc_.random_world(40, seed + B))


def track_case(B=8, G=4, seed=11):
    """make_race_grid in the track world's 1,040 circles."""
    return ContactCase("track", workload.make_race_grid(B // G, G, seed), G, wc_.track_world())


GRID = 1024      # clearance_grid's cap: a larger batch strides, a workgroup takes car b and then b + GRID
PASS = 8         # kClearPoses: the rows of a car that one pass takes
PASS_ROWS = (PASS, PASS + 1, 2 * PASS + 1)  # one whole pass; a second of one row; a third, after two whole ones
OFFSETS = (0.0, CENTER_OFFSET)


def rows_case(rows, off=CENTER_OFFSET, seed=101):
    """Two races of G = 3 in 40 circles, every row scattered anew within 3.2 m (a centre left over from the
    pass before is metres off, as is a mate read at row p for row r0 + p), and one circle over car 0 at the
    last row: at rows = 9 and 17 the nearest of the only pose of a pass cut short."""
    x = poses(rows, 6, seed + rows) * [8.0, 8.0, 1.0]
    ci = wc_.random_world(40, seed + rows + 1)
    # (|off| - 1) - 0.3 <= -1.13: under any mate's -0.6 and any other circle's (0 - 0.6) - 0.3
    ci[-1] = [x[rows - 1, 0, 0], x[rows - 1, 0, 1], 1.0]
    return ContactCase(f"rows {rows} G 3 off {off}", x, 3, ci, off)


def stride_case(per_car=True, off=CENTER_OFFSET, rows=2, G=5, C=3, seed=111):
    """B = GRID + 6 = 1030 cars within 3.2 m in races of G: the workgroups of cars 0..5 take cars 1024..1029
    too, on the same LDS. G = 5: races 204 (cars 1020..1024) and 205 (1025..1029) have their mates in other
    workgroups' strides. per_car: every car its own C circles, other ones for car b than for car b + GRID."""
    B = GRID + 6
    x = poses(rows, B, seed + rows + G) * [8.0, 8.0, 1.0]
    ci = wc_.random_world(C, seed + 1, B if per_car else None, spread=3.0)
    if per_car:
        assert (ci[:B - GRID] != ci[GRID:]).any(axis=(1, 2)).all(), "car b and car b + GRID: different worlds"
    return ContactCase(f"stride B {B} rows {rows} G {G} C {C} world_rows {B if per_car else 1} off {off}", x, G, ci, off)


def stride_rows_case(off=CENTER_OFFSET):
    """The second pass of the second car of a workgroup: B = 1030 in pairs, rows = 9, one circle per car."""
    return stride_case(True, off, rows=PASS + 1, G=2, C=1)


def oracle_cases():
    out = [random_case(False), random_case(True), random_case(False, 0.0), random_case(True, 0.0), crowd_case(), track_case()]
    out += [edge_case(C, rows) for C in (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1) for rows in (1, 5)]
    out += [batch_case(B, rows) for B in (1, 63, 65, 257) for rows in (1, 5)]
    out += [rows_case(rows, off) for rows in PASS_ROWS for off in OFFSETS]
    out += [stride_case(per_car, off) for per_car in (True, False) for off in OFFSETS]
    out += [stride_rows_case(off) for off in OFFSETS]
    return out


# ---- the rollout scene: a car a few plant steps short of a large circle straight ahead ------------------

BLOCK_R, BLOCK_GAP = 1.0, 0.012  # the circle's radius and the clearance of car 0 at row 0


def block_ahead(x, gap):
    """The circle of radius BLOCK_R whose face is `gap` metres ahead of the body of the car at pose x."""
    q = x[:2] + CENTER_OFFSET * np.array([np.cos(x[2]), np.sin(x[2])])
    c = q + (CAR_RADIUS + BLOCK_R + gap) * np.array([np.cos(x[2]), np.sin(x[2])])
    return [c[0], c[1], BLOCK_R]


WALLS = 1000  # make_world's first rows: the two walls of 500 circles


def crash_scene(B=8, G=4, seed=41, gap=BLOCK_GAP, blocked=(0,), gaps=None, per_car=False):
    """(x0 [B,3], circles [C,3]): make_race_grid in the track world, plus one circle of radius BLOCK_R per car of
    `blocked`, its face gaps[i] (default: `gap`) metres ahead of that car's body (a gap < 0: in contact at row 0).
    Without a path a car applies fail_u (0.5 m/s): 5 mm a tick, so the body reaches the face within three ticks.
    per_car: circles [B,1001,3], every car a world of its own: the track's walls and one more circle, the car's
    block or, for a car that has none, a circle out of everybody's reach."""
    x0 = workload.make_race_grid(B // G, G, seed)
    gaps = [gap] * len(blocked) if gaps is None else gaps
    blocks = [block_ahead(x0[b], g) for b, g in zip(blocked, gaps)]
    if not per_car:
        return x0, np.ascontiguousarray(np.concatenate([wc_.track_world(), blocks]))
    w = np.empty((B, WALLS + 1, 3))
    w[:, :WALLS] = wc_.track_world()[:WALLS]
    w[:, WALLS] = [60.0, 60.0, 0.1]
    w[list(blocked), WALLS] = blocks
    return x0, w


# The second scene: 65 races of four (two workgroups of the plant step, a last wave of four lanes). The races
# start at seeded places of one 58 m track and overlap there, which harms nothing (a car touches and sees its
# own race only) but for the blocks: hence crash_scene's per-car worlds. They hold the track's walls only: its
# obstacles stand 0.9 m off the path, and of 260 cars 0.4 m off it some would start inside one.
# Nine ticks, one more than the eight that would hold every crash: a free car plans at tick 0, solves at ticks 1 .. 6,
# holds at tick 7 and plans again at tick 8, and that second plan list is the one the waves ballot for with parked
# lanes among them.
WIDE_B, WIDE_G, WIDE_T = 260, 4, 9
# car -> gap: the first and the last lane of a wave (0 and 63, 64 and 255), both sides of the workgroup edge
# (255, 256), the batch's last car; one in contact at row 0, the others 5 mm a tick from their block (a car
# this close to a wall finds no plan), so at ticks 1 .. 5. Race 64 holds two of them, the second crashing
# behind the first.
WIDE_BLOCKED = {0: -0.05, 63: 0.003, 64: 0.007, 255: 0.012, 256: 0.017, 259: 0.022}


def wide_crash_scene():
    """(x0 [260,3], circles [260,1001,3])."""
    return crash_scene(WIDE_B, WIDE_G, 43, blocked=tuple(WIDE_BLOCKED), gaps=list(WIDE_BLOCKED.values()), per_car=True)


if __name__ == "__main__":
    for c in oracle_cases():
        v = np.sort(c.all_values(), axis=2)
        gap = float(np.nanmin(np.where(np.isfinite(v[..., 1]), v[..., 1] - v[..., 0], np.inf))) if v.shape[2] > 1 else np.inf
        print(f"{c.name:40s} tol {c.tol:.2e} closest pair {gap:.3e} skipped {int(c.skip().sum())} of {c.skip().size}")
