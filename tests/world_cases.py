"""The simulated LiDAR's CPU side (test_gpu_world_scan.py, test_gpu_rollout_world.py): the numpy oracle
(workload._ray_circles on the angles of include/f110qp.h), the grazing classifier and the worlds.

Tolerance, derived: |gpu - oracle| <= ulp32(oracle) + 4e-9 m on every beam that is not grazing. A device
sincos within a few ulp moves d2 by about 1e-13 m^2 at these coordinates (|p| up to ~20 m, 2 |p|^2 eps64).
A beam is grazing if, in the oracle, some circle has t > 0 and |d2 - r^2| < 1e-9 m^2, or |th| < 1e-9, or
|t| < 1e-9: there a hit can flip. Off such beams the square root moves by at most 1e-13 / (2 sqrt(1e-9)) =
1.6e-9 m, and the float rounding can then differ by one ulp and no more. A case may skip at most 0.1 % of
its beams; the check asserts that cap.

    python tests/world_cases.py      # the grazing count of every hand-made case and of the track world
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "f110-mpc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from f110qp import workload  # noqa: E402

LIDAR_OFFSET, MAX_RANGE = 0.275, 10.0
TILE = 256            # F110QP_CAST_CIRCLE_TILE
GRAZE = 1e-9          # the three grazing thresholds
ABS_TOL = 4e-9        # metres, next to one float32 ulp
SKIP_CAP = 1e-3       # grazing beams a case may skip


def geometry(beams, kind="2pi"):
    """(angle_min, angle_increment, angle_max) as float32: a full turn from -pi (the last beam one
    increment short of +pi: the interval wraps between beams R - 1 and 0) or the 270 degree scan."""
    if kind == "2pi":
        return workload.scan_geometry(beams)
    amin = np.float32(-0.75 * np.pi)
    ainc = np.float32(1.5 * np.pi / max(beams - 1, 1))
    return amin, ainc, np.float32(amin + ainc * (beams - 1))


def _terms(x, circles, geom, beams, lidar_offset=LIDAR_OFFSET):
    """The oracle's intermediate values, [B, R, C] each, in workload._ray_circles' expressions."""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    ci = np.broadcast_to(circles, (B,) + circles.shape[-2:]) if circles.ndim == 2 else circles
    ang = x[:, 2:3] + (geom[0] + geom[1] * np.arange(beams, dtype=np.float64))[None, :]
    ox, oy = x[:, 0] + lidar_offset * np.cos(x[:, 2]), x[:, 1] + lidar_offset * np.sin(x[:, 2])
    dx, dy = np.cos(ang), np.sin(ang)
    with np.errstate(invalid="ignore", over="ignore"):
        px = ci[:, None, :, 0] - ox[:, None, None]
        py = ci[:, None, :, 1] - oy[:, None, None]
        t = px * dx[..., None] + py * dy[..., None]
        d2 = px * px + py * py - t * t
        r2 = (ci[:, :, 2] * ci[:, :, 2])[:, None, :]
        th = t - np.sqrt(np.maximum(r2 - d2, 0.0))
    return ox, oy, ang, ci, t, d2, r2, th


def _per_car(fn, x, circles, *a):
    """fn car by car (its [R, C] intermediates of a 1,040-circle world are 9 MB a car), stacked. A finite
    circle whose near face is more than max_range + 1 m from the pose is left out: its th exceeds max_range
    by 0.7 m at least (the LiDAR is 0.275 m from the pose), so it changes neither the minimum nor a hit
    below max_range; dropping it from the classifier can only keep more beams in the comparison."""
    x = np.asarray(x, np.float64)
    out = []
    for b in range(len(x)):
        ci = circles if circles.ndim == 2 else circles[b]
        with np.errstate(invalid="ignore", over="ignore"):
            far = np.hypot(ci[:, 0] - x[b, 0], ci[:, 1] - x[b, 1]) - np.abs(ci[:, 2]) > MAX_RANGE + 1.0
        out.append(fn(x[b:b + 1], ci[~(far & np.isfinite(ci).all(axis=1))][None], *a))
    return np.concatenate(out)


def oracle_scan(x, circles, geom, beams, max_range=MAX_RANGE, lidar_offset=LIDAR_OFFSET):
    """ranges [B, R] float32 of poses x [B, 3] in circles [C, 3] or [B, C, 3]: workload._ray_circles."""
    if len(x) > 1:
        return _per_car(oracle_scan, x, circles, geom, beams, max_range, lidar_offset)
    ox, oy, ang, ci, *_ = _terms(x, circles, geom, beams, lidar_offset)
    if ci.shape[1] == 0:
        return np.full((len(ox), beams), np.float32(max_range))
    with np.errstate(invalid="ignore", over="ignore"):
        return workload._ray_circles(ox, oy, ang, ci[:, :, 0], ci[:, :, 1], ci[:, :, 2], max_range).astype(np.float32)


def grazing(x, circles, geom, beams, lidar_offset=LIDAR_OFFSET):
    """[B, R] bool: the beams on which a hit can flip under a few ulp of sincos (module docstring)."""
    if len(x) > 1:
        return _per_car(grazing, x, circles, geom, beams, lidar_offset)
    *_, ci, t, d2, r2, th = _terms(x, circles, geom, beams, lidar_offset)
    if ci.shape[1] == 0:
        return np.zeros(t.shape[:2], bool)
    with np.errstate(invalid="ignore"):
        g = ((t > 0) & (np.abs(d2 - r2) < GRAZE)) | (np.abs(th) < GRAZE) | (np.abs(t) < GRAZE)
    return g.any(axis=2)


def check_scan(got, x, circles, geom, beams, what="", max_range=MAX_RANGE):
    """got [B, R] float32 against the oracle on every non-grazing beam, and the cap on the skipped ones.
    Returns (skipped, worst error in units of the bound)."""
    want = oracle_scan(x, circles, geom, beams, max_range)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    skip = grazing(x, circles, geom, beams)
    assert skip.sum() <= SKIP_CAP * skip.size, f"{what}: {int(skip.sum())} of {skip.size} beams are grazing"
    w = want.astype(np.float64)
    bound = np.spacing(want).astype(np.float64) + ABS_TOL
    err = np.abs(got.astype(np.float64) - w)
    bad = (err > bound) & ~skip
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])
    return int(skip.sum()), float((err / bound)[~skip].max())


# ---- worlds ------------------------------------------------------------------------------------------

def track_world():
    """The issue's track world: walls + 40 obstacles from default_rng(5), [1040, 3]."""
    return workload.make_world(seed=5, obstacles=40)


def track_poses(B, seed=3):
    """make_scenes poses as states [B, 3] (x, y, yaw)."""
    pose = workload.make_scenes(B, seed=seed)["pose"]
    return np.ascontiguousarray(np.stack([pose[:, 0], pose[:, 1], 2.0 * np.arctan2(pose[:, 2], pose[:, 3])], 1))


def random_world(C, seed, B=None, spread=9.0):
    """C circles of radius 0.05 .. 0.6 scattered within `spread` metres of the origin (some past max_range
    of any pose near it), [C, 3] or, with B, one world per car [B, C, 3]."""
    rng = np.random.default_rng(seed)
    shape = (C,) if B is None else (B, C)
    rad = rng.uniform(0.8, spread * 1.3, shape)
    phi = rng.uniform(-np.pi, np.pi, shape)
    return np.ascontiguousarray(np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(0.05, 0.6, shape)], -1))


def poses_near_origin(B, seed, yaws=()):
    """B poses within 0.4 m of the origin; the first len(yaws) take those headings."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-0.4, 0.4, B), rng.uniform(-0.4, 0.4, B), rng.uniform(-np.pi, np.pi, B)], 1)
    for i, y in enumerate(yaws[:B]):
        x[i, 2] = y
    return x


YAWS = (np.pi, -np.pi, np.pi / 2, -np.pi / 2)


def _ahead(x, dist, r, bearing=0.0):
    """A circle whose centre is `dist` from the LiDAR of pose x at `bearing` from the heading."""
    ox, oy = x[0] + LIDAR_OFFSET * np.cos(x[2]), x[1] + LIDAR_OFFSET * np.sin(x[2])
    return [ox + dist * np.cos(x[2] + bearing), oy + dist * np.sin(x[2] + bearing), r]


def hand_cases(geom, beams):
    """name -> (x [B, 3], circles [C, 3], what the case is about) for a scan geometry. The cases built to
    sit on a threshold compare only the beams the classifier keeps. "Dead ahead" is along beam R // 2, so
    that one beam meets the near face head-on: its range is the face distance to a few ulp64."""
    f = np.float32
    x = np.array([[0.3, -0.2, 0.4]])
    on_beam = float(geom[0]) + float(geom[1]) * (beams // 2)
    cases = {}
    # the near face exactly at max_range and at its two float32 neighbours: centre distance = face + r
    for name, face in (("at max_range", 10.0), ("one float below max_range", float(np.nextafter(f(10), f(0)))),
                       ("one float above max_range", float(np.nextafter(f(10), f(20))))):
        cases[name] = (x, np.array([_ahead(x[0], face + 0.5, 0.5, on_beam)]), "a circle dead ahead, near face " + name)
    cases["behind"] = (x, np.array([_ahead(x[0], 3.0, 0.4, np.pi - 0.002), _ahead(x[0], 5.0, 0.3, 0.301)]),
                       "a circle behind the LiDAR (t < 0 on the front beams) next to one ahead")
    cases["inside"] = (x, np.array([_ahead(x[0], 0.1, 0.6, 0.7), _ahead(x[0], 4.0, 0.3, -0.2003)]),
                       "the LiDAR inside a circle: it sees through it to the one beyond")
    fin = [_ahead(x[0], 3.0, 0.4, 0.1007), _ahead(x[0], 2.0, 0.2, -1.0003)]
    bad = []
    for k in range(3):
        for v in (np.nan, np.inf, -np.inf):
            c = _ahead(x[0], 2.5, 0.3, 0.0501)
            c[k] = v
            bad.append(c)
    cases["non-finite"] = (x, np.array(bad[:5] + fin[:1] + bad[5:] + fin[1:]),
                           "NaN and +-inf in each field, between finite circles")
    # two rows of small circles at 3 m and 3.05 m, offset by half a pitch: the nearer hit alternates
    alt = [_ahead(x[0], 3.0 + 0.05 * (k % 2), 0.02, -0.5 + k * 0.0117) for k in range(86)]
    cases["alternating"] = (x, np.array(alt), "two rows whose nearer hit alternates from beam to beam")
    return cases


if __name__ == "__main__":
    for beams in (1080,):
        for kind in ("2pi", "270"):
            g = geometry(beams, kind)
            for name, (x, ci, _) in hand_cases(g, beams).items():
                print(f"{kind:4s} {name:28s} grazing {int(grazing(x, ci, g, beams).sum())} of {beams}")
    w, xs = track_world(), track_poses(64)
    g = geometry(1080)
    print("track world:", int(grazing(xs, w, g, 1080).sum()), "of", 64 * 1080, "beams grazing;",
          "in-range circles per car", np.sort((np.hypot(w[None, :, 0] - xs[:, None, 0], w[None, :, 1] - xs[:, None, 1])
                                              - w[None, :, 2] <= 10.3).sum(1))[[0, -1]])
