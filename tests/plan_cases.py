"""Adversarial scenes for the planning stage (csrc/plan_kernels.hip against oracle/plan_oracle.c):
dilation offset counts on both sides of the kernel's precomputed 8, scans whose computed beam count
disagrees with their length, waypoint lists full of exact and within-ulp distance ties, lists of 0
to 5,000 points, candidate tables with duplicated rows, the extreme table and grid shapes the ABI
admits, and poses far from the origin, at yaw +-pi and with non-unit quaternions. Every builder
returns the workload.make_scenes dict (plus "table" where it builds one). Shared by the CPU
restatement check (test_plan.py) and the GPU parity tests (test_gpu_plan_edges.py)."""
import numpy as np

from f110qp import workload

SEED = 31

# (dilation, discrete, offsets per axis of FillOccGrid's float loop): 1 is dilation 0 (the first
# offset is -0.0f), 8 the last count the kernel precomputes, 9 and 24 run its nested float loops
DILATION_CASES = ((0.0, 0.1, 1), (0.35, 0.1, 8), (0.4, 0.1, 9), (0.2, 0.05, 9), (0.6, 0.05, 24))
BEAM_COUNTS = (1, 63, 255, 257, 720)
WAYPOINT_COUNTS = (0, 1, 2, 63, 65, 255, 257)
TABLE_SHAPES = ((1, 2), (255, 1024), (255, 7), (7, 1023), (30, 333))  # (steer_discrete, traj_discrete)
GRID_SHAPES = ((7, 0.2, 35), (5, 0.3, 16), (1, 1.0, 1), (20, 0.1, 200), (10, 0.05, 200))  # (size, discrete, G)
FAR_SHIFT = (1000.0, -700.0)
QUAT_SCALES = (0.5, 3.0)


def dilation_over(dilation, discrete):
    return dict(dilation=np.float32(dilation), discrete=np.float32(discrete))


def grid_over(size, discrete):
    return dict(size=size, discrete=np.float32(discrete))


def base(B, seed=SEED):
    return workload.make_scenes(B, seed=seed)


def num_scans(sc):
    """FillOccGrid's beam count (occupancy_grid.cpp:66) in float32, before any clamp."""
    f = np.float32
    return int((f(sc["angle_max"]) - f(sc["angle_min"])) / f(sc["angle_inc"]) + f(1))


# ---- scan length ---------------------------------------------------------------------------------

def scan_truncated(B, beams=700):
    """The first `beams` ranges under the 1,080-beam angles: the computed count exceeds the scan."""
    sc = base(B)
    return dict(sc, ranges=np.ascontiguousarray(sc["ranges"][:, :beams]))


def scan_half_angle(B):
    """angle_max halved: the computed count stops short of the scan, whose unused tail holds 0.3 m
    returns that would mark cells around the car."""
    sc = base(B)
    sc = dict(sc, angle_max=np.float32(sc["angle_max"] / 2), ranges=sc["ranges"].copy())
    sc["ranges"][:, num_scans(sc):] = 0.3
    return sc


def scan_beams(B, beams):
    """The first `beams` ranges with an angle_max that makes the computed count exactly `beams`
    (half an increment past the last beam, so the float division cannot land on either side)."""
    sc = base(B)
    amax = np.float32(np.float64(sc["angle_min"]) + (beams - 0.5) * np.float64(sc["angle_inc"]))
    return dict(sc, ranges=np.ascontiguousarray(sc["ranges"][:, :beams]), angle_max=amax)


def scan_reversed(B):
    """angle_max < angle_min: a negative beam count, the fill loop never runs."""
    sc = base(B)
    return dict(sc, angle_min=sc["angle_max"], angle_max=sc["angle_min"])


# ---- waypoints -----------------------------------------------------------------------------------

def doubled_lap(B):
    """Two laps in one list: every waypoint distance ties exactly with its twin 500 places on."""
    sc = base(B)
    return dict(sc, waypoints=np.concatenate([sc["waypoints"]] * 2))


def tripled_lap(B):
    """A lap, its first row again (a closed CSV), then two more laps."""
    sc = base(B)
    wp = sc["waypoints"]
    return dict(sc, waypoints=np.concatenate([wp, wp[:1], wp, wp]))


def _near_lookahead(target, theta, span=24):
    """A float32 point near polar (target, theta) whose double distance from the origin is as close
    to `target` as the float32 lattice around it allows (search of (2 span + 1)^2 neighbours)."""
    f = np.float32
    x0, y0 = f(target * np.cos(theta)), f(target * np.sin(theta))
    k = np.arange(-span, span + 1)
    xs = (x0 + k * np.spacing(x0)).astype(np.float32)
    ys = (y0 + k * np.spacing(y0)).astype(np.float32)
    X, Y = np.meshgrid(xs.astype(np.float64), ys.astype(np.float64), indexing="ij")
    i, j = np.unravel_index(np.argmin(np.abs(np.sqrt(X * X + Y * Y) - target)), X.shape)
    return np.float64(xs[i]), np.float64(ys[j])


def ulp_tie_waypoints(seed, W=40, lookahead=2.5):
    """W waypoints ahead of a car at the origin with yaw 0, at radii lookahead + d where the d are
    a fraction of a float32 ulp apart on both sides of one float32 value, shuffled. Returns
    (waypoints [W,2], d [W] float64 = the reference's |dist - lookahead| of each, in double)."""
    rng = np.random.default_rng(seed)
    fbase = np.float32(rng.uniform(0.2, 1.2))
    ulp = np.float64(np.spacing(fbase))
    steps = rng.integers(-3, 4, W) * rng.choice([0.1, 0.25, 0.5, 0.49, 0.51, 1.0], W)
    wp = np.array([_near_lookahead(lookahead + np.float64(fbase) + s * ulp, th)
                   for s, th in zip(steps, rng.uniform(-1.2, 1.2, W))])
    wp = wp[rng.permutation(W)]
    d = np.abs(np.sqrt(wp[:, 0] ** 2 + wp[:, 1] ** 2) - np.float64(np.float32(lookahead)))
    return wp, d


def ulp_tie_scene(seed, beams=64):
    """One scene: the car at the origin with the identity quaternion (the rotation is exactly the
    identity, so the car-frame point is the float32 waypoint itself), nothing in range."""
    wp, d = ulp_tie_waypoints(seed)
    amin, ainc, amax = workload.scan_geometry(beams)
    sc = dict(pose=np.array([[0.0, 0.0, 0.0, 1.0]]), ranges=np.full((1, beams), 10.0, np.float32),
              angle_min=amin, angle_inc=ainc, angle_max=amax, waypoints=wp)
    return sc, d


def last_only_pose(wp):
    """A pose with only the last waypoint of `wp` ahead of it (car-frame x >= 0): just inside the
    convex path at that waypoint, facing out along the path's normal there."""
    L = wp[-1]
    n = np.array([L[0] / 12.0 ** 2, L[1] / 6.0 ** 2])  # outward normal of the 12 x 6 ellipse
    n /= np.hypot(*n)
    others = wp[:-1][np.any(wp[:-1] != L, axis=1)]
    depth = -((others - L) @ n)  # how far every other waypoint lies behind the tangent at L
    eps = 0.5 * depth.min() if len(depth) else 0.1
    yaw = np.arctan2(n[1], n[0])
    return np.array([L[0] - eps * n[0], L[1] - eps * n[1], np.sin(yaw / 2), np.cos(yaw / 2)])


def waypoint_count(B, W, special=4):
    """W waypoints sub-sampled evenly from the lap (W <= 2: its first points). The first `special`
    scenes have only the last waypoint ahead of the car, and a clear scan."""
    sc = base(B)
    full = sc["waypoints"]
    wp = full[:W] if W <= 2 else full[(np.arange(W) * len(full)) // W]
    sc = dict(sc, waypoints=np.ascontiguousarray(wp), pose=sc["pose"].copy(), ranges=sc["ranges"].copy())
    if W >= 1:
        sc["pose"][:special] = last_only_pose(wp)
        sc["ranges"][:special] = 10.0
    return sc


def fine_lap(B, W=5000, lo=4050, hi=4550):
    """A W-point resampling of the lap, with B cars whose nearest waypoint has an index in
    [lo, hi) (the lookahead adds 170 to 330 places there, short of the wrap): the winner lives in
    the last strides of the kernel's 256-thread folds."""
    wp = workload.track_waypoints(W)
    sc = workload.make_scenes(16 * B, seed=SEED, waypoints=wp)
    near = np.argmin(np.hypot(sc["pose"][:, None, 0] - wp[None, :, 0], sc["pose"][:, None, 1] - wp[None, :, 1]), 1)
    pick = np.nonzero((near >= lo) & (near < hi))[0][:B]
    assert len(pick) == B, len(pick)
    return dict(sc, pose=sc["pose"][pick].copy(), ranges=sc["ranges"][pick].copy())


# ---- candidate table -------------------------------------------------------------------------------

def duplicated_table(B, table, seed=SEED):
    """The table with every row listed twice, in a shuffled order. Returns (scenes with "table",
    rows [2T]: the row of the original table at each place)."""
    T = table.shape[0]
    rows = np.random.default_rng(seed).permutation(np.concatenate([np.arange(T), np.arange(T)]))
    return dict(base(B), table=np.ascontiguousarray(table[rows])), rows


# ---- pose --------------------------------------------------------------------------------------------

def far_origin(B, shift=FAR_SHIFT):
    sc = base(B)
    pose = sc["pose"].copy()
    pose[:, :2] += shift
    return dict(sc, pose=pose, waypoints=sc["waypoints"] + np.asarray(shift))


def axis_yaws(B):
    """Yaw exactly +-pi (qw = +-0, qz = +-1: the sign of the zero picks atan2's branch) and +-pi/2,
    cycled over the scenes."""
    h = np.sqrt(0.5)
    quats = [(1.0, 0.0), (1.0, -0.0), (-1.0, 0.0), (-1.0, -0.0), (h, h), (-h, h), (h, -h), (-h, -h)]
    sc = base(B)
    pose = sc["pose"].copy()
    pose[:, 2:] = [quats[b % len(quats)] for b in range(B)]
    return dict(sc, pose=pose)


def scaled_quaternions(B, scale):
    """Non-unit quaternions: tf2's setRotation normalises by 2 / |q|^2, GetCarOrientation does not."""
    sc = base(B)
    pose = sc["pose"].copy()
    pose[:, 2:] *= scale
    return dict(sc, pose=pose)
