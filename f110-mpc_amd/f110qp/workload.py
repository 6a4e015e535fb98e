"""Synthetic tick batches for the f110qp hot path, numpy only.

The reference ships no datasets; its inputs come from the simulator. The generator follows
the reference's own recipe for a candidate trajectory:
  - mini paths: Traj_Plan::generate_traj_table (src/trajectory_planner.cpp:26-72), i.e.
    `traj_discrete`=50 states from (0,0,0) by Model::simulate_dynamics (src/model.cpp:61-75,
    CAR_LENGTH = 0.35) at constant speed and steer, dt = 0.01;
  - car -> world with Transforms::CarPointToWorldPoint (src/transforms.cpp:3-20), as float;
  - ori = 0 for every reference state (src/project.cpp:147), or the true heading;
  - u_lin = (4.5, steer): v is forced to 4.5 before MPC::Update (src/project.cpp:170);
  - half spaces from FindHalfSpaces on a synthetic 1080-beam scan with one guaranteed gap.
All arrays are in the include/f110qp.h layouts (float32, row-major).
"""
from __future__ import annotations

import math

import numpy as np

CAR_LENGTH = 0.35  # src/model.cpp:2
TRAJ_POINTS = 50   # params.yaml:57 traj_discrete
SPEED = 4.5        # params.yaml:46 umax; project.cpp:170


def mini_paths(steer, speed=SPEED, dt=0.01, points=TRAJ_POINTS):
    """Vectorised generate_traj_table rollouts: steer [B] -> car-frame states [B, points, 3]."""
    steer = np.asarray(steer, np.float64).reshape(-1)
    B = steer.shape[0]
    out = np.zeros((B, points, 3))
    s = np.zeros((B, 3))
    for k in range(1, points):  # trajectory_planner.cpp:291-297
        d0 = speed * np.cos(s[:, 2])
        d1 = speed * np.sin(s[:, 2])
        d2 = np.tan(steer) * speed / CAR_LENGTH
        s = s + np.stack([d0, d1, d2], 1) * dt
        out[:, k] = s
    return out


def car_to_world(px, py, pose):
    """CarPointToWorldPoint: rotate by the pose yaw, add the (float) position -> float32."""
    th = pose[:, 2:3].astype(np.float64)
    c, s = np.cos(th), np.sin(th)
    wx = c * px - s * py + pose[:, 0:1].astype(np.float32).astype(np.float64)
    wy = s * px + c * py + pose[:, 1:2].astype(np.float32).astype(np.float64)
    return wx.astype(np.float32), wy.astype(np.float32)


def make_batch(batch: int, horizon: int, seed: int = 0, heading: str = "zero", lateral: float = 0.3,
               steer_range: float = 0.4):
    """Independent ticks (configs C2/C3 of BASELINE.json). Returns dict(x0, u_lin, x_ref)."""
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-50, 50, batch), rng.uniform(-50, 50, batch),
                   rng.uniform(-np.pi, np.pi, batch)], 1).astype(np.float32)
    u_lin = np.stack([np.full(batch, SPEED), rng.uniform(-steer_range, steer_range, batch)], 1).astype(np.float32)
    steer = rng.uniform(-steer_range, steer_range, batch)
    off = rng.uniform(-lateral, lateral, batch)
    path = mini_paths(steer)
    x_ref = _to_ref(path, off, x0, horizon, heading)
    return dict(x0=x0, u_lin=u_lin, x_ref=x_ref)


def _to_ref(path, off, x0, horizon, heading):
    px = path[:, :horizon, 0]
    py = path[:, :horizon, 1] + off[:, None]
    wx, wy = car_to_world(px, py, x0)
    if heading == "zero":
        ori = np.zeros_like(wx)
    else:
        ori = (x0[:, 2:3].astype(np.float64) + path[:, :horizon, 2]).astype(np.float32)
    return np.ascontiguousarray(np.stack([wx, wy, ori], 2), np.float32)


def make_grouped_batch(scenarios: int, horizon: int, seed: int = 0, lanes=(0.0, 0.25, -0.25, 0.5, -0.5, 0.75),
                       steers: int = 20, steer_range: float = 0.4, heading: str = "zero"):
    """Config C4: per scenario one car state and linearisation point shared by
    len(lanes) x steers candidate mini paths (lateral lane offset x steer value)."""
    rng = np.random.default_rng(seed)
    G = len(lanes) * steers
    x0s = np.stack([rng.uniform(-50, 50, scenarios), rng.uniform(-50, 50, scenarios),
                    rng.uniform(-np.pi, np.pi, scenarios)], 1).astype(np.float32)
    uls = np.stack([np.full(scenarios, SPEED), rng.uniform(-steer_range, steer_range, scenarios)], 1).astype(np.float32)
    steer_vals = np.linspace(-steer_range, steer_range, steers)
    st = np.tile(steer_vals, len(lanes))
    off = np.repeat(np.asarray(lanes, np.float64), steers)
    path = mini_paths(st)
    x0 = np.repeat(x0s, G, 0)
    u_lin = np.repeat(uls, G, 0)
    x_ref = _to_ref(np.tile(path, (scenarios, 1, 1)), np.tile(off, scenarios), x0, horizon, heading)
    return dict(x0=x0, u_lin=u_lin, x_ref=x_ref, group_size=G)


SCAN_BEAMS = 1080


def scan_geometry(beams: int = SCAN_BEAMS):
    amin = np.float32(-np.pi)
    ainc = np.float32(2 * np.pi / beams)
    amax = np.float32(amin + ainc * (beams - 1))
    return amin, ainc, amax


def make_scans(batch: int, seed: int = 0, beams: int = SCAN_BEAMS, gap_center=0.6, gap_width=(0.3, 0.9)):
    """Synthetic LaserScans: short returns (1-2.5 m, below follow_gap_thresh = 3,
    params.yaml:49) everywhere except one arc of long returns (4-10 m) near the heading."""
    rng = np.random.default_rng(seed + 7919)
    amin, ainc, amax = scan_geometry(beams)
    ang = amin + ainc * np.arange(beams, dtype=np.float64)
    r = rng.uniform(1.0, 2.5, (batch, beams)).astype(np.float32)
    ctr = rng.uniform(-gap_center, gap_center, batch)
    w = rng.uniform(gap_width[0], gap_width[1], batch)
    m = np.abs(ang[None, :] - ctr[:, None]) < (w[:, None] / 2)
    r[m] = rng.uniform(4.0, 10.0, int(m.sum())).astype(np.float32)
    return r, amin, ainc, amax


def make_stream(batch: int, horizon: int, ticks: int, seed: int = 0, dt: float = 0.01, heading_change_every: int = 0):
    """Config C5: `ticks` consecutive control ticks of `batch` independent cars. Each car keeps
    its mini path (the reference re-plans only near the path end, src/project.cpp:180-188)
    while x0 advances 4.5*dt along the heading per tick; u_lin keeps v = 4.5 and the steer of
    the previous tick. With heading_change_every = k > 0 a tenth of the cars also turn by a
    small angle every k ticks (their linearisation point changes). Returns a list of dicts."""
    base = make_batch(batch, horizon, seed=seed)
    rng = np.random.default_rng(seed + 17)
    x0 = base["x0"].astype(np.float64).copy()
    ticks_out = []
    turners = rng.random(batch) < 0.1
    for t in range(ticks):
        if t > 0:
            x0[:, 0] += SPEED * dt * np.cos(x0[:, 2])
            x0[:, 1] += SPEED * dt * np.sin(x0[:, 2])
            if heading_change_every and t % heading_change_every == 0:
                x0[turners, 2] += rng.uniform(-0.05, 0.05, int(turners.sum()))
        ticks_out.append(dict(x0=x0.astype(np.float32), u_lin=base["u_lin"].copy(), x_ref=base["x_ref"].copy()))
    return ticks_out


def simulate_dynamics(x, u, dt=0.01):
    """Model::simulate_dynamics (src/model.cpp:61-75, CAR_LENGTH = 0.35), vectorised fp64:
    x [B,3] (x, y, ori), u [B,2] (v, steer) -> the state one Euler step later."""
    x = np.asarray(x, np.float64)
    u = np.asarray(u, np.float64)
    d = np.stack([u[:, 0] * np.cos(x[:, 2]), u[:, 0] * np.sin(x[:, 2]), np.tan(u[:, 1]) * u[:, 0] / CAR_LENGTH], 1)
    return x + d * dt


def closed_loop_stream(solve, batch: int, horizon: int, ticks: int, seed: int = 0, dt: float = 0.01,
                       replan_every: int = 5, lateral: float = 0.3, steer_range: float = 0.4):
    """Config C5 as a closed receding-horizon loop (project::OdomCallback's MPC branch,
    src/project.cpp:160-198, driven by a simulated car). Per tick and car:
      - x0 = the car's pose (x, y, GetCarOrientation), so theta0 changes every tick;
      - u_lin = GetNextInput() with v forced to 4.5 (project.cpp:163-170): the steer of the
        previous solution's next input u*_1 (u*_0 is applied first);
      - x_ref = the first N states of the car's current mini path; the path is re-planned from the
        current pose every `replan_every` ticks (the reference re-plans within 1.98 m of the end
        of its 2.2 m mini path, project.cpp:180-188), staggered over the cars;
      - then the plant advances: x0 <- simulate_dynamics(x0, u*_0, dt) (model.cpp:61-75).
    `solve(x0, u_lin, x_ref) -> u [B, N, 2]` is the solver that closes the loop (a GPU back end or
    the oracle). Returns the list of tick dicts (x0, u_lin, x_ref), float32 ABI layouts."""
    rng = np.random.default_rng(seed)
    base = make_batch(batch, horizon, seed=seed, lateral=lateral, steer_range=steer_range)
    x = base["x0"].astype(np.float64)
    ul = base["u_lin"].copy()
    xr = base["x_ref"].copy()
    out = []
    for t in range(ticks):
        if t > 0:
            rp = (np.arange(batch) + t) % replan_every == 0
            n = int(rp.sum())
            if n:
                x0f = x[rp].astype(np.float32)
                path = mini_paths(rng.uniform(-steer_range, steer_range, n))
                xr[rp] = _to_ref(path, rng.uniform(-lateral, lateral, n), x0f, horizon, "zero")
        x0 = x.astype(np.float32)
        tick = dict(x0=x0, u_lin=ul.copy(), x_ref=xr.copy())
        out.append(tick)
        u = np.asarray(solve(tick["x0"], tick["u_lin"], tick["x_ref"]), np.float64)
        ok = np.isfinite(u).all(axis=(1, 2))
        u0 = np.where(ok[:, None], u[:, 0], np.stack([np.full(batch, 0.5), np.zeros(batch)], 1))  # Input(0.5, 0)
        x = simulate_dynamics(x, u0, dt)
        nxt = u[:, 1] if horizon > 1 else u[:, 0]
        ul = np.stack([np.full(batch, SPEED), np.where(ok, nxt[:, 1], ul[:, 1])], 1).astype(np.float32)
    return out


def warm_key_hit_rate(ticks) -> float:
    """Fraction of (car, tick > 0) whose linearisation point bits (theta0, v, steer) equal the
    previous tick's: the wave back end's warm W = H^-1 cache hits exactly then."""
    hits = tot = 0
    for a, b in zip(ticks[:-1], ticks[1:]):
        same = (a["x0"][:, 2].view(np.uint32) == b["x0"][:, 2].view(np.uint32)) & \
               (a["u_lin"].view(np.uint32) == b["u_lin"].view(np.uint32)).all(axis=1)
        hits += int(same.sum())
        tot += same.size
    return hits / max(1, tot)


# ---- planning scenes (pose + LaserScan + global path) for the device planning stage -----------

def track_waypoints(n: int = 500, a: float = 12.0, b: float = 6.0) -> np.ndarray:
    """A closed elliptical global path of n points (x, y as float32 values, like the CSV)."""
    t = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    return np.stack([a * np.cos(t), b * np.sin(t)], 1).astype(np.float32).astype(np.float64)


def _ray_circles(ox, oy, ang, cx, cy, rad, max_range):
    """Ray casting: ranges [B, R] from origins (ox, oy) [B] along angles [B, R] against circles
    (cx, cy, rad) [B, C]."""
    dx, dy = np.cos(ang), np.sin(ang)                       # [B, R]
    px = cx[:, None, :] - ox[:, None, None]                 # [B, 1, C]
    py = cy[:, None, :] - oy[:, None, None]
    t = px * dx[..., None] + py * dy[..., None]             # projection, [B, R, C]
    d2 = px * px + py * py - t * t
    r2 = (rad * rad)[:, None, :]
    hit = (d2 <= r2) & (t > 0)
    th = t - np.sqrt(np.maximum(r2 - d2, 0.0))
    th = np.where(hit & (th > 0), th, np.inf)
    return np.minimum(th.min(axis=2), max_range)


def make_scenes(batch: int, seed: int = 0, beams: int = SCAN_BEAMS, obstacles: int = 6, waypoints=None,
                max_range: float = 10.0):
    """Scenarios for project::OdomCallback's planning branch: a car near the global path with the
    path heading (+ noise), its 1080-beam 2*pi LaserScan (from the lidar 0.275 m ahead, as
    OccGrid::FillOccGrid assumes, occupancy_grid.cpp:63-64) of the two track walls (circles along
    the path at +-1.6 m) and a few obstacles. Returns dict(pose [B,4] f64 (x, y, qz, qw),
    ranges [B,beams] f32, geometry, waypoints [W,2] f64)."""
    rng = np.random.default_rng(seed)
    wp = track_waypoints() if waypoints is None else np.asarray(waypoints, np.float64)[:, :2]
    W = wp.shape[0]
    k = rng.integers(0, W, batch)
    nxt = wp[(k + 1) % W]
    hd = np.arctan2(nxt[:, 1] - wp[k, 1], nxt[:, 0] - wp[k, 0])
    yaw = hd + rng.uniform(-0.3, 0.3, batch)
    off = rng.uniform(-0.4, 0.4, batch)
    x = wp[k, 0] - np.sin(hd) * off
    y = wp[k, 1] + np.cos(hd) * off
    pose = np.stack([x, y, np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    # walls: circles of radius 0.12 every ~0.25 m along the path, +-1.6 m laterally
    hw = np.arctan2(np.roll(wp[:, 1], -1) - wp[:, 1], np.roll(wp[:, 0], -1) - wp[:, 0])
    wall = np.concatenate([wp + 1.6 * np.stack([-np.sin(hw), np.cos(hw)], 1),
                           wp - 1.6 * np.stack([-np.sin(hw), np.cos(hw)], 1)])
    # only the wall circles within max_range of the car matter
    amin, ainc, amax = scan_geometry(beams)
    ang = yaw[:, None] + (amin + ainc * np.arange(beams, dtype=np.float64))[None, :]
    lx, ly = x + 0.275 * np.cos(yaw), y + 0.275 * np.sin(yaw)
    d = np.hypot(wall[None, :, 0] - lx[:, None], wall[None, :, 1] - ly[:, None])
    near = np.argsort(d, axis=1)[:, :160]
    cx = np.take_along_axis(np.broadcast_to(wall[:, 0], d.shape), near, 1)
    cy = np.take_along_axis(np.broadcast_to(wall[:, 1], d.shape), near, 1)
    rad = np.full(cx.shape, 0.12)
    # obstacles 1-4 m ahead in a +-60 degree cone
    ob_r = rng.uniform(1.0, 4.0, (batch, obstacles))
    ob_a = yaw[:, None] + rng.uniform(-1.0, 1.0, (batch, obstacles))
    cx = np.concatenate([cx, lx[:, None] + ob_r * np.cos(ob_a)], 1)
    cy = np.concatenate([cy, ly[:, None] + ob_r * np.sin(ob_a)], 1)
    rad = np.concatenate([rad, rng.uniform(0.1, 0.35, (batch, obstacles))], 1)
    ranges = _ray_circles(lx, ly, ang, cx, cy, rad, max_range).astype(np.float32)
    return dict(pose=pose, ranges=ranges, angle_min=amin, angle_inc=ainc, angle_max=amax, waypoints=wp)


def drive_stream(ticks: int, seed: int = 0, step: float = 0.09, beams: int = SCAN_BEAMS, obstacles: int = 40,
                 max_range: float = 10.0):
    """A scripted drive for the project node's callbacks: the car follows the elliptical path
    (4.5 m/s x 20 ms per tick = 0.09 m, src/project.cpp:233-235) with a small lateral wobble; the
    world holds the two track walls and `obstacles` static circles beside the path. Returns
    dict(pose [T,4] f64, ranges [T,beams] f32, geometry, waypoints [W,2])."""
    rng = np.random.default_rng(seed)
    wp = track_waypoints()
    W = wp.shape[0]
    seg = np.hypot(*(np.roll(wp, -1, 0) - wp).T)
    s_along = np.concatenate([[0.0], np.cumsum(seg)])
    total = s_along[-1]
    s0 = rng.uniform(0, total)
    s = (s0 + step * np.arange(ticks)) % total
    k = np.searchsorted(s_along, s, side="right") - 1
    frac = (s - s_along[k]) / seg[k]
    nxt = wp[(k + 1) % W]
    base = wp[k] + (nxt - wp[k]) * frac[:, None]
    hd = np.arctan2(nxt[:, 1] - wp[k, 1], nxt[:, 0] - wp[k, 0])
    lat = 0.2 * np.sin(np.arange(ticks) * 0.15)
    x = base[:, 0] - np.sin(hd) * lat
    y = base[:, 1] + np.cos(hd) * lat
    yaw = hd + 0.05 * np.cos(np.arange(ticks) * 0.2)
    pose = np.stack([x, y, np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    hw = np.arctan2(np.roll(wp[:, 1], -1) - wp[:, 1], np.roll(wp[:, 0], -1) - wp[:, 0])
    nrm = np.stack([-np.sin(hw), np.cos(hw)], 1)
    wall = np.concatenate([wp + 1.6 * nrm, wp - 1.6 * nrm])
    oi = rng.integers(0, W, obstacles)
    obst = wp[oi] + nrm[oi] * rng.choice([-0.9, 0.9], obstacles)[:, None]
    cxs = np.concatenate([wall[:, 0], obst[:, 0]])
    cys = np.concatenate([wall[:, 1], obst[:, 1]])
    rads = np.concatenate([np.full(len(wall), 0.12), rng.uniform(0.15, 0.3, obstacles)])
    amin, ainc, amax = scan_geometry(beams)
    ang = yaw[:, None] + (amin + ainc * np.arange(beams, dtype=np.float64))[None, :]
    lx, ly = x + 0.275 * np.cos(yaw), y + 0.275 * np.sin(yaw)
    d = np.hypot(cxs[None, :] - lx[:, None], cys[None, :] - ly[:, None])
    near = np.argsort(d, axis=1)[:, :200]
    ranges = _ray_circles(lx, ly, ang, cxs[near], cys[near], rads[near], max_range).astype(np.float32)
    return dict(pose=pose, ranges=ranges, angle_min=amin, angle_inc=ainc, angle_max=amax, waypoints=wp)


def make_world(seed: int = 0, obstacles: int = 40) -> np.ndarray:
    """The static world drive_stream(seed=seed, obstacles=obstacles) builds internally, as circles [C, 3]
    float64 = (cx, cy, r): the two track walls (radius 0.12 at +-1.6 m of every waypoint) followed by the
    `obstacles` circles beside the path, drawn from the same generator in the same order. The input of
    the device ray casting (f110qp_cast_scans_dev, f110qp_rollout_world[_dev])."""
    rng = np.random.default_rng(seed)
    wp = track_waypoints()
    W = wp.shape[0]
    rng.uniform(0, np.hypot(*(np.roll(wp, -1, 0) - wp).T).sum())  # drive_stream draws its start first
    hw = np.arctan2(np.roll(wp[:, 1], -1) - wp[:, 1], np.roll(wp[:, 0], -1) - wp[:, 0])
    nrm = np.stack([-np.sin(hw), np.cos(hw)], 1)
    wall = np.concatenate([wp + 1.6 * nrm, wp - 1.6 * nrm])
    oi = rng.integers(0, W, obstacles)
    obst = wp[oi] + nrm[oi] * rng.choice([-0.9, 0.9], obstacles)[:, None]
    rads = np.concatenate([np.full(len(wall), 0.12), rng.uniform(0.15, 0.3, obstacles)])
    return np.ascontiguousarray(np.concatenate([np.concatenate([wall, obst]), rads[:, None]], 1))


# ---- head-to-head races (f110qp_cast_scans_race_dev, f110qp_rollout_race[_dev]) ------------------------

def race_circles(x, group_size: int, car_radius: float = 0.3, center_offset: float = 0.1651) -> np.ndarray:
    """The opponent circles of include/f110qp.h's race model, [B, G - 1, 3] float64: the B poses x [B, 3] are
    B / G races of G consecutive cars, and row b holds, for every other car m of b's race in the order of
    the car index (the own car left out), (x_m + center_offset cos(ori_m), y_m + center_offset sin(ori_m),
    car_radius). The oracle of what the device builds; at center_offset = 0 the centres are the poses' bits."""
    x = np.asarray(x, np.float64)
    B, G = x.shape[0], int(group_size)
    if G < 1 or B % G:
        raise ValueError(f"group_size must be >= 1 and divide B = {B}, got {G}")
    with np.errstate(invalid="ignore"):
        c = np.stack([x[:, 0] + center_offset * np.cos(x[:, 2]), x[:, 1] + center_offset * np.sin(x[:, 2]),
                      np.full(B, float(car_radius))], 1)
    own = np.arange(B) % G
    k = np.arange(G - 1)[None, :]
    mate = (np.arange(B) - own)[:, None] + k + (k >= own[:, None])
    return np.ascontiguousarray(c[mate].reshape(B, G - 1, 3))


def clearance(x, circles, group_size: int = 1, car_radius: float = 0.3, center_offset: float = 0.1651):
    """The contact model of include/f110qp.h (f110qp_clearance_dev) in numpy, the device kernel's expressions in
    its order: poses x [rows, B, 3] (or [B, 3]) in circles [C, 3], [B, C, 3] or None -> (clearance [rows, B]
    float64, nearest [rows, B] int32). Body centre q = (x + off cos(ori), y + off sin(ori)); per static circle
    v = (sqrt(dx dx + dy dy) - |r|) - R with d = c - q; per race-mate (race_circles at the same row, its centre
    minus q) v = (d - R) - R; the minimum, the lowest index on equal values (j, or C + i for the mate with index
    i inside the race), NaN values never chosen, +inf and -1 without a candidate."""
    x = np.asarray(x, np.float64)
    one = x.ndim == 2
    x = x[None] if one else x
    rows, B = x.shape[:2]
    G, R = int(group_size), float(car_radius)
    ci = np.zeros((0, 3)) if circles is None else np.asarray(circles, np.float64)
    Cn = ci.shape[-2]
    own = np.arange(B) % G
    k = np.arange(G - 1)[None, :]
    mate_idx = Cn + k + (k >= own[:, None])                      # [B, G - 1]: C + index inside the race
    clear = np.full((rows, B), np.inf)
    near = np.full((rows, B), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rows):
            qx = x[r, :, 0] + center_offset * np.cos(x[r, :, 2])
            qy = x[r, :, 1] + center_offset * np.sin(x[r, :, 2])
            cw = np.broadcast_to(ci, (B, Cn, 3)) if ci.ndim == 2 else ci
            dx, dy = cw[:, :, 0] - qx[:, None], cw[:, :, 1] - qy[:, None]
            v = (np.sqrt(dx * dx + dy * dy) - np.abs(cw[:, :, 2])) - R
            idx = np.broadcast_to(np.arange(Cn)[None, :], (B, Cn))
            if G > 1:
                m = race_circles(x[r], G, car_radius, center_offset)
                dx, dy = m[:, :, 0] - qx[:, None], m[:, :, 1] - qy[:, None]
                v = np.concatenate([v, (np.sqrt(dx * dx + dy * dy) - R) - R], 1)
                idx = np.concatenate([idx, mate_idx], 1)
            if v.shape[1] == 0:
                continue
            v = np.where(np.isnan(v), np.inf, v)
            a = np.argmin(v, axis=1)                             # the first of equal values: the lowest index
            best = v[np.arange(B), a]
            hit = best < np.inf
            clear[r] = np.where(hit, best, np.inf)
            near[r] = np.where(hit, idx[np.arange(B), a], -1)
    return (clear[0], near[0]) if one else (clear, near)


# ---- rectangular car bodies (f110qp_clearance_body_dev, f110qp_cast_scans_body_dev) ------------------------
# The model of include/f110qp.h "rectangular car bodies" in numpy, in csrc/body_geom.h's expressions and order.
# np.fmin / np.fmax are the kernels' fmin / fmax (of a NaN and a number: the number).

HALF_LENGTH, HALF_WIDTH = 0.29, 0.155  # f110qp_default_body_config


def body_sd(px, py, qx, qy, c, s, hl, hw):
    """Signed distance of the points (px, py) to the rectangles (centre (qx, qy), axes (c, s), half extents
    (hl, hw)): rule 1, negative inside, a NaN in gives a NaN out."""
    dx, dy = px - qx, py - qy
    u = dx * c + dy * s
    w = dy * c - dx * s
    au, aw = np.abs(u) - hl, np.abs(w) - hw
    ex, ey = np.where(au < 0.0, 0.0, au), np.where(aw < 0.0, 0.0, aw)
    return np.where((au <= 0.0) & (aw <= 0.0), np.fmax(au, aw), np.sqrt(ex * ex + ey * ey))


def _body_corner_min(ax, ay, ac, as_, bx, by, bc, bs, hl, hw):
    fx, fy = hl * ac, hl * as_
    lx, ly = hw * as_, hw * ac
    v0 = body_sd((ax + fx) - lx, (ay + fy) + ly, bx, by, bc, bs, hl, hw)
    v1 = body_sd((ax + fx) + lx, (ay + fy) - ly, bx, by, bc, bs, hl, hw)
    v2 = body_sd((ax - fx) - lx, (ay - fy) + ly, bx, by, bc, bs, hl, hw)
    v3 = body_sd((ax - fx) + lx, (ay - fy) - ly, bx, by, bc, bs, hl, hw)
    return np.fmin(np.fmin(v0, v1), np.fmin(v2, v3))


def body_pair(bx, by, bc, bs, mx, my, mc, ms, hl, hw):
    """Rectangle b against rectangle m (rule 3): the largest separating-axis gap when it is <= 0, otherwise the
    least of the eight corner distances. The same bits with b and m swapped."""
    dx, dy = mx - bx, my - by
    cc = np.abs(bc * mc + bs * ms)
    cr = np.abs(mc * bs - ms * bc)
    el = hl * cc + hw * cr
    ew = hl * cr + hw * cc
    gfb = (np.abs(dx * bc + dy * bs) - hl) - el
    glb = (np.abs(dy * bc - dx * bs) - hw) - ew
    gfm = (np.abs(dx * mc + dy * ms) - hl) - el
    glm = (np.abs(dy * mc - dx * ms) - hw) - ew
    g = np.fmax(np.fmax(gfb, gfm), np.fmax(glb, glm))
    far = np.fmin(_body_corner_min(mx, my, mc, ms, bx, by, bc, bs, hl, hw),
                  _body_corner_min(bx, by, bc, bs, mx, my, mc, ms, hl, hw))
    return np.where(g <= 0.0, g, far)


def _mates(B, G):
    """[B, G - 1]: the cars of b's race in the order of the car index, the own car left out."""
    own = np.arange(B) % G
    k = np.arange(G - 1)[None, :]
    return (np.arange(B) - own)[:, None] + k + (k >= own[:, None])


def clearance_body(x, circles, group_size: int = 1, center_offset: float = 0.1651, half_length: float = HALF_LENGTH,
                   half_width: float = HALF_WIDTH):
    """f110qp_clearance_body_dev in numpy, the device kernel's expressions in its order: clearance() with the car
    and its race-mates rectangles. Poses x [rows, B, 3] (or [B, 3]) in circles [C, 3], [B, C, 3] or None ->
    (clearance [rows, B] float64, nearest [rows, B] int32)."""
    x = np.asarray(x, np.float64)
    one = x.ndim == 2
    x = x[None] if one else x
    rows, B = x.shape[:2]
    G, hl, hw = int(group_size), float(half_length), float(half_width)
    if G < 1 or B % G:
        raise ValueError(f"group_size must be >= 1 and divide B = {B}, got {G}")
    ci = np.zeros((0, 3)) if circles is None else np.asarray(circles, np.float64)
    Cn = ci.shape[-2]
    own = np.arange(B) % G
    k = np.arange(G - 1)[None, :]
    mate_idx = Cn + k + (k >= own[:, None])
    mate = _mates(B, G)
    clear = np.full((rows, B), np.inf)
    near = np.full((rows, B), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rows):
            c, s = np.cos(x[r, :, 2]), np.sin(x[r, :, 2])
            qx, qy = x[r, :, 0] + center_offset * c, x[r, :, 1] + center_offset * s
            cw = np.broadcast_to(ci, (B, Cn, 3)) if ci.ndim == 2 else ci
            v = body_sd(cw[:, :, 0], cw[:, :, 1], qx[:, None], qy[:, None], c[:, None], s[:, None], hl, hw) \
                - np.abs(cw[:, :, 2])
            idx = np.broadcast_to(np.arange(Cn)[None, :], (B, Cn))
            if G > 1:
                vm = body_pair(qx[:, None], qy[:, None], c[:, None], s[:, None], qx[mate], qy[mate], c[mate], s[mate],
                               hl, hw)
                v = np.concatenate([v, vm], 1)
                idx = np.concatenate([idx, mate_idx], 1)
            if v.shape[1] == 0:
                continue
            v = np.where(np.isnan(v), np.inf, v)
            a = np.argmin(v, axis=1)                             # the first of equal values: the lowest index
            best = v[np.arange(B), a]
            hit = best < np.inf
            clear[r] = np.where(hit, best, np.inf)
            near[r] = np.where(hit, idx[np.arange(B), a], -1)
    return (clear[0], near[0]) if one else (clear, near)


def body_slab(of, ol, c, s, dx, dy, hl, hw):
    """The slab test of rule 5 on broadcastable arrays: (th, hit)."""
    def axis(o, d, h):
        zero = d == 0.0
        dd = np.where(zero, 1.0, d)                              # no 0 / 0: the d == 0 lanes are replaced below
        t1, t2 = (-h - o) / dd, (h - o) / dd
        inside = np.abs(o) <= h
        lo = np.where(zero, np.where(inside, -np.inf, np.inf), np.fmin(t1, t2))
        hi = np.where(zero, np.where(inside, np.inf, -np.inf), np.fmax(t1, t2))
        return lo, hi
    lo_f, hi_f = axis(of, dx * c + dy * s, hl)
    lo_l, hi_l = axis(ol, dy * c - dx * s, hw)
    th = np.fmax(lo_f, lo_l)
    return th, (th <= np.fmin(hi_f, hi_l)) & (th > 0.0)


def ray_bodies(x, geom, beams, group_size, center_offset: float = 0.1651, half_length: float = HALF_LENGTH,
               half_width: float = HALF_WIDTH, lidar_offset: float = 0.275, max_range: float = 10.0):
    """The opponents' part of f110qp_cast_scans_body_dev in numpy: ranges [B, beams] float64 of every car's beams
    against the rectangles of its race-mates at the poses x [B, 3] (geom = (angle_min, angle_increment, ...) as
    float32), max_range where nothing is hit. The scan is np.minimum of this and the static circles' ranges
    (_ray_circles) before the cast to float32. An opponent with a non-finite pose hits nothing."""
    x = np.asarray(x, np.float64)
    B, G, hl, hw = x.shape[0], int(group_size), float(half_length), float(half_width)
    if G < 1 or B % G:
        raise ValueError(f"group_size must be >= 1 and divide B = {B}, got {G}")
    out = np.full((B, beams), float(max_range))
    if G == 1:
        return out
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c, s = np.cos(x[:, 2]), np.sin(x[:, 2])
        ox, oy = x[:, 0] + lidar_offset * c, x[:, 1] + lidar_offset * s
        qx, qy = x[:, 0] + center_offset * c, x[:, 1] + center_offset * s
        ang = x[:, 2:3] + (np.float64(geom[0]) + np.float64(geom[1]) * np.arange(beams, dtype=np.float64))[None, :]
        dx, dy = np.cos(ang)[:, :, None], np.sin(ang)[:, :, None]          # [B, R, 1]
        mate = _mates(B, G)
        px, py = qx[mate] - ox[:, None], qy[mate] - oy[:, None]           # [B, G - 1]
        cm, sm = c[mate], s[mate]
        of, ol = -(px * cm + py * sm), -(py * cm - px * sm)
        ok = np.isfinite(x[mate]).all(axis=2) & np.isfinite(x).all(axis=1)[:, None]
        th, hit = body_slab(of[:, None, :], ol[:, None, :], cm[:, None, :], sm[:, None, :], dx, dy, hl, hw)
        th = np.where(hit & ok[:, None, :], th, np.inf)
        return np.minimum(th.min(axis=2), out)


# ---- straight walls (f110qp_cast_scans_walls_dev, f110qp_clearance_walls_dev) -------------------------------
# The model of include/f110qp.h "straight walls" in numpy, in csrc/wall_geom.h's expressions and order.

def ray_segments(ox, oy, dx, dy, segments, max_range: float = 10.0):
    """Rule W1: ranges (float64, the shape of dx) of beams from the origins (ox, oy) along (dx, dy) against the
    segments [S, 4] or [..., S, 4] = (ax, ay, bx, by), max_range where nothing is hit. ox, oy, dx, dy broadcast
    against each other; a leading world axis of segments broadcasts against them too."""
    sg = np.asarray(segments, np.float64)
    ox, oy, dx, dy = (np.asarray(v, np.float64)[..., None] for v in np.broadcast_arrays(ox, oy, dx, dy))
    if sg.shape[-2] == 0:
        return np.full(dx.shape[:-1], float(max_range))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ax, ay, bx, by = sg[..., 0] - ox, sg[..., 1] - oy, sg[..., 2] - ox, sg[..., 3] - oy
        ca = dx * ay - dy * ax
        cb = dx * by - dy * bx
        ta = ax * dx + ay * dy
        tb = bx * dx + by * dy
        den = ca - cb
        straddle = ((ca <= 0.0) & (cb >= 0.0)) | ((ca >= 0.0) & (cb <= 0.0))
        th = ta + (tb - ta) * (ca / np.where(den != 0.0, den, 1.0))
        th = np.where(straddle & (den != 0.0) & (th > 0.0), th, np.inf)
        return np.minimum(th.min(axis=-1), float(max_range))


def ray_walls(x, geom, beams, segments, lidar_offset: float = 0.275, max_range: float = 10.0):
    """The segments' part of f110qp_cast_scans_walls_dev in numpy: ranges [B, beams] float64 of every car's beams
    at the poses x [B, 3] against segments [S, 4] or [B, S, 4] (geom = (angle_min, angle_increment, ...) as
    float32). The scan is np.minimum of this, the static circles' and the opponents' ranges before the cast to
    float32."""
    x = np.asarray(x, np.float64)
    sg = np.asarray(segments, np.float64)
    with np.errstate(invalid="ignore"):
        ox, oy = x[:, 0] + lidar_offset * np.cos(x[:, 2]), x[:, 1] + lidar_offset * np.sin(x[:, 2])
        ang = x[:, 2:3] + (np.float64(geom[0]) + np.float64(geom[1]) * np.arange(beams, dtype=np.float64))[None, :]
        return ray_segments(ox[:, None], oy[:, None], np.cos(ang), np.sin(ang), sg if sg.ndim == 2 else sg[:, None],
                            max_range)


def _wall_sd(u, w, hl, hw):
    au, aw = np.abs(u) - hl, np.abs(w) - hw
    ex, ey = np.where(au < 0.0, 0.0, au), np.where(aw < 0.0, 0.0, aw)
    return np.where((au <= 0.0) & (aw <= 0.0), np.fmax(au, aw), np.sqrt(ex * ex + ey * ey))


def _slab_axis(o, d, h):
    zero = d == 0.0
    dd = np.where(zero, 1.0, d)
    t1, t2 = (-h - o) / dd, (h - o) / dd
    inside = np.abs(o) <= h
    return (np.where(zero, np.where(inside, -np.inf, np.inf), np.fmin(t1, t2)),
            np.where(zero, np.where(inside, np.inf, -np.inf), np.fmax(t1, t2)))


def segment_body(ax, ay, bx, by, qx, qy, c, s, hl: float = HALF_LENGTH, hw: float = HALF_WIDTH):
    """Rule W2 on broadcastable arrays: the body (centre (qx, qy), axes (c, s), half extents (hl, hw)) against the
    segment from (ax, ay) to (bx, by): <= 0 when the segment crosses or touches the rectangle, otherwise the exact
    distance; +inf for a NaN or infinite field or pose."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dax, day, dbx, dby = ax - qx, ay - qy, bx - qx, by - qy
        ua, wa = dax * c + day * s, day * c - dax * s
        ub, wb = dbx * c + dby * s, dby * c - dbx * s
        ex, ey = ub - ua, wb - wa
        ee = ex * ex + ey * ey
        lo_f, hi_f = _slab_axis(ua, ex, hl)
        lo_l, hi_l = _slab_axis(wa, ey, hw)
        m = np.fmin(_wall_sd(ua, wa, hl, hw), _wall_sd(ub, wb, hl, hw))
        cross = np.fmax(np.fmax(lo_f, lo_l), 0.0) <= np.fmin(np.fmin(hi_f, hi_l), 1.0)

        def corner(cx, cy):
            gx, gy = cx - ua, cy - wa
            t = (gx * ex + gy * ey) / np.where(ee == 0.0, 1.0, ee)
            t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
            t = np.where(ee == 0.0, 0.0, t)
            rx, ry = gx - t * ex, gy - t * ey
            return np.sqrt(rx * rx + ry * ry)
        k = np.fmin(np.fmin(corner(hl, hw), corner(hl, -hw)), np.fmin(corner(-hl, hw), corner(-hl, -hw)))
        v = np.where(cross, np.fmin(m, 0.0), np.fmin(m, k))
        return np.where(ee < np.inf, v, np.inf)


def clearance_walls(x, circles, segments, group_size: int = 1, center_offset: float = 0.1651,
                    half_length: float = HALF_LENGTH, half_width: float = HALF_WIDTH):
    """f110qp_clearance_walls_dev in numpy: clearance_body() with the segments [S, 4], [B, S, 4] or None as a third
    stretch of the obstacle list, segment k at index C + G + k. -> (clearance [rows, B], nearest [rows, B])."""
    x = np.asarray(x, np.float64)
    one = x.ndim == 2
    x = x[None] if one else x
    rows, B = x.shape[:2]
    G, hl, hw = int(group_size), float(half_length), float(half_width)
    clear, near = clearance_body(x, circles, G, center_offset, hl, hw)
    sg = np.zeros((0, 4)) if segments is None else np.asarray(segments, np.float64)
    S = sg.shape[-2]
    Cn = 0 if circles is None else np.asarray(circles).shape[-2]
    if S:
        sw = np.broadcast_to(sg, (B, S, 4)) if sg.ndim == 2 else sg
        with np.errstate(invalid="ignore"):
            c, s = np.cos(x[..., 2]), np.sin(x[..., 2])
            qx, qy = x[..., 0] + center_offset * c, x[..., 1] + center_offset * s
        v = segment_body(sw[None, :, :, 0], sw[None, :, :, 1], sw[None, :, :, 2], sw[None, :, :, 3], qx[..., None],
                         qy[..., None], c[..., None], s[..., None], hl, hw)          # [rows, B, S]
        v = np.where(np.isnan(v), np.inf, v)
        a = np.argmin(v, axis=2)                                                     # the lowest index on equal values
        best = np.take_along_axis(v, a[..., None], 2)[..., 0]
        take = best < clear                                                          # equal: the lower index stays
        clear = np.where(take, best, clear)
        near = np.where(take, Cn + G + a, near).astype(np.int32)
    return (clear[0], near[0]) if one else (clear, near)


def make_wall_world(seed: int = 0, obstacles: int = 40, every: int = 4):
    """make_world(seed, obstacles) with straight walls: (segments [S, 4], circles [obstacles, 3]) float64. The two
    walls of make_world as two closed polylines through every `every`-th wall point (consecutive segments share the
    vertex's bits, the last closes on the first), left wall first; the obstacle circles are make_world's own,
    drawn from the same generator in the same order."""
    w = make_world(seed, obstacles)
    W = (w.shape[0] - obstacles) // 2
    segs = []
    for wall in (w[:W, :2], w[W:2 * W, :2]):
        v = wall[::every]
        segs.append(np.concatenate([v, np.roll(v, -1, 0)], 1))
    return np.ascontiguousarray(np.concatenate(segs)), np.ascontiguousarray(w[2 * W:])


# ---- a noisy LiDAR (f110qp_cast_scans_noisy_dev, f110qp_rollout_noisy[_dev]; rules Z1 to Z3 of f110qp.h) -------

NOISE_K = np.uint64(0x9E3779B97F4A7C15)
NOISE_U = float.fromhex("0x1.bb67ae86627e8p-16")  # the double nearest to sqrt(3 / (2^32 - 1))


def _noise_mix(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def scan_noise_draws(seed: int, car: int, tick: int, num_ranges: int):
    """Rule Z1 for the beams 0 .. num_ranges - 1 of car `car` (car_base + b) at tick `tick`: (h uint64, g int64 in
    [-131070, 131070], d uint64 below 2^24), all in wrapping unsigned 64-bit arithmetic."""
    u = lambda v: np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)  # noqa: E731
    m = np.uint64(0xFFFF)
    with np.errstate(over="ignore"):
        kc = _noise_mix(u(seed) + NOISE_K * u(int(car) + 1))
        kt = _noise_mix(kc + NOISE_K * u(int(tick) + 1))
        h = _noise_mix(kt + NOISE_K * np.arange(1, int(num_ranges) + 1, dtype=np.uint64))
        d = _noise_mix(h + NOISE_K) >> np.uint64(40)
    g = ((h & m) + ((h >> np.uint64(16)) & m) + ((h >> np.uint64(32)) & m) + (h >> np.uint64(48))).astype(np.int64)
    return h, g - 131070, d


def noisy_scan(ranges, seed: int, car_base: int, tick: int, sigma_abs: float, sigma_rel: float, dropout: float,
               max_range: float = 10.0) -> np.ndarray:
    """Rule Z2 on the noise-free scans ranges [B, R] float32 (the walls cast's): car b draws from stream
    car_base + b. A no-return beam (== (float)max_range) is untouched, a dropped beam becomes one, every other
    becomes (float)fmin(fmax(q + (sigma * g) * U, 0), max_range) with sigma = sigma_abs + sigma_rel * q."""
    r = np.ascontiguousarray(ranges, np.float32)
    if r.ndim != 2:
        raise ValueError("ranges must be [B, R]")
    mr = np.float32(max_range)
    drop24 = int(np.floor(np.float64(dropout) * 16777216.0))
    out = np.empty_like(r)
    for b in range(r.shape[0]):
        _, g, d = scan_noise_draws(seed, int(car_base) + b, tick, r.shape[1])
        q = r[b].astype(np.float64)
        sigma = np.float64(sigma_abs) + np.float64(sigma_rel) * q
        e = (sigma * g.astype(np.float64)) * NOISE_U
        v = np.fmin(np.fmax(q + e, 0.0), np.float64(max_range)).astype(np.float32)
        out[b] = np.where(r[b] == mr, r[b], np.where(d < np.uint64(drop24), mr, v))
    return out


# ---- race standings (f110qp_path_lengths, f110qp_progress_dev, f110qp_standings_dev) ------------------------

def path_lengths(wp) -> np.ndarray:
    """cum [W + 1] of the closed path wp [W, 2] (f110qp_path_lengths): cum[0] = 0, cum[j + 1] = cum[j] +
    sqrt(ex ex + ey ey) with e = wp[(j + 1) % W] - wp[j], summed in index order."""
    wp = np.asarray(wp, np.float64)
    e = np.roll(wp, -1, 0) - wp
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([[0.0], np.cumsum(np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]))])


def progress(x, wp):
    """The projection of include/f110qp.h (f110qp_progress_dev) in numpy, the device kernel's expressions in its
    order: poses x [rows, B, 3] (or [B, 3]) on the closed path wp [W, 2] -> (seg [rows, B] int32, s [rows, B],
    lateral [rows, B]). Per segment t = clamp((w.e) / (e.e)) (0 when e.e == 0), d2 = |p - (a + t e)|^2; the
    minimum, the lowest index on equal values, NaN values never chosen, seg -1 and NaN without a candidate;
    s = cum[j] + t (cum[j + 1] - cum[j]), lateral = sqrt(d2), negated unless ex wy - ey wx >= 0."""
    x = np.asarray(x, np.float64)
    one = x.ndim == 2
    x = x[None] if one else x
    wp = np.asarray(wp, np.float64)
    rows, B = x.shape[:2]
    cum = path_lengths(wp)
    ax, ay = wp[None, :, 0], wp[None, :, 1]
    seg = np.full((rows, B), -1, np.int32)
    s = np.full((rows, B), np.nan)
    lat = np.full((rows, B), np.nan)
    car = np.arange(B)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nx, ny = np.roll(wp[:, 0], -1)[None, :], np.roll(wp[:, 1], -1)[None, :]
        ex, ey = nx - ax, ny - ay
        ee = ex * ex + ey * ey
        for r in range(rows):
            px, py = x[r, :, 0:1], x[r, :, 1:2]
            wx, wy = px - ax, py - ay
            t = (wx * ex + wy * ey) / ee
            t = np.where(ee == 0, 0.0, np.where(t < 0, 0.0, np.where(t > 1, 1.0, t)))
            dx, dy = px - (ax + t * ex), py - (ay + t * ey)
            d2 = dx * dx + dy * dy
            d2 = np.where(np.isnan(d2), np.inf, d2)
            j = np.argmin(d2, axis=1)                            # the first of equal values: the lowest index
            best = d2[car, j]
            hit = best < np.inf
            tj = t[car, j]
            sv = cum[j] + tj * (cum[j + 1] - cum[j])
            root = np.sqrt(best)
            left = ex[0, j] * wy[car, j] - ey[0, j] * wx[car, j] >= 0
            seg[r] = np.where(hit, j, -1)
            s[r] = np.where(hit, sv, np.nan)
            lat[r] = np.where(hit, np.where(left, root, -root), np.nan)
    return (seg[0], s[0], lat[0]) if one else (seg, s, lat)


def standings(s, L: float, group_size: int = 1):
    """The standings of include/f110qp.h (f110qp_standings_dev) in numpy: s [rows, B] (or [B]) on a path of
    length L, the B cars being B / G races -> (dist [rows, B], lap [rows, B] int32, rank [rows, B] int32). Row 0
    relative to the race's first car, every later row the row before plus the wrapped step, in row order; lap =
    floor((dist - dist[0]) / L), INT_MIN where dist is NaN; rank = the race-mates ahead (a larger dist, or an
    equal one with a lower index; NaN behind every number, the lower index ahead among NaN)."""
    s = np.asarray(s, np.float64)
    one = s.ndim == 1
    s = s[None] if one else s
    rows, B = s.shape
    G, L = int(group_size), float(L)
    if G < 1 or B % G:
        raise ValueError(f"group_size must be >= 1 and divide B = {B}, got {G}")
    half = 0.5 * L

    def wrap(v):
        return np.where(v > half, v - L, np.where(v <= -half, v + L, v))

    dist = np.empty((rows, B))
    lap = np.empty((rows, B), np.int32)
    rank = np.empty((rows, B), np.int32)
    first = np.arange(B) - np.arange(B) % G
    m = np.arange(G)
    with np.errstate(invalid="ignore"):
        for r in range(rows):
            if r == 0:
                s0 = s[0, first]
                dist[0] = s0 + wrap(s[0] - s0)
            else:
                dist[r] = dist[r - 1] + wrap(s[r] - s[r - 1])
            d = dist[r]
            num = ~np.isnan(d)
            lp = np.floor((d - dist[0]) / L)
            lap[r] = np.where(num, np.where(num, lp, 0.0).astype(np.int64), np.iinfo(np.int32).min).astype(np.int32)
            dr = d.reshape(B // G, G)
            dm, db = dr[:, None, :], dr[:, :, None]              # [race, car, mate]
            lower = m[None, None, :] < m[None, :, None]
            ahead = np.where(np.isnan(db), ~np.isnan(dm) | lower, (dm > db) | ((dm == db) & lower))
            rank[r] = ahead.sum(axis=2).reshape(B)
    return (dist[0], lap[0], rank[0]) if one else (dist, lap, rank)


def make_race_grid(races: int, group_size: int, seed: int = 0, spacing: float = 1.2, lateral: float = 0.4) -> np.ndarray:
    """Start states [races * group_size, 3] float64 (x, y, yaw) of `races` races on track_waypoints(): a race
    starts at a seeded position on the path; its car i stands i * spacing metres behind car 0 along the path,
    alternately +lateral and -lateral off it, heading along the path."""
    rng = np.random.default_rng(seed)
    wp = track_waypoints()
    W, G = wp.shape[0], int(group_size)
    seg = np.hypot(*(np.roll(wp, -1, 0) - wp).T)
    s_along = np.concatenate([[0.0], np.cumsum(seg)])
    total = s_along[-1]
    s0 = rng.uniform(0, total, races)
    i = np.arange(G)
    s = ((s0[:, None] - spacing * i[None, :]) % total).reshape(-1)
    k = np.minimum(np.searchsorted(s_along, s, side="right") - 1, W - 1)
    nxt = wp[(k + 1) % W]
    base = wp[k] + (nxt - wp[k]) * ((s - s_along[k]) / seg[k])[:, None]
    hd = np.arctan2(nxt[:, 1] - wp[k, 1], nxt[:, 0] - wp[k, 0])
    lat = np.tile(np.where(i % 2 == 0, lateral, -lateral), races)
    return np.ascontiguousarray(np.stack([base[:, 0] - np.sin(hd) * lat, base[:, 1] + np.cos(hd) * lat, hd], 1))


# ---- Monte Carlo outcomes (f110qp_mc_fan_dev, f110qp_mc_survival_dev, f110qp_mc_outcomes_dev) ---------------

MC_PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
MC_NAN_BITS = np.uint64(0x7FF8000000000000)
_MC_SIGN = np.uint64(0x8000000000000000)


def mc_keys(v) -> np.ndarray:
    """Rule M1 and M2 of include/f110qp.h: the uint64 keys of float64 values, ~u when the sign bit is set and
    u | 1 << 63 otherwise; a NaN (either sign, any payload) gets MC_PAD_KEY, which no number maps to."""
    u = np.ascontiguousarray(v, np.float64).view(np.uint64)
    key = np.where(u & _MC_SIGN != 0, ~u, u | _MC_SIGN)
    return np.where((u & ~_MC_SIGN) > np.uint64(0x7FF0000000000000), MC_PAD_KEY, key)


def mc_values(key) -> np.ndarray:
    """The float64 values of keys: the inverse of mc_keys on numbers."""
    key = np.asarray(key, np.uint64)
    return np.where(key & _MC_SIGN != 0, key ^ _MC_SIGN, ~key).view(np.float64)


def _mc_layout(B, M, G):
    M, G = int(M), int(G)
    if M < 1 or G < 1 or B < 1 or B % (M * G):
        raise ValueError(f"hypotheses x group_size must divide B = {B}, got {M} x {G}")
    return B // (M * G), M, G


def mc_fan(v, M: int, G: int, prob):
    """The fan of include/f110qp.h (f110qp_mc_fan_dev) in numpy: v [rows, B] (or [B]) -> (fan [rows, K, Q],
    count [rows, K] int32). The M members of set k = s G + g are the cars (s M + m) G + g. The uint64 keys are
    sorted, not the doubles: the NaN keys sort last, count is the number of the others, and quantile q is the key
    at floor(prob[q] * (count - 1)) turned back into its bits (0x7ff8000000000000 for count 0)."""
    v = np.asarray(v, np.float64)
    one = v.ndim == 1
    v = v[None] if one else v
    rows, B = v.shape
    S, M, G = _mc_layout(B, M, G)
    prob = np.asarray(prob, np.float64).reshape(-1)
    if prob.size < 1 or not ((prob >= 0) & (prob <= 1)).all():
        raise ValueError("every prob must be in [0, 1]")
    key = np.sort(mc_keys(v).reshape(rows, S, M, G).transpose(0, 1, 3, 2).reshape(rows, S * G, M), axis=2)
    n = (key != MC_PAD_KEY).sum(axis=2).astype(np.int32)
    pos = np.floor(prob[None, None, :] * (n[:, :, None] - 1).astype(np.float64)).astype(np.int64)
    got = np.take_along_axis(key, np.maximum(pos, 0), axis=2)
    bits = np.where(n[:, :, None] > 0, mc_values(got).view(np.uint64), MC_NAN_BITS)
    fan = np.ascontiguousarray(bits).view(np.float64)
    return (fan[0], n[0]) if one else (fan, n)


def mc_survival(crash_tick, T: int, M: int, G: int):
    """Rule M4 (f110qp_mc_survival_dev): crash_tick [B] -> (alive [T + 1, K] int32, crashed [K] int32)."""
    ct = np.asarray(crash_tick, np.int64).reshape(-1)
    S, M, G = _mc_layout(ct.size, M, G)
    c = ct.reshape(S, M, G).transpose(0, 2, 1).reshape(S * G, M)
    r = np.arange(int(T) + 1)[:, None, None]
    alive = ((c[None] < 0) | (c[None] > r)).sum(axis=2).astype(np.int32)
    return alive, ((c >= 0) & (c <= int(T))).sum(axis=1).astype(np.int32)


def mc_outcomes(clear, status=None, kind=None):
    """Rule M5 (f110qp_mc_outcomes_dev): clear [T + 1, B], status and kind [T, B] or None -> a dict of min_clear,
    min_row and, with status, unsolved and first_unsolved, and, with kind, plan_failed (each [B]). MPC ticks are
    kind 0, PLAN_FAILED ticks kind 3; a usable status is 1 or 2."""
    clear = np.asarray(clear, np.float64)
    B = clear.shape[1]
    c = np.where(np.isnan(clear), np.inf, clear)
    row = np.argmin(c, axis=0)                                  # the first of equal values: the lowest row
    best = c[row, np.arange(B)]
    o = dict(min_clear=best, min_row=np.where(best < np.inf, row, -1).astype(np.int32))
    if status is not None:
        status = np.asarray(status)
        bad = ((status != 1) & (status != 2)) & (True if kind is None else np.asarray(kind) == 0)
        o["unsolved"] = bad.sum(axis=0).astype(np.int32)
        o["first_unsolved"] = np.where(bad.any(axis=0), np.argmax(bad, axis=0), -1).astype(np.int32)
    if kind is not None:
        o["plan_failed"] = (np.asarray(kind) == 3).sum(axis=0).astype(np.int32)
    return o


def make_mc_batch(x0, M: int, G: int = 1) -> np.ndarray:
    """Starts [S G, 3] (S situations of G cars) tiled into the Monte Carlo layout [S M G, 3]: car (s M + m) G + g
    starts where car s G + g of x0 does, for every m."""
    x0 = np.asarray(x0, np.float64)
    M, G = int(M), int(G)
    if x0.ndim != 2 or M < 1 or G < 1 or x0.shape[0] % G:
        raise ValueError(f"x0 must be [S * G, 3] with G = {G}, got {x0.shape}")
    S = x0.shape[0] // G
    return np.ascontiguousarray(np.tile(x0.reshape(S, 1, G, -1), (1, M, 1, 1)).reshape(S * M * G, -1))


# ---- occupancy-grid maps (f110qp_cast_scans_grid_dev, f110qp_clearance_grid_dev, f110qp_rollout_grid[_dev]) -----
# Rules G1 and G2 of include/f110qp.h in numpy, in csrc/grid_geom.h's expressions and order. A map is (grid, cfg):
# grid [H, W] uint8, nonzero occupied, row j at y and column i at x; cfg anything with origin_x, origin_y,
# resolution and reach (a GridSpec here, a capi.GridConfig as well).

class GridSpec:
    """f110qp_grid_config's fields without the library."""

    def __init__(self, width=0, height=0, origin_x=0.0, origin_y=0.0, resolution=0.05, reach=1.0):
        self.width, self.height = int(width), int(height)
        self.origin_x, self.origin_y = float(origin_x), float(origin_y)
        self.resolution, self.reach = float(resolution), float(reach)

    def __repr__(self):
        return (f"GridSpec({self.width} x {self.height}, origin ({self.origin_x}, {self.origin_y}), "
                f"resolution {self.resolution}, reach {self.reach})")


def ray_grid(ox, oy, dx, dy, grid, cfg, max_range: float = 10.0):
    """Rule G1: ranges (float64, the broadcast shape of the arguments) of beams from the origins (ox, oy) along
    (dx, dy) against the map, max_range where nothing is hit: the walk of the rule, every boundary's parameter
    computed afresh from the integer boundary, x first on a tie."""
    g = np.asarray(grid)
    ox, oy, dx, dy = (np.asarray(v, np.float64) for v in np.broadcast_arrays(ox, oy, dx, dy))
    shape = dx.shape
    out = np.full(dx.size, float(max_range))
    if g.size == 0:
        return out.reshape(shape)
    H, W = g.shape
    ox, oy, dx, dy = (v.ravel() for v in (ox, oy, dx, dy))
    res, x0, y0 = np.float64(cfg.resolution), np.float64(cfg.origin_x), np.float64(cfg.origin_y)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        px, py = (ox - x0) / res, (oy - y0) / res
        ok = (px >= 0.0) & (px < W) & (py >= 0.0) & (py < H)
        a = np.flatnonzero(ok)                                   # the beams still walking
        ix, iy = np.floor(px[a]).astype(np.int64), np.floor(py[a]).astype(np.int64)
        inside = g[iy, ix] != 0
        out[a[inside]] = 0.0
        a, ix, iy = a[~inside], ix[~inside], iy[~inside]
        px, py, dx, dy = px[a], py[a], dx[a], dy[a]
        gx, gy = dx / res, dy / res
        sx, sy = np.where(dx > 0.0, 1, -1), np.where(dy > 0.0, 1, -1)

        def bound(i, p, d, gd):
            k = np.where(d > 0.0, i + 1, i).astype(np.float64)
            return np.where((d > 0.0) | (d < 0.0), (k - p) / gd, np.inf)
        tx, ty = bound(ix, px, dx, gx), bound(iy, py, dy, gy)
        for _ in range(W + H + 2):
            if a.size == 0:
                break
            stepx = tx <= ty
            t = np.where(stepx, tx, ty)
            ix, iy = ix + np.where(stepx, sx, 0), iy + np.where(stepx, 0, sy)
            tx, ty = np.where(stepx, bound(ix, px, dx, gx), tx), np.where(stepx, ty, bound(iy, py, dy, gy))
            go = (t <= max_range) & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
            hit = go.copy()
            hit[go] = g[iy[go], ix[go]] != 0
            out[a[hit]] = t[hit] + 0.0
            keep = go & ~hit
            a, ix, iy, px, py, dx, dy, gx, gy, sx, sy, tx, ty = (v[keep] for v in (a, ix, iy, px, py, dx, dy, gx, gy,
                                                                                   sx, sy, tx, ty))
    return out.reshape(shape)


def ray_map(x, geom, beams, grid, cfg, lidar_offset: float = 0.275, max_range: float = 10.0):
    """The map's part of f110qp_cast_scans_grid_dev in numpy: ranges [B, beams] float64 of every car's beams at the
    poses x [B, 3] (geom = (angle_min, angle_increment, ...) as float32). The noise-free scan is np.minimum of this,
    the circles', the opponents' and the segments' ranges before the cast to float32; rule Z2 runs on that."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        ox, oy = x[:, 0] + lidar_offset * np.cos(x[:, 2]), x[:, 1] + lidar_offset * np.sin(x[:, 2])
        ang = x[:, 2:3] + (np.float64(geom[0]) + np.float64(geom[1]) * np.arange(beams, dtype=np.float64))[None, :]
        return ray_grid(ox[:, None], oy[:, None], np.cos(ang), np.sin(ang), grid, cfg, max_range)


def cell_body(i, j, cfg, qx, qy, c, s, hl: float = HALF_LENGTH, hw: float = HALF_WIDTH):
    """Rule G2's value of the cells (i, j) (integer arrays) against the body (qx, qy, c, s), all broadcastable."""
    res, ox, oy = np.float64(cfg.resolution), np.float64(cfg.origin_x), np.float64(cfg.origin_y)
    i, j = np.asarray(i), np.asarray(j)
    x0, x1 = ox + i.astype(np.float64) * res, ox + (i + 1).astype(np.float64) * res
    y0, y1 = oy + j.astype(np.float64) * res, oy + (j + 1).astype(np.float64) * res
    v = np.inf
    for ax, ay, bx, by in ((x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)):
        v = np.fmin(v, segment_body(ax, ay, bx, by, qx, qy, c, s, hl, hw))
    centre = (x0 <= qx) & (qx < x1) & (y0 <= qy) & (qy < y1)
    return np.where(centre, np.fmin(v, 0.0), v)


def clearance_grid(x, circles, segments, grid, cfg, group_size: int = 1, center_offset: float = 0.1651,
                   half_length: float = HALF_LENGTH, half_width: float = HALF_WIDTH):
    """f110qp_clearance_grid_dev in numpy: clearance_walls() with the occupied cells of the map as a fourth stretch
    of the obstacle list, cell (i, j) at index C + G + S + j W + i, seen through rule G2's window.
    -> (clearance [rows, B], nearest [rows, B])."""
    x = np.asarray(x, np.float64)
    one = x.ndim == 2
    x = x[None] if one else x
    rows, B = x.shape[:2]
    G, hl, hw = int(group_size), float(half_length), float(half_width)
    clear, near = clearance_walls(x, circles, segments, G, center_offset, hl, hw)
    clear, near = np.array(clear), np.array(near)
    g = np.asarray(grid)
    if g.size:
        H, W = g.shape
        Cn = 0 if circles is None else np.asarray(circles).shape[-2]
        S = 0 if segments is None else np.asarray(segments).shape[-2]
        res, ox, oy = np.float64(cfg.resolution), np.float64(cfg.origin_x), np.float64(cfg.origin_y)
        R = np.sqrt(np.float64(hl) * hl + np.float64(hw) * hw) + np.float64(cfg.reach)
        for r in range(rows):
            for b in range(B):
                with np.errstate(invalid="ignore"):
                    c, s = np.cos(x[r, b, 2]), np.sin(x[r, b, 2])
                    qx, qy = x[r, b, 0] + center_offset * c, x[r, b, 1] + center_offset * s
                if not (np.isfinite(qx) and np.isfinite(qy)):
                    continue
                i0, i1 = max(np.floor((qx - R - ox) / res), 0.0), min(np.floor((qx + R - ox) / res), W - 1.0)
                j0, j1 = max(np.floor((qy - R - oy) / res), 0.0), min(np.floor((qy + R - oy) / res), H - 1.0)
                if not (i0 <= i1 and j0 <= j1):
                    continue
                i0, i1, j0, j1 = int(i0), int(i1), int(j0), int(j1)
                jj, ii = np.nonzero(g[j0:j1 + 1, i0:i1 + 1])     # row-major: ascending index
                if ii.size == 0:
                    continue
                ii, jj = ii + i0, jj + j0
                v = cell_body(ii, jj, cfg, qx, qy, c, s, hl, hw)
                v = np.where(np.isnan(v), np.inf, v)
                k = int(np.argmin(v))                            # the first of equal values: the lowest index
                if v[k] < clear[r, b]:                           # equal: the lower index stays
                    clear[r, b] = v[k]
                    near[r, b] = Cn + G + S + jj[k] * W + ii[k]
    return (clear[0], near[0]) if one else (clear, near.astype(np.int32))


def rasterize_walls(segments, circles, cfg) -> np.ndarray:
    """The map [cfg.height, cfg.width] uint8 of segments [S, 4] and circles [C, 3] (either may be None): every cell
    whose closed square a segment touches or a disc overlaps is occupied, the squares taken 1e-9 cells larger, so
    the cells of a segment are 4-connected and a closed polyline leaks no beam."""
    W, H = int(cfg.width), int(cfg.height)
    res, ox, oy = float(cfg.resolution), float(cfg.origin_x), float(cfg.origin_y)
    g = np.zeros((H, W), np.uint8)
    eps = 1e-9
    for ax, ay, bx, by in (np.zeros((0, 4)) if segments is None else np.asarray(segments, np.float64).reshape(-1, 4)):
        ax, ay, bx, by = (ax - ox) / res, (ay - oy) / res, (bx - ox) / res, (by - oy) / res  # in cells
        if not np.isfinite([ax, ay, bx, by]).all():
            continue
        i0, i1 = max(int(np.floor(min(ax, bx) - eps)), 0), min(int(np.floor(max(ax, bx) + eps)), W - 1)
        j0, j1 = max(int(np.floor(min(ay, by) - eps)), 0), min(int(np.floor(max(ay, by) + eps)), H - 1)
        if i0 > i1 or j0 > j1:
            continue
        jj, ii = np.mgrid[j0:j1 + 1, i0:i1 + 1]
        ex, ey = bx - ax, by - ay
        lo, hi = np.zeros(ii.shape), np.ones(ii.shape)           # the clip of a + s e, s in [0, 1], to the square
        for o, e, c0 in ((ax, ex, ii), (ay, ey, jj)):
            a0, a1 = c0 - eps - o, c0 + 1.0 + eps - o
            if e == 0.0:
                miss = (a0 > 0.0) | (a1 < 0.0)
                lo, hi = np.where(miss, np.inf, lo), np.where(miss, -np.inf, hi)
            else:
                lo, hi = np.maximum(lo, np.minimum(a0 / e, a1 / e)), np.minimum(hi, np.maximum(a0 / e, a1 / e))
        g[j0:j1 + 1, i0:i1 + 1] |= (lo <= hi).astype(np.uint8)
    for cx, cy, r in (np.zeros((0, 3)) if circles is None else np.asarray(circles, np.float64).reshape(-1, 3)):
        cx, cy, r = (cx - ox) / res, (cy - oy) / res, abs(r) / res
        if not np.isfinite([cx, cy, r]).all():
            continue
        i0, i1 = max(int(np.floor(cx - r - eps)), 0), min(int(np.floor(cx + r + eps)), W - 1)
        j0, j1 = max(int(np.floor(cy - r - eps)), 0), min(int(np.floor(cy + r + eps)), H - 1)
        if i0 > i1 or j0 > j1:
            continue
        jj, ii = np.mgrid[j0:j1 + 1, i0:i1 + 1]
        ddx = np.maximum(np.maximum(ii - cx, cx - (ii + 1.0)), 0.0)
        ddy = np.maximum(np.maximum(jj - cy, cy - (jj + 1.0)), 0.0)
        g[j0:j1 + 1, i0:i1 + 1] |= (np.hypot(ddx, ddy) <= r + eps).astype(np.uint8)
    return g


def make_grid_world(seed: int = 0, obstacles: int = 40, resolution: float = 0.05, reach: float = 1.0,
                    margin: float = 1.0):
    """make_wall_world(seed, obstacles) rasterised: (grid [H, W] uint8, GridSpec). The map covers the walls and the
    obstacle circles with `margin` metres to spare; its origin is a whole number of cells from (0, 0)."""
    sg, ci = make_wall_world(seed, obstacles)
    pts = np.concatenate([sg[:, :2], sg[:, 2:], ci[:, :2]])
    lo = np.floor((pts.min(0) - margin) / resolution)
    hi = np.ceil((pts.max(0) + margin) / resolution)
    cfg = GridSpec(int(hi[0] - lo[0]), int(hi[1] - lo[1]), lo[0] * resolution, lo[1] * resolution, resolution, reach)
    return rasterize_walls(sg, ci, cfg), cfg


def crop_map(grid, cfg, i0: int, j0: int, width: int, height: int):
    """The cells [i0, i0 + width) x [j0, j0 + height) of a map as a map of their own (same cell corners up to the
    rounding of the new origin)."""
    g = np.ascontiguousarray(np.asarray(grid)[j0:j0 + height, i0:i0 + width])
    return g, GridSpec(g.shape[1], g.shape[0], cfg.origin_x + i0 * cfg.resolution, cfg.origin_y + j0 * cfg.resolution,
                       cfg.resolution, cfg.reach)


# ---- the map's distance field (f110qp_grid_distance_dev, f110qp_grid_inflate_dev, f110qp_grid_lookup_dev) ---------
# Rules D1 to D4 of include/f110qp.h in numpy, expression for expression, np.float64 where a double is touched.

FIELD_NONE = np.int32(np.iinfo(np.int32).max)  # d2 of a cell on a map without an occupied cell
FIELD_NAN_BITS = np.uint64(0x7FF8000000000000)


def grid_distance(grid, chunk: int = 1 << 22):
    """Rules D1 and D2 as they are written: every cell against every occupied cell, the candidates in linear-index
    order so that argmin's first minimum is the least index. grid [H, W] -> (d2 [H, W] int32, nearest [H, W] int32).
    Cost: cells x occupied cells (in slices of `chunk` pairs): for maps of a few thousand cells."""
    g = np.asarray(grid)
    H, W = g.shape
    d2 = np.full(H * W, FIELD_NONE, np.int32)
    near = np.full(H * W, -1, np.int32)
    occ = np.flatnonzero(g.reshape(-1) != 0).astype(np.int64)    # ascending linear index q W + p
    if occ.size:
        q, p = occ // W, occ % W
        step = max(1, chunk // occ.size)
        for k0 in range(0, H * W, step):
            k = np.arange(k0, min(k0 + step, H * W), dtype=np.int64)
            j, i = k // W, k % W
            v = (i[:, None] - p[None, :]) ** 2 + (j[:, None] - q[None, :]) ** 2
            a = np.argmin(v, axis=1)
            d2[k] = v[np.arange(k.size), a]
            near[k] = occ[a]
    return d2.reshape(H, W), near.reshape(H, W)


def grid_dist_metres(d2, cfg):
    """Rule D3: resolution * sqrt((double)d2), +inf where d2 is INT_MAX."""
    d2 = np.asarray(d2, np.int32)
    with np.errstate(invalid="ignore"):
        m = np.float64(cfg.resolution) * np.sqrt(d2.astype(np.float64))
    return np.where(d2 == FIELD_NONE, np.inf, m)


def grid_inflate(d2, cfg, radius: float):
    """The inflation: (dist(d2) <= radius) as uint8."""
    return (grid_dist_metres(d2, cfg) <= np.float64(radius)).astype(np.uint8)


def grid_lookup(x, d2, nearest, cfg):
    """Rule D4 at the poses x [rows, B, 3] (or [B, 3]; the heading is not read) -> (dist float64, cell int32), NaN
    (0x7ff8000000000000) and -1 outside the map. nearest None: cell is None."""
    x = np.asarray(x, np.float64)
    d2 = np.asarray(d2, np.int32)
    H, W = d2.shape
    with np.errstate(invalid="ignore", over="ignore"):
        px = (x[..., 0] - np.float64(cfg.origin_x)) / np.float64(cfg.resolution)
        py = (x[..., 1] - np.float64(cfg.origin_y)) / np.float64(cfg.resolution)
        ok = (px >= 0.0) & (px < W) & (py >= 0.0) & (py < H)
        ix = np.where(ok, np.floor(px), 0.0).astype(np.int64)
        iy = np.where(ok, np.floor(py), 0.0).astype(np.int64)
    if d2.size == 0:
        ok = np.zeros(px.shape, bool)
        d2, ix, iy = np.full((1, 1), FIELD_NONE, np.int32), ix * 0, iy * 0
    dist = np.where(ok, grid_dist_metres(d2, cfg)[iy, ix], FIELD_NAN_BITS.view(np.float64))
    if nearest is None:
        return dist, None
    near = np.asarray(nearest, np.int32)
    near = near if near.size else np.full((1, 1), -1, np.int32)
    return dist, np.where(ok, near[iy, ix], -1).astype(np.int32)


# ---- the raster LiDAR through the field (f110qp_grid_cast_dev, f110qp_rollout_field[_dev]) ----------------------
# Rule F1 of include/f110qp.h in plain Python floats (IEEE doubles, every operation rounded once), one beam at a
# time, in csrc/grid_geom.h's expressions and order.

FIELD_JUMP_FIX = 4  # kGridJumpFix: corrections of a jump's estimate before the moves are taken singly


def _field_beam(px, py, ix, iy, dx, dy, res, d2, W, H, limit):
    """Rule F1 for one beam from cell (ix, iy) whose field value is > 0: (th or None, visits)."""
    inf = math.inf
    gx, gy = dx / res, dy / res
    sx, sy = (1 if dx > 0.0 else -1), (1 if dy > 0.0 else -1)
    mx, my = dx > 0.0 or dx < 0.0, dy > 0.0 or dy < 0.0
    kx, ky = (ix + 1 if dx > 0.0 else ix), (iy + 1 if dy > 0.0 else iy)

    def X(k):  # the k-th boundary parameter ahead in x: rule G1's expression on the integer boundary
        return (float(kx + sx * k) - px) / gx if mx else inf

    def Y(k):
        return (float(ky + sy * k) - py) / gy if my else inf

    visits, D, A, B = 1, int(d2[iy, ix]), 0, 0
    if not mx and not my:
        return None, visits
    ax, ay = abs(gx), abs(gy)
    x0, y0 = (X(0) if mx else 0.0), (Y(0) if my else 0.0)
    left = W + H + 2
    while left > 0:
        m = min(max(1, math.isqrt(D - 1)), left)
        left -= m
        n = A + B + m
        if not mx:
            a = 0
        elif not my:
            a = n
        else:
            te = (n - 1 + x0 * ax + y0 * ay) / (ax + ay)
            a = int(min(max(math.floor((te - x0) * ax) + 1.0, A), A + m))
            for _ in range(FIELD_JUMP_FIX):
                b = n - a
                if a > 0 and not X(a - 1) <= Y(b):
                    a -= 1
                elif b > 0 and not Y(b - 1) < X(a):
                    a += 1
                else:
                    break
            else:  # the m moves singly
                a, b = A, B
                for _ in range(m):
                    if X(a) <= Y(b):
                        a += 1
                    else:
                        b += 1
        A, B = a, n - a
        t = max(X(A - 1), Y(B - 1)) if A > 0 and B > 0 else X(A - 1) if A > 0 else Y(B - 1)
        if not t <= limit:
            return None, visits
        cx, cy = ix + sx * A, iy + sy * B
        if cx < 0 or cx >= W or cy < 0 or cy >= H:
            return None, visits
        D = int(d2[cy, cx])
        visits += 1
        if D <= 0:
            return t + 0.0, visits
    return None, visits


def ray_field(ox, oy, dx, dy, d2, cfg, max_range: float = 10.0):
    """Rule F1: (ranges float64, visits int32), each the broadcast shape of the arguments, of beams from the origins
    (ox, oy) along (dx, dy) against the map whose distance field is d2 [H, W] int (grid_distance's, or
    f110qp_grid_distance_dev's): a beam reads d2 where it stands and jumps isqrt(d2 - 1) cells of rule G1's walk
    at once. ranges equals ray_grid's bit for bit; visits counts the cells of d2 each beam read."""
    f = np.asarray(d2)
    ox, oy, dx, dy = (np.asarray(v, np.float64) for v in np.broadcast_arrays(ox, oy, dx, dy))
    shape = dx.shape
    out = np.full(dx.size, float(max_range))
    vis = np.zeros(dx.size, np.int32)
    if f.size == 0:
        return out.reshape(shape), vis.reshape(shape)
    H, W = f.shape
    res, x0, y0 = float(cfg.resolution), float(cfg.origin_x), float(cfg.origin_y)
    limit = float(max_range)
    for k, (bx, by, ddx, ddy) in enumerate(zip(ox.ravel().tolist(), oy.ravel().tolist(), dx.ravel().tolist(),
                                               dy.ravel().tolist())):
        px, py = (bx - x0) / res, (by - y0) / res
        if not (px >= 0.0 and px < W and py >= 0.0 and py < H):
            continue
        ix, iy = int(math.floor(px)), int(math.floor(py))
        vis[k] = 1
        if f[iy, ix] <= 0:
            out[k] = 0.0
            continue
        th, vis[k] = _field_beam(px, py, ix, iy, ddx, ddy, res, f, W, H, limit)
        if th is not None:
            out[k] = th
    return out.reshape(shape), vis.reshape(shape)


def _pgm_tokens(data: bytes, count: int):
    """The first `count` whitespace-separated header tokens of a PGM (comments from '#' to the line's end skipped)
    and the offset of the byte behind the single whitespace that ends the last one."""
    tok, pos = [], 0
    while len(tok) < count:
        while pos < len(data) and (data[pos:pos + 1].isspace() or data[pos:pos + 1] == b"#"):
            if data[pos:pos + 1] == b"#":
                while pos < len(data) and data[pos:pos + 1] != b"\n":
                    pos += 1
            else:
                pos += 1
        start = pos
        while pos < len(data) and not data[pos:pos + 1].isspace() and data[pos:pos + 1] != b"#":
            pos += 1
        if start == pos:
            raise ValueError("truncated PGM header")
        tok.append(data[start:pos])
    return tok, pos + 1


def read_pgm(path) -> np.ndarray:
    """A binary (P5, 8 or 16 bit) or ASCII (P2) PGM as [rows, cols] float64 in [0, 255], top row first."""
    data = open(path, "rb").read()
    (magic, w, h, mx), pos = _pgm_tokens(data, 4)
    w, h, mx = int(w), int(h), int(mx)
    if magic not in (b"P2", b"P5") or w < 0 or h < 0 or not 0 < mx < 65536:
        raise ValueError(f"not a PGM this reader knows: {magic!r} {w} x {h} max {mx}")
    if magic == b"P5":
        px = np.frombuffer(data, np.uint8 if mx < 256 else np.dtype(">u2"), w * h, pos)
    else:
        body = b"\n".join(line.split(b"#")[0] for line in data[pos - 1:].split(b"\n"))
        px = np.array(body.split()[:w * h], np.int64)
        if px.size != w * h:
            raise ValueError("truncated PGM")
    return px.astype(np.float64).reshape(h, w) * (255.0 / mx)


def load_map(pgm_path, yaml_path, reach: float = 1.0):
    """A map_server map -> (grid [H, W] uint8, GridSpec): the image of pgm_path and the keys `resolution`, `origin`
    ([x, y, yaw]; the yaw must be 0), `negate` and `occupied_thresh` of yaml_path, read by hand (flat `key: value`
    lines). map_server's rule: a pixel p in [0, 255] has occupancy (255 - p) / 255, or p / 255 with negate, and is
    occupied above occupied_thresh (default 0.65); its image has the top row first, the grid row 0 at origin_y."""
    keys = {}
    for line in open(yaml_path):
        line = line.split("#")[0]
        if ":" in line:
            k, v = line.split(":", 1)
            keys[k.strip()] = v.strip()
    if "resolution" not in keys or "origin" not in keys:
        raise ValueError("the map's yaml needs resolution and origin")
    origin = [float(v) for v in keys["origin"].strip("[]").split(",")]
    if len(origin) < 2 or (len(origin) > 2 and origin[2] != 0.0):
        raise ValueError(f"origin must be [x, y, 0], got {origin}")
    negate = int(float(keys.get("negate", "0")))
    thresh = float(keys.get("occupied_thresh", "0.65"))
    p = read_pgm(pgm_path)
    occ = (p if negate else 255.0 - p) / 255.0
    grid = np.ascontiguousarray((occ > thresh)[::-1].astype(np.uint8))
    return grid, GridSpec(grid.shape[1], grid.shape[0], origin[0], origin[1], float(keys["resolution"]), reach)
