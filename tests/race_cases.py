"""The races' CPU side (test_gpu_race_scan.py, test_gpu_rollout_race.py, test_race_cases.py): every case whose
device scan is judged by world_cases.check_scan is built here, so that a CPU test can assert from the oracle
alone that it stays within world_cases.SKIP_CAP grazing beams (test_race_cases.py). The oracle of a race scan
is world_cases.oracle_scan on per-car circle rows: the static world followed by workload.race_circles(...).
No tolerance of its own: world_cases' bound (one float32 ulp + ABS_TOL on non-grazing beams) and cap.

    python tests/race_cases.py      # the grazing count of every case
"""
import numpy as np
import world_cases as wc_

from f110qp import workload

CAR_RADIUS, CENTER_OFFSET = 0.3, 0.1651  # f110qp_default_race_config
R = 1080
GEOM = wc_.geometry(R)


def rows_with_opponents(x, static, G, car_radius=CAR_RADIUS, center_offset=CENTER_OFFSET):
    """Per-car circle rows [B, C + G - 1, 3]: car b's static circles (static [C, 3], [B, C, 3] or None) followed
    by its race-mates' circles at the poses x."""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    opp = workload.race_circles(x, G, car_radius, center_offset)
    if static is None or static.shape[-2] == 0:
        return opp
    st = np.broadcast_to(static, (B,) + static.shape[-2:])
    return np.ascontiguousarray(np.concatenate([st, opp], axis=1))


class RaceCase:
    """Poses x [B, 3] in races of G, the static world (`static` [C, 3] or None) and the scan; `cars`: the cars
    compared with the oracle (all when None)."""

    def __init__(self, name, x, G, static, geom=GEOM, beams=R, cars=None, center_offset=CENTER_OFFSET):
        self.name, self.x, self.G, self.static, self.geom, self.beams = name, np.ascontiguousarray(x, np.float64), G, static, geom, beams
        self.cars = np.arange(len(self.x)) if cars is None else np.asarray(cars)
        self.center_offset = center_offset

    def rows(self, x=None):
        return rows_with_opponents(self.x if x is None else x, self.static, self.G, center_offset=self.center_offset)

    def check(self, got, x=None, what=""):
        """got [B, R] (the device's scans at poses x, the case's own by default) against the oracle on `cars`."""
        x = self.x if x is None else np.asarray(x, np.float64)
        c = self.cars
        return wc_.check_scan(np.ascontiguousarray(got[c]), x[c], np.ascontiguousarray(self.rows(x)[c]), self.geom, self.beams,
                              f"{self.name} {what}")

    def grazing(self):
        c = self.cars
        g = wc_.grazing(self.x[c], np.ascontiguousarray(self.rows()[c]), self.geom, self.beams)
        return int(g.sum()), g.size


def track_race(races=2, G=4, seed=11):
    """B = races x G cars on the grid of workload.make_race_grid in the track world (1,040 circles)."""
    return RaceCase(f"track {races}x{G}", workload.make_race_grid(races, G, seed), G, wc_.track_world())


GAP = 1.5  # metres between the two cars of the pair cases


def pair_in_line(yaw=0.0):
    """Two cars and no static circle: car 1 GAP metres straight ahead of car 0, both heading `yaw`. The
    follower's nearest return is GAP + CENTER_OFFSET - LIDAR_OFFSET - CAR_RADIUS on the beam along the
    heading; the leader's forward beams see nothing."""
    x = np.array([[0.2, -0.1, yaw], [0.2 + GAP * np.cos(yaw), -0.1 + GAP * np.sin(yaw), yaw]])
    return RaceCase("pair in line", x, 2, None)


def crowd(C, seed=21, G=258):
    """One race of 258 cars scattered within 8 m, 64 beams, C static circles (C = 250: static circles and
    opponents share the first circle tile and the opponents span two). Six of the cars meet the oracle."""
    rng = np.random.default_rng(seed)
    rad, phi = 8.0 * np.sqrt(rng.uniform(0, 1, G)), rng.uniform(-np.pi, np.pi, G)
    x = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(-np.pi, np.pi, G)], 1)
    beams = 64
    return RaceCase(f"crowd C {C}", x, G, wc_.random_world(C, seed + 1) if C else None, wc_.geometry(beams), beams,
                    cars=[0, 1, 100, 128, 256, 257])


def rollout_race_start(B=8, G=4, seed=13):
    """The start of the recorded-scans rollout: the grid of make_race_grid in the track world. The scans of the
    later ticks are cast at poses the device produces; their cap is asserted where they are compared."""
    return RaceCase(f"rollout start {B // G}x{G}", workload.make_race_grid(B // G, G, seed), G, wc_.track_world())


def follower_start(gap=GAP, seed=5):
    """Two cars and no static circle on make_race_grid(1, 2, lateral = 0): car 1 `gap` metres behind car 0
    along the path."""
    return RaceCase(f"follower {gap} m", workload.make_race_grid(1, 2, seed, spacing=gap, lateral=0.0), 2, None)


CAST_GRID = 768  # cast_scans_grid's cap: a larger batch strides


def stride_race(B=CAST_GRID + 12, G=4, seed=51, beams=64):
    """B = 780 cars within 1.6 m of the origin in races of 4, every car its own world of three circles, other
    ones for car b than for car b + CAST_GRID: twelve workgroups of the race instantiation take a second car.
    Compared with the plain cast (oracle-tested above its cap by world_cases.per_car_case) at center_offset = 0,
    so it is no oracle case."""
    x = wc_.poses_near_origin(B, seed)
    x[:, :2] *= 4.0
    static = wc_.random_world(3, seed + 1, B, spread=3.0)
    assert B > CAST_GRID and B % G == 0 and (static[:B - CAST_GRID] != static[CAST_GRID:]).any(axis=(1, 2)).all()
    return RaceCase(f"stride B {B} G {G}", x, G, static, wc_.geometry(beams), beams, center_offset=0.0)


def oracle_cases():
    return [track_race(), pair_in_line(), crowd(250), crowd(0), rollout_race_start(), follower_start()]


if __name__ == "__main__":
    for c in oracle_cases():
        n, of = c.grazing()
        print(f"{c.name:24s} grazing {n} of {of}")
