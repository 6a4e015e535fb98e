"""workload.race_circles and workload.make_race_grid, and the races' test cases judged by the oracle alone
(no GPU): every case of race_cases.py that the device tests compare through world_cases.check_scan keeps its
grazing beams within world_cases.SKIP_CAP, and shows what it was built to show."""
import numpy as np
import pytest
import race_cases as rc_
import world_cases as wc_

from f110qp import workload


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def poses(B, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-5, 5, B), rng.uniform(-5, 5, B), rng.uniform(-np.pi, np.pi, B)], 1)


def test_race_circles_shapes_and_self_exclusion():
    x = poses(12, 1)
    assert workload.race_circles(x, 1).shape == (12, 0, 3)
    for G in (2, 3, 4, 12):
        c = workload.race_circles(x, G, 0.25, 0.1)
        assert c.shape == (12, G - 1, 3) and c.dtype == np.float64 and c.flags.c_contiguous
        assert (c[:, :, 2] == 0.25).all()
        full = np.stack([x[:, 0] + 0.1 * np.cos(x[:, 2]), x[:, 1] + 0.1 * np.sin(x[:, 2])], 1)
        for b in range(12):
            mates = [m for m in range(b - b % G, b - b % G + G) if m != b]  # by car index, the own car left out
            assert (bits(c[b, :, :2]) == bits(full[mates])).all(), (G, b)
    for G in (0, -1, 5, 24):
        with pytest.raises(ValueError):
            workload.race_circles(x, G)


def test_race_circles_races_are_disjoint():
    """A race's rows depend on that race's poses only."""
    x = poses(12, 2)
    c = workload.race_circles(x, 4)
    y = x.copy()
    y[4:8] = poses(4, 3)
    d = workload.race_circles(y, 4)
    assert (bits(c[:4]) == bits(d[:4])).all() and (bits(c[8:]) == bits(d[8:])).all()
    assert (bits(c[4:8]) != bits(d[4:8])).any()
    assert (bits(d[4:8]) == bits(workload.race_circles(y[4:8], 4))).all()


def test_race_circles_offset_zero_keeps_the_pose_bits():
    x = poses(6, 4)
    x[1, 2], x[2, 2] = 1e300, np.pi  # any finite heading: 0 * cos is a zero
    c = workload.race_circles(x, 3, 0.3, 0.0)
    for b in range(6):
        mates = [m for m in range(b - b % 3, b - b % 3 + 3) if m != b]
        assert (bits(c[b, :, :2]) == bits(x[mates, :2])).all()


def test_race_circles_permuting_a_race_permutes_the_rows():
    x = poses(8, 5)
    c = workload.race_circles(x, 4)
    perm = np.array([2, 0, 3, 1, 7, 6, 5, 4])  # within each race
    d = workload.race_circles(x[perm], 4)
    key = lambda rows: sorted(map(tuple, bits(rows).tolist()))  # noqa: E731
    for b in range(8):
        assert key(d[b]) == key(c[perm[b]]), b  # the same circles; their order follows the car index


def test_make_race_grid():
    wp = workload.track_waypoints()
    g = workload.make_race_grid(3, 4, seed=7)
    assert g.shape == (12, 3) and g.dtype == np.float64 and g.flags.c_contiguous
    assert (bits(g) == bits(workload.make_race_grid(3, 4, seed=7))).all()
    assert (bits(g) != bits(workload.make_race_grid(3, 4, seed=8))).any()
    d = np.hypot(g[:, None, 0] - wp[None, :, 0], g[:, None, 1] - wp[None, :, 1])
    k = d.argmin(axis=1)
    assert (np.abs(d.min(axis=1) - 0.4) < 0.02).all()  # +-lateral off the path
    hd = np.arctan2(wp[(k + 1) % 500, 1] - wp[k - 1, 1], wp[(k + 1) % 500, 0] - wp[k - 1, 0])
    assert np.abs(np.angle(np.exp(1j * (g[:, 2] - hd)))).max() < 0.03  # heading along the path
    side = np.sign(np.cos(hd) * (g[:, 1] - wp[k, 1]) - np.sin(hd) * (g[:, 0] - wp[k, 0]))
    assert (side.reshape(3, 4) == [1, -1, 1, -1]).all()  # alternately left and right
    line = workload.make_race_grid(2, 3, seed=7, spacing=1.5, lateral=0.0).reshape(2, 3, 3)
    step = np.hypot(*(line[:, 1:, :2] - line[:, :-1, :2]).transpose(2, 0, 1))
    assert np.abs(step - 1.5).max() < 0.02  # the chord of 1.5 m of arc
    # car i is in front of car i + 1
    fwd = np.cos(line[:, 1:, 2]) * (line[:, :-1, 0] - line[:, 1:, 0]) + np.sin(line[:, 1:, 2]) * (line[:, :-1, 1] - line[:, 1:, 1])
    assert (fwd > 1.4).all()


@pytest.mark.parametrize("case", rc_.oracle_cases(), ids=lambda c: c.name)
def test_cases_keep_the_grazing_cap(case):
    n, of = case.grazing()
    assert n <= wc_.SKIP_CAP * of, f"{case.name}: {n} of {of} beams are grazing"


def test_cases_show_what_they_are_for():
    """From the oracle alone: opponents are in the scans, the pair's figures are the header's."""
    c = rc_.track_race()
    with_opp = wc_.oracle_scan(c.x, c.rows(), c.geom, c.beams)
    alone = wc_.oracle_scan(c.x, c.static, c.geom, c.beams)
    assert ((with_opp != alone).sum(axis=1) >= 10).all()  # every car sees a race-mate on ten beams at least
    p = rc_.pair_in_line()
    s = wc_.oracle_scan(p.x, p.rows(), p.geom, p.beams)
    want = rc_.GAP + rc_.CENTER_OFFSET - wc_.LIDAR_OFFSET - rc_.CAR_RADIUS
    assert abs(float(s[0].min()) - want) <= np.spacing(np.float32(want)) + wc_.ABS_TOL
    ang = p.geom[0] + p.geom[1] * np.arange(p.beams, dtype=np.float64)
    assert (s[1][np.abs(ang) < np.pi / 2] == np.float32(wc_.MAX_RANGE)).all() and (s[1] < wc_.MAX_RANGE).any()
    f = rc_.follower_start()
    s = wc_.oracle_scan(f.x, f.rows(), f.geom, f.beams)
    assert s[1].min() < 1.2 and (s[0][np.abs(ang) < np.pi / 2] == np.float32(wc_.MAX_RANGE)).all()
    for C in (250, 0):
        k = rc_.crowd(C)
        assert len(k.x) == 258 and k.rows().shape == (258, C + 257, 3) and np.hypot(k.x[:, 0], k.x[:, 1]).max() <= 8.0
