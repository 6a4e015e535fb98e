"""The rectangular-body oracles on the CPU (workload.clearance_body, workload.ray_bodies): every case of
body_cases.py stays under the skip cap from the oracle alone, and the model's own properties."""
import body_cases as bc_
import numpy as np
import pytest
import world_cases as wc_

from f110qp import workload

HL, HW = bc_.HL, bc_.HW


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def pair(b, m, hl=HL, hw=HW, off=0.0):
    """The clearance of two cars alone, poses b and m: (value of b, value of m)."""
    v, n = workload.clearance_body(np.array([b, m], np.float64), None, 2, off, hl, hw)
    assert (n == [1, 0]).all() or not np.isfinite(v).all()
    return v[0], v[1]


@pytest.mark.parametrize("c", bc_.oracle_cases(), ids=lambda c: c.name)
def test_clearance_cases_stay_under_the_skip_cap(c):
    sk = c.skip()
    assert sk.sum() <= wc_.SKIP_CAP * sk.size, (c.name, int(sk.sum()), sk.size)
    want, near = c.oracle()
    assert want.shape == (c.rows, c.B) and near.dtype == np.int32
    assert (bits(np.where(np.isinf(want), 0, want)) == bits(np.where(np.isinf(want), 0, c.all_values().min(axis=2)))).all()


@pytest.mark.parametrize("c", bc_.scan_cases(), ids=lambda c: c.name)
def test_scan_cases_stay_under_the_skip_cap(c):
    g = c.grazing()
    assert g.sum() <= wc_.SKIP_CAP * g.size, (c.name, int(g.sum()), g.size)


def test_case_shapes_reach_the_kernel_paths():
    assert bc_.ROWS == (1, 8, 9, 17)
    s = bc_.stride_case()
    assert s.B == 1030 and s.B > 2 * bc_.CLEAR_GRID and s.G == 5
    c = bc_.crowd_case()
    assert c.G == 258 and c.C == 255 and c.C < wc_.TILE < c.C + c.G - 1
    assert bc_.heading0_case().exact and not bc_.rows_case(9).exact
    t = bc_.stride_scan()
    assert len(t.x) == 780 and len(t.x) > bc_.CAST_GRID
    assert bc_.track_scan(1200, races=1).beams > 1152  # a second beam tile


def test_pair_symmetry_in_bits():
    rng = np.random.default_rng(5)
    x = np.stack([rng.uniform(-1.5, 1.5, 4000), rng.uniform(-1.5, 1.5, 4000), rng.uniform(-np.pi, np.pi, 4000)], 1)
    v, n = workload.clearance_body(x, None, 2, bc_.CENTER_OFFSET)
    assert (bits(v[0::2]) == bits(v[1::2])).all()
    assert (v < 0).sum() > 100 and (v > 0).sum() > 100, "overlapping and disjoint pairs"


def test_order_independence():
    c = bc_.of(bc_.cc_.track_case())
    want, near = c.oracle()
    perm = np.random.default_rng(8).permutation(c.C)
    wp, npm = workload.clearance_body(c.x, c.circles[perm], c.G, c.off)
    assert (bits(wp) == bits(want)).all()
    st = near < c.C
    assert (perm[npm[st]] == near[st]).all() and (npm[~st] == near[~st]).all()
    rp = np.concatenate([g * c.G + np.random.default_rng(9 + g).permutation(c.G) for g in range(c.B // c.G)])
    wr, _ = workload.clearance_body(c.x[:, rp], c.circles, c.G, c.off)
    assert (bits(wr) == bits(want[:, rp])).all()
    # and the scan
    s = bc_.track_scan(64)
    a = bc_.oracle_scan(s.x, s.static, s.G, s.geom, s.beams)
    b = bc_.oracle_scan(s.x[rp], s.static[perm], s.G, s.geom, s.beams)
    assert (a[rp].view(np.int32) == b.view(np.int32)).all()


def test_circle_dead_ahead_at_heading_0():
    d, r = 1.25, 0.5
    v, n = workload.clearance_body(np.array([[0.0, 0.0, 0.0]]), np.array([[d, 0.0, r], [d, 0.0, -r]]), 1, 0.0)
    assert v[0] == (d - HL) - r and n[0] == 0, "the lower index of a tie, a negative radius as |r|"
    off = bc_.CENTER_OFFSET  # with the offset: the centre is x + off exactly as the oracle rounds it
    v, _ = workload.clearance_body(np.array([[0.0, 0.0, 0.0]]), np.array([[d, 0.0, r]]), 1, off)
    assert v[0] == ((d - (0.0 + off)) - HL) - r


def test_parallel_cars_side_by_side():
    for gap, hw in ((0.5, HW), (0.5, 0.125), (0.25, 0.125), (0.2, HW)):
        a, b = pair([0.0, 0.0, 0.0], [0.0, gap, 0.0], hw=hw)
        assert a == b == (gap - hw) - hw
    a, _ = pair([0.0, 0.0, 0.0], [0.0, 0.5, 0.0], hw=0.125)
    assert a == 0.25  # gap - 2 hw, exact in dyadic numbers
    assert pair([0.0, 0.0, 0.0], [0.0, 0.25, 0.0], hw=0.125)[0] == 0.0  # touching
    # 0.5 m apart: the 0.3 m discs overlap, the 0.31 m wide rectangles do not
    disc, _ = workload.clearance(np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.0]]), None, 2, 0.3, 0.0)
    assert disc[0] < 0 < pair([0.0, 0.0, 0.0], [0.0, 0.5, 0.0])[0]


def test_cross_shaped_overlap():
    """A car across another, centres 0.05 m apart: no corner of either is inside the other, v < 0."""
    b, m = [0.0, 0.0, 0.0], [0.05, 0.0, np.pi / 2]
    c, s = np.cos(m[2]), np.sin(m[2])
    for sx in (-1, 1):
        for sy in (-1, 1):
            assert workload.body_sd(sx * HL, sy * HW, m[0], m[1], c, s, HL, HW) > 0
            assert workload.body_sd(m[0] + sx * HL * c - sy * HW * s, m[1] + sx * HL * s + sy * HW * c, 0.0, 0.0, 1.0, 0.0,
                                    HL, HW) > 0
    a, bb = pair(b, m)
    # the least translation that separates them: along b's long axis, 0.05 - hl - hw
    assert a == bb and a < 0 and abs(a - ((0.05 - HL) - HW)) < 1e-15


def test_corner_to_corner_approach_is_continuous_through_zero():
    """Car m rotated 45 degrees, its corner approaching car b's corner along the diagonal: the value passes
    through 0 without a jump (the gap branch and the corner branch meet there)."""
    rc = np.hypot(HL, HW)
    th = np.pi / 4 + np.arctan2(HW, HL)  # m's corner points back along the diagonal towards b's corner
    eps = np.concatenate([-np.logspace(-12, -3, 10)[::-1], np.logspace(-12, -3, 10)])
    vals = []
    for e in eps:
        k = (e + rc) / np.sqrt(2.0)
        vals.append(pair([0.0, 0.0, 0.0], [HL + k, HW + k, th - np.pi])[0])
    vals = np.array(vals)
    assert (np.diff(vals) > 0).all() and (vals[:10] < 0).all() and (vals[10:] > 0).all()
    assert np.abs(vals - eps).max() < 1e-3 and np.abs(vals[8:12]).max() < 1e-10
    assert (np.abs(vals) <= np.abs(eps) * 1.0001 + 1e-15).all(), "never farther than the corners are"


def test_beam_from_behind_returns_the_rear_face():
    s = bc_.parallel_scan()
    r = workload.ray_bodies(s.x, s.geom, s.beams, 2, bc_.CENTER_OFFSET)
    rear = ((2.0 + bc_.CENTER_OFFSET) - (0.0 + wc_.LIDAR_OFFSET)) - HL  # q_m - o, less the half length
    assert abs(r[0, 2] - rear) < 1e-15 and (r[0, [0, 4]] == wc_.MAX_RANGE).all()
    assert (r[1] == wc_.MAX_RANGE).all(), "the leader looks ahead"
    # seen from behind the car is 0.31 m wide, the disc 0.6 m: fewer beams hit
    g = wc_.geometry(1080)
    wide = wc_.oracle_scan(s.x[:1], workload.race_circles(s.x, 2)[:1], g, 1080)
    thin = workload.ray_bodies(s.x, g, 1080, 2)[:1]
    assert 0 < (thin < 10).sum() < 0.7 * (wide < 10).sum()


def test_lidar_inside_a_rectangle_sees_through_it():
    s = bc_.inside_scan()
    c, sn = np.cos(s.x[:, 2]), np.sin(s.x[:, 2])
    o = s.x[0, :2] + wc_.LIDAR_OFFSET * np.array([c[0], sn[0]])
    q1 = s.x[1, :2] + bc_.CENTER_OFFSET * np.array([c[1], sn[1]])
    assert workload.body_sd(o[0], o[1], q1[0], q1[1], c[1], sn[1], HL, HW) < -0.05
    both = workload.ray_bodies(s.x, s.geom, s.beams, 3)[0]
    alone = workload.ray_bodies(s.x[[0, 2, 2]], s.geom, s.beams, 3)[0]  # car 1 replaced by a copy of car 2
    assert (both == alone).all() and (both < 10).any()


def test_non_finite_poses():
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.2, 0.3], [np.nan, 0.0, 0.0], [0.5, np.inf, 0.0], [0.0, 1.0, np.nan]])
    x = np.concatenate([x, [[2.0, 2.0, 1.0]]])
    v, n = workload.clearance_body(x, np.array([[3.0, 0.0, 0.5], [np.nan, 0.0, 0.5]]), 6)
    assert np.isposinf(v[2:5]).all() and (n[2:5] == -1).all()
    assert np.isfinite(v[[0, 1, 5]]).all() and not np.isin(n[[0, 1, 5]], [1, 2 + 2, 2 + 3, 2 + 4]).any()
    r = workload.ray_bodies(x, wc_.geometry(64), 64, 6)
    assert (r[2:5] == 10).all() and np.isfinite(r).all()
