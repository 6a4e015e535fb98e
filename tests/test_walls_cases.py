"""The straight-wall model on the CPU (walls_cases.py): every case the GPU tests use stays under the skip cap by
the oracle alone, workload.ray_segments is watertight on polylines that share their vertices' bits, and
workload.segment_body agrees with a dense sampling of body_sd along the segment, sign case by sign case."""
import numpy as np
import pytest
import walls_cases as wl_
import world_cases as wc_

from f110qp import workload


@pytest.mark.parametrize("c", wl_.scan_cases(), ids=lambda c: c.name)
def test_scan_cases_stay_under_the_skip_cap(c):
    g = c.grazing()
    print(f"{c.name}: {int(g.sum())} of {g.size} beams grazing")
    assert g.sum() <= wc_.SKIP_CAP * g.size
    want = c.oracle()
    assert (want < wc_.MAX_RANGE).any(), "the case hits something"


@pytest.mark.parametrize("c", wl_.oracle_cases(), ids=lambda c: c.name)
def test_clearance_cases_stay_under_the_skip_cap(c):
    sk = c.skip()
    print(f"{c.name}: {int(sk.sum())} of {sk.size} poses skipped, tol {c.tol:.2e}")
    assert sk.sum() <= wc_.SKIP_CAP * sk.size
    assert np.isfinite(c.oracle()[0]).any()


def test_bounds_come_from_the_formats():
    assert wl_.beam_tol(wc_.P_ENVELOPE) <= wc_.ABS_TOL and wl_.GRAZE_V >= 2 * wc_.ABS_TOL
    assert wl_.abs_tol(20.0) < 3e-13


def aimed(sg, origins):
    """Beams from every origin at every vertex of sg and one ulp of the angle to either side: (ox, oy, dx, dy)
    [O, 3 V]."""
    v = sg[:, :2]
    ang = np.arctan2(v[None, :, 1] - origins[:, None, 1], v[None, :, 0] - origins[:, None, 0])
    ang = np.concatenate([np.nextafter(ang, -np.inf), ang, np.nextafter(ang, np.inf)], 1)
    return origins[:, 0:1], origins[:, 1:2], np.cos(ang), np.sin(ang)


def parameter_form(ox, oy, dx, dy, sg, max_range):
    """The usual test (the segment's own parameter in [0, 1]), for comparison: it leaks."""
    ax, ay = sg[:, 0] - ox[..., None], sg[:, 1] - oy[..., None]
    ex, ey = sg[:, 2] - sg[:, 0], sg[:, 3] - sg[:, 1]
    den = dx[..., None] * ey - dy[..., None] * ex
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (ax * ey - ay * ex) / den
        s = (ax * dy[..., None] - ay * dx[..., None]) / den
    th = np.where((s >= 0) & (s <= 1) & (t > 0), t, np.inf)
    return np.minimum(th.min(axis=-1), max_range)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ray_segments_is_watertight_on_star_polygons(seed):
    sg = wl_.star_polygon(37, seed)
    rng = np.random.default_rng(100 + seed)
    origins = rng.uniform(-1.0, 1.0, (200, 2))  # inside the polygon (its vertices are at 2 m and more)
    ox, oy, dx, dy = aimed(sg, origins)
    r = workload.ray_segments(ox, oy, dx, dy, sg, 100.0)
    far = np.hypot(sg[:, 0], sg[:, 1]).max() + np.sqrt(2.0)
    leaks = int((r >= 100.0).sum())
    usual = int((parameter_form(np.broadcast_to(ox, dx.shape), np.broadcast_to(oy, dx.shape), dx, dy, sg, 100.0) >= 100.0).sum())
    print(f"seed {seed}: W1 leaks {leaks}, the parameter form {usual} of {r.size} beams")
    assert leaks == 0 and (r <= far).all()


def test_ray_segments_is_watertight_on_the_track():
    sg, _ = wl_.track()
    assert sg.shape == (250, 4)
    for w in (sg[:125], sg[125:]):  # two closed polylines that share their vertices' bits
        assert (w[:, 2:] == np.roll(w[:, :2], -1, 0)).all()
    x = wc_.track_poses(64, 3)
    ox, oy, dx, dy = wl_._beams(x, wc_.geometry(1080), 1080)
    r = workload.ray_segments(ox[:, None], oy[:, None], dx, dy, sg, 1e3)
    assert (r < 1e3).all(), "64 x 1,080 beams between the walls: none gets out"
    # aimed at the vertices of the inner and the outer wall from between them
    o = np.stack([ox, oy], 1)
    axx, ayy, adx, ady = aimed(sg, o)
    ra = workload.ray_segments(axx, ayy, adx, ady, sg, 1e3)
    assert (ra < 1e3).all()


def test_make_wall_world_is_make_world():
    sg, ci = workload.make_wall_world(5, 40)
    w = workload.make_world(5, 40)
    assert (ci == w[1000:]).all() and sg.shape == (250, 4) and ci.shape == (40, 3)
    assert (sg[:125, :2] == w[0:500:4, :2]).all() and (sg[125:, :2] == w[500:1000:4, :2]).all()
    ln = np.hypot(sg[:, 2] - sg[:, 0], sg[:, 3] - sg[:, 1])
    assert 0.0 < ln.min() and ln.max() < 0.7
    sg2, ci2 = workload.make_wall_world(5, 40, every=2)
    assert sg2.shape == (500, 4) and (ci2 == ci).all()


def sampled(sg, n=2000):
    """The least body_sd of n points along the segment for the body at the origin, heading 0."""
    t = np.linspace(0.0, 1.0, n)
    px, py = sg[0] + t * (sg[2] - sg[0]), sg[1] + t * (sg[3] - sg[1])
    return workload.body_sd(px, py, 0.0, 0.0, 1.0, 0.0, wl_.HL, wl_.HW).min()


@pytest.mark.parametrize("name", list(wl_.sign_cases()))
def test_segment_body_sign_cases(name):
    sg, want, holds = wl_.sign_cases()[name]
    sg = np.array(sg)
    v = float(workload.segment_body(sg[0], sg[1], sg[2], sg[3], 0.0, 0.0, 1.0, 0.0))
    lo = sampled(sg)
    step = float(np.hypot(sg[2] - sg[0], sg[3] - sg[1])) / 1999.0
    tol = wl_.abs_tol(2.0, 0.0)
    print(f"{name}: v {v!r} sampled {lo!r} step {step:.2e}")
    assert {"< 0": v < 0, "== 0": v == 0.0, "> 0": v > 0}[holds], (name, v)
    assert abs(v - want) <= tol, (name, v, want)
    if v > 0:  # not crossing: the exact distance, which the sampling never undercuts and reaches within a step
        assert lo >= v - tol and lo <= v + step
    else:      # crossing: the least signed distance of the ends, capped at 0
        ends = min(workload.body_sd(sg[0], sg[1], 0.0, 0.0, 1.0, 0.0, wl_.HL, wl_.HW),
                   workload.body_sd(sg[2], sg[3], 0.0, 0.0, 1.0, 0.0, wl_.HL, wl_.HW))
        assert v == min(ends, 0.0) and lo <= tol


def test_segment_body_against_a_dense_sampling():
    rng = np.random.default_rng(7)
    sg = wl_.random_segments(300, 9, spread=0.7, length=(0.2, 1.5))
    q = rng.uniform(-0.3, 0.3, (300, 2))
    yaw = rng.uniform(-np.pi, np.pi, 300)
    c, s = np.cos(yaw), np.sin(yaw)
    v = workload.segment_body(sg[:, 0], sg[:, 1], sg[:, 2], sg[:, 3], q[:, 0], q[:, 1], c, s)
    t = np.linspace(0.0, 1.0, 2000)[None, :]
    px = sg[:, 0:1] + t * (sg[:, 2:3] - sg[:, 0:1])
    py = sg[:, 1:2] + t * (sg[:, 3:4] - sg[:, 1:2])
    lo = workload.body_sd(px, py, q[:, 0:1], q[:, 1:2], c[:, None], s[:, None], wl_.HL, wl_.HW).min(axis=1)
    step = np.hypot(sg[:, 2] - sg[:, 0], sg[:, 3] - sg[:, 1]) / 1999.0
    tol = wl_.abs_tol(3.0)
    apart = v > 0
    assert apart.sum() > 50 and (~apart).sum() > 50
    assert (lo[apart] >= v[apart] - tol).all() and (lo[apart] <= v[apart] + step[apart]).all()
    assert (lo[~apart] <= tol).all(), "a crossing segment has a point inside or on the rectangle"
    assert (v[~apart] <= 0).all()


def test_non_finite_fields_are_never_chosen():
    x = np.zeros((1, 3))
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            sg = np.array([[0.5, -1.0, 0.5, 1.0], [1.0, -1.0, 1.0, 1.0]])
            sg[0, k] = bad
            clear, near = workload.clearance_walls(x, None, sg, 1, 0.0)
            assert near[0] == 0 + 1 + 1 and clear[0] == 1.0 - wl_.HL, (bad, k)  # C + G + k
            r = workload.ray_segments(0.0, 0.0, np.array([1.0]), np.array([0.0]), sg, 10.0)
            assert r[0] == 1.0, (bad, k)
