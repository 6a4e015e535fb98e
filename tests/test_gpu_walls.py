"""The straight-wall kernels on MI355X (f110qp_cast_scans_walls_dev, f110qp_clearance_walls_dev; include/f110qp.h
"straight walls") against the numpy oracles workload.ray_segments and workload.clearance_walls: walls_cases'
derived bounds and skip rules, bit equality where sincos is exact, S = 0 against the body twins, tile edges, a
closed polygon aimed at its vertices, a segment set per car, the device-side list, the grid stride, permutations
and odd inputs. Every scan row starts as the sentinel; every clearance call writes between two guard rows."""
import body_cases as bc_
import numpy as np
import pytest
import walls_cases as wl_
import world_cases as wc_
from test_gpu_body import bits, body_cast
from test_gpu_body import clearance as body_clearance
from test_gpu_rollout import same_bits
from test_gpu_rollout_replan import dev
from test_gpu_rollout_scan import scan_config
from test_gpu_world_scan import SENTINEL

from f110qp import workload

pytestmark = pytest.mark.gpu


def walls_of(capi, segments, B):
    S = 0 if segments is None else segments.shape[-2]
    return capi.default_walls_config(num_segments=S, wall_rows=1 if segments is None or segments.ndim == 2 else B)


def wall_cast(capi, cuda, x, static, segments, G, geom, beams, listed=None, count=None, off=wl_.CENTER_OFFSET):
    """f110qp_cast_scans_walls_dev on host arrays into rows pre-filled with the sentinel -> ranges [B, R]."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    B = x.shape[0]
    C = 0 if static is None else static.shape[-2]
    w = capi.default_world_config(num_circles=C, world_rows=1 if static is None or static.ndim == 2 else static.shape[0])
    race = capi.default_race_config(group_size=G, center_offset=off)
    wl = walls_of(capi, segments, B)
    out = torch.full((B, beams), float(SENTINEL), dtype=torch.float32, device=cuda)
    capi.cast_scans_walls_dev(scan_config(capi, beams, geom), w, race, capi.default_body_config(), wl, dev(cuda, x),
                              dev(cuda, static) if C else None, dev(cuda, segments) if wl.num_segments else None, out,
                              list_=None if listed is None else dev(cuda, np.asarray(listed, np.int32)),
                              count=None if listed is None else dev(cuda, np.int32([count])))
    torch.cuda.synchronize(cuda)
    return out.cpu().numpy()


def clearance(capi, cuda, x, circles, segments, G, off=wl_.CENTER_OFFSET, nearest=True):
    """f110qp_clearance_walls_dev on x [rows,B,3] -> (clearance [rows,B], nearest [rows,B] or None) as numpy."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    x = x[None] if x.ndim == 2 else x
    rows, B = x.shape[:2]
    Cn = 0 if circles is None else circles.shape[-2]
    wc = capi.default_world_config(num_circles=Cn, world_rows=1 if circles is None or circles.ndim == 2 else B)
    race = capi.default_race_config(group_size=G, center_offset=off)
    wl = walls_of(capi, segments, B)
    out = torch.full((rows + 2, B), -7.0, dtype=torch.float64, device=cuda)  # a guard row at either end
    near = torch.full((rows + 2, B), -7, dtype=torch.int32, device=cuda) if nearest else None
    capi.clearance_walls_dev(wc, race, capi.default_body_config(), wl, dev(cuda, x),
                             None if circles is None else dev(cuda, circles),
                             dev(cuda, segments) if wl.num_segments else None, out[1:-1], near[1:-1] if nearest else None)
    torch.cuda.synchronize(cuda)
    out = out.cpu().numpy()
    assert (out[[0, -1]] == -7.0).all(), "clearance: a guard row was written"
    if not nearest:
        return np.ascontiguousarray(out[1:-1]), None
    near = near.cpu().numpy()
    assert (near[[0, -1]] == -7).all(), "nearest: a guard row was written"
    return np.ascontiguousarray(out[1:-1]), np.ascontiguousarray(near[1:-1])


def run(capi, cuda, c):
    return clearance(capi, cuda, c.x, c.circles, c.segments, c.G, c.off)


def scan(capi, cuda, c, **kw):
    return wall_cast(capi, cuda, c.x, c.static, c.segments, c.G, c.geom, c.beams, off=c.off, **kw)


# ---- the cast ------------------------------------------------------------------------------------------------

def test_one_wall_across_the_path(capi, cuda):
    """Heading 0, a wall across the path at x = 2 from y = -1 to 1, five beams at -0.5 .. 0.5 rad: beam 2 (angle 0,
    sincos exact) reads 2 - 0.275 bit for bit, the others (2 - 0.275) / cos within the bound or max_range beside."""
    g = (np.float32(-0.5), np.float32(0.25), np.float32(0.5))
    x = np.zeros((1, 3))
    sg = np.array([[2.0, -1.0, 2.0, 1.0]])
    got = wall_cast(capi, cuda, x, None, sg, 1, g, 5)
    d = 2.0 - wc_.LIDAR_OFFSET
    assert got[0, 2] == np.float32(d)
    ang = np.float64(g[0]) + np.float64(g[1]) * np.arange(5)
    want = np.where(np.abs(d * np.tan(ang)) < 1.0, d / np.cos(ang), wc_.MAX_RANGE).astype(np.float32)
    assert (want < 10).all(), "all five beams meet the 2 m wall"
    assert (np.abs(got[0].astype(np.float64) - want) <= np.spacing(want) + wc_.ABS_TOL).all(), (got, want)
    wide = wall_cast(capi, cuda, x, None, np.array([[2.0, -0.2, 2.0, 0.2]]), 1, g, 5)
    assert (wide[0, [0, 1, 3, 4]] == 10).all() and wide[0, 2] == np.float32(d), "max_range beside the wall"
    assert got[0, 2] == wl_.oracle_scan(x, None, sg, 1, g, 5)[0, 2]


@pytest.mark.parametrize("G", [1, 3])
def test_no_segments_is_the_body_twin(capi, cuda, G):
    c = bc_.track_scan(64, races=2, G=G) if G > 1 else bc_.ScanCase("alone", wc_.track_poses(5), 1, wc_.track_world(), beams=64)
    x = c.x[:6] if G == 3 else c.x
    for static in (c.static, None):
        same_bits(wall_cast(capi, cuda, x, static, None, G, c.geom, c.beams), body_cast(capi, cuda, x, static, G, c.geom, c.beams),
                  f"cast G {G} C {0 if static is None else len(static)}")
        a, an = clearance(capi, cuda, x, static, None, G)
        b, bn = body_clearance(capi, cuda, x, static, G)
        assert (bits(a) == bits(b)).all() and (an == bn).all(), (G, static is None)


@pytest.mark.parametrize("c", wl_.scan_cases(), ids=lambda c: c.name)
def test_scans_against_the_oracle(capi, cuda, c):
    """The track at 64 poses, S = 255, 256, 257, the first segment in the last slot of a tile and the first of the
    next, segments only, a segment set per car, B = 2 x 512 + 6."""
    got = scan(capi, cuda, c)
    assert (got != SENTINEL).all()
    c.check(got)
    assert (c.oracle() < wc_.MAX_RANGE).any()


def test_tile_layout_of_the_edge_cases():
    a, b = wl_.tile_scan(3, C=wl_.TILE - 3, G=3), wl_.tile_scan(3, C=wl_.TILE - 2, G=3)
    assert a.static.shape[0] + (a.G - 1) == wl_.TILE - 1 and b.static.shape[0] + (b.G - 1) == wl_.TILE


def test_closed_polygon_aimed_at_its_vertices(capi, cuda):
    """37 cars inside a star polygon, angle_min = 0, car k's heading aims beam 0 at vertex k: no beam of any car
    returns max_range and every range is at most the farthest vertex."""
    sg = wl_.star_polygon(37, 4)
    rng = np.random.default_rng(5)
    xy = rng.uniform(-1.0, 1.0, (37, 2))
    yaw0 = np.arctan2(sg[:, 1] - xy[:, 1], sg[:, 0] - xy[:, 0])
    x = np.concatenate([xy, yaw0[:, None]], 1)
    for _ in range(3):  # the LiDAR sits 0.275 m ahead of the pose: aim from there
        ox, oy = x[:, 0] + wc_.LIDAR_OFFSET * np.cos(x[:, 2]), x[:, 1] + wc_.LIDAR_OFFSET * np.sin(x[:, 2])
        x[:, 2] = np.arctan2(sg[:, 1] - oy, sg[:, 0] - ox)
    g = (np.float32(0.0), np.float32(2 * np.pi / 360), np.float32(2 * np.pi * 359 / 360))
    got = wall_cast(capi, cuda, x, None, sg, 1, g, 360)
    far = np.hypot(sg[:, 0], sg[:, 1]).max() + 1.0 + wc_.LIDAR_OFFSET + 0.5
    assert far < wc_.MAX_RANGE and (got < wc_.MAX_RANGE).all() and (got <= np.float32(far)).all()
    want = wl_.oracle_scan(x, None, sg, 1, g, 360)
    assert (want < wc_.MAX_RANGE).all()


def test_listed_mode(capi, cuda):
    c = wl_.tile_scan(40, C=5, G=1, B=8)
    full = scan(capi, cuda, c)
    got = scan(capi, cuda, c, listed=[5, 2, 7, 0, 0, 0, 0, 0], count=2)
    same_bits(got[[5, 2]], full[[5, 2]], "listed rows")
    assert (np.delete(got, [5, 2], axis=0) == SENTINEL).all(), "unlisted rows stay"
    none = scan(capi, cuda, c, listed=[5, 2, 7, 0, 0, 0, 0, 0], count=0)
    assert (none == SENTINEL).all(), "count = 0 writes nothing"


def test_order_independence(capi, cuda):
    c = wl_.tile_scan(257, C=7, G=3)
    full = scan(capi, cuda, c)
    perm = np.random.default_rng(8).permutation(c.segments.shape[0])
    same_bits(wall_cast(capi, cuda, c.x, c.static, c.segments[perm], c.G, c.geom, c.beams), full, "permuted segments")
    k = wl_.rows_case(9)
    clear, near = run(capi, cuda, k)
    cp, npm = clearance(capi, cuda, k.x, k.circles, k.segments[::-1].copy(), k.G)  # reversed
    assert (bits(cp) == bits(clear)).all()
    first = k.C + k.G
    wall = near >= first
    assert wall.any() and ((k.S - 1 - (npm[wall] - first)) == near[wall] - first).all() and (npm[~wall] == near[~wall]).all()


def test_odd_inputs(capi, cuda):
    g = (np.float32(-0.5), np.float32(0.25), np.float32(0.5))
    x = np.zeros((1, 3))
    wall = [2.0, -1.0, 2.0, 1.0]
    ref = wall_cast(capi, cuda, x, None, np.array([wall]), 1, g, 5)
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for k in range(4):
            s = [1.0, -1.0, 1.0, 1.0]  # nearer than the wall: it would win every beam it met
            s[k] = v
            bad.append(s)
    odd = np.array(bad + [wall] + [[1.0, 0.0, 1.0, 0.0]])  # and a zero-length segment on beam 2
    same_bits(wall_cast(capi, cuda, x, None, odd, 1, g, 5), ref, "NaN, infinite and zero-length segments hit nothing")
    # a LiDAR exactly on a wall does not see it; a wall edge-on at heading 0 (along beam 2) hits nothing on that beam
    on = np.array([[wc_.LIDAR_OFFSET, -1.0, wc_.LIDAR_OFFSET, 1.0], wall])
    same_bits(wall_cast(capi, cuda, x, None, on, 1, g, 5), ref, "the LiDAR on a wall")
    edge = wall_cast(capi, cuda, x, None, np.array([[1.0, 0.0, 1.5, 0.0], wall]), 1, g, 5)
    same_bits(edge, ref, "a wall edge-on")
    c0, n0 = clearance(capi, cuda, x, None, odd, 1, off=0.0)
    assert n0[0, 0] == 0 + 1 + 13 and c0[0, 0] == 1.0 - wl_.HL, "the zero-length segment 1 m ahead is the nearest"
    cn, nn = clearance(capi, cuda, x, None, np.array(bad), 1, off=0.0)
    assert np.isposinf(cn).all() and (nn == -1).all()
    xn = np.array([[np.nan, 0.0, 0.0], [0.0, 0.0, np.inf]])
    cx, nx = clearance(capi, cuda, xn, None, np.array([wall]), 1)
    assert np.isposinf(cx).all() and (nx == -1).all()


# ---- clearance -----------------------------------------------------------------------------------------------

def test_heading_zero_is_bit_equal(capi, cuda):
    c = wl_.heading0_case()
    assert c.exact
    c.check(*run(capi, cuda, c))


@pytest.mark.parametrize("rows", wl_.ROWS)
def test_row_passes(capi, cuda, rows):
    c = wl_.rows_case(rows)
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    assert (c.oracle()[1] >= c.C + c.G).any(), "a segment is somebody's nearest"
    no_idx, _ = clearance(capi, cuda, c.x, c.circles, c.segments, c.G, nearest=False)  # nearest NULL
    assert (bits(no_idx) == bits(clear)).all()


def test_three_index_ranges(capi, cuda):
    c = wl_.ranges_case()
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    assert near[0].tolist() == [0, c.C + 2, c.C + 1, c.C + c.G + 1]


@pytest.mark.parametrize("name", ["track", "per_car", "stride"])
def test_other_shapes(capi, cuda, name):
    c = {"track": wl_.track_case, "per_car": wl_.per_car_case, "stride": wl_.stride_case}[name]()
    c.check(*run(capi, cuda, c))


@pytest.mark.parametrize("name", list(wl_.sign_cases()))
def test_sign_cases(capi, cuda, name):
    c, want = wl_.sign_case(name)
    assert c.exact
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    holds = wl_.sign_cases()[name][2]
    v = float(clear[0, 0])
    assert {"< 0": v < 0, "== 0": v == 0.0, "> 0": v > 0}[holds] and near[0, 0] == 0 + 1 + 0
    assert v == float(workload.clearance_walls(c.x, None, c.segments, 1, 0.0)[0][0, 0])
