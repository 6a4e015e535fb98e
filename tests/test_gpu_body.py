"""The rectangular-body kernels on MI355X (f110qp_clearance_body_dev, f110qp_cast_scans_body_dev; include/f110qp.h
"rectangular car bodies") against the numpy oracles workload.clearance_body and workload.ray_bodies: body_cases'
derived bounds and skip rules, bit equality where every heading is 0, the passes, the grid stride, mates across
the tile edge, ties, permutations, non-finite and odd inputs, symmetry. Every clearance call writes between two
guard rows; every scan row starts as a sentinel. The cases are built in body_cases.py (test_body_cases.py holds
them to the skip cap on the CPU)."""
import body_cases as bc_
import contact_cases as cc_
import numpy as np
import pytest
import world_cases as wc_
from test_gpu_rollout import same_bits
from test_gpu_rollout_replan import dev
from test_gpu_rollout_scan import scan_config
from test_gpu_world_scan import SENTINEL, cast

from f110qp import workload

pytestmark = pytest.mark.gpu


def clearance(capi, cuda, x, circles, G, off=bc_.CENTER_OFFSET, hl=bc_.HL, hw=bc_.HW, nearest=True):
    """f110qp_clearance_body_dev on x [rows,B,3] -> (clearance [rows,B], nearest [rows,B] or None) as numpy."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    x = x[None] if x.ndim == 2 else x
    rows, B = x.shape[:2]
    Cn = 0 if circles is None else circles.shape[-2]
    wc = capi.default_world_config(num_circles=Cn, world_rows=1 if circles is None or circles.ndim == 2 else B)
    race = capi.default_race_config(group_size=G, center_offset=off)
    body = capi.default_body_config(half_length=hl, half_width=hw)
    out = torch.full((rows + 2, B), -7.0, dtype=torch.float64, device=cuda)  # a guard row at either end
    near = torch.full((rows + 2, B), -7, dtype=torch.int32, device=cuda) if nearest else None
    capi.clearance_body_dev(wc, race, body, dev(cuda, x), None if circles is None else dev(cuda, circles), out[1:-1],
                            near[1:-1] if nearest else None)
    torch.cuda.synchronize(cuda)
    out = out.cpu().numpy()
    assert (out[[0, -1]] == -7.0).all(), "clearance: a guard row was written"
    if not nearest:
        return np.ascontiguousarray(out[1:-1]), None
    near = near.cpu().numpy()
    assert (near[[0, -1]] == -7).all(), "nearest: a guard row was written"
    return np.ascontiguousarray(out[1:-1]), np.ascontiguousarray(near[1:-1])


def run(capi, cuda, c):
    return clearance(capi, cuda, c.x, c.circles, c.G, c.off, c.hl, c.hw)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def body_cast(capi, cuda, x, static, G, geom, beams, listed=None, count=None, off=bc_.CENTER_OFFSET):
    """f110qp_cast_scans_body_dev on host arrays into rows pre-filled with the sentinel -> ranges [B, R]."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    B = x.shape[0]
    C = 0 if static is None else static.shape[-2]
    w = capi.default_world_config(num_circles=C, world_rows=1 if static is None or static.ndim == 2 else static.shape[0])
    race = capi.default_race_config(group_size=G, center_offset=off)
    out = torch.full((B, beams), float(SENTINEL), dtype=torch.float32, device=cuda)
    capi.cast_scans_body_dev(scan_config(capi, beams, geom), w, race, capi.default_body_config(), dev(cuda, x),
                             dev(cuda, static) if C else None, out,
                             list_=None if listed is None else dev(cuda, np.asarray(listed, np.int32)),
                             count=None if listed is None else dev(cuda, np.int32([count])))
    torch.cuda.synchronize(cuda)
    return out.cpu().numpy()


# ---- clearance ---------------------------------------------------------------------------------------------

def test_heading_zero_is_bit_equal(capi, cuda):
    c = bc_.heading0_case()
    assert c.exact
    c.check(*run(capi, cuda, c))
    want = c.oracle()[0]
    assert (want < 0).any() and (want > 0).any(), "cars in contact and cars clear"


@pytest.mark.parametrize("rows", bc_.ROWS)
def test_row_passes(capi, cuda, rows):
    """rows = 1, 8, 9, 17: one row, a whole pass, a second pass of one row, a third behind two whole ones."""
    c = bc_.rows_case(rows)
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    wnear = c.oracle()[1]
    assert (wnear >= c.C).any() or rows == 1
    no_idx, _ = clearance(capi, cuda, c.x, c.circles, c.G, nearest=False)  # nearest NULL
    assert (bits(no_idx) == bits(clear)).all()


def test_grid_stride(capi, cuda):
    """B = 1030 = 2 x 512 + 6 in races of 5, a world per car: six workgroups take a third car."""
    c = bc_.stride_case()
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    wnear = c.oracle()[1][:, 2 * bc_.CLEAR_GRID - 4:]
    assert (wnear >= c.C).any() and (wnear < c.C).any()


def test_mates_cross_the_tile_edge(capi, cuda):
    c = bc_.crowd_case()
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    # mate 0 (index 255) is the only one in the first tile: the nearest lie in both tiles, circles and mates
    assert c.C < wc_.TILE < c.C + c.G - 1 and (near >= wc_.TILE).any() and (near < c.C).any()


@pytest.mark.parametrize("name", ["no_circles", "group_of_one", "world_per_car", "track"])
def test_other_shapes(capi, cuda, name):
    c = {"no_circles": lambda: bc_.of(cc_.edge_case(0, 5)), "group_of_one": lambda: bc_.of(cc_.batch_case(65, 1)),
         "world_per_car": lambda: bc_.of(cc_.random_case(True)), "track": lambda: bc_.of(cc_.track_case())}[name]()
    if name == "no_circles":
        assert c.circles is None and c.G == 2
    if name == "group_of_one":
        assert c.G == 1
    c.check(*run(capi, cuda, c))


def test_ties_and_permutations(capi, cuda):
    c = bc_.of(cc_.track_case())
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    b = int(np.flatnonzero(near[0] < c.C)[0])  # a car whose nearest is a circle
    k = near[0, b]
    dup = np.concatenate([c.circles, c.circles[k:k + 1]])  # its nearest again, last: the lower index wins
    cd, nd = clearance(capi, cuda, c.x, dup, c.G)
    assert nd[0, b] == k and (bits(cd) == bits(clear)).all()
    first = np.concatenate([c.circles[k:k + 1], c.circles])
    cf, nf = clearance(capi, cuda, c.x, first, c.G)
    assert nf[0, b] == 0 and (bits(cf) == bits(clear)).all()
    perm = np.random.default_rng(8).permutation(c.C)
    cp, npm = clearance(capi, cuda, c.x, c.circles[perm], c.G)
    assert (bits(cp) == bits(clear)).all()
    static = near < c.C
    assert (perm[npm[static]] == near[static]).all() and (npm[~static] == near[~static]).all()
    rp = np.concatenate([g * c.G + np.random.default_rng(9 + g).permutation(c.G) for g in range(c.B // c.G)])
    cr, _ = clearance(capi, cuda, c.x[:, rp], c.circles, c.G)
    assert (bits(cr) == bits(clear[:, rp])).all()
    # an exact tie between two mates at heading 0: cars at equal distances to either side of car 1
    x = np.array([[0.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.0, -0.5, 0.0]])
    ct, nt = clearance(capi, cuda, x, None, 3, off=0.0)
    assert nt[0, 1] == 0 and ct[0, 1] == (0.5 - bc_.HW) - bc_.HW and (bits(ct) == bits(workload.clearance_body(x, None, 3, 0.0)[0])).all()


def test_non_finite_and_odd_inputs(capi, cuda):
    x = cc_.poses(1, 4, 33)[0]
    base = wc_.random_world(20, 34)
    near_c = [x[0, 0] + 0.2, x[0, 1], 0.1]
    bad = []
    for k, vals in ((0, (np.nan, np.inf, -np.inf)), (1, (np.nan, np.inf, -np.inf)), (2, (np.nan,))):
        for v in vals:
            cbad = list(near_c)
            cbad[k] = v
            bad.append(cbad)
    ci = np.concatenate([base[:10], bad, base[10:]])
    clear, near = clearance(capi, cuda, x, ci, 1)
    ref_c, ref_n = clearance(capi, cuda, x, base, 1)
    assert (bits(clear) == bits(ref_c)).all(), "a NaN or infinite circle is never chosen and disturbs nobody"
    assert not np.isin(near, np.arange(10, 10 + len(bad))).any()
    bc_.BodyCase("non-finite circles", x, 1, ci).check(clear, near)
    xn = x.copy()
    xn[1, 2] = np.nan  # a NaN mate is never chosen; the car with the NaN pose gets +inf and -1
    cn, nn = clearance(capi, cuda, xn, base, 4)
    assert np.isposinf(cn[0, 1]) and nn[0, 1] == -1 and not (nn[0, [0, 2, 3]] == 20 + 1).any()
    bc_.BodyCase("NaN pose", xn, 4, base).check(cn, nn)
    xi = x.copy()
    xi[2, 0] = np.inf
    ci_, ni_ = clearance(capi, cuda, xi, base, 4)
    assert np.isposinf(ci_[0, 2]) and ni_[0, 2] == -1 and not (ni_[0, [0, 1, 3]] == 20 + 2).any()
    bc_.BodyCase("infinite pose", xi, 4, base).check(ci_, ni_)
    neg = base.copy()
    neg[::2, 2] *= -1.0  # a negative radius gives the bits of its absolute value
    cg, ng = clearance(capi, cuda, x, neg, 1)
    assert (bits(cg) == bits(ref_c)).all() and (ng == ref_n).all()
    c0, n0 = clearance(capi, cuda, x, None, 1)  # nothing to touch
    assert np.isposinf(c0).all() and (n0 == -1).all()


def test_pair_symmetry(capi, cuda):
    """Pairs whose nearest obstacle is the other car, overlapping and apart: the same bits from either side."""
    x = cc_.poses(5, 6, 44) * [4.0, 4.0, 1.0]
    x[:, 1::2, :2] = x[:, 0::2, :2] + [0.45, 0.2]
    clear, near = clearance(capi, cuda, x, wc_.random_world(30, 45) * [5.0, 5.0, 0.2], 2)
    assert (near[:, 0::2] == 30 + 1).all() and (near[:, 1::2] == 30 + 0).all()
    assert (bits(clear[:, 0::2]) == bits(clear[:, 1::2])).all() and (clear < 0).any() and (clear > 0).any()


# ---- the cast ----------------------------------------------------------------------------------------------

def test_group_of_one_is_the_plain_cast(capi, cuda):
    x, w = wc_.track_poses(5), wc_.track_world()
    g = wc_.geometry(1080)
    same_bits(body_cast(capi, cuda, x, w, 1, g, 1080), cast(capi, cuda, x, w, g, 1080), "G = 1")
    same_bits(body_cast(capi, cuda, x, None, 1, g, 1080), cast(capi, cuda, x, np.zeros((0, 3)), g, 1080), "G = 1, C = 0")


@pytest.mark.parametrize("c", bc_.scan_cases(), ids=lambda c: c.name)
def test_opponents_against_the_oracle(capi, cuda, c):
    got = body_cast(capi, cuda, c.x, c.static, c.G, c.geom, c.beams, off=c.off)
    assert (got != SENTINEL).all()
    c.check(got)
    if c.name == "body parallel":
        rear = ((2.0 + bc_.CENTER_OFFSET) - wc_.LIDAR_OFFSET) - bc_.HL
        assert got[0, 2] == np.float32(rear) and (got[0, [0, 4]] == 10).all() and (got[1] == 10).all()
    if c.name == "body inside":
        alone = body_cast(capi, cuda, c.x[[0, 2, 2]], None, 3, c.geom, c.beams)
        same_bits(got[0], alone[0], "the LiDAR inside car 1 sees through it")
        assert (got[0] < 10).any()
    if c.name == "body seam":
        assert got[0, 0] < 10 and got[0, -1] < 10 and (got[0] < 10).sum() >= 4, "car 1 across the first and last beam"


def test_listed_mode(capi, cuda):
    c = bc_.track_scan(64)
    full = body_cast(capi, cuda, c.x, c.static, c.G, c.geom, c.beams)
    got = body_cast(capi, cuda, c.x, c.static, c.G, c.geom, c.beams, listed=[5, 2, 7, 0, 0, 0, 0, 0], count=2)
    same_bits(got[[5, 2]], full[[5, 2]], "listed rows")
    assert (np.delete(got, [5, 2], axis=0) == SENTINEL).all(), "unlisted rows stay"


def test_order_independence(capi, cuda):
    c = bc_.track_scan(64)
    full = body_cast(capi, cuda, c.x, c.static, c.G, c.geom, c.beams)
    rp = np.concatenate([g * c.G + np.random.default_rng(9 + g).permutation(c.G) for g in range(len(c.x) // c.G)])
    perm = np.random.default_rng(8).permutation(len(c.static))
    same_bits(body_cast(capi, cuda, c.x[rp], c.static[perm], c.G, c.geom, c.beams), full[rp], "permuted")
