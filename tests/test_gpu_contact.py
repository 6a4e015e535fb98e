"""The clearance kernel on MI355X (f110qp_clearance_dev, include/f110qp.h "contact") against the numpy oracle
workload.clearance: bit equality at center_offset = 0, contact_cases' derived bound and skip rule with the
default offset, the tile and tail edges, more rows than a pass takes, more cars than workgroups, ties,
permutations, non-finite and odd inputs, symmetry. Every call writes between two guard rows that must stay as
they were. Every case is built in contact_cases.py (test_contact_cases.py holds them to the skip cap on the
CPU)."""
import contact_cases as cc_
import numpy as np
import pytest
import world_cases as wc_
from test_gpu_rollout_replan import dev

pytestmark = pytest.mark.gpu


def clearance(capi, cuda, x, circles, G, off=cc_.CENTER_OFFSET, R=cc_.CAR_RADIUS, nearest=True):
    """f110qp_clearance_dev on x [rows,B,3] -> (clearance [rows,B], nearest [rows,B] or None) as numpy."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    x = x[None] if x.ndim == 2 else x
    rows, B = x.shape[:2]
    Cn = 0 if circles is None else circles.shape[-2]
    wc = capi.default_world_config(num_circles=Cn, world_rows=1 if circles is None or circles.ndim == 2 else B)
    race = capi.default_race_config(group_size=G, car_radius=R, center_offset=off)
    # one guard row in front of the call's rows and one behind: the call must leave both as they are
    out = torch.full((rows + 2, B), -7.0, dtype=torch.float64, device=cuda)
    near = torch.full((rows + 2, B), -7, dtype=torch.int32, device=cuda) if nearest else None
    capi.clearance_dev(wc, race, dev(cuda, x), None if circles is None else dev(cuda, circles), out[1:-1],
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
    return clearance(capi, cuda, c.x, c.circles, c.G, c.off, c.R)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("per_car", [False, True], ids=["one_world", "world_per_car"])
def test_bit_equality_without_an_offset(capi, cuda, per_car):
    """center_offset = 0: the centres are the poses' bits, clearance and nearest equal the oracle's."""
    c = cc_.random_case(per_car, 0.0)
    c.check(*run(capi, cuda, c))
    assert (c.oracle()[0] < 0).any() and (c.oracle()[0] > 0).any(), "cars in contact and cars clear"


@pytest.mark.parametrize("per_car", [False, True], ids=["one_world", "world_per_car"])
def test_default_offset_within_the_bound(capi, cuda, per_car):
    c = cc_.random_case(per_car)
    worst = c.check(*run(capi, cuda, c))
    print(f"{c.name}: worst error {worst:.3f} of the bound {c.tol:.2e}")


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("C", [0, 1, cc_.TILE - 1, cc_.TILE, cc_.TILE + 1, 2 * cc_.TILE + 1])
def test_tile_edges(capi, cuda, C, rows):
    """The nearest circle placed last; C = 0 with circles NULL and G = 2."""
    c = cc_.edge_case(C, rows)
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    if C:
        assert c.oracle()[1][0, 0] == C - 1, "the last circle is the nearest of the first pose"
    no_idx, _ = clearance(capi, cuda, c.x, c.circles, c.G, nearest=False)  # nearest NULL
    assert (bits(no_idx) == bits(clear)).all()


def test_mates_span_two_tiles(capi, cuda):
    c = cc_.crowd_case()
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    assert (near >= c.C + cc_.TILE).any() and (near < c.C + cc_.TILE).any()


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_batch_sizes(capi, cuda, B, rows):
    c = cc_.batch_case(B, rows)
    c.check(*run(capi, cuda, c))


@pytest.mark.parametrize("off", cc_.OFFSETS, ids=["offset_0", "default_offset"])
@pytest.mark.parametrize("rows", cc_.PASS_ROWS)
def test_row_passes(capi, cuda, rows, off):
    """More rows than one pass of eight takes: a whole pass, a second pass of one row, a third behind two whole
    ones. Every row is scattered anew and G = 3, so a centre kept from the pass before, or an output or a mate's
    row indexed inside the pass instead of inside the call, is metres off. The circle over car 0 at the last
    row is the nearest there."""
    c = cc_.rows_case(rows, off)
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    wnear = c.oracle()[1]
    assert wnear[rows - 1, 0] == c.C - 1 and (wnear[:rows - 1, 0] != c.C - 1).any()
    assert (wnear >= c.C).any() and (wnear < c.C).any(), "mates and circles are both somebody's nearest"
    if off == 0.0:
        no_idx, _ = clearance(capi, cuda, c.x, c.circles, c.G, off, nearest=False)  # nearest NULL
        assert (bits(no_idx) == bits(clear)).all()


@pytest.mark.parametrize("off", cc_.OFFSETS, ids=["offset_0", "default_offset"])
@pytest.mark.parametrize("per_car", [True, False], ids=["world_per_car", "one_world"])
def test_grid_stride(capi, cuda, per_car, off):
    """B = GRID + 6: six workgroups take a second car, whose world lies past the cap's offset, and the races
    around car 1,024 have their mates in other workgroups' strides."""
    c = cc_.stride_case(per_car, off)
    assert c.B == cc_.GRID + 6 and c.B % c.G == 0 and (cc_.GRID // c.G) * c.G < cc_.GRID < (cc_.GRID // c.G + 1) * c.G
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    wnear = c.oracle()[1][:, cc_.GRID - 4:]
    assert (wnear >= c.C).any() and (wnear < c.C).any(), "past the cap: mates and circles are both somebody's nearest"
    if per_car and off == 0.0:
        no_idx, _ = clearance(capi, cuda, c.x, c.circles, c.G, off, nearest=False)  # nearest NULL
        assert (bits(no_idx) == bits(clear)).all()


@pytest.mark.parametrize("off", cc_.OFFSETS, ids=["offset_0", "default_offset"])
def test_grid_stride_with_a_second_pass(capi, cuda, off):
    """B = GRID + 6 and rows = 9: the second pass of the second car of a workgroup."""
    c = cc_.stride_rows_case(off)
    assert c.B == cc_.GRID + 6 and c.rows == cc_.PASS + 1 and c.world_rows == c.B
    c.check(*run(capi, cuda, c))


def test_ties_and_permutations(capi, cuda):
    """A duplicated circle reports the lower index; a permuted circle list (the track world's 1,040 circles) and
    a permuted race give every car the same clearance bits."""
    c = cc_.track_case()
    clear, near = run(capi, cuda, c)
    c.check(clear, near)
    dup = np.concatenate([c.circles, c.circles[near[0, 0]:near[0, 0] + 1]])  # car 0's nearest again, last
    cd, nd = clearance(capi, cuda, c.x, dup, c.G)
    assert nd[0, 0] == near[0, 0] and (bits(cd) == bits(clear)).all()
    first = np.concatenate([c.circles[near[0, 0]:near[0, 0] + 1], c.circles])     # and again, first
    cf, nf = clearance(capi, cuda, c.x, first, c.G)
    assert nf[0, 0] == 0 and (bits(cf) == bits(clear)).all()
    perm = np.random.default_rng(8).permutation(c.C)
    cp, npm = clearance(capi, cuda, c.x, c.circles[perm], c.G)
    assert (bits(cp) == bits(clear)).all()
    static = near < c.C
    assert (perm[npm[static]] == near[static]).all() and (npm[~static] == near[~static]).all()
    rp = np.concatenate([g * c.G + np.random.default_rng(9 + g).permutation(c.G) for g in range(c.B // c.G)])
    cr, _ = clearance(capi, cuda, c.x[:, rp], c.circles, c.G)
    assert (bits(cr) == bits(clear[:, rp])).all()


def test_non_finite_and_odd_inputs(capi, cuda):
    x = cc_.poses(1, 4, 33)[0]
    base = wc_.random_world(20, 34)
    near_c = [x[0, 0] + 0.2, x[0, 1], 0.1]  # would be car 0's nearest, were it finite
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
    cc_.ContactCase("non-finite circles", x, 1, ci).check(clear, near)
    # an infinite radius is, by the stated arithmetic, contact with everything: -inf, as the oracle says
    cinf = np.concatenate([base, [[0.0, 0.0, np.inf]]])
    ci_, ni_ = clearance(capi, cuda, x, cinf, 1)
    assert np.isneginf(ci_).all() and (ni_ == 20).all()
    # a NaN mate is never chosen; the car with the NaN pose gets +inf and -1
    xn = x.copy()
    xn[1, 2] = np.nan
    cn, nn = clearance(capi, cuda, xn, base, 4)
    assert np.isposinf(cn[0, 1]) and nn[0, 1] == -1
    assert not (nn[0, [0, 2, 3]] == 20 + 1).any()
    cc_.ContactCase("NaN pose", xn, 4, base).check(cn, nn)
    xi = x.copy()
    xi[2, 0] = np.inf
    cc_.ContactCase("infinite pose", xi, 4, base).check(*clearance(capi, cuda, xi, base, 4))
    # a negative radius gives the bits of its absolute value
    neg = base.copy()
    neg[::2, 2] *= -1.0
    cg, ng = clearance(capi, cuda, x, neg, 1)
    assert (bits(cg) == bits(ref_c)).all() and (ng == ref_n).all()
    # nothing to touch
    c0, n0 = clearance(capi, cuda, x, None, 1)
    assert np.isposinf(c0).all() and (n0 == -1).all()


def test_pair_symmetry(capi, cuda):
    """Pairs whose nearest obstacle is the other car: the two clearances are the same bits."""
    x = cc_.poses(5, 6, 44) * [4.0, 4.0, 1.0]
    x[:, 1::2, :2] = x[:, 0::2, :2] + [0.45, 0.2]  # the mate's pose 0.49 m away: bodies that overlap or nearly
    clear, near = clearance(capi, cuda, x, wc_.random_world(30, 45) * [5.0, 5.0, 0.2], 2)
    assert (near[:, 0::2] == 30 + 1).all() and (near[:, 1::2] == 30 + 0).all()
    assert (bits(clear[:, 0::2]) == bits(clear[:, 1::2])).all() and (clear < 0).any() and (clear > 0).any()
