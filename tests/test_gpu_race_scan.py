"""The ray-cast kernel's race instantiation on MI355X (f110qp_cast_scans_race_dev): the cars of a race see each
other. Against the plain cast it is bit equality (G = 1; center_offset = 0, where the opponents' centres are
the poses' bits and the plain cast at world_rows = B can be given the same circles); against the numpy oracle
it is world_cases' bound and cap on per-car circle rows built by workload.race_circles (race_cases.py)."""
import numpy as np
import pytest
import race_cases as rc_
import world_cases as wc_
from test_gpu_rollout import same_bits
from test_gpu_rollout_scan import scan_config
from test_gpu_world_scan import SENTINEL, cast

from f110qp import workload

pytestmark = pytest.mark.gpu


def race_cast(capi, cuda, x, static, G, geom, beams, listed=None, count=None, center_offset=rc_.CENTER_OFFSET,
              car_radius=rc_.CAR_RADIUS):
    """f110qp_cast_scans_race_dev on host arrays into rows pre-filled with the sentinel -> ranges [B, R].
    static: [C, 3], [B, C, 3] or None (C = 0: circles NULL)."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    B = x.shape[0]
    C = 0 if static is None else static.shape[-2]
    w = capi.default_world_config(num_circles=C, world_rows=1 if static is None or static.ndim == 2 else static.shape[0])
    race = capi.default_race_config(group_size=G, center_offset=center_offset, car_radius=car_radius)
    out = torch.full((B, beams), float(SENTINEL), dtype=torch.float32, device=cuda)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    capi.cast_scans_race_dev(scan_config(capi, beams, geom), w, race, dev(x), dev(static) if C else None, out,
                             list_=None if listed is None else dev(np.asarray(listed, np.int32)),
                             count=None if listed is None else dev(np.int32([count])))
    torch.cuda.synchronize(cuda)
    return out.cpu().numpy()


def plain_route(capi, cuda, x, static, G, geom, beams, car_radius=rc_.CAR_RADIUS):
    """The same scans at center_offset = 0 from f110qp_cast_scans_dev at world_rows = B: every car's row is
    its static circles followed by race_circles(...) built in numpy (exact at offset 0)."""
    return cast(capi, cuda, x, rc_.rows_with_opponents(x, static, G, car_radius, 0.0), geom, beams)


def test_group_of_one_is_the_plain_cast(capi, cuda):
    """1. G = 1 through the race call equals f110qp_cast_scans_dev bit for bit: the track world, and C = 0."""
    x = wc_.track_poses(5)
    w = wc_.track_world()
    same_bits(race_cast(capi, cuda, x, w, 1, rc_.GEOM, rc_.R), cast(capi, cuda, x, w, rc_.GEOM, rc_.R), "track world")
    got = race_cast(capi, cuda, x, None, 1, rc_.GEOM, rc_.R)
    same_bits(got, cast(capi, cuda, x, np.zeros((0, 3)), rc_.GEOM, rc_.R), "C = 0")
    assert (got == np.float32(wc_.MAX_RANGE)).all()


@pytest.mark.parametrize("B,G,R,C", [(6, 3, 1080, 40), (4, 2, 1200, 40)], ids=["B6-G3-R1080", "B4-G2-R1200"])
def test_offset_zero_equals_the_plain_cast_on_built_rows(capi, cuda, B, G, R, C):
    """2. center_offset = 0: bit-equal to the plain cast whose per-car rows hold the opponents' circles."""
    g = wc_.geometry(R)
    x = wc_.poses_near_origin(B, 300 + R)
    x[:, :2] *= 4.0  # within 1.6 m: the cars see each other, some from inside a circle
    w = wc_.random_world(C, 301 + R)
    got = race_cast(capi, cuda, x, w, G, g, R, center_offset=0.0)
    same_bits(got, plain_route(capi, cuda, x, w, G, g, R), f"B {B} G {G} R {R}")
    # from the oracle: every car but one (B = 4: car 2's LiDAR is inside its opponent's circle) sees an opponent
    assert (got != cast(capi, cuda, x, w, g, R)).any(axis=1).sum() >= B - 1


def test_default_offset_against_the_oracle(capi, cuda):
    """3. The default offset against the oracle on rows from race_circles: two races of four in the track
    world; and two cars in an empty world, one 1.5 m ahead of the other."""
    c = rc_.track_race()
    got = race_cast(capi, cuda, c.x, c.static, c.G, c.geom, c.beams)
    skipped, worst = c.check(got)
    alone = cast(capi, cuda, c.x, c.static, c.geom, c.beams)
    assert ((got != alone).sum(axis=1) >= 10).all(), "every car sees a race-mate"
    p = rc_.pair_in_line()
    got = race_cast(capi, cuda, p.x, None, 2, p.geom, p.beams)
    _, w2 = p.check(got)
    want = rc_.GAP + rc_.CENTER_OFFSET - wc_.LIDAR_OFFSET - rc_.CAR_RADIUS
    assert abs(float(got[0].min()) - want) <= np.spacing(np.float32(want)) + wc_.ABS_TOL, (got[0].min(), want)
    ang = p.geom[0] + p.geom[1] * np.arange(p.beams, dtype=np.float64)
    assert (got[1][np.abs(ang) < np.pi / 2] == np.float32(wc_.MAX_RANGE)).all(), "the leader sees nothing ahead"
    print(f"track race: {skipped} skipped, worst {worst:.3f} of the bound; pair: worst {w2:.3f}")


@pytest.mark.parametrize("C", [250, 0])
def test_opponents_across_circle_tiles(capi, cuda, C):
    """4. One race of 258 cars, 64 beams: with C = 250 the static circles and the first opponents share a
    circle tile and the opponents span two; C = 0 is the opponents alone in two tiles. Six cars against the
    oracle at the default offset; all cars bit-equal to the plain cast's route at offset 0."""
    c = rc_.crowd(C)
    got = race_cast(capi, cuda, c.x, c.static, c.G, c.geom, c.beams)
    _, worst = c.check(got)
    assert (got < wc_.MAX_RANGE).any(axis=1).all()
    zero = race_cast(capi, cuda, c.x, c.static, c.G, c.geom, c.beams, center_offset=0.0)
    same_bits(zero, plain_route(capi, cuda, c.x, c.static, c.G, c.geom, c.beams), f"crowd C {C} at offset 0")
    print(f"crowd C {C}: worst {worst:.3f} of the bound")


def test_more_cars_than_workgroups(capi, cuda):
    """4b. B = 780 in races of 4, above the grid cap of 768, one world of three circles per car, at offset 0:
    bit-equal to the plain cast on built rows. The plain kernel above its cap meets the oracle in
    test_gpu_world_scan_edges.py, so this ties the race instantiation's stride and per-car world offset to it."""
    c = rc_.stride_race()
    got = race_cast(capi, cuda, c.x, c.static, c.G, c.geom, c.beams, center_offset=0.0)
    same_bits(got, plain_route(capi, cuda, c.x, c.static, c.G, c.geom, c.beams), c.name)
    alone = cast(capi, cuda, c.x, c.static, c.geom, c.beams)
    past = slice(rc_.CAST_GRID - c.G, None)  # the races with a car past the cap
    assert (got[past] != alone[past]).any(axis=1).sum() >= 8, "the cars past the cap see their race-mates"
    assert (alone[past] < wc_.MAX_RANGE).any(axis=1).sum() >= 8, "... and their own circles"


def test_order_independence(capi, cuda):
    """5. Permuting the cars inside each race permutes the scans, bit for bit (and so does the order of the
    static circles)."""
    x = workload.make_race_grid(3, 4, 31)
    w = wc_.track_world()
    base = race_cast(capi, cuda, x, w, 4, rc_.GEOM, rc_.R)
    perm = np.array([3, 1, 0, 2, 5, 4, 7, 6, 10, 11, 8, 9])
    same_bits(race_cast(capi, cuda, x[perm], w[::-1], 4, rc_.GEOM, rc_.R), base[perm], "permuted races")


def test_races_are_disjoint(capi, cuda):
    """6. Two races at identical poses: each car's row is what its race gives cast alone."""
    one = workload.make_race_grid(1, 3, 32)
    w = wc_.random_world(40, 33) + np.array([one[0, 0], one[0, 1], 0.0])
    alone = race_cast(capi, cuda, one, w, 3, rc_.GEOM, rc_.R)
    both = race_cast(capi, cuda, np.concatenate([one, one]), w, 3, rc_.GEOM, rc_.R)
    same_bits(both[:3], alone, "first race")
    same_bits(both[3:], alone, "second race")
    assert (alone != cast(capi, cuda, one, w, rc_.GEOM, rc_.R)).any(axis=1).all()


def test_listed_mode(capi, cuda):
    """7. A list naming one car per race writes those rows with the all-cars call's bits (the unlisted
    race-mates' poses are read from x) and touches no other row; count 0 changes nothing."""
    x = workload.make_race_grid(3, 3, 34)
    w = wc_.track_world()
    every = race_cast(capi, cuda, x, w, 3, rc_.GEOM, rc_.R)
    listed = [7, 0, 5]
    got = race_cast(capi, cuda, x, w, 3, rc_.GEOM, rc_.R, listed=listed + [1] * 6, count=3)
    same_bits(got[listed], every[listed], "listed rows")
    rest = np.setdiff1d(np.arange(9), listed)
    assert (got[rest] == SENTINEL).all()
    none = race_cast(capi, cuda, x, w, 3, rc_.GEOM, rc_.R, listed=listed + [1] * 6, count=0)
    assert (none == SENTINEL).all()


def test_a_non_finite_opponent(capi, cuda):
    """8. One race-mate's pose is NaN and another's heading is infinite: their own rows are what the plain
    cast gives for such a pose, and every other car's row equals the cast of the race without them."""
    x = workload.make_race_grid(1, 5, 35, spacing=1.0)
    w = wc_.track_world()
    bad = x.copy()
    bad[1, 0] = np.nan
    bad[3, 2] = np.inf
    got = race_cast(capi, cuda, bad, w, 5, rc_.GEOM, rc_.R)
    plain = cast(capi, cuda, bad, w, rc_.GEOM, rc_.R)
    same_bits(got[[1, 3]], plain[[1, 3]], "the non-finite cars' own rows")
    keep = [0, 2, 4]
    same_bits(got[keep], race_cast(capi, cuda, x[keep], w, 3, rc_.GEOM, rc_.R), "the others, without them")
    assert (got[keep] != plain[keep]).any(axis=1).all(), "the finite cars still see each other"
