"""The ray-cast kernel on MI355X (f110qp_cast_scans_dev) against the numpy oracle of world_cases.py:
|gpu - oracle| <= ulp32(oracle) + 4e-9 m on every non-grazing beam, at most 0.1 % of a case's beams grazing
(the derivation is in world_cases.py). Between two device runs: bit equality."""
import numpy as np
import pytest
import world_cases as wc_
from test_gpu_rollout import same_bits
from test_gpu_rollout_scan import scan_config

pytestmark = pytest.mark.gpu

TILE = wc_.TILE
SENTINEL = np.float32(-7.0)


def cast(capi, cuda, x, circles, geom, beams, listed=None, count=None, max_range=wc_.MAX_RANGE,
         lidar_offset=wc_.LIDAR_OFFSET):
    """f110qp_cast_scans_dev on host arrays into rows pre-filled with the sentinel -> ranges [B, R]."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    B = x.shape[0]
    C = circles.shape[-2]
    w = capi.default_world_config(num_circles=C, world_rows=1 if circles.ndim == 2 else circles.shape[0],
                                  max_range=max_range, lidar_offset=lidar_offset)
    out = torch.full((B, beams), float(SENTINEL), dtype=torch.float32, device=cuda)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    capi.cast_scans_dev(scan_config(capi, beams, geom), w, dev(x), dev(circles) if C else None, out,
                        list_=None if listed is None else dev(np.asarray(listed, np.int32)),
                        count=None if listed is None else dev(np.int32([count])))
    torch.cuda.synchronize(cuda)
    return out.cpu().numpy()


SHAPES = [(R, C) for R in (1, 63, 64, 65, 257, 1080) for C in (0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)]


@pytest.mark.parametrize("R,C", SHAPES, ids=[f"R{r}-C{c}" for r, c in SHAPES])
def test_cast_matches_oracle_over_shapes(capi, cuda, R, C):
    """Every beam count with every circle count (none, one, around the LDS tile, several tiles), B = 1, 3
    and 5 cars, one world for all and one per car, the full-turn scan (an interval that wraps between beams
    R - 1 and 0) and the 270 degree scan, the first cars heading +-pi and +-pi/2. A scan config takes
    angle_increment > 0 only: there is no reversed geometry to test. C = 0: max_range everywhere."""
    worst = 0.0
    for B in (1, 3, 5):
        for kind in ("2pi", "270"):
            g = wc_.geometry(R, kind)
            x = wc_.poses_near_origin(B, 100 + R + B, wc_.YAWS[B % 4:] + wc_.YAWS[:B % 4])
            for per_car in (False, True):
                if per_car and C == 0:
                    continue
                ci = wc_.random_world(C, 7 * R + C + B, B if per_car else None)
                got = cast(capi, cuda, x, ci, g, R)
                what = f"R {R} C {C} B {B} {kind} {'per-car' if per_car else 'shared'}"
                _, w = wc_.check_scan(got, x, ci, g, R, what)
                worst = max(worst, w)
                if C == 0:
                    assert (got == np.float32(wc_.MAX_RANGE)).all()
                elif C >= TILE - 1 and R >= 63:
                    assert (got < wc_.MAX_RANGE).any(), what
    print(f"R {R} C {C}: worst error {worst:.3f} of the bound")


@pytest.mark.parametrize("kind", ["2pi", "270"])
def test_cast_hand_made_circles(capi, cuda, kind):
    """The circles built to sit on a rule, 1,080 beams: the near face of a circle dead ahead at max_range
    and its float neighbours (only the lower one is seen, by the beam that meets it head-on), a circle
    behind the LiDAR, the LiDAR inside a circle (it sees through it), NaN / +-inf in each field between
    finite circles (they hit nothing and hide nothing), two rows whose nearer hit alternates beam by beam."""
    R = 1080
    g = wc_.geometry(R, kind)
    for name, (x, ci, about) in wc_.hand_cases(g, R).items():
        got = cast(capi, cuda, x, ci, g, R)
        wc_.check_scan(got, x, ci, g, R, f"{kind}: {about}")
        want = wc_.oracle_scan(x, ci, g, R)
        seen = want < wc_.MAX_RANGE
        if name == "at max_range" or name == "one float above max_range":
            assert not seen.any() and (got == np.float32(wc_.MAX_RANGE)).all(), name
        elif name == "one float below max_range":
            assert seen.sum() == 1 and got[seen][0] == np.nextafter(np.float32(10), np.float32(0)), name
        else:
            assert seen.sum() > 20, name
        if name == "non-finite":
            fin = np.isfinite(ci).all(axis=1)
            same_bits(got, cast(capi, cuda, x, ci[fin], g, R), "the finite circles alone give the same scan")
        if name == "inside":
            same_bits(got, cast(capi, cuda, x, ci[1:], g, R), "the circle around the LiDAR is not seen")
        if name == "alternating":
            hits = want[0, seen[0]]
            assert (np.diff(np.sign(np.diff(hits))) != 0).sum() > 40, "the nearer row changes from beam to beam"


def test_cast_does_not_depend_on_the_circle_order(capi, cuda):
    """The track world (1,040 circles: five tiles) at 5 make_scenes poses, and the same circles permuted, so
    that every circle lands in another tile, thread and lane group: bit-identical scans."""
    R = 1080
    g = wc_.geometry(R)
    x, w = wc_.track_poses(5), wc_.track_world()
    a = cast(capi, cuda, x, w, g, R)
    wc_.check_scan(a, x, w, g, R, "track world")
    for seed in (1, 2):
        b = cast(capi, cuda, x, w[np.random.default_rng(seed).permutation(len(w))], g, R)
        same_bits(a, b, f"permutation {seed}")
    same_bits(a, cast(capi, cuda, x, w[::-1], g, R), "reversed")


def test_cast_track_world_64_cars(capi, cuda):
    """make_scenes(64, seed=3) poses in the walls + 40 obstacles of default_rng(5): 69,120 beams, none of
    them grazing in the oracle (asserted), every one within the bound. Longer scans: 2,500 beams are three
    beam tiles of the kernel."""
    R = 1080
    g = wc_.geometry(R)
    x, w = wc_.track_poses(64), wc_.track_world()
    got = cast(capi, cuda, x, w, g, R)
    skipped, worst = wc_.check_scan(got, x, w, g, R, "track world, 64 cars")
    assert skipped == 0
    print(f"track world: worst error {worst:.3f} of the bound")
    R = 2500
    g = wc_.geometry(R)
    got = cast(capi, cuda, x[:3], w, g, R)
    wc_.check_scan(got, x[:3], w, g, R, "2,500 beams")


@pytest.mark.parametrize("B", [5, 900])
def test_cast_listed_mode(capi, cuda, B):
    """A scrambled list: the listed cars' rows equal the all-cars run bit for bit, every other row keeps the
    sentinel; entries past the count name cars too and are ignored; count 0 touches nothing; a count above
    B is B. 900 cars: more than the 768-workgroup grid, a workgroup takes a second car."""
    R, C = 65, 40
    g = wc_.geometry(R)
    x = wc_.poses_near_origin(B, 5 + B)
    ci = wc_.random_world(C, 6 + B)
    full = cast(capi, cuda, x, ci, g, R)
    wc_.check_scan(full, x, ci, g, R, f"all {B} cars")
    order = np.random.default_rng(B).permutation(B).astype(np.int32)
    for count in (0, 1, B // 2 + 1, B, B + 7):
        got = cast(capi, cuda, x, ci, g, R, listed=order, count=count)
        listed = np.zeros(B, bool)
        listed[order[:min(count, B)]] = True
        same_bits(got[listed], full[listed], f"count {count}: listed rows")
        assert (got[~listed] == SENTINEL).all(), f"count {count}: an unlisted row was written"
