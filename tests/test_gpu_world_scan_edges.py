"""The ray-cast kernel on MI355X at the thresholds of its own cull (the cases of world_cases.py, each shown to
be what it claims by test_world_cases.py): scans of more than a turn, coarse and minute increments, circles
narrower than a beam, of zero and negative radius, the LiDAR on a circle's face and at its centre, centres
on the atan2 seam and on the end beams, the near face at max_range for three max_range, three LiDAR offsets,
headings of 1e6 rad, one world per car past the grid. Every beam of every case is judged by
world_cases.check_scan_strict: no grazing beam is skipped. Each test prints its grazing beams and its worst
error in units of the bound."""
import numpy as np
import pytest
import world_cases as wc_
from test_gpu_rollout import same_bits
from test_gpu_world_scan import SENTINEL, cast

pytestmark = pytest.mark.gpu


def run(capi, cuda, c, ci=None):
    return cast(capi, cuda, c.x, c.ci if ci is None else ci, c.geom, c.R, **c.kw)


def judge(capi, cuda, c):
    """One case on the device against the oracle -> (ranges, grazing beams, worst error / bound)."""
    got = run(capi, cuda, c)
    n, worst = wc_.check_scan_strict(got, c.x, c.ci, c.geom, c.R, c.name, tol=c.tol, **c.kw)
    assert (got < np.float32(c.max_range)).sum() >= min(c.seen, 1), c.name
    return got, n, worst


@pytest.mark.parametrize("name", list(wc_.EDGE_GEOMETRIES))
def test_cast_scan_geometries(capi, cuda, name):
    """A row of world_cases.EDGE_GEOMETRIES: 40 and TILE + 1 random circles with a wall, a 1 mm circle on
    beam 0, a circle on the last beam and a negative radius, LiDAR offsets 0, -0.3 and 0.275, 3 poses."""
    graze, worst = 0, 0.0
    for c in wc_.geometry_cases(name):
        _, n, w = judge(capi, cuda, c)
        graze, worst = graze + n, max(worst, w)
    print(f"{name}: {graze} grazing beams, worst error {worst:.3f} of the bound")


@pytest.mark.parametrize("family", wc_.THRESHOLD_FAMILIES)
def test_cast_threshold_circles(capi, cuda, family):
    """A family of world_cases.threshold_cases. Beyond the oracle: the circles permuted give the same bits;
    a circle narrower than a beam is seen by exactly the beams the case names (the scan without it differs
    on that many beams); a circle around or on the LiDAR changes nothing; a negative radius is seen exactly
    as the positive one."""
    graze, worst = 0, 0.0
    for c in wc_.threshold_cases(family):
        got, n, w = judge(capi, cuda, c)
        graze, worst = graze + n, max(worst, w)
        perm = np.random.default_rng(len(c.name)).permutation(len(c.ci))
        same_bits(got, run(capi, cuda, c, c.ci[perm]), f"{c.name}: circles permuted")
        if c.hits is not None:
            changed = int((got != run(capi, cuda, c, np.delete(c.ci, c.target, axis=0))).sum())
            assert changed in (c.hits if isinstance(c.hits, tuple) else (c.hits,)), (c.name, changed)
        if family == "negative":
            flipped = c.ci.copy()
            flipped[:, 2] = np.abs(flipped[:, 2])
            same_bits(got, run(capi, cuda, c, flipped), f"{c.name}: |r| in place of r")
    print(f"{family}: {graze} grazing beams, worst error {worst:.3f} of the bound")


def test_cast_large_headings(capi, cuda):
    """Yaw +-1e3, +-1e6 and +-(2 pi k + 1e-12), k = 0, 1, 100: the interval's low edge loses ulp(|ori|) (1.2e-10
    rad at 1e6), far below a beam of 0.0245 rad. The oracle adds the same doubles."""
    _, n, worst = judge(capi, cuda, wc_.heading_case())
    print(f"headings: {n} grazing beams, worst error {worst:.3f} of the bound")


def test_cast_per_car_worlds_past_the_grid(capi, cuda):
    """800 cars with three circles each of their own (world_rows = B): a workgroup of the 768 takes a second
    car and must read that car's world. Each row against the oracle of its own world; then a scrambled list
    of 400: the listed rows bit for bit, the others untouched."""
    c = wc_.per_car_case()
    B = len(c.x)
    full, n, worst = judge(capi, cuda, c)
    assert (full < np.float32(c.max_range)).any(axis=1).sum() > B // 4, "most cars see one of their circles"
    order = np.random.default_rng(B).permutation(B).astype(np.int32)
    got = cast(capi, cuda, c.x, c.ci, c.geom, c.R, listed=order, count=400)
    listed = np.zeros(B, bool)
    listed[order[:400]] = True
    same_bits(got[listed], full[listed], "listed rows")
    assert (got[~listed] == SENTINEL).all(), "an unlisted row was written"
    print(f"per-car worlds: {n} grazing beams, worst error {worst:.3f} of the bound")
