"""The edge suite of the ray-cast kernel (test_gpu_world_scan_edges.py) from the oracle alone: every case is
what it claims to be. The hit counts it names, the |p| envelope its tolerance was derived for, the strict
check passing on the oracle's own output, and the number of grazing beams per case (printed; the families
built to graze must have some)."""
import numpy as np
import pytest
import world_cases as wc_


def judge(c):
    """One case against its own claims -> grazing beams."""
    want, hits, pmax = wc_.case_facts(c)
    assert pmax <= c.pmax, (c.name, "a kept circle outside the envelope of the tolerance", pmax, c.pmax)
    assert c.tol == wc_.ABS_TOL * max(1.0, (c.pmax / 20.0) ** 2), c.name
    assert (want < np.float32(c.max_range)).sum() >= c.seen, (c.name, int((want < c.max_range).sum()))
    if c.hits is not None:
        assert hits in (c.hits if isinstance(c.hits, tuple) else (c.hits,)), (c.name, hits)
        # nothing stands in front of the target: the scan without it differs on exactly those beams
        without = wc_.oracle_scan(c.x, np.delete(c.ci, c.target, axis=0), c.geom, c.R, **c.kw)
        assert (without != want).sum() == hits, c.name
    n, worst = wc_.check_scan_strict(want, c.x, c.ci, c.geom, c.R, c.name, tol=c.tol, **c.kw)
    assert worst == 0.0, c.name
    print(f"{c.name:50s} grazing {n:4d} of {want.size}")
    return n


@pytest.mark.parametrize("name", list(wc_.EDGE_GEOMETRIES))
def test_geometry_cases(name):
    """Every geometry of the table with R at most 1,300 and every case seeing something."""
    cases = wc_.geometry_cases(name)
    assert len(cases) == 6 * len(wc_.EDGE_GEOMETRIES[name])
    for c in cases:
        assert c.R <= 1300 and c.ci.shape[0] <= wc_.TILE + 5 and c.geom[1].dtype == np.float32
        judge(c)
    if name == "turn_edge":  # the wall's arc with its margin, either side of a full turn
        w = np.arcsin(1 / (1 + 2e-5)) + 1e-9
        assert [2 * w + 4 * float(c.geom[1]) < 2 * np.pi for c in cases[::6]] == [True, False]
    if name == "inc_min":
        assert [float(c.geom[1]) >= 1e-9 for c in cases[::6]] == [False, False, True]


@pytest.mark.parametrize("family", wc_.THRESHOLD_FAMILIES)
def test_threshold_cases(family):
    """Every threshold family; on_circle (both radii) and near_face have grazing beams in every geometry, so
    the strict branch of check_scan_strict runs on them."""
    graze = {}
    for c in wc_.threshold_cases(family):
        assert c.ci.shape[0] <= 40
        graze[c.name] = judge(c)
    if family == "on_circle":
        for kind, _ in wc_.THRESHOLD_GEOMETRIES:
            for ra in ("0.5", "50"):
                for e in ("0", "5e-07", "1e-06", "2e-06", "0.001"):
                    assert graze[f"on_circle {kind} ra {ra} e {e}"] > 0, (kind, ra, e)
    if family == "near_face":
        assert all(n > 0 for n in graze.values()), graze
    if family == "sub_beam":  # the circles narrower than a beam are seen by one beam or by none
        assert len(graze) == 20


def test_heading_and_per_car_cases():
    c = wc_.heading_case()
    # inside the bound: the ulp of |ori| + |angle_min| + pi is below a millionth of a beam
    assert np.spacing(np.abs(c.x[:, 2]).max() + np.pi + np.pi) < 1e-6 * float(c.geom[1])
    judge(c)
    c = wc_.per_car_case()
    assert c.ci.shape == (800, 3, 3) and len(c.x) == 800
    judge(c)
    assert (wc_.case_facts(c)[0] < np.float32(c.max_range)).any(axis=1).sum() > 200, "most cars see a circle"


def test_strict_check_rejects_what_it_should():
    """check_scan_strict on a tampered oracle scan: a non-grazing beam one float32 off passes, 1 mm off
    fails; a grazing beam may be the firm value or the flippable circle's, and nothing in between."""
    c = [k for k in wc_.threshold_cases("on_circle") if k.name == "on_circle 2pi ra 0.5 e 0.001"][0]
    want, _, _ = wc_.case_facts(c)
    args = (c.x, c.ci, c.geom, c.R, c.name)
    g = wc_.grazing(c.x, c.ci, c.geom, c.R, c.lidar_offset, c.max_range)
    assert g.sum() >= 1
    firm = np.flatnonzero(~g[0] & (want[0] < c.max_range))[0]
    ok = want.copy()
    ok[0, firm] = np.nextafter(ok[0, firm], np.float32(0))
    wc_.check_scan_strict(ok, *args, tol=c.tol, **c.kw)
    for delta in (1e-3, -1e-3):
        bad = want.copy()
        bad[0, firm] += np.float32(delta)
        with pytest.raises(AssertionError):
            wc_.check_scan_strict(bad, *args, tol=c.tol, **c.kw)
    i = c.R // 2 + 20  # the tangent beam: what is behind the circle or the tangent point, t = sqrt(D^2 - r^2)
    assert g[0, i]
    t = np.sqrt((0.5 * 1.001) ** 2 - 0.25)
    for v, good in ((want[0, i], True), (np.float32(t), True), (np.float32(t - 3e-5), True),
                    (np.float32(t - 1e-3), False), (np.float32(t + 1e-3), False)):
        alt = want.copy()
        alt[0, i] = v
        if good:
            wc_.check_scan_strict(alt, *args, tol=c.tol, **c.kw)
        else:
            with pytest.raises(AssertionError):
                wc_.check_scan_strict(alt, *args, tol=c.tol, **c.kw)
