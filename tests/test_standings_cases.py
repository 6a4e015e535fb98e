"""The standings oracle on the CPU (workload.path_lengths, progress, standings): the properties the model of
include/f110qp.h "race standings" promises, on the oracle alone. test_gpu_standings.py holds the device to the
oracle bit for bit on the cases of standings_cases.py."""
import numpy as np
import pytest
import standings_cases as sc_

from f110qp import workload

EPS = 2.0 ** -52


def test_path_lengths_are_the_cumulative_sum_of_rounded_roots():
    for wp in (workload.track_waypoints(), sc_.ellipse(2), sc_.rectangle(), sc_.duplicate_case().wp):
        cum = workload.path_lengths(wp)
        W = len(wp)
        want = [0.0]
        for j in range(W):  # one segment at a time, in order
            ex, ey = wp[(j + 1) % W, 0] - wp[j, 0], wp[(j + 1) % W, 1] - wp[j, 1]
            want.append(want[-1] + np.sqrt(ex * ex + ey * ey))
        assert sc_.same(cum, np.array(want)) and cum.shape == (W + 1,)
        e = np.roll(wp, -1, 0) - wp
        assert sc_.same(cum[1:], np.cumsum(np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])))
    assert workload.path_lengths(sc_.rectangle(100, 60))[-1] == 320.0


@pytest.mark.parametrize("c", sc_.all_cases(), ids=lambda c: c.name)
def test_ranks_are_a_permutation_and_outputs_consistent(c):
    o = c.oracle()
    fin = np.isfinite(c.x[..., :2]).all(axis=2)
    assert ((o["seg"] >= 0) == fin).all() or not c.ranked  # a finite pose on a finite path always has a segment
    assert (o["seg"][~fin] == -1).all() and np.isnan(o["s"][~fin]).all() and np.isnan(o["lateral"][~fin]).all()
    if not c.ranked:
        assert not np.isin(o["seg"], (6, 7)).any() and (o["seg"][fin] >= 0).all()
        return
    L = c.cum[-1]
    ok = o["seg"] >= 0
    assert (o["s"][ok] >= 0).all() and (o["s"][ok] <= L).all()
    r = o["rank"].reshape(c.rows, c.B // c.G, c.G)
    assert (np.sort(r, axis=2) == np.arange(c.G)).all()
    nan = np.isnan(o["dist"])
    assert (o["lap"][nan] == sc_.INT_MIN).all() and (o["lap"][0][~nan[0]] == 0).all()
    assert (np.maximum.accumulate(nan, axis=0) == nan).all(), "a NaN dist stays NaN"


def test_bad_waypoint_leaves_the_other_segments_alone():
    for c in sc_.bad_waypoint_cases():
        clean = sc_.ellipse(40)
        seg0, _, lat0 = workload.progress(c.x, clean)
        o = c.oracle()
        keep = ~np.isin(seg0, (6, 7))
        assert keep.any() and (~keep).any()
        assert (o["seg"][keep] == seg0[keep]).all() and sc_.same(o["lateral"][keep], lat0[keep])


def test_exact_ties_take_the_lowest_index():
    plain, rolled = sc_.tie_case()
    seg = plain.oracle()["seg"][0]
    n = (len(seg) + 1) // 2
    k = np.arange(35, 65, 3)
    assert (seg[:n] == k).all(), "bottom segment k over the top segment above it"
    assert (seg[n:] == k[1:] - 1).all(), "on a vertex column: the segment that ends there"
    assert (plain.oracle()["lateral"][0] == 30.0).all()
    rs = rolled.oracle()["seg"][0]  # the list rotated by 130: old segment j is (j + 130) % 320
    top = 160 + 99 - k
    assert (rs[:n] == np.minimum((k + 130) % 320, (top + 130) % 320)).all()
    for c in sc_.vertex_case():
        o = c.oracle()
        assert (np.abs(o["lateral"]) <= 1e-15 * np.abs(c.x[..., :2]).max()).all()
    v = sc_.vertex_case()[1].oracle()
    assert (v["lateral"] == 0).all() and v["seg"][0, 0] == 0 and v["s"][0, 0] == 0.0, "vertex 0 is s = 0, never L"


@pytest.mark.parametrize("races,G,seed", sc_.GRIDS)
def test_race_grids_rank_in_grid_order(races, G, seed):
    """make_race_grid puts car i of a race 1.2 m behind car i - 1 along the path, 0.4 m to either side, at a seeded
    place: several races straddle s = 0, where only the leader-relative wrap of row 0 keeps the order."""
    c = sc_.grid_case(races, G, seed)
    o = c.oracle()
    L = c.cum[-1]
    assert (o["rank"][0] == np.arange(c.B) % G).all()
    d = o["dist"][0].reshape(races, G)
    assert (np.abs((d[:, :-1] - d[:, 1:]) - 1.2) <= 0.011).all()
    assert (np.abs(np.abs(o["lateral"][0]) - 0.4) <= 2e-4).all()
    assert (o["lateral"][0].reshape(races, G)[:, 0::2] > 0).all() and (o["lateral"][0].reshape(races, G)[:, 1::2] < 0).all()
    s = o["s"][0].reshape(races, G)
    if (races, G) != (2, 8):
        assert ((s.max(axis=1) - s.min(axis=1)) > L / 2).any(), "a race of this grid straddles s = 0"
        naive = (s[:, None, :] > s[:, :, None]).sum(axis=2)
        assert (naive != np.arange(G)).any(), "ranking by s alone gets such a race wrong"


def _round_the_ellipse(turns, steps, start=0.3):
    th = start + np.linspace(0.0, 2 * np.pi * turns, steps)
    return np.stack([12.0 * np.cos(th), 6.0 * np.sin(th), np.zeros_like(th)], 1)[:, None, :]


def test_laps_forwards_and_backwards():
    wp = workload.track_waypoints()
    L = workload.path_lengths(wp)[-1]
    for turns, laps in ((2.5, [0, 1, 2]), (-2.5, [-1, -2, -3])):
        x = _round_the_ellipse(turns, 400)
        _, s, _ = workload.progress(x, wp)
        dist, lap, rank = workload.standings(s, L, 1)
        assert abs((dist[-1, 0] - dist[0, 0]) - turns * L) < 0.05
        step = np.diff(lap[:, 0])
        assert (step == np.sign(turns)).sum() == len(laps) - (turns > 0) and (step * np.sign(turns) >= 0).all()
        assert sorted(set(lap[1:, 0]), key=abs) == laps and lap[0, 0] == 0 and (rank == 0).all()
        if turns < 0:
            assert lap[1, 0] == -1


def test_crossing_s0_back_and_forth_keeps_dist_continuous():
    wp = workload.track_waypoints()
    L = workload.path_lengths(wp)[-1]
    y = 0.3 * np.array([1, -1, 1, -1, -1, 1, 1, -1, 1.0])  # either side of waypoint 0 = (12, 0)
    x = np.stack([np.full_like(y, 12.0), y, np.zeros_like(y)], 1)[:, None, :]
    _, s, _ = workload.progress(x, wp)
    assert (np.abs(np.diff(s[:, 0])) > L / 2).sum() >= 5, "s itself jumps by the path's length"
    dist, lap, _ = workload.standings(s, L, 1)
    assert (np.abs(np.diff(dist[:, 0])) < 0.7).all()
    assert set(lap[:, 0]) == {0, -1}


def test_dist_differences_do_not_depend_on_where_the_list_starts():
    """Rotating the waypoint list moves s = 0: every dist of a race moves by one constant. Tolerance: every cum
    entry carries at most W roundings of half an ulp of L, an s three more, a dist two s per row: the differences
    inside a race agree within L 2^-52 rows (W + 8)."""
    c = sc_.grid_case(64, 4, 91)
    wp = c.wp
    rows = 6
    x = np.stack([c.x[0]] * rows)
    x[1:, :, :2] += np.random.default_rng(3).normal(0, 0.3, (rows - 1, c.B, 2)).cumsum(axis=0)
    L = c.cum[-1]
    base = workload.standings(workload.progress(x, wp)[1], L, 4)
    tol = L * EPS * rows * (c.W + 8)
    rel = lambda d: (d.reshape(rows, -1, 4) - d.reshape(rows, -1, 4)[:1, :, :1])  # noqa: E731
    for k in (1, 137, 499):
        w2 = np.roll(wp, k, 0)
        got = workload.standings(workload.progress(x, w2)[1], workload.path_lengths(w2)[-1], 4)
        assert np.abs(rel(got[0]) - rel(base[0])).max() <= tol
        assert (got[2] == base[2]).all()


def test_synthetic_s_rules():
    s, L, G = sc_.synthetic_s()
    dist, lap, rank = workload.standings(s, L, G)
    assert (np.sort(rank.reshape(len(s), -1, G), axis=2) == np.arange(G)).all()
    assert np.isnan(dist[:, G:2 * G]).all(), "a NaN first car at row 0 takes its race with it"
    assert np.isnan(dist[3:, 2]).all() and np.isfinite(dist[:3, 2]).all()
    assert np.isnan(dist[4:, 2 * G + 3]).all(), "a NaN that comes back as a number stays NaN"
    assert (rank[4:, 2 * G + 3] == G - 1).all() and (rank[2:, 3 * G] == G - 2).all() and (rank[2:, 3 * G + 1] == G - 1).all()
    assert (rank[:, 0] + 1 == rank[:, 1])[:3].all(), "equal dist: the lower index is ahead"
    assert (lap[np.isnan(dist)] == sc_.INT_MIN).all()
    assert (np.abs(np.diff(dist[:, 0])) <= 12.0 + 1e-9).all()
