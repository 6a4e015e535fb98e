"""The rollout with a refreshed MPC scan on MI355X (f110qp_rollout_refresh[_dev]) at T = 6, B = 8, G = 2, N = 5 on
the scene of test_gpu_rollout_walls.py: every = 0 and every > T - 1 are the walls call bit for bit; at a refresh
tick the rows are those of that tick's scan at that tick's pose and between two refreshes those of the held record;
gap rows INACTIVE computes the rows and ignores them; ranges_traj given and NULL agree; the host call equals the
device call; a parked car's record is still refreshed; and a circle that closes a gap while the car approaches it
reaches the rows at every = 1 and does not at every = 0. Everything between two device routes is bit equality."""
import numpy as np
import pytest
import refresh_cases as rf_
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_contact import check_parked, check_races_before_a_crash
from test_gpu_rollout_replan import P
from test_gpu_rollout_scan import scan_config, split_rows
from test_gpu_rollout_walls import B, G, N, T, rollout_walls_dev, scene
from test_gpu_rollout_world import GEOM, R
from test_gpu_walls import wall_cast
from world_loop import rollout_dev

pytestmark = pytest.mark.gpu


def rollout_refresh_dev(capi, cuda, s, case, stop, every, ticks=T, null=()):
    """One Solver.rollout_refresh_dev call on fresh device arrays -> every array as numpy."""
    return rollout_dev(capi, cuda, s, "refresh", case, ticks, G, stop, every=every, null=null)


_RUNS = {}


def run(capi, cuda, gap, stop, every, null=(), walls=False):
    """A run of the scene, computed once: the refresh call at `every`, or (walls) the walls call."""
    key = (gap, stop, every, null, walls)
    if key not in _RUNS:
        s = solver(capi, N, gap=gap, x_ref_points=P)
        _RUNS[key] = rollout_walls_dev(capi, cuda, s, scene(), stop, null=null) if walls else \
            rollout_refresh_dev(capi, cuda, s, scene(), stop, every, null=null)
        s.close()
    return _RUNS[key]


def same_run(a, b, what, skip=()):
    assert set(a) == set(b), what
    for k in a:
        if k not in skip:
            same_bits(a[k], b[k], f"{what}: {k}")


def check_rows(capi, cuda, a, every, what, case=None):
    """hs_traj against the rule: row t holds the rows of the record of scan row r(t) at x_traj row t, r(t) the last
    refresh tick at or before t (0 without one); ranges_traj row t is f110qp_cast_scans_walls_dev at x_traj row t."""
    _, _, circles, sg, _ = case or scene()
    for t in range(T):
        same_bits(a["ranges_traj"][t], wall_cast(capi, cuda, a["x_traj"][t], circles, sg, G, GEOM, R),
                  f"{what}: scan of tick {t}")
        src = t - t % every if every else 0
        want, _ = split_rows(capi, cuda, a["x_traj"][t], np.ascontiguousarray(a["ranges_traj"][src]), GEOM)
        same_bits(a["hs_traj"][t], want, f"{what}: rows of tick {t} from the scan of tick {src}")


@pytest.mark.parametrize("stop", [0, 1])
@pytest.mark.parametrize("gap", [False, True])
def test_every_zero_is_the_walls_call(capi, cuda, gap, stop):
    same_run(run(capi, cuda, gap, stop, 0), run(capi, cuda, gap, stop, 0, walls=True), f"gap {gap} stop {stop}")


def test_a_period_beyond_the_call_is_every_zero(capi, cuda):
    same_run(run(capi, cuda, True, 0, T + 1), run(capi, cuda, True, 0, 0), "every 7")


@pytest.mark.parametrize("every", [1, 2])
def test_rows_follow_the_refreshed_scan(capi, cuda, every):
    a = run(capi, cuda, True, 0, every)
    check_rows(capi, cuda, a, every, f"every {every}")
    if every == 2:  # rows 1, 3 and 5 are those of the held record: the scan of the tick before
        assert [t - t % every for t in range(T)] == [0, 0, 2, 2, 4, 4]


def test_every_zero_rows_are_the_first_scans(capi, cuda):
    check_rows(capi, cuda, run(capi, cuda, True, 0, 0), 0, "every 0")


def test_gap_inactive_computes_the_rows_and_ignores_them(capi, cuda):
    a, w = run(capi, cuda, False, 0, 1), run(capi, cuda, False, 0, 0, walls=True)
    same_run(a, w, "INACTIVE, every 1", skip=("hs_traj",))
    check_rows(capi, cuda, a, 1, "INACTIVE, every 1")


def test_gap_inactive_without_rows_is_the_walls_call(capi, cuda):
    null = ("hs_traj",)
    same_run(run(capi, cuda, False, 0, 1, null=null), run(capi, cuda, False, 0, 0, null=null, walls=True),
             "INACTIVE, hs_traj NULL, every 1")


@pytest.mark.parametrize("every", [1, 2])
def test_ranges_traj_given_and_null_agree(capi, cuda, every):
    a, want = run(capi, cuda, True, 1, every, null=("ranges_traj",)), run(capi, cuda, True, 1, every)
    for k in a:
        same_bits(a[k], want[k], k)


@pytest.mark.parametrize("stop", [0, 1])
def test_host_call_equals_the_device_call(capi, cuda, stop):
    x0, ul, circles, sg, wp = scene()
    s = solver(capi, N, gap=True, x_ref_points=P)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    h = s.rollout_refresh(x0, ul, circles, sg, capi.default_race_config(group_size=G),
                          capi.default_contact_config(stop_on_contact=stop), capi.default_body_config(),
                          capi.default_refresh_config(every=1), scan_config(capi, R, GEOM), rp,
                          capi.traj_table(rp.plan), wp, T, scans=True)
    s.close()
    a = run(capi, cuda, True, stop, 1)
    for k in ("x_traj", "u_lin_traj", "u_applied", "status", "hs_traj", "kind", "clear_traj", "nearest_traj", "crash_tick",
              "ranges_traj"):
        same_bits(np.asarray(h[k]).reshape(a[k].shape), a[k], k)


def test_a_parked_car_is_still_refreshed(capi, cuda):
    a, free = run(capi, cuda, False, 1, 1), run(capi, cuda, False, 0, 1)
    k = int(a["crash_tick"][0])
    assert 0 < k < T and a["crash_tick"][1] == -1, a["crash_tick"]
    check_parked(capi, a, "refresh stop 1")
    check_races_before_a_crash(a, free, G, "refresh stop 1")
    check_rows(capi, cuda, a, 1, "refresh stop 1")


# ---- the point of the feature -------------------------------------------------------------------------------------

def closing_scene():
    """The scene without the wall across car 0's path and with the circle of refresh_cases ahead of car 0: its beams
    read above ftg_thresh at row 0 and below it by row T - 1."""
    x0, ul, circles, sg, wp = scene()
    return x0, ul, np.ascontiguousarray(np.concatenate([circles, rf_.circle_ahead(x0[0])[None]])), \
        np.ascontiguousarray(sg[:-1]), wp


def test_the_rows_follow_a_gap_that_closes(capi, cuda):
    case = closing_scene()
    _, _, circles, sg, _ = case
    s = solver(capi, N, x_ref_points=P)
    held = rollout_refresh_dev(capi, cuda, s, case, 0, 0)
    fresh = rollout_refresh_dev(capi, cuda, s, case, 0, 1)
    s.close()
    # the fixture, from the numpy ray casts: car 0's gap record at row 0 and at row T - 1 differ
    first = rf_.oracle_record(held["x_traj"][0], circles, sg, G, GEOM)
    last = rf_.oracle_record(held["x_traj"][T - 1], circles, sg, G, GEOM)
    print(f"car 0 closes {np.hypot(*(held['x_traj'][T - 1, 0, :2] - held['x_traj'][0, 0, :2])):.4f} m; record {first} "
          f"at row 0, {last} at row {T - 1}")
    assert first != last, "the fixture: the circle closes the gap of row 0 by row T - 1"
    same_bits(fresh["x_traj"], held["x_traj"], "gap rows INACTIVE: the same drive")
    x = held["x_traj"][T - 1]
    of_first, rec0 = split_rows(capi, cuda, x, np.ascontiguousarray(held["ranges_traj"][0]), GEOM)
    of_last, rec1 = split_rows(capi, cuda, x, np.ascontiguousarray(fresh["ranges_traj"][T - 1]), GEOM)
    assert (rec0["lo"][0], rec0["hi"][0]) != (rec1["lo"][0], rec1["hi"][0]), "the device's two records differ too"
    same_bits(held["hs_traj"][T - 1, 0], of_first[0], "every 0: the rows of the row-0 record")
    same_bits(fresh["hs_traj"][T - 1, 0], of_last[0], "every 1: the rows of the row-(T-1) record")
    assert (fresh["hs_traj"][T - 1, 0] != held["hs_traj"][T - 1, 0]).any(), "the two differ"
    check_rows(capi, cuda, fresh, 1, "closing gap, every 1", case)
