"""The rollout with straight walls on MI355X (f110qp_rollout_walls[_dev]) at T = 6, B = 8, G = 2, N = 5: the call
equals its own pieces called row by row (f110qp_cast_scans_walls_dev and f110qp_clearance_walls_dev at every row
of x_traj, bit for bit), equals f110qp_rollout_body_dev in every array at S = 0, a wall a few ticks ahead of one
car parks it at the first row the oracle has at or under 0 while its race-mate drives on, ranges_traj given and
NULL agree, and the host call equals the device call."""
import numpy as np
import pytest
import rollout_cases as roc_
import walls_cases as wl_
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_body import rollout_body_dev
from test_gpu_rollout_contact import check_parked, check_races_before_a_crash, first_row
from test_gpu_rollout_replan import P
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_world import GEOM, R
from test_gpu_walls import bits, clearance, wall_cast
from world_loop import rollout_dev

from f110qp import workload

pytestmark = pytest.mark.gpu

T, B, G, N = 6, 8, 2, 5
# metres between the front of car 0 and the wall across its path. With the wall in its scan the car's planner finds
# no way and the car creeps at fail_u = 0.5 m/s, 5 mm a tick: contact at row 3 (at 4.5 m/s it would be row 1)
AHEAD = 0.012


def scene(ahead=AHEAD):
    """Four races of two on the track, 1.2 m apart along it; 20 circles far from the cars; the track's 250 wall
    segments and one more wall across the path of car 0, `ahead` metres in front of its body."""
    x0 = workload.make_race_grid(B // G, G, seed=91)
    sg, ci = wl_.track()
    c, s = np.cos(x0[0, 2]), np.sin(x0[0, 2])
    front = wl_.CENTER_OFFSET + wl_.HL + ahead
    mid = x0[0, :2] + front * np.array([c, s])
    across = 0.3 * np.array([-s, c])
    wall = np.concatenate([mid - across, mid + across])[None]
    return x0, np.tile([roc_.V_LIN, 0.0], (B, 1)), ci[:20], np.ascontiguousarray(np.concatenate([sg, wall])), workload.track_waypoints()


def rollout_walls_dev(capi, cuda, s, case, stop, ticks=T, null=(), segments=True):
    """One Solver.rollout_walls_dev call on fresh device arrays -> every array as numpy."""
    return rollout_dev(capi, cuda, s, "walls", case, ticks, G, stop, null=null, segments=segments)


_RUNS = {}


def runs(capi, cuda):
    """The stop = 0 and stop = 1 runs of the scene, computed once."""
    if not _RUNS:
        s = solver(capi, N, x_ref_points=P)
        _RUNS[0] = rollout_walls_dev(capi, cuda, s, scene(), 0)
        _RUNS[1] = rollout_walls_dev(capi, cuda, s, scene(), 1)
        s.close()
    return _RUNS


def test_the_call_equals_its_pieces(capi, cuda):
    a = runs(capi, cuda)[0]
    _, _, circles, sg, _ = scene()
    clear, near = clearance(capi, cuda, a["x_traj"], circles, sg, G)
    assert (bits(a["clear_traj"]) == bits(clear)).all() and (a["nearest_traj"] == near).all()
    assert (a["crash_tick"] == first_row(a["clear_traj"], 0.0)).all()
    for t in range(T):
        same_bits(a["ranges_traj"][t], wall_cast(capi, cuda, a["x_traj"][t], circles, sg, G, GEOM, R), f"scan of tick {t}")
    want, wnear = workload.clearance_walls(a["x_traj"], circles, sg, G)
    c = wl_.WallCase("rollout rows", a["x_traj"], G, circles, sg)
    c.check(a["clear_traj"], a["nearest_traj"])


def test_no_segments_is_the_body_rollout(capi, cuda):
    x0, ul, circles, sg, wp = scene()
    s = solver(capi, N, x_ref_points=P)
    a = rollout_walls_dev(capi, cuda, s, scene(), 1, segments=False)
    b = rollout_body_dev(capi, cuda, s, (x0, ul, circles, wp), 1, ticks=T, group=G)
    s.close()
    assert set(a) == set(b)
    for k in a:
        same_bits(a[k], b[k], k)


def test_a_wall_ahead_parks_the_car(capi, cuda):
    r = runs(capi, cuda)
    a, free = r[1], r[0]
    _, _, circles, sg, _ = scene()
    want = workload.clearance_walls(free["x_traj"], circles, sg, G)[0]
    k = int(first_row(want, 0.0)[0])
    assert 0 < k < T, (k, want[:, 0])
    assert a["crash_tick"][0] == k and free["crash_tick"][0] == k
    assert a["nearest_traj"][k, 0] == len(circles) + G + len(sg) - 1, "the wall across the path"
    assert a["crash_tick"][1] == -1, "the race-mate behind does not crash"
    check_parked(capi, a, "walls stop 1")
    check_races_before_a_crash(a, free, G, "walls stop 1")
    for name in ("x_traj", "u_lin_traj"):
        same_bits(a[name][:k + 1, 1], free[name][:k + 1, 1], f"the race-mate's {name} up to row {k}")


def test_ranges_traj_given_and_null_agree(capi, cuda):
    s = solver(capi, N, x_ref_points=P)
    a = rollout_walls_dev(capi, cuda, s, scene(), 1, null=("ranges_traj",))
    s.close()
    want = runs(capi, cuda)[1]
    for k in a:
        same_bits(a[k], want[k], k)


@pytest.mark.parametrize("stop", [0, 1])
def test_host_call_equals_the_device_call(capi, cuda, stop):
    x0, ul, circles, sg, wp = scene()
    s = solver(capi, N, x_ref_points=P)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    h = s.rollout_walls(x0, ul, circles, sg, capi.default_race_config(group_size=G),
                        capi.default_contact_config(stop_on_contact=stop), capi.default_body_config(),
                        scan_config(capi, R, GEOM), rp, capi.traj_table(rp.plan), wp, T, scans=True)
    s.close()
    a = runs(capi, cuda)[stop]
    for k in ("x_traj", "u_lin_traj", "u_applied", "clear_traj", "nearest_traj", "crash_tick", "ranges_traj"):
        same_bits(np.asarray(h[k]).reshape(a[k].shape), a[k], k)
