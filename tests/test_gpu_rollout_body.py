"""The rollout with rectangular car bodies on MI355X (f110qp_rollout_body[_dev]): the call equals its parts
(f110qp_clearance_body_dev and the oracle scans at every row of x_traj), equals the contact rollout wherever no
body enters (G = 1), host call equals device call, parking follows the contact rollout's rule, and two cars side
by side 0.5 m apart touch as discs and not as rectangles. Scenes of 8 and 260 cars, T <= 12."""
import body_cases as bc_
import contact_cases as cc_
import numpy as np
import pytest
import rollout_cases as roc_
from test_gpu_body import bits, clearance
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_contact import G, N, T, check_parked, check_races_before_a_crash, first_row, rollout_contact_dev, scene
from test_gpu_rollout_replan import P
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_world import GEOM, R
from world_loop import rollout_dev

from f110qp import workload

pytestmark = pytest.mark.gpu


def rollout_body_dev(capi, cuda, s, case, stop, margin=0.0, ticks=T, nearest=True, group=G, null=()):
    """One Solver.rollout_body_dev call on fresh device arrays -> every array as numpy (rollout_contact_dev's)."""
    return rollout_dev(capi, cuda, s, "body", case, ticks, group, stop, margin, nearest=nearest, null=null)


_RUNS = {}


def runs(capi, cuda):
    """The stop = 0 and stop = 1 runs of contact's scene, computed once."""
    if not _RUNS:
        s = solver(capi, N, x_ref_points=P)
        _RUNS[0] = rollout_body_dev(capi, cuda, s, scene(), 0)
        _RUNS[1] = rollout_body_dev(capi, cuda, s, scene(), 1)
        s.close()
    return _RUNS


def test_the_call_equals_its_parts(capi, cuda):
    a = runs(capi, cuda)[0]
    circles = scene()[2]
    clear, near = clearance(capi, cuda, a["x_traj"], circles, G)
    assert (bits(a["clear_traj"]) == bits(clear)).all() and (a["nearest_traj"] == near).all()
    assert (a["crash_tick"] == first_row(a["clear_traj"], 0.0)).all()
    c = bc_.ScanCase("rollout rows", a["x_traj"][0], G, circles)
    for t in range(T):
        c.check(a["ranges_traj"][t], a["x_traj"][t], f"tick {t}")


def test_group_of_one_equals_the_contact_rollout(capi, cuda):
    s = solver(capi, N, x_ref_points=P)
    a = rollout_body_dev(capi, cuda, s, scene(), 0, group=1)
    b = rollout_contact_dev(capi, cuda, s, scene(), 0, group=1)
    s.close()
    for k in a:
        if k not in ("clear_traj", "nearest_traj", "crash_tick"):
            same_bits(a[k], b[k], k)
    clear, near = clearance(capi, cuda, a["x_traj"], scene()[2], 1)
    assert (bits(a["clear_traj"]) == bits(clear)).all() and (a["nearest_traj"] == near).all()


@pytest.mark.parametrize("stop", [0, 1])
def test_host_call_equals_the_device_call(capi, cuda, stop):
    x0, ul, circles, wp = scene()
    s = solver(capi, N, x_ref_points=P)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    h = s.rollout_body(x0, ul, circles, capi.default_race_config(group_size=G),
                       capi.default_contact_config(stop_on_contact=stop), capi.default_body_config(),
                       scan_config(capi, R, GEOM), rp, capi.traj_table(rp.plan), wp, T, scans=True)
    s.close()
    a = runs(capi, cuda)[stop]
    for k in ("x_traj", "u_lin_traj", "u_applied", "clear_traj", "nearest_traj", "crash_tick", "ranges_traj"):
        same_bits(np.asarray(h[k]).reshape(a[k].shape), a[k], k)


def test_parking_follows_the_contact_rule(capi, cuda):
    r = runs(capi, cuda)
    a, free = r[1], r[0]
    assert a["crash_tick"][0] > 0, a["crash_tick"]
    check_parked(capi, a, "body stop 1")
    check_races_before_a_crash(a, free, G, "body stop 1")


def test_wide_scene_parks(capi, cuda):
    """260 cars in races of four, a world per car (contact_cases.wide_crash_scene), nine ticks."""
    x0, circles = cc_.wide_crash_scene()
    case = (x0, np.tile([roc_.V_LIN, 0.0], (cc_.WIDE_B, 1)), circles, workload.track_waypoints())
    s = solver(capi, N, x_ref_points=P)
    free = rollout_body_dev(capi, cuda, s, case, 0, ticks=cc_.WIDE_T, group=cc_.WIDE_G)
    a = rollout_body_dev(capi, cuda, s, case, 1, ticks=cc_.WIDE_T, group=cc_.WIDE_G)
    s.close()
    clear, near = clearance(capi, cuda, a["x_traj"], circles, cc_.WIDE_G)
    assert (bits(a["clear_traj"]) == bits(clear)).all() and (a["nearest_traj"] == near).all()
    assert (a["crash_tick"] >= 0).any() and (a["crash_tick"] == -1).any()
    check_parked(capi, a, "wide body stop 1")
    check_races_before_a_crash(a, free, cc_.WIDE_G, "wide body stop 1")


def test_side_by_side_cars_touch_as_discs_only(capi, cuda):
    """Two cars 0.5 m apart across the path: in contact at row 0 of the contact rollout, clear in this call."""
    x0 = workload.make_race_grid(1, 2, 5, spacing=0.0, lateral=0.0)
    nrm = np.array([-np.sin(x0[0, 2]), np.cos(x0[0, 2])])
    x0[0, :2] += 0.25 * nrm
    x0[1, :2] -= 0.25 * nrm
    x0[1, 2] = x0[0, 2]
    case = (x0, np.tile([roc_.V_LIN, 0.0], (2, 1)), np.array([[60.0, 60.0, 0.1]]), workload.track_waypoints())
    s = solver(capi, N, x_ref_points=P)
    disc = rollout_contact_dev(capi, cuda, s, case, 0, ticks=2, group=2)
    rect = rollout_body_dev(capi, cuda, s, case, 0, ticks=2, group=2)
    s.close()
    assert (disc["crash_tick"] == 0).all() and (disc["clear_traj"][0] < 0).all()
    assert (rect["crash_tick"] == -1).all() and (rect["clear_traj"] > 0.15).all(), rect["clear_traj"]


def test_all_optional_outputs_null(capi, cuda):
    null = ("nearest_traj", "iters", "cost", "u_plan", "x_plan", "hs_traj", "kind", "plan_status", "best_traj",
            "best_global", "pose_traj", "ranges_traj")
    s = solver(capi, N, x_ref_points=P)
    a = rollout_body_dev(capi, cuda, s, scene(), 1, null=null)
    s.close()
    want = runs(capi, cuda)[1]
    for k in ("x_traj", "u_lin_traj", "u_applied", "status", "clear_traj", "crash_tick"):
        same_bits(a[k], want[k], k)
