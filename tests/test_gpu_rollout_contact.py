"""The closed loop with contact on MI355X: f110qp_rollout_contact[_dev] (include/f110qp.h, "contact"). With
stop_on_contact = 0 the call is f110qp_rollout_race_dev plus its records, bit for bit; with 1 a crashed car
parks. The scene (contact_cases.crash_scene): two races of four on make_race_grid in the track world, and one
large circle a few plant steps ahead of car 0."""
import contact_cases as cc_
import numpy as np
import pytest
import race_cases as rc_
import replan_cases as rp_
import rollout_cases as roc_
import world_cases as wc_
from test_gpu_contact import bits, clearance
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_race import rollout_race_dev
from test_gpu_rollout_replan import P, dev, full, replan_buffers
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_world import GEOM, ON_MPC, ON_PLAN, OUT, R, compare

from f110qp import workload

pytestmark = pytest.mark.gpu

B, G, N, T = 8, 4, 20, 12


def scene(gap=cc_.BLOCK_GAP):
    x0, circles = cc_.crash_scene(B, G, gap=gap)
    return x0, np.tile([roc_.V_LIN, 0.0], (B, 1)), circles, workload.track_waypoints()


def rollout_contact_dev(capi, cuda, s, case, stop, margin=0.0, ticks=T, nearest=True):
    import torch

    x0, ul, circles, wp = case
    nb = x0.shape[0]
    d = replan_buffers(cuda, x0, ul, nb, s.horizon, ticks)
    d["ranges_traj"] = full(cuda, (ticks, nb, R), torch.float32, -7.0)
    d["clear_traj"] = full(cuda, (ticks + 1, nb), torch.float64, -7.0)
    if nearest:
        d["nearest_traj"] = full(cuda, (ticks + 1, nb), torch.int32, -7)
    d["crash_tick"] = full(cuda, (nb,), torch.int32, -7)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    s.rollout_contact_dev(capi.default_rollout_config(ticks=ticks), scan_config(capi, R, GEOM), rp,
                          capi.default_world_config(num_circles=circles.shape[0]), capi.default_race_config(group_size=G),
                          capi.default_contact_config(stop_on_contact=stop, margin=margin),
                          dev(cuda, capi.traj_table(rp.plan)), dev(cuda, wp), d["x_ref"], d["have_path"], dev(cuda, circles),
                          d["x_traj"], d["u_lin_traj"], d["u_applied"], d["status"], d["clear_traj"], d["crash_tick"],
                          d.get("nearest_traj"), d["iters"], d["cost"], d["u_plan"], d["x_plan"], d["hs_traj"], d["kind"],
                          d["plan_status"], d["best_traj"], d["best_global"], d["pose_traj"], d["ranges_traj"])
    torch.cuda.synchronize(cuda)
    return {k: v.cpu().numpy() for k, v in d.items()}


_RUNS = {}


def runs(capi, cuda):
    """The stop = 0 and stop = 1 runs of the scene and the race rollout, computed once."""
    if not _RUNS:
        s = solver(capi, N, x_ref_points=P)
        _RUNS["race"] = rollout_race_dev(capi, cuda, s, scene(), G, T)
        _RUNS[0] = rollout_contact_dev(capi, cuda, s, scene(), 0)
        _RUNS[1] = rollout_contact_dev(capi, cuda, s, scene(), 1)
        s.close()
    return _RUNS


def first_row(clear, margin):
    hit = clear <= margin
    return np.where(hit.any(axis=0), hit.argmax(axis=0), -1).astype(np.int32)


def test_recording_changes_nothing(capi, cuda):
    """stop = 0: every shared array equals f110qp_rollout_race_dev's; clear_traj and nearest_traj equal
    f110qp_clearance_dev on the returned x_traj; crash_tick is the first row <= margin."""
    r = runs(capi, cuda)
    a, race = r[0], r["race"]
    compare(a, race, "stop 0", True, True)
    same_bits(a["pose_traj"], race["pose_traj"], "pose_traj")
    clear, near = clearance(capi, cuda, a["x_traj"], scene()[2], G)
    assert (bits(a["clear_traj"]) == bits(clear)).all() and (a["nearest_traj"] == near).all()
    assert (a["crash_tick"] == first_row(a["clear_traj"], 0.0)).all()
    assert a["crash_tick"][0] > 0 and (a["crash_tick"][G:] == -1).all(), a["crash_tick"]
    assert a["nearest_traj"][a["crash_tick"][0], 0] == scene()[2].shape[0] - 1, "car 0 meets the block"


def test_margin_moves_the_crash_tick(capi, cuda):
    a = runs(capi, cuda)[0]
    margin = float(np.sort(a["clear_traj"][:, 1])[T // 2])  # a value car 1 passes on its way
    s = solver(capi, N, x_ref_points=P)
    m = rollout_contact_dev(capi, cuda, s, scene(), 0, margin=margin, nearest=False)
    s.close()
    assert (bits(m["clear_traj"]) == bits(a["clear_traj"])).all()
    want = first_row(a["clear_traj"], margin)
    assert (m["crash_tick"] == want).all() and (want != a["crash_tick"]).any(), (want, a["crash_tick"])


def test_crashed_cars_park(capi, cuda):
    r = runs(capi, cuda)
    free, a = r[0], r[1]
    ct = a["crash_tick"]
    assert 0 < ct[0] < T, f"car 0 crashes inside the run: {ct}"
    assert (ct[G:] == -1).all(), f"nobody of the second race crashes: {ct}"
    assert (a["crash_tick"] == first_row(a["clear_traj"], 0.0)).all()
    crashed = np.flatnonzero(ct >= 0)
    for b in crashed:
        k = ct[b]
        for name in ("x_traj", "u_lin_traj", "pose_traj"):  # the rows from the crash on repeat its row
            rows = a[name][k:, b]
            assert (bits(rows) == bits(rows[:1])).all(), f"car {b}: {name} repeats row {k}"
        assert (a["u_applied"][k:, b] == 0).all() and not np.signbit(a["u_applied"][k:, b]).any()
        assert (a["kind"][k:, b] == capi.TICK_CRASHED).all() and (a["kind"][:k, b] != capi.TICK_CRASHED).all()
        assert (a["status"][k:, b] == capi.NO_SOLVE).all()
        assert not np.isin(a["kind"][k:, b], (rp_.PLAN, rp_.PLAN_FAILED)).any(), "no PLAN after the crash"
    assert (a["kind"][:, ct < 0] != capi.TICK_CRASHED).all()
    # the first car to crash: everything before its crash is the free run's
    b0 = crashed[np.argmin(ct[crashed])]
    k0 = ct[b0]
    for name in ("x_traj", "u_lin_traj", "pose_traj", "clear_traj"):
        same_bits(a[name][:k0 + 1], free[name][:k0 + 1], f"{name} up to the first crash")
    for name in ("u_applied", "status", "kind", "hs_traj"):
        same_bits(a[name][:k0], free[name][:k0], f"{name} before the first crash")
    assert (a["x_traj"][T, b0] != free["x_traj"][T, b0]).any(), "the free run drives on"
    # the race without a crash is the stop = 0 run, bit for bit
    other = {k: (v[:, G:] if v.ndim > 1 and v.shape[1] == B else v[G:]) for k, v in a.items()}
    other_free = {k: (v[:, G:] if v.ndim > 1 and v.shape[1] == B else v[G:]) for k, v in free.items()}
    for k in OUT + ("pose_traj", "hs_traj", "ranges_traj", "clear_traj", "nearest_traj", "crash_tick"):
        same_bits(other[k], other_free[k], f"race without a crash: {k}")
    mpc, plan = other["kind"] == rp_.MPC, np.isin(other["kind"], (rp_.PLAN, rp_.PLAN_FAILED))
    for k in ON_MPC:
        same_bits(other[k][mpc], other_free[k][mpc], f"race without a crash: {k}")
    for k in ON_PLAN:
        same_bits(other[k][plan], other_free[k][plan], f"race without a crash: {k}")
    assert (a["kind"][:, G:] != capi.TICK_CRASHED).all()


def test_follower_sees_the_parked_leader(capi, cuda):
    """The followers' recorded scans match race_cases' oracle at every tick's poses, the leader at its parked
    pose (world_cases' bound and cap, as test_gpu_rollout_race.py applies them)."""
    a = runs(capi, cuda)[1]
    x0, _, circles, _ = scene()
    c = rc_.RaceCase("parked leader", x0, G, circles)
    k = a["crash_tick"][0]
    for t in range(T):
        c.check(a["ranges_traj"][t], a["x_traj"][t], f"tick {t}")
    assert (bits(a["x_traj"][k:, 0]) == bits(a["x_traj"][k, 0])).all()
    alone = wc_.oracle_scan(a["x_traj"][T - 1, 1:2], circles, GEOM, R)
    assert (a["ranges_traj"][T - 1, 1] != alone[0]).sum() >= 10, "the parked leader is in car 1's last scan"


def test_contact_at_row_zero(capi, cuda):
    s = solver(capi, N, x_ref_points=P)
    a = rollout_contact_dev(capi, cuda, s, scene(gap=-0.05), 1, ticks=4)
    s.close()
    assert a["crash_tick"][0] == 0 and a["clear_traj"][0, 0] < 0
    assert (bits(a["x_traj"][:, 0]) == bits(a["x_traj"][0, 0])).all(), "the car never moves"
    assert (bits(a["pose_traj"][:, 0]) == bits(a["pose_traj"][0, 0])).all()
    assert (a["kind"][:, 0] == capi.TICK_CRASHED).all() and (a["u_applied"][:, 0] == 0).all()
    assert (a["crash_tick"][G:] == -1).all()


@pytest.mark.parametrize("stop", [0, 1])
def test_host_call_equals_the_device_call(capi, cuda, stop):
    """f110qp_rollout_contact on host pointers equals f110qp_rollout_contact_dev bit for bit (the pattern of
    test_gpu_rollout_host_dev.py: what a tick does not write is compared on the ticks of its kind)."""
    case = scene()
    x0, ul, circles, wp = case
    s = solver(capi, N, x_ref_points=P)
    a = rollout_contact_dev(capi, cuda, s, case, stop, ticks=5)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    h = s.rollout_contact(x0, ul, circles, capi.default_race_config(group_size=G),
                          capi.default_contact_config(stop_on_contact=stop), scan_config(capi, R, GEOM), rp,
                          capi.traj_table(rp.plan), wp, 5, plans=True, objective=True, scans=True)
    s.close()
    compare(a, h, f"host call, stop {stop}", True, True)
    for k in ("pose_traj", "clear_traj", "nearest_traj", "crash_tick"):
        same_bits(a[k], h[k], k)
    assert a["crash_tick"][0] > 0
