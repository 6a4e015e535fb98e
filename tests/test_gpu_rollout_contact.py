"""The closed loop with contact on MI355X: f110qp_rollout_contact[_dev] (include/f110qp.h, "contact"). With
stop_on_contact = 0 the call is f110qp_rollout_race_dev plus its records, bit for bit; with 1 a crashed car
parks. The scene (contact_cases.crash_scene): two races of four on make_race_grid in the track world, and one
large circle a few plant steps ahead of car 0. The second scene (contact_cases.wide_crash_scene): 65 races of
four, two workgroups of the plant step, six blocked cars at the edges of waves and workgroups that crash at
ticks 0 to 5 of 9; its three runs are computed once (wide_runs). Parking is also run with the optional outputs
NULL and with gap rows that feed the QP."""
import contact_cases as cc_
import numpy as np
import pytest
import race_cases as rc_
import replan_cases as rp_
import rollout_cases as roc_
import world_cases as wc_
from test_gpu_contact import bits, clearance
from test_gpu_rollout import bits as ubits
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_race import rollout_race_dev
from test_gpu_rollout_replan import P
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_world import GEOM, ON_MPC, ON_PLAN, OUT, R, compare
from world_loop import rollout_dev

from f110qp import workload

pytestmark = pytest.mark.gpu

B, G, N, T = 8, 4, 20, 12


def scene(gap=cc_.BLOCK_GAP):
    x0, circles = cc_.crash_scene(B, G, gap=gap)
    return x0, np.tile([roc_.V_LIN, 0.0], (B, 1)), circles, workload.track_waypoints()


def rollout_contact_dev(capi, cuda, s, case, stop, margin=0.0, ticks=T, nearest=True, group=G, null=()):
    """One Solver.rollout_contact_dev call on fresh device arrays -> every array as numpy. circles [C,3] or
    [B,C,3]; null: the optional arrays passed as NULL."""
    return rollout_dev(capi, cuda, s, "contact", case, ticks, group, stop, margin, nearest=nearest, null=null)


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


# ---- parking across lanes, waves, workgroups and races; its NULL options; gap rows -------------------------

def check_parked(capi, a, what, margin=0.0):
    """Every car with crash_tick = k >= 0 of a stop = 1 run: what the header says of ticks t >= k. Absent
    (NULL) arrays are left out."""
    ct, ticks = a["crash_tick"], a["status"].shape[0]
    assert (ct == first_row(a["clear_traj"], margin)).all(), what
    for b in np.flatnonzero(ct >= 0):
        k = ct[b]
        for name in ("x_traj", "u_lin_traj", "pose_traj"):
            if name in a:
                assert (ubits(a[name][k:, b]) == ubits(a[name][k, b])).all(), f"{what}: car {b}: {name} repeats row {k}"
        assert (ubits(a["u_applied"][k:, b]) == 0).all(), f"{what}: car {b}: u_applied is +0 from tick {k}"
        assert (a["status"][k:, b] == capi.NO_SOLVE).all(), f"{what}: car {b}: status"
        if "kind" in a:
            assert (a["kind"][k:, b] == capi.TICK_CRASHED).all(), f"{what}: car {b}: kind from tick {k}: {a['kind'][:, b]}"
            assert (a["kind"][:k, b] != capi.TICK_CRASHED).all(), f"{what}: car {b}: kind before tick {k}"
        if "hs_traj" in a and k < ticks:  # row k: the start kernel's (k = 0) or the free step's at the pose of row k
            assert (ubits(a["hs_traj"][k:, b]) == ubits(a["hs_traj"][k, b])).all(), f"{what}: car {b}: hs_traj follows the pose"
    if "kind" in a:
        assert (a["kind"][:, ct < 0] != capi.TICK_CRASHED).all(), what


def check_races_before_a_crash(a, free, group, what):
    """Race by race, k_r its first crash tick (the number of ticks when there is none): rows <= k_r of the state
    and clearance arrays and rows < k_r of what a tick writes are the stop = 0 run's bits; a race without a
    crash equals it in every output. -> the races without a crash."""
    ct, ticks = a["crash_tick"], a["status"].shape[0]
    nb = ct.shape[0]
    whole = []
    for r in range(nb // group):
        cars = slice(r * group, (r + 1) * group)
        hit = ct[cars][ct[cars] >= 0]
        k = int(hit.min()) if hit.size else ticks
        for name in ("x_traj", "u_lin_traj", "pose_traj", "clear_traj", "nearest_traj"):
            if name in a:
                same_bits(a[name][:k + 1, cars], free[name][:k + 1, cars], f"{what}: race {r}: {name} up to row {k}")
        for name in ("u_applied", "status", "kind", "hs_traj", "ranges_traj"):
            if name in a:
                same_bits(a[name][:k, cars], free[name][:k, cars], f"{what}: race {r}: {name} before tick {k}")
        if "kind" in a:
            kind = free["kind"][:k, cars]
            mpc, plan = kind == rp_.MPC, np.isin(kind, (rp_.PLAN, rp_.PLAN_FAILED))
            for name in ON_MPC:
                same_bits(a[name][:k, cars][mpc], free[name][:k, cars][mpc], f"{what}: race {r}: {name} on MPC ticks")
            for name in ON_PLAN:
                same_bits(a[name][:k, cars][plan], free[name][:k, cars][plan], f"{what}: race {r}: {name} on PLAN ticks")
        if not hit.size:
            whole.append(r)
            for name in ("x_ref", "have_path", "crash_tick"):
                same_bits(a[name][cars], free[name][cars], f"{what}: race {r} without a crash: {name}")
    return whole


WB, WG, WT = cc_.WIDE_B, cc_.WIDE_G, cc_.WIDE_T
_WIDE = {}


def wide_scene():
    x0, circles = cc_.wide_crash_scene()
    return x0, np.tile([roc_.V_LIN, 0.0], (WB, 1)), circles, workload.track_waypoints()


def wide_runs(capi, cuda):
    """The race rollout and the stop = 0 and stop = 1 runs of the 260-car scene, computed once."""
    if not _WIDE:
        s = solver(capi, N, x_ref_points=P)
        _WIDE["race"] = rollout_race_dev(capi, cuda, s, wide_scene(), WG, WT)
        _WIDE[0] = rollout_contact_dev(capi, cuda, s, wide_scene(), 0, ticks=WT, group=WG)
        _WIDE[1] = rollout_contact_dev(capi, cuda, s, wide_scene(), 1, ticks=WT, group=WG)
        s.close()
    return _WIDE


def test_wide_scene_is_what_it_was_built_to_be(capi, cuda):
    """260 cars, 65 races, two workgroups of the plant step: the blocked cars crash at the first and last lane of
    a wave, on both sides of the workgroup edge and at the batch's end, one at row 0, the others at several
    ticks; nobody else is in contact at row 0, and at least half of the races never crash."""
    a = wide_runs(capi, cuda)[1]
    ct = a["crash_tick"]
    blocked = np.array(sorted(cc_.WIDE_BLOCKED))
    print("crash ticks of the blocked cars:", dict(zip(blocked.tolist(), ct[blocked].tolist())), "others:",
          np.flatnonzero(ct >= 0).tolist())
    assert {0, 63, 64, 255, 256, 259} <= set(blocked.tolist()) and WB > 256 and WB % 64 == 4
    assert np.flatnonzero(a["clear_traj"][0] <= 0.0).tolist() == [b for b, g in cc_.WIDE_BLOCKED.items() if g < 0] == [0]
    assert ((ct[blocked] >= 0) & (ct[blocked] < WT)).all(), ct[blocked]
    assert ct[0] == 0 and len(set(ct[blocked].tolist())) >= 4, "one crash at row 0, the others at several ticks"
    crashed_races = np.unique(np.flatnonzero(ct >= 0) // WG)
    assert 2 * len(crashed_races) <= WB // WG, crashed_races
    assert len(np.unique(blocked // WG)) >= 5 and (ct[256:260] >= 0).sum() >= 2, "several races; two crashes in one"


def test_wide_recording_changes_nothing(capi, cuda):
    """stop = 0 at 260 cars: f110qp_rollout_race_dev's bits, f110qp_clearance_dev's on the returned x_traj,
    crash_tick the first row at or under the margin."""
    r = wide_runs(capi, cuda)
    a, race = r[0], r["race"]
    compare(a, race, "wide stop 0", True, True)
    same_bits(a["pose_traj"], race["pose_traj"], "pose_traj")
    clear, near = clearance(capi, cuda, a["x_traj"], wide_scene()[2], WG)
    assert (bits(a["clear_traj"]) == bits(clear)).all() and (a["nearest_traj"] == near).all()
    assert (a["crash_tick"] == first_row(a["clear_traj"], 0.0)).all()


def test_wide_parking(capi, cuda):
    """stop = 1 at 260 cars: every crashed car parks as the header says, its half-space rows included; every race
    is the stop = 0 run up to its first crash; no parked car plans again, and around it the wave's ballot goes
    on: a free race-mate still plans and solves."""
    r = wide_runs(capi, cuda)
    free, a = r[0], r[1]
    check_parked(capi, a, "wide")
    whole = check_races_before_a_crash(a, free, WG, "wide")
    assert 2 * len(whole) >= WB // WG
    ct = a["crash_tick"]
    for b in np.flatnonzero(ct >= 0):
        assert not np.isin(a["kind"][ct[b] + 1:, b], (rp_.PLAN, rp_.PLAN_FAILED)).any(), f"car {b}: no PLAN after the crash"
        assert (a["plan_status"][ct[b] + 1:, b] == -7).all(), f"car {b}: on no plan list after the crash"
    for race in np.unique(np.flatnonzero(ct >= 0) // WG):
        cars = np.arange(race * WG, (race + 1) * WG)
        k = ct[cars][ct[cars] >= 0].min()
        after = a["kind"][k + 1:, cars[ct[cars] < 0]]
        print(f"race {race}: first crash at tick {k}, the free mates' kinds after it:", after.T.tolist())
        assert ((after == rp_.PLAN).any(axis=0) & (after == rp_.MPC).any(axis=0)).any(), (race, after.T.tolist())
        planned = a["kind"][WT - 1, cars] == rp_.PLAN
        assert (a["plan_status"][WT - 1, cars[planned]] == 0).all(), f"race {race}: the last tick's plans were made"
    moved = (bits(a["x_traj"][WT]) != bits(free["x_traj"][WT])).any(axis=1)
    assert moved[ct >= 0][ct[ct >= 0] < WT - 1].all(), "the free run drives on"


def test_wide_follower_sees_the_parked_leader(capi, cuda):
    """Race 64, in the second workgroup: car 257's last scan holds car 256 where it parked."""
    a = wide_runs(capi, cuda)[1]
    circles = wide_scene()[2]
    lead, foll = 256, 257
    k = a["crash_tick"][lead]
    assert 0 <= k < WT - 1 and a["crash_tick"][foll] == -1
    assert (bits(a["x_traj"][k:, lead]) == bits(a["x_traj"][k, lead])).all()
    alone = wc_.oracle_scan(a["x_traj"][WT - 1, foll:foll + 1], circles[foll], GEOM, R)
    assert (a["ranges_traj"][WT - 1, foll] != alone[0]).sum() >= 10, "the parked leader is in car 257's last scan"
    race = rc_.RaceCase("race 64", a["x_traj"][WT - 1, 256:260], WG, np.ascontiguousarray(circles[256:260]), cars=[foll - 256])
    race.check(a["ranges_traj"][WT - 1, 256:260], what="last tick")


OPTIONAL = ("nearest_traj", "iters", "cost", "u_plan", "x_plan", "hs_traj", "kind", "plan_status", "best_traj",
            "best_global", "pose_traj", "ranges_traj")


@pytest.mark.parametrize("null", [OPTIONAL, ("kind",), ("pose_traj",)], ids=["all", "kind_traj", "pose_traj"])
def test_parking_with_null_options(capi, cuda, null):
    """stop = 1 with optional outputs NULL: the kinds in the two-row buffer (park_car writes both rows), the pose
    row in place, casts on the plan list only, no gap rows. NULL in the first variant: nearest_traj, iters, cost,
    u_plan, x_plan, hs_traj, kind, plan_status, best_traj, best_global, pose_traj, ranges_traj; u_applied is not
    optional in the device call's argument check and stays. The two partial variants point at one route each.
    Every array left equals the all-outputs run bit for bit."""
    want = runs(capi, cuda)[1]
    s = solver(capi, N, x_ref_points=P)
    a = rollout_contact_dev(capi, cuda, s, scene(), 1, null=null)
    s.close()
    assert not set(null) & set(a) and want["crash_tick"][0] > 0
    for k in ("x_traj", "u_lin_traj", "status", "clear_traj", "crash_tick", "u_applied", "x_ref", "have_path"):
        same_bits(a[k], want[k], f"NULL {null}: {k}")
    for k in ("kind", "pose_traj", "hs_traj", "ranges_traj", "nearest_traj"):
        if k in a:
            same_bits(a[k], want[k], f"NULL {null}: {k}")
    kind = want["kind"]
    for names, mask in ((ON_MPC, kind == rp_.MPC), (ON_PLAN, np.isin(kind, (rp_.PLAN, rp_.PLAN_FAILED)))):
        for k in names:
            if k in a:
                same_bits(a[k][mask], want[k][mask], f"NULL {null}: {k}")
    check_parked(capi, a, f"NULL {null}")


def test_parking_with_gap_rows(capi, cuda):
    """gap_mode = GAP_ACTIVE, where the half-space rows feed the QP: stop = 0 is the race rollout with the same
    solver; at stop = 1 the parked car's rows follow the unchanged pose, and both races are the stop = 0 run up
    to their first crash. Car 0, a hand's breadth from its block, has a scan without a gap and so NaN rows; a
    margin that cars out on the track pass on their way parks cars whose rows are numbers."""
    s = solver(capi, N, gap=True, x_ref_points=P)
    race = rollout_race_dev(capi, cuda, s, scene(), G, T)
    free = rollout_contact_dev(capi, cuda, s, scene(), 0)
    a = rollout_contact_dev(capi, cuda, s, scene(), 1)
    # a margin that parks a car out on the track at a tick k >= 1: a clearance of the free run that is its car's
    # lowest so far, at a row whose half-space rows are numbers and differ from the row's before
    clear, hs = free["clear_traj"], free["hs_traj"]
    picks = [(k, b) for b in range(1, B) for k in range(1, T - 1)
             if clear[k, b] < clear[:k, b].min() and np.isfinite(hs[k - 1:k + 1, b]).all()
             and (ubits(hs[k, b]) != ubits(hs[k - 1, b])).any()]
    assert picks, "no car of the free run comes closer to anything than it started"
    k_m, b_m = picks[len(picks) // 2]
    margin = float(clear[k_m, b_m])
    am = rollout_contact_dev(capi, cuda, s, scene(), 1, margin=margin)
    s.close()
    compare(free, race, "gap rows, stop 0", True, True)
    same_bits(free["pose_traj"], race["pose_traj"], "pose_traj")
    plain = runs(capi, cuda)[0]
    assert (free["status"] != plain["status"]).any() or (ubits(free["x_traj"]) != ubits(plain["x_traj"])).any(), \
        "the rows reach the QP"
    assert 0 < a["crash_tick"][0] < T and (a["crash_tick"][G:] == -1).all(), a["crash_tick"]
    check_parked(capi, a, "gap rows")
    assert check_races_before_a_crash(a, free, G, "gap rows") == [1]
    ct = am["crash_tick"]
    print(f"gap rows: margin {margin} parks car {b_m} at tick {k_m} ({len(picks)} candidates), crash ticks {ct.tolist()}")
    check_parked(capi, am, "gap rows with a margin", margin)
    check_races_before_a_crash(am, free, G, "gap rows with a margin")
    assert ct[b_m] == k_m and np.isfinite(am["hs_traj"][k_m:, b_m]).all(), (b_m, k_m, ct.tolist())
    assert (ubits(am["hs_traj"][k_m, b_m]) != ubits(am["hs_traj"][k_m - 1, b_m])).any(), \
        "a car parks whose rows are numbers and moved with its pose until it parked"
