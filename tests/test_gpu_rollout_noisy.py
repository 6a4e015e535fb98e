"""The rollout with a noisy LiDAR on MI355X (f110qp_rollout_noisy[_dev]; include/f110qp.h rules Z1 to Z3) at T = 6,
B = 8, G = 2, N = 5 on the scene and helpers of test_gpu_rollout_refresh.py: the all-zero config is the refresh call
bit for bit; with noise every row of ranges_traj is f110qp_cast_scans_noisy_dev at that row's poses with that tick and
workload.noisy_scan of the walls cast there, the rows obey the refresh rule on the noisy scans, ranges_traj given and
NULL agree, the host call equals the device call and parked cars stay parked; noise flips the gap record of a face
15 mm beyond the threshold; and car_base shifts the hypotheses of a batch. Everything is bit equality."""
import noise_cases as nz
import numpy as np
import pytest
import refresh_cases as rf_
from test_gpu_noise import noisy_cast
from test_gpu_rollout import same_bits, solver
from test_gpu_rollout_contact import check_parked
from test_gpu_rollout_refresh import closing_scene, rollout_refresh_dev, same_run
from test_gpu_rollout_refresh import run as refresh_run
from test_gpu_rollout_replan import P
from test_gpu_rollout_scan import scan_config, split_rows
from test_gpu_rollout_walls import B, G, N, T, scene
from test_gpu_rollout_world import GEOM, R
from test_gpu_walls import wall_cast
from world_loop import rollout_dev

pytestmark = pytest.mark.gpu

SEED = 7  # with sigma_abs = 0.05 it flips car 0's record on closing_scene() (asserted on the fixture below)
NOISE = (0.05, 0.01, 0.02)


def rollout_noisy_dev(capi, cuda, s, case, stop, every, noise, ticks=T, null=(), group=G):
    """One Solver.rollout_noisy_dev call on fresh device arrays -> every array as numpy."""
    return rollout_dev(capi, cuda, s, "noisy", case, ticks, group, stop, every=every, noise=noise, null=null)


def noise_of(capi, setting=NOISE, seed=SEED, car_base=0):
    return nz.noise_config(capi, seed, car_base, setting)


_RUNS = {}


def run(capi, cuda, stop, null=()):
    """The noisy run of the scene at every = 1, gap rows on, computed once."""
    key = (stop, null)
    if key not in _RUNS:
        s = solver(capi, N, gap=True, x_ref_points=P)
        _RUNS[key] = rollout_noisy_dev(capi, cuda, s, scene(), stop, 1, noise_of(capi), null=null)
        s.close()
    return _RUNS[key]


@pytest.mark.parametrize("stop", [0, 1])
@pytest.mark.parametrize("every", [0, 1])
def test_zero_noise_is_the_refresh_call(capi, cuda, every, stop):
    s = solver(capi, N, gap=True, x_ref_points=P)
    a = rollout_noisy_dev(capi, cuda, s, scene(), stop, every, capi.default_noise_config())
    s.close()
    same_run(a, refresh_run(capi, cuda, True, stop, every), f"every {every} stop {stop}")


def test_scans_and_rows_follow_the_rule(capi, cuda):
    a = run(capi, cuda, 0)
    _, _, circles, sg, _ = scene()
    moved = 0
    for t in range(T):
        x = a["x_traj"][t]
        same_bits(a["ranges_traj"][t], noisy_cast(capi, cuda, x, circles, sg, G, GEOM, R, noise_of(capi), t),
                  f"scan of tick {t}: f110qp_cast_scans_noisy_dev with tick {t}")
        clean = wall_cast(capi, cuda, x, circles, sg, G, GEOM, R)
        same_bits(a["ranges_traj"][t], nz.oracle(clean, SEED, 0, t, NOISE), f"scan of tick {t}: noisy_scan of the walls cast")
        moved += int((a["ranges_traj"][t] != clean).sum())
        # check_rows' rule at every = 1 on the noisy scans: row t holds the rows of scan row t at x_traj row t
        want, _ = split_rows(capi, cuda, x, np.ascontiguousarray(a["ranges_traj"][t]), GEOM)
        same_bits(a["hs_traj"][t], want, f"rows of tick {t} from the noisy scan of tick {t}")
    assert moved > T * B * R // 2, "the scans carry noise"
    quiet = refresh_run(capi, cuda, True, 0, 1)
    assert (a["ranges_traj"][0] != quiet["ranges_traj"][0]).any()


def test_ranges_traj_given_and_null_agree(capi, cuda):
    a, want = run(capi, cuda, 1, null=("ranges_traj",)), run(capi, cuda, 1)
    assert "ranges_traj" not in a
    for k in a:
        same_bits(a[k], want[k], k)


@pytest.mark.parametrize("stop", [0, 1])
def test_host_call_equals_the_device_call(capi, cuda, stop):
    x0, ul, circles, sg, wp = scene()
    s = solver(capi, N, gap=True, x_ref_points=P)
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    h = s.rollout_noisy(x0, ul, circles, sg, capi.default_race_config(group_size=G),
                        capi.default_contact_config(stop_on_contact=stop), capi.default_body_config(),
                        capi.default_refresh_config(every=1), noise_of(capi), scan_config(capi, R, GEOM), rp,
                        capi.traj_table(rp.plan), wp, T, scans=True)
    s.close()
    a = run(capi, cuda, stop)
    for k in ("x_traj", "u_lin_traj", "u_applied", "status", "hs_traj", "kind", "clear_traj", "nearest_traj", "crash_tick",
              "ranges_traj"):
        same_bits(np.asarray(h[k]).reshape(a[k].shape), a[k], k)


def test_parked_cars_stay_parked(capi, cuda):
    """check_parked on every array but hs_traj: its clause there ("the rows follow the pose") holds for a held or a
    noise-free scan, and a parked car's LiDAR is as noisy as any other, so at every = 1 its rows are those of tick
    t's noisy scan at the unchanged pose: the rule of test_scans_and_rows_follow_the_rule, checked here on every car
    of the stop = 1 run."""
    a = run(capi, cuda, 1)
    parked = np.flatnonzero(a["crash_tick"] >= 0)
    assert parked.size and (a["crash_tick"][parked] < T - 1).any(), a["crash_tick"]
    check_parked(capi, {k: v for k, v in a.items() if k != "hs_traj"}, "noisy stop 1")
    for t in range(T):
        want, _ = split_rows(capi, cuda, a["x_traj"][t], np.ascontiguousarray(a["ranges_traj"][t]), GEOM)
        same_bits(a["hs_traj"][t], want, f"stop 1: rows of tick {t} from the noisy scan of tick {t}")
    b = int(parked[0])
    k = int(a["crash_tick"][b])
    assert (a["ranges_traj"][k + 1:, b] != a["ranges_traj"][k, b]).any(), "a parked car's scan keeps its noise"


# ---- the point of the feature -------------------------------------------------------------------------------------

def test_noise_flips_a_gap_at_the_threshold(capi, cuda):
    """closing_scene(): car 0's face sits 15 mm beyond ftg_thresh, sigma_abs = 0.05 m."""
    case = closing_scene()
    x0, _, circles, sg, _ = case
    setting = (0.05, 0.0, 0.0)
    # the fixture, in numpy: the record of the noisy oracle scan differs from the noise-free one's at seed 7
    clean = rf_.wl_.oracle_scan(np.ascontiguousarray(x0, np.float64), circles, sg, G, GEOM, R)
    first = rf_.record(clean[0], GEOM)
    noisy = rf_.record(nz.oracle(clean, SEED, 0, 0, setting)[0], GEOM)
    print(f"car 0's record at row 0: {first} noise-free, {noisy} at seed {SEED}")
    assert first != noisy, "the fixture: the chosen seed flips the record"
    s = solver(capi, N, gap=True, x_ref_points=P)
    quiet = rollout_refresh_dev(capi, cuda, s, case, 0, 1)
    loud = rollout_noisy_dev(capi, cuda, s, case, 0, 1, noise_of(capi, setting))
    s.close()
    _, rq = split_rows(capi, cuda, x0, np.ascontiguousarray(quiet["ranges_traj"][0]), GEOM)
    _, rl = split_rows(capi, cuda, x0, np.ascontiguousarray(loud["ranges_traj"][0]), GEOM)
    assert (rq["lo"][0], rq["hi"][0]) != (rl["lo"][0], rl["hi"][0]), "car 0's gap record at row 0 differs"
    assert (loud["hs_traj"][0, 0] != quiet["hs_traj"][0, 0]).any(), "and so do the rows tick 0's solve reads"


def test_sharding_identity(capi, cuda):
    """G = 1, eight identical starts: the car_base = 1 rollout's cars 0 to 6 are the car_base = 0 rollout's 1 to 7."""
    x0, ul, circles, sg, wp = scene()
    case = (np.ascontiguousarray(np.repeat(x0[1:2], B, axis=0)), ul, circles, np.ascontiguousarray(sg[:-1]), wp)
    s = solver(capi, N, gap=True, x_ref_points=P)
    a = rollout_noisy_dev(capi, cuda, s, case, 0, 1, noise_of(capi, car_base=0), group=1)
    b = rollout_noisy_dev(capi, cuda, s, case, 0, 1, noise_of(capi, car_base=1), group=1)
    s.close()
    for k in ("x_traj", "u_applied", "status", "ranges_traj"):
        same_bits(b[k][:, :B - 1], a[k][:, 1:], f"{k}: car b at car_base 1 is car b + 1 at car_base 0")
    assert any((a["ranges_traj"][:, i] != a["ranges_traj"][:, j]).any() for i in range(B) for j in range(i)), \
        "the hypotheses differ"
