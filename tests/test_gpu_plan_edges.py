"""The planning kernel (plan_kernels.hip) on the inputs its other tests never reach: the dilation
fallback loops and the boundary of the precomputed offsets, scans whose computed beam count is not
their length, waypoint lists with exact and within-ulp distance ties and with 0 to 5,000 points,
end-point ties, the table and grid shapes at the ABI's limits, poses a kilometre out, at yaw +-pi
and with non-unit quaternions, and the host entry f110qp_plan_batch across calls of different
sizes. Every device output is compared bit for bit with the CPU oracle (plan_oracle.c), and every
case first proves from the oracle's own answers that it sits where it is meant to."""
import numpy as np
import plan_cases as pc
import pytest
from test_gpu_plan import check_against_oracle, run_plan_dev

from f110qp import capi

pytestmark = pytest.mark.gpu


def plan_and_check(oracle, cuda, sc, over=None, table=None):
    """Device against oracle for one batch of scenes under the config overrides `over`, with the
    library's table unless the scenes or the caller bring one. Returns (device outputs, oracle
    answers, config)."""
    over = over or {}
    pp = oracle.plan_params(**over)
    cfg = capi.default_plan_config(**over)
    if table is None:
        table = sc["table"] if "table" in sc else capi.traj_table(cfg)
    dev = run_plan_dev(cuda, cfg, sc, table)
    return dev, check_against_oracle(oracle, pp, sc, table, dev), cfg


def statuses(ans):
    return np.array([r["status"] for r in ans])


@pytest.mark.parametrize("dilation,discrete,count", pc.DILATION_CASES)
def test_dilation_offset_counts(oracle, cuda, dilation, discrete, count):
    """1 offset per axis (dilation 0, the offset is -0.0f), 8 (the last precomputed count), 9 and
    24 (the kernel's nested float loops)."""
    over = pc.dilation_over(dilation, discrete)
    assert len(oracle.dilation_offsets(oracle.plan_params(**over))) == count
    dev, ans, _ = plan_and_check(oracle, cuda, pc.base(32), over)
    assert dev["grid"].sum() > 0


def test_scan_longer_than_its_ranges(oracle, cuda):
    """700 ranges under the 1,080-beam angles. The reference would read past the vector here
    (occupancy_grid.cpp:66-70), so the project's clamp to num_ranges is the specification."""
    sc = pc.scan_truncated(32)
    assert pc.num_scans(sc) == 1080 and sc["ranges"].shape[1] == 700
    dev, _, _ = plan_and_check(oracle, cuda, sc)
    assert dev["grid"].sum() > 0


def test_scan_shorter_than_its_ranges(oracle, cuda):
    """angle_max halved: the beams past the computed count hold 0.3 m returns and must be ignored."""
    sc = pc.scan_half_angle(32)
    n = pc.num_scans(sc)
    assert 256 < n < 1080 - 256 and (sc["ranges"][:, n:] == np.float32(0.3)).all()
    dev, ans, _ = plan_and_check(oracle, cuda, sc)
    pp = oracle.plan_params()
    whole = oracle.fill_occ_grid(pp, sc["pose"][0], sc["ranges"][0], sc["angle_min"], sc["angle_inc"],
                                 pc.base(1)["angle_max"])[0]
    assert whole.sum() > ans[0]["grid"].sum() > 0  # reading the tail would mark more cells


@pytest.mark.parametrize("beams", pc.BEAM_COUNTS)
def test_scan_beam_counts(oracle, cuda, beams):
    """num_ranges of 1, below one wave, either side of the 256-thread stride, and a 720-beam lidar."""
    sc = pc.scan_beams(32, beams)
    assert pc.num_scans(sc) == beams == sc["ranges"].shape[1]
    dev, _, _ = plan_and_check(oracle, cuda, sc)
    assert dev["grid"].sum() > 0


def test_scan_reversed_angles_fill_nothing(oracle, cuda):
    """angle_max < angle_min: a negative beam count, an empty grid, and statuses of an empty grid."""
    sc = pc.scan_reversed(32)
    assert pc.num_scans(sc) < 0
    dev, ans, _ = plan_and_check(oracle, cuda, sc)
    assert dev["grid"].sum() == 0 and all(r["grid"].sum() == 0 for r in ans)
    assert dev["valid"].all() and (dev["status"] == 0).all()


def test_doubled_lap_exact_ties(oracle, cuda):
    """Every distance ties exactly with its twin one lap on: the sequential float minimum lands on
    the first copy where float(d) rounded down or exactly, on the second where it rounded up."""
    sc = pc.doubled_lap(64)
    dev, ans, _ = plan_and_check(oracle, cuda, sc)
    bg = np.array([r["best_global"] for r in ans])[statuses(ans) == 0]
    assert ((bg >= 0) & (bg < 500)).sum() >= 8 and (bg >= 500).sum() >= 8, bg


def test_tripled_lap_with_closing_duplicate(oracle, cuda):
    sc = pc.tripled_lap(64)
    assert sc["waypoints"].shape[0] == 1501
    dev, ans, _ = plan_and_check(oracle, cuda, sc)
    bg = np.array([r["best_global"] for r in ans])[statuses(ans) == 0]
    assert (bg < 501).sum() >= 8 and (bg >= 1001).sum() >= 8, bg


def test_within_ulp_ties(oracle, cuda):
    """40 waypoints whose |dist - lookahead| lie within a few float32 ulps of one float32 value,
    on both sides of it: the reference's answer (a running minimum kept in a float) is not the
    argmin of the double distances, and the two-pass device form must reproduce it."""
    quirks = 0
    for seed in range(8):
        sc, d = pc.ulp_tie_scene(seed)
        assert len(np.unique(d.astype(np.float32))) < len(np.unique(d))  # distinct doubles share a float
        dev, ans, _ = plan_and_check(oracle, cuda, sc)
        assert ans[0]["status"] == 0
        quirks += ans[0]["best_global"] != int(np.argmin(d))
    assert quirks >= 1


@pytest.mark.parametrize("W", pc.WAYPOINT_COUNTS)
def test_waypoint_counts(oracle, cuda, W):
    """0, 1, 2 waypoints and counts either side of a wave and of the 256-thread stride; the first
    four scenes have only the last waypoint ahead of the car."""
    sc = pc.waypoint_count(32, W)
    assert sc["waypoints"].shape == (W, 2)
    dev, ans, _ = plan_and_check(oracle, cuda, sc)
    st = statuses(ans)
    if W == 0:
        anyv = dev["valid"].any(axis=1)
        assert anyv.any() and not anyv.all()  # both outcomes: no waypoint (2) and no candidate (1)
        np.testing.assert_array_equal(dev["status"], np.where(anyv, 2, 1))
        assert (dev["best_global"] == -1).all() and (dev["best_traj"] == -1).all()
        return
    pp = oracle.plan_params()
    table = capi.traj_table(capi.default_plan_config())
    for b in range(4):
        assert st[b] == 0 and ans[b]["best_global"] == W - 1
        r = oracle.plan(pp, sc["pose"][b], ans[b]["grid"], oracle.fill_occ_grid(
            pp, sc["pose"][b], sc["ranges"][b], sc["angle_min"], sc["angle_inc"], sc["angle_max"])[1], table,
            sc["waypoints"][:-1])
        assert r["status"] == 2  # without the last waypoint nothing is ahead
    assert (st[4:] == 0).any()


def test_five_thousand_waypoints_late_winner(oracle, cuda):
    sc = pc.fine_lap(32)
    assert sc["waypoints"].shape[0] == 5000
    dev, ans, _ = plan_and_check(oracle, cuda, sc)
    bg = np.array([r["best_global"] for r in ans])[statuses(ans) == 0]
    assert len(bg) >= 16 and (bg > 4000).all(), bg


def test_end_point_ties_smaller_index_wins(oracle, cuda):
    """Every candidate twice in a shuffled 62-row table: twins have the same validity and the same
    end-point distance to the bit, and the reference's strict `<` keeps the first."""
    cfg0 = capi.default_plan_config()
    sc, rows = pc.duplicated_table(64, capi.traj_table(cfg0))
    assert sc["table"].shape == (62, 50, 3) and sorted(rows) == sorted(list(range(31)) * 2)
    dev, ans, _ = plan_and_check(oracle, cuda, sc, dict(steer_discrete=61))
    first = {r: int(np.nonzero(rows == r)[0][0]) for r in range(31)}
    second = {r: int(np.nonzero(rows == r)[0][1]) for r in range(31)}
    n0 = 0
    for r in ans:
        if r["status"] != 0:
            continue
        n0 += 1
        row = rows[r["best_traj"]]
        assert r["best_traj"] == first[row] and r["valid"][second[row]] == 1
    assert n0 >= 32


@pytest.mark.parametrize("steer_discrete,traj_discrete", pc.TABLE_SHAPES)
def test_table_shape_limits(oracle, cuda, steer_discrete, traj_discrete):
    """T x P from 2 x 2 to 256 x 1024 (T P = 2^18, the bound of the candidate-of-point index).
    Device and oracle both read the library's table."""
    over = dict(steer_discrete=steer_discrete, traj_discrete=traj_discrete)
    dev, ans, _ = plan_and_check(oracle, cuda, pc.base(8), over)
    valid = np.array([r["valid"] for r in ans])
    assert valid.shape == (8, steer_discrete + 1)
    if (steer_discrete, traj_discrete) == (255, 1024):
        assert valid.any() and not valid.all()  # 46 m of path: a mix of valid and invalid candidates


@pytest.mark.parametrize("size,discrete,G", pc.GRID_SHAPES)
def test_grid_shape_limits(oracle, cuda, size, discrete, G):
    """Odd G (G G not a multiple of the 4-byte words the LDS clear writes), G = 1 and G = 200."""
    over = pc.grid_over(size, discrete)
    assert capi.grid_blocks(capi.default_plan_config(**over)) == G
    dev, ans, _ = plan_and_check(oracle, cuda, pc.base(8), over)
    assert dev["grid"].shape == (8, G, G)
    assert G == 1 or dev["grid"].sum() > 0


def test_pose_far_from_the_origin(oracle, cuda):
    dev, ans, _ = plan_and_check(oracle, cuda, pc.far_origin(32))
    assert (statuses(ans) == 0).sum() >= 16 and dev["grid"].sum() > 0


def test_pose_axis_yaws(oracle, cuda):
    sc = pc.axis_yaws(32)
    dev, ans, _ = plan_and_check(oracle, cuda, sc)
    yaw = dev["x0"][:, 2]
    assert yaw[0] == np.float32(np.pi) and yaw[1] == -np.float32(np.pi)  # the zero's sign picks the branch
    assert set(np.abs(yaw)) == {np.float32(np.pi), np.float32(np.pi / 2)}


@pytest.mark.parametrize("scale", pc.QUAT_SCALES)
def test_pose_non_unit_quaternion(oracle, cuda, scale):
    """basis() normalises by 2 / |q|^2 as tf2 does, GetCarOrientation does not: the heading of
    the scaled scene is not the unit scene's, the rotation of the candidates is."""
    dev, ans, _ = plan_and_check(oracle, cuda, pc.scaled_quaternions(32, scale))
    qz, qw = pc.base(32)["pose"][:, 2:].T
    unit_yaw = np.arctan2(2 * qw * qz, 1 - 2 * qz * qz).astype(np.float32)
    oracle_yaw = np.array([r["x0"][2] for r in ans])
    assert (oracle_yaw != unit_yaw).mean() > 0.9 and (statuses(ans) == 0).any()


def _host_outputs(rows, cfg, want):
    T, P, G = cfg.steer_discrete + 1, cfg.traj_discrete, capi.grid_blocks(cfg)
    out = dict(x_ref=np.full((rows, P, 3), -7.0, np.float32), x0=np.full((rows, 3), -7.0, np.float32),
               best_traj=np.full(rows, -77, np.int32), best_global=np.full(rows, -77, np.int32),
               status=np.full(rows, -77, np.int32))
    if want:
        out["valid"] = np.full((rows, T), 0x5A, np.uint8)
        out["grid"] = np.full((rows, G, G), 0x5A, np.uint8)
    return out


def test_host_entry_across_calls(cuda):
    """f110qp_plan_batch keeps grow-only device buffers per host thread: four calls on one thread
    that shrink, grow, change every shape and shrink again. Each call's outputs are bit-equal to
    plan_batch_dev's on the same inputs, and only the first B rows of the caller's arrays change."""
    other = dict(size=7, discrete=np.float32(0.2), traj_discrete=30)
    calls = ((pc.base(40), {}, True), (pc.base(3, seed=32), {}, False),
             (pc.waypoint_count(64, 63), other, True), (pc.base(1, seed=33), {}, True))
    for sc, over, want in calls:
        cfg = capi.default_plan_config(**over)
        table = capi.traj_table(cfg)
        B = sc["pose"].shape[0]
        dev = run_plan_dev(cuda, cfg, sc, table, want_grid=want)
        out = _host_outputs(B + 5, cfg, want)
        sentinel = {k: v[B:].copy() for k, v in out.items()}
        capi.plan_batch(cfg, sc["pose"], sc["ranges"], sc["angle_min"], sc["angle_inc"], sc["angle_max"], table,
                        sc["waypoints"], **out)
        for k, v in out.items():
            np.testing.assert_array_equal(v[B:], sentinel[k], err_msg=f"B={B} {k}: rows past the batch")
            np.testing.assert_array_equal(v[:B].view(np.uint32 if v.dtype == np.float32 else v.dtype),
                                          dev[k].view(np.uint32 if v.dtype == np.float32 else v.dtype),
                                          err_msg=f"B={B} {k}")
        assert (out["status"][:B] == 0).any()
