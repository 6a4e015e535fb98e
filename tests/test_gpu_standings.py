"""The standings kernels on MI355X (f110qp_progress_dev, f110qp_standings_dev, f110qp_race_standings;
include/f110qp.h "race standings") against the numpy oracle, bit for bit on every output: the tile, pass and
grid edges, races wider than a workgroup, exact ties, vertices, a duplicated and a non-finite waypoint, non-finite
and far poses, optional outputs, permuted races, the host-pointer call, and one closed loop with contact. Every
case is built in standings_cases.py (test_standings_cases.py holds the oracle to the model on the CPU)."""
import numpy as np
import pytest
import standings_cases as sc_
from test_gpu_rollout_replan import dev

from f110qp import workload

pytestmark = pytest.mark.gpu


def progress(capi, cuda, x, wp, seg=True, lateral=True):
    """f110qp_progress_dev on numpy arrays -> dict of seg, s, lateral (None where left out), the path's lengths
    from f110qp_path_lengths."""
    import torch

    x = np.ascontiguousarray(x, np.float64)
    rows, B = x.shape[:2]
    s = torch.full((rows, B), -7.0, dtype=torch.float64, device=cuda)
    sg = torch.full((rows, B), -7, dtype=torch.int32, device=cuda) if seg else None
    lt = torch.full((rows, B), -7.0, dtype=torch.float64, device=cuda) if lateral else None
    capi.progress_dev(dev(cuda, x), dev(cuda, wp), dev(cuda, capi.path_lengths(wp)), s, sg, lt)
    torch.cuda.synchronize(cuda)
    return dict(seg=sg.cpu().numpy() if seg else None, s=s.cpu().numpy(), lateral=lt.cpu().numpy() if lateral else None)


def standings(capi, cuda, s, L, G, lap=True):
    import torch

    rows, B = s.shape
    dist = torch.full((rows, B), -7.0, dtype=torch.float64, device=cuda)
    rank = torch.full((rows, B), -7, dtype=torch.int32, device=cuda)
    lp = torch.full((rows, B), -7, dtype=torch.int32, device=cuda) if lap else None
    capi.standings_dev(capi.default_race_config(group_size=G), dev(cuda, s), L, dist, rank, lp)
    torch.cuda.synchronize(cuda)
    return dict(dist=dist.cpu().numpy(), lap=lp.cpu().numpy() if lap else None, rank=rank.cpu().numpy())


def run(capi, cuda, c, optional=True):
    """Both device calls on a case (the second on the first's s), every output or the required ones only."""
    out = progress(capi, cuda, c.x, c.wp, optional, optional)
    if c.ranked:
        out.update(standings(capi, cuda, out["s"], float(capi.path_lengths(c.wp)[-1]), c.G, optional))
    return out


@pytest.mark.parametrize("W", sc_.TILE_W)
def test_tile_edges(capi, cuda, W):
    c = sc_.tile_case(W)
    c.check(run(capi, cuda, c))


@pytest.mark.parametrize("rows", sc_.PASS_ROWS)
def test_pass_edges(capi, cuda, rows):
    c = sc_.rows_case(rows)
    c.check(run(capi, cuda, c))


@pytest.mark.parametrize("B", sc_.BATCHES)
def test_batch_sizes(capi, cuda, B):
    """The last one is past progress_grid's cap: the first workgroups take a second car."""
    c = sc_.batch_case(B)
    c.check(run(capi, cuda, c))


@pytest.mark.parametrize("G", sc_.GROUPS)
def test_race_sizes(capi, cuda, G):
    c = sc_.group_case(G)
    got = run(capi, cuda, c)
    c.check(got)
    if G > 1:
        assert got["rank"][0, G - 1] == got["rank"][0, 0] + (2 if G > 4 else 1), "twins rank by index"


def test_vertices_segments_and_exact_ties(capi, cuda):
    for c in sc_.vertex_case() + sc_.tie_case():
        c.check(run(capi, cuda, c))
    plain = sc_.tie_case()[0]
    seg = run(capi, cuda, plain)["seg"][0]
    assert (seg[:10] == np.arange(35, 65, 3)).all(), "the lowest index of two opposite segments"


def test_duplicated_and_non_finite_waypoints(capi, cuda):
    c = sc_.duplicate_case()
    c.check(run(capi, cuda, c))
    for c in sc_.bad_waypoint_cases():
        got = run(capi, cuda, c)
        c.check(got)
        assert not np.isin(got["seg"], (6, 7)).any() and (got["seg"] >= 0).all()
        clean = progress(capi, cuda, c.x, sc_.ellipse(40))
        keep = ~np.isin(clean["seg"], (6, 7))
        assert (got["seg"][keep] == clean["seg"][keep]).all() and sc_.same(got["lateral"][keep], clean["lateral"][keep])


@pytest.mark.parametrize("G", [1, 4])
def test_non_finite_poses(capi, cuda, G):
    c = sc_.bad_pose_case(G)
    got = run(capi, cuda, c)
    c.check(got)
    bad = ~np.isfinite(c.x[..., :2]).all(axis=2)
    assert bad.sum() == 6 and np.isnan(c.x[-1, 0, 2]) and np.isfinite(got["s"][-1, 0]), "a NaN heading is not read"
    assert (got["seg"][bad] == -1).all() and np.isnan(got["s"][bad]).all() and np.isnan(got["lateral"][bad]).all()
    gone = np.maximum.accumulate(bad, axis=0)  # from its first bad row on
    assert np.isnan(got["dist"][gone]).all() and (got["lap"][gone] == sc_.INT_MIN).all()
    assert np.isfinite(got["dist"][~gone]).all()
    if G > 1:
        assert (got["rank"][gone] == G - 1).all(), "ranked last"
        fine = c.x.copy()
        fine[bad] = c.x[0, 0]  # the same races with a number in the bad car's place: the mates keep their order
        ref = run(capi, cuda, sc_.StandingsCase("mates", fine, c.wp, G))
        mates = ~gone
        assert sc_.same(got["dist"][mates], ref["dist"][mates])

        def order(o):  # per row and race: the mates by rank
            return [[[int(b) for b in g + np.argsort(o["rank"][r, g:g + G]) if mates[r, b]] for g in range(0, c.B, G)]
                    for r in range(c.rows)]

        assert order(got) == order(ref), "the mates' order among themselves is undisturbed"


def test_far_poses_and_grids(capi, cuda):
    c = sc_.far_case()
    c.check(run(capi, cuda, c))
    for g in sc_.GRIDS[2:]:
        c = sc_.grid_case(*g)
        got = run(capi, cuda, c)
        c.check(got)
        assert (got["rank"][0] == np.arange(c.B) % c.G).all()


def test_optional_outputs_left_out(capi, cuda):
    c = sc_.rows_case(9)
    full, part = run(capi, cuda, c), run(capi, cuda, c, optional=False)
    assert part["seg"] is None and part["lateral"] is None and part["lap"] is None
    c.check(part)
    for k in ("s", "dist", "rank"):
        assert sc_.same(part[k], full[k])


def test_standings_alone_on_synthetic_s(capi, cuda):
    s, L, G = sc_.synthetic_s()
    got = standings(capi, cuda, s, L, G)
    for k, want in zip(("dist", "lap", "rank"), workload.standings(s, L, G)):
        assert sc_.same(got[k], want), k


def test_permuted_race(capi, cuda):
    """The cars of every race listed in another order: the projection and the ranks move with the cars (dist moves
    by a constant per race, with the race's first car)."""
    c = sc_.grid_case(8, 4, 11)
    x = np.stack([c.x[0]] * 5)
    x[1:, :, :2] += np.random.default_rng(12).normal(0, 0.4, (4, c.B, 2)).cumsum(axis=0)
    base = run(capi, cuda, sc_.StandingsCase("base", x, c.wp, 4))
    perm = np.concatenate([g + np.random.default_rng(20 + g).permutation(4) for g in range(0, c.B, 4)])
    pc = sc_.StandingsCase("permuted", x[:, perm], c.wp, 4)
    got = run(capi, cuda, pc)
    pc.check(got)
    for k in ("seg", "s", "lateral"):
        assert sc_.same(got[k], base[k][:, perm]), k
    assert (got["rank"] == base["rank"][:, perm]).all(), "no two cars of a race share a dist here"


def test_host_call_equals_the_device_calls(capi, cuda):
    for c in (sc_.rows_case(9), sc_.group_case(2), sc_.bad_pose_case(4), sc_.tile_case(257)):
        want = run(capi, cuda, c)
        got = capi.race_standings(capi.default_race_config(group_size=c.G), c.x, c.wp)
        for k, w in want.items():
            assert sc_.same(got[k], w), (c.name, k)
        c.check(got)
        part = capi.race_standings(capi.default_race_config(group_size=c.G), c.x, c.wp, seg=False, lateral=False, lap=False)
        assert part["seg"] is None and part["lateral"] is None and part["lap"] is None
        for k in ("s", "dist", "rank"):
            assert sc_.same(part[k], want[k]), (c.name, k)


def test_closed_loop_with_contact(capi, cuda):
    """f110qp_rollout_contact_dev at B = 8, G = 4, T = 12 on make_race_grid(2, 4, seed=11) in make_world, crashed
    cars parking: the standings of its x_traj equal the oracle's, row 0 ranks in grid order, and a car that crashed
    at row k has a constant dist from row k on (if any car crashes: the scene is not built around one)."""
    from test_gpu_rollout import solver
    import rollout_cases as roc_
    from test_gpu_rollout_contact import B, G, N, rollout_contact_dev
    from test_gpu_rollout_replan import P

    x0 = workload.make_race_grid(2, 4, seed=11)
    assert x0.shape[0] == B and G == 4
    case = (x0, np.tile([roc_.V_LIN, 0.0], (B, 1)), workload.make_world(), workload.track_waypoints())
    s = solver(capi, N, x_ref_points=P)
    out = rollout_contact_dev(capi, cuda, s, case, 1)
    s.close()
    c = sc_.StandingsCase("closed loop", out["x_traj"], case[3], G)
    got = run(capi, cuda, c)
    c.check(got)
    assert (got["rank"][0] == np.arange(B) % G).all()
    moved = got["dist"][-1] - got["dist"][0]
    print(f"crash_tick {out['crash_tick']}, dist gained {np.round(moved, 3)}")
    for b in np.flatnonzero(out["crash_tick"] >= 0):
        k = out["crash_tick"][b]
        assert sc_.same(got["dist"][k:, b], np.full(len(got["dist"]) - k, got["dist"][k, b])), f"car {b} parked at {k}"
