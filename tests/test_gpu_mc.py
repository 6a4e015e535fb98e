"""The Monte Carlo kernels on MI355X (f110qp_mc_fan_dev, f110qp_mc_survival_dev, f110qp_mc_outcomes_dev,
f110qp_mc_summary; include/f110qp.h "Monte Carlo outcomes") against the numpy oracle, bit for bit on every output:
set sizes on both sides of the wave / LDS switch and of every padding, strides, rows past the grid caps, sets
packed unevenly into waves, special values and NaN shares, the probabilities' edge cases, optional outputs, the
host-pointer call, and one noisy closed loop. Every case is built in mc_cases.py (test_mc_cases.py holds the oracle
to the model on the CPU)."""
import mc_cases as mc_
import numpy as np
import pytest
from test_gpu_rollout_replan import dev

from f110qp import workload

pytestmark = pytest.mark.gpu


def fan(capi, cuda, c, count=True, v=None):
    """f110qp_mc_fan_dev on a case -> dict of fan and count (None when left out)."""
    import torch

    out = torch.full((c.rows, c.K, c.Q), -7.0, dtype=torch.float64, device=cuda)
    n = torch.full((c.rows, c.K), -7, dtype=torch.int32, device=cuda) if count else None
    mc = capi.default_mc_config(hypotheses=c.M, group_size=c.G, prob=c.prob)
    capi.mc_fan_dev(mc, dev(cuda, c.v if v is None else v), out, n)
    torch.cuda.synchronize(cuda)
    return dict(fan=out.cpu().numpy(), count=n.cpu().numpy() if count else None)


def survival(capi, cuda, c, crashed=True):
    import torch

    alive = torch.full((c.T + 1, c.K), -7, dtype=torch.int32, device=cuda)
    hit = torch.full((c.K,), -7, dtype=torch.int32, device=cuda) if crashed else None
    capi.mc_survival_dev(capi.default_mc_config(hypotheses=c.M, group_size=c.G), dev(cuda, c.crash), c.T, alive, hit)
    torch.cuda.synchronize(cuda)
    return dict(alive=alive.cpu().numpy(), crashed=hit.cpu().numpy() if crashed else None)


RECORDS = ("min_row", "unsolved", "first_unsolved", "plan_failed")


def outcomes(capi, cuda, c, status=True, kind=True, leave=()):
    """f110qp_mc_outcomes_dev on a case; leave: optional outputs not given."""
    import torch

    want = [k for k in RECORDS if k not in leave and (status or k not in ("unsolved", "first_unsolved"))
            and (kind or k != "plan_failed")]
    o = {k: torch.full((c.B,), -7, dtype=torch.int32, device=cuda) for k in want}
    mn = torch.full((c.B,), -7.0, dtype=torch.float64, device=cuda)
    capi.mc_outcomes_dev(dev(cuda, c.clear), mn, dev(cuda, c.status) if status else None,
                         dev(cuda, c.kind) if kind else None, **o)
    torch.cuda.synchronize(cuda)
    return dict(min_clear=mn.cpu().numpy(), **{k: v.cpu().numpy() for k, v in o.items()})


@pytest.mark.parametrize("M", mc_.SET_SIZES)
def test_set_sizes(capi, cuda, M):
    c = mc_.size_case(M)
    c.check(fan(capi, cuda, c))


@pytest.mark.parametrize("G,M", mc_.STRIDES)
def test_strides(capi, cuda, G, M):
    c = mc_.stride_case(G, M)
    got = fan(capi, cuda, c)
    c.check(got)
    r, k = c.rows - 1, c.K - 1
    assert got["fan"][r, k, 0] == 1e6 * r + 1e4 * (k // G) + k % G, "the last set's minimum names its (r, s, g)"


@pytest.mark.parametrize("rows", mc_.ROWS)
def test_rows(capi, cuda, rows):
    c = mc_.rows_case(rows)
    c.check(fan(capi, cuda, c))
    if rows == 1:  # one row given as [B]
        c.check(fan(capi, cuda, c, v=c.v[0]), "one row")


@pytest.mark.parametrize("i", [0, 1])
def test_past_the_grid_cap(capi, cuda, i):
    """rows x K past mc_fan_grid's cap of the wave path (0) and of the LDS path (1): the first take a second item."""
    c = mc_.grid_cases()[i]
    c.check(fan(capi, cuda, c))


def test_sets_packed_unevenly_into_waves(capi, cuda):
    for c in mc_.packing_cases():
        c.check(fan(capi, cuda, c))


@pytest.mark.parametrize("M", [13, 100])
def test_values_and_nan_shares(capi, cuda, M):
    c = mc_.value_case(M)
    got = fan(capi, cuda, c)
    c.check(got)
    assert mc_.same(got["fan"][:, 0], got["fan"][:, 1]), "a shuffled set has the same fan"
    assert got["count"][-2:].tolist() == [[1, 1], [0, 0]]
    assert (got["fan"][-1].view(np.uint64) == 0x7FF8000000000000).all(), "n = 0"
    assert (got["fan"][-2].view(np.uint64) == 0x8000000000000000).all(), "the one sample, a -0, at every quantile"
    part = fan(capi, cuda, c, count=False)
    assert part["count"] is None and mc_.same(part["fan"], got["fan"]), "count given and NULL: the same fan"


def test_probabilities(capi, cuda):
    for c in mc_.prob_cases():
        c.check(fan(capi, cuda, c))
    # entries of prob past num_probs are not read
    import torch

    c = mc_.prob_cases()[0]
    out = torch.full((c.rows, c.K, 1), -7.0, dtype=torch.float64, device=cuda)
    capi.mc_fan_dev(capi.default_mc_config(hypotheses=c.M, prob=(0.5, 7.0, float("nan")), num_probs=1), dev(cuda, c.v), out)
    torch.cuda.synchronize(cuda)
    c.check(dict(fan=out.cpu().numpy()))


@pytest.mark.parametrize("M,G", mc_.SURVIVAL)
def test_survival(capi, cuda, M, G):
    c = mc_.survival_case(M, G)
    got = survival(capi, cuda, c)
    c.check(got)
    part = survival(capi, cuda, c, crashed=False)
    assert part["crashed"] is None and mc_.same(part["alive"], got["alive"])
    assert (got["alive"][-1] + got["crashed"] == M).all(), "after row T a member is alive or crashed"


@pytest.mark.parametrize("i", range(len(mc_.OUTCOME_TICKS) + 1))
def test_car_records(capi, cuda, i):
    c = mc_.outcomes_cases()[i]
    full = outcomes(capi, cuda, c)
    c.check(full)
    assert set(full) == {"min_clear", *RECORDS}
    no_kind = outcomes(capi, cuda, c, kind=False)
    c.check(no_kind, with_kind=False)
    assert "plan_failed" not in no_kind and no_kind["unsolved"][6] == c.T and full["unsolved"][6] == 0
    c.check(outcomes(capi, cuda, c, status=False))
    alone = outcomes(capi, cuda, c, status=False, kind=False)
    assert set(alone) == {"min_clear", "min_row"}
    c.check(alone)
    for k in RECORDS:  # each optional output left out: the others keep their bits
        part = outcomes(capi, cuda, c, leave=(k,))
        assert k not in part
        c.check(part)


def test_host_call_equals_the_device_calls(capi, cuda):
    """f110qp_mc_summary on the arrays of two record cases, in the layouts (M, G) = (5, 2) and (35, 1) (B = 70),
    with crash ticks of a survival case."""
    for c, M, G in ((mc_.outcomes_cases()[1], 5, 2), (mc_.outcomes_cases()[0], 35, 1), (mc_.outcomes_cases()[2], 100, 3)):
        crash = mc_.survival_case(M, G, T=c.T, S=c.B // (M * G)).crash
        fc = mc_.FanCase(c.name, c.clear, M, G)
        sv = mc_.SurvivalCase(c.name, crash, c.T, M, G)
        want = {**fan(capi, cuda, fc), **survival(capi, cuda, sv), **outcomes(capi, cuda, c)}
        got = capi.mc_summary(capi.default_mc_config(hypotheses=M, group_size=G, prob=fc.prob), c.clear, crash, c.status,
                              c.kind)
        for k, w in want.items():
            assert mc_.same(got[k], w), (c.name, k)
        fc.check(got)
        sv.check(got)
        c.check(got)
        part = capi.mc_summary(capi.default_mc_config(hypotheses=M, group_size=G, prob=fc.prob), c.clear, crash,
                               count=False, crashed=False, min_row=False)
        assert all(part[k] is None for k in ("count", "crashed", "min_row", "unsolved", "first_unsolved", "plan_failed"))
        for k in ("fan", "alive", "min_clear"):
            assert mc_.same(part[k], want[k]), (c.name, k)


def test_closed_loop(capi, cuda):
    """f110qp_rollout_noisy_dev on the scene of test_gpu_rollout_noisy.py, the starts one race tiled to S = 1, M = 4,
    G = 2: the fan, the survival and the records of its arrays equal the oracle's; with the all-zero noise config
    the four hypotheses are the same bits, so every fan is flat and every alive entry is 0 or M."""
    from test_gpu_rollout import solver
    from test_gpu_rollout_noisy import noise_of, rollout_noisy_dev
    from test_gpu_rollout_replan import P
    from test_gpu_rollout_walls import B, G, N, T, scene

    M = 4
    x0, ul, circles, sg, wp = scene()
    assert B == M * G and x0.shape[0] == B
    case = (workload.make_mc_batch(x0[:G], M, G), workload.make_mc_batch(ul[:G], M, G), circles, sg, wp)
    s = solver(capi, N, gap=True, x_ref_points=P)
    loud = rollout_noisy_dev(capi, cuda, s, case, 1, 1, noise_of(capi))
    quiet = rollout_noisy_dev(capi, cuda, s, case, 1, 1, capi.default_noise_config())
    s.close()
    mc = capi.default_mc_config(hypotheses=M, group_size=G, prob=mc_.PROB)
    for name, a in (("noisy", loud), ("zero noise", quiet)):
        fc = mc_.FanCase(name, a["clear_traj"], M, G)
        sv = mc_.SurvivalCase(name, a["crash_tick"], T, M, G)
        oc = mc_.OutcomesCase(name, a["clear_traj"], a["status"], a["kind"])
        got = {**fan(capi, cuda, fc), **survival(capi, cuda, sv), **outcomes(capi, cuda, oc)}
        fc.check(got)
        sv.check(got)
        oc.check(got)
        host = capi.mc_summary(mc, a["clear_traj"], a["crash_tick"], a["status"], a["kind"])
        for k, w in got.items():
            assert mc_.same(host[k], w), (name, k)
        print(f"{name}: crash_tick {a['crash_tick']}, alive at T {got['alive'][-1]}, min_clear {np.round(got['min_clear'], 3)}")
    fq = fan(capi, cuda, mc_.FanCase("zero noise", quiet["clear_traj"], M, G))
    assert mc_.same(fq["fan"][..., 0], fq["fan"][..., -1]), "zero noise: the hypotheses are the same bits"
    alive = survival(capi, cuda, mc_.SurvivalCase("zero noise", quiet["crash_tick"], T, M, G))["alive"]
    assert np.isin(alive, (0, M)).all(), alive
