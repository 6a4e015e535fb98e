"""The Monte Carlo oracle (workload.mc_keys, mc_fan, mc_survival, mc_outcomes, make_mc_batch) held to the model of
include/f110qp.h without a GPU, by a second formulation of each rule: np.sort of the values where a set holds
neither NaN nor signed zeros, a brute-force count for the survival, a Python loop for the car records; and the
key order, the NaN rule and the n = 0 answer asserted on their own. The cases are the ones test_gpu_mc.py runs."""
import math

import mc_cases as mc_
import numpy as np
import pytest

from f110qp import workload


def test_key_order_and_round_trip():
    v = np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf])
    key = workload.mc_keys(v)
    assert key.dtype == np.uint64 and (key[1:] > key[:-1]).all(), "a strict total order, -0 below +0"
    assert mc_.same(workload.mc_values(key), v), "a key gives back the value's own bits"
    u = v.view(np.uint64)
    want = [(~int(b)) & (2 ** 64 - 1) if int(b) >> 63 else int(b) | 1 << 63 for b in u]
    assert [int(k) for k in key] == want, "rule M1 word for word"
    assert (key != workload.MC_PAD_KEY).all(), "no number maps to the pad key"


def test_both_nan_signs_are_dropped_and_the_empty_set():
    nans = np.array([mc_.NAN_POS, mc_.NAN_NEG, mc_.NAN_PAYLOAD, mc_.NAN_NEG_PAYLOAD])
    assert np.isnan(nans).all() and (workload.mc_keys(nans) == workload.MC_PAD_KEY).all()
    fan, n = workload.mc_fan(np.array([3.0, mc_.NAN_NEG, -2.0, mc_.NAN_POS, mc_.NAN_PAYLOAD]), 5, 1, (0.0, 0.5, 1.0))
    assert n.tolist() == [2] and fan.tolist() == [[-2.0, -2.0, 3.0]]
    fan, n = workload.mc_fan(nans, 4, 1, (0.0, 0.5, 1.0))
    assert n.tolist() == [0] and (fan.view(np.uint64) == 0x7FF8000000000000).all(), "n = 0: the one NaN"
    fan, n = workload.mc_fan(np.array([0.0, -0.0, 0.0, -0.0]), 4, 1, (0.0, 0.34, 0.67, 1.0))
    assert n.tolist() == [4] and np.signbit(fan[0]).tolist() == [True, True, False, False], "a -0 stays a -0"


@pytest.mark.parametrize("c", mc_.fan_cases(), ids=lambda c: c.name)
def test_fan_is_the_sorted_values_indexed(c):
    """Per set, read off the layout's formula: without NaN and zeros np.sort of the doubles is the ascending
    order; with them the order is built from Python's own comparison with the sign of a zero as the tie-break."""
    o = c.oracle()
    assert o["fan"].shape == (c.rows, c.K, c.Q) and o["count"].shape == (c.rows, c.K)
    step = max(1, (c.rows * c.K) // 400)  # every set of a small case, a spread of a large one
    for i in range(0, c.rows * c.K, step):
        r, k = divmod(i, c.K)
        vals = mc_.members(c, r, k)
        num = vals[~np.isnan(vals)]
        n = len(num)
        assert o["count"][r, k] == n
        if n == 0:
            assert (o["fan"][r, k].view(np.uint64) == 0x7FF8000000000000).all()
            continue
        if (num == 0).any():
            order = np.array(sorted(num.tolist(), key=lambda x: (x, 0 if math.copysign(1.0, x) < 0 else 1)))
        else:
            order = np.sort(num)
        want = np.array([order[int(math.floor(p * float(n - 1)))] for p in c.prob])
        assert mc_.same(o["fan"][r, k], want), (c.name, r, k)


def test_stride_cases_name_their_set():
    for G, M in mc_.STRIDES:
        c = mc_.stride_case(G, M)
        fan = c.oracle()["fan"]
        for r in range(c.rows):
            for k in range(c.K):
                s, g = divmod(k, c.G)
                assert fan[r, k, 0] == 1e6 * r + 1e4 * s + g and fan[r, k, 2] == fan[r, k, 0] + 10.0 * (M - 1)


def test_value_case_shuffled_situation_has_the_same_fan():
    for M in (13, 100):
        o = mc_.value_case(M).oracle()
        assert mc_.same(o["fan"][:, 0], o["fan"][:, 1]) and (o["count"][:, 0] == o["count"][:, 1]).all()
        assert o["count"][:, 0].tolist() == [M] * 6 + [M - max(1, M // 3), 1, 0]


@pytest.mark.parametrize("c", mc_.survival_cases(), ids=lambda c: c.name)
def test_survival_is_a_count(c):
    o = c.oracle()
    assert o["alive"].shape == (c.T + 1, c.K) and o["crashed"].shape == (c.K,)
    for k in range(c.K):
        s, g = divmod(k, c.G)
        ct = [int(c.crash[(s * c.M + m) * c.G + g]) for m in range(c.M)]
        assert o["crashed"][k] == sum(1 for t in ct if 0 <= t <= c.T)
        for r in range(c.T + 1):
            assert o["alive"][r, k] == sum(1 for t in ct if t < 0 or t > r)
    assert set(c.crash.tolist()) >= {-1, 0, c.T, c.T + 1, np.iinfo(np.int32).max}


@pytest.mark.parametrize("c", mc_.outcomes_cases(), ids=lambda c: c.name)
@pytest.mark.parametrize("with_kind", [True, False])
def test_records_by_a_loop(c, with_kind):
    o = c.oracle(with_kind)
    assert ("plan_failed" in o) == with_kind
    for b in range(c.B):
        best, idx = math.inf, -1
        for r in range(c.T + 1):
            v = float(c.clear[r, b])
            if v < best or (v == best and r < idx):
                best, idx = v, r
        assert o["min_clear"][b] == best and o["min_row"][b] == idx
        bad = [t for t in range(c.T) if (not with_kind or c.kind[t, b] == mc_.TICK_MPC)
               and c.status[t, b] not in (mc_.SOLVED, mc_.SOLVED_INACCURATE)]
        assert o["unsolved"][b] == len(bad) and o["first_unsolved"][b] == (bad[0] if bad else -1)
        if with_kind:
            assert o["plan_failed"][b] == sum(1 for t in range(c.T) if c.kind[t, b] == mc_.TICK_PLAN_FAILED)
    assert o["min_row"][1] == 0 and o["min_row"][2] == -1 and o["min_row"][3] == -1 and o["min_row"][4] == 0
    assert o["min_clear"][2] == np.inf and not np.signbit(o["min_clear"][4])
    assert o["unsolved"][5] == 0 and o["unsolved"][7] == c.T and o["first_unsolved"][7] == 0
    assert o["unsolved"][6] == (0 if with_kind else c.T)


def test_make_mc_batch_layout():
    x0 = np.arange(18.0).reshape(6, 3)  # S = 3 situations of G = 2 cars
    x = workload.make_mc_batch(x0, 4, 2)
    assert x.shape == (24, 3)
    for s in range(3):
        for m in range(4):
            for g in range(2):
                assert (x[(s * 4 + m) * 2 + g] == x0[s * 2 + g]).all()
    assert (workload.make_mc_batch(x0, 1, 2) == x0).all()
    with pytest.raises(ValueError):
        workload.make_mc_batch(x0, 2, 4)
    with pytest.raises(ValueError):
        workload.mc_fan(np.zeros(6), 4, 1, (0.5,))
    with pytest.raises(ValueError):
        workload.mc_fan(np.zeros(6), 3, 1, (1.5,))
