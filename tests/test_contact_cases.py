"""The contact model's numpy oracle (workload.clearance) on the CPU: its own properties, and that every case
the GPU tests compare with it stays inside the cap on poses that may skip the nearest comparison
(contact_cases' module docstring)."""
import contact_cases as cc_
import numpy as np
import pytest
import world_cases as wc_

from f110qp import workload

CASES = cc_.oracle_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_stay_inside_the_skip_cap(case):
    sk = case.skip()
    assert sk.shape == (case.rows, case.B)
    assert sk.sum() <= wc_.SKIP_CAP * sk.size, (case.name, int(sk.sum()), sk.size)
    clear, near = case.oracle()
    assert clear.shape == sk.shape and near.dtype == np.int32
    # the oracle against the candidate values computed one by one
    v = case.all_values()
    if v.shape[2]:
        assert (clear.view(np.int64) == v.min(axis=2).view(np.int64)).all()
    assert 1e-16 < case.tol < 1e-12  # the derived bound at these coordinates


def test_bound_is_the_derived_formula():
    assert cc_.abs_tol(20.0) == 2.0 ** -52 * (4 * 0.1651 + 400.0)
    assert cc_.abs_tol(20.0, 0.0) == 2.0 ** -52 * 400.0


def test_mate_symmetry_bit_for_bit():
    """Car a against b and b against a: the squares are the same bits. Pairs with nothing else around."""
    x = cc_.poses(6, 2, 5) * [4.0, 4.0, 1.0]
    clear, near = workload.clearance(x, None, 2)
    assert (clear[:, 0].view(np.int64) == clear[:, 1].view(np.int64)).all()
    assert (near[:, 0] == 1).all() and (near[:, 1] == 0).all()


def test_order_independence():
    c = cc_.random_case(False)
    clear, near = c.oracle()
    perm = np.random.default_rng(3).permutation(c.C)
    clear_p, near_p = workload.clearance(c.x, c.circles[perm], c.G, c.R, c.off)
    assert (clear.view(np.int64) == clear_p.view(np.int64)).all()
    static = near < c.C
    assert (perm[near_p[static]] == near[static]).all() and (near_p[~static] == near[~static]).all()
    # the race's cars permuted inside each race: each car keeps its clearance bits
    rp = np.concatenate([g * c.G + np.random.default_rng(4 + g).permutation(c.G) for g in range(c.B // c.G)])
    clear_r, _ = workload.clearance(c.x[:, rp], c.circles, c.G, c.R, c.off)
    assert (clear_r.view(np.int64) == clear[:, rp].view(np.int64)).all()


def test_two_cars_in_line():
    """Two cars 1.5 m apart in line at yaw 0 and center_offset 0: exactly 1.5 - 2 R. With R = 0.25 every value
    is a binary fraction and the statement holds as written; with the default 0.3 (no binary fraction) the
    model's own order of operations, (1.5 - R) - R, is the exact statement: 1.5 - 2 R rounds once, not twice."""
    x = np.array([[0.25, -1.0, 0.0], [1.75, -1.0, 0.0]])
    clear, near = workload.clearance(x, None, 2, 0.25, 0.0)
    assert (clear == 1.5 - 2 * 0.25).all() and near.tolist() == [1, 0]
    clear, near = workload.clearance(x, None, 2, 0.3, 0.0)
    assert (clear == (1.5 - 0.3) - 0.3).all() and abs(clear[0] - (1.5 - 2 * 0.3)) <= 2.0 ** -52 and near.tolist() == [1, 0]


def test_nothing_to_touch():
    clear, near = workload.clearance(np.zeros((2, 3, 3)), None, 1)
    assert np.isposinf(clear).all() and (near == -1).all() and clear.shape == (2, 3)
    clear, near = workload.clearance(np.zeros((3, 3)), np.zeros((0, 3)), 1)
    assert np.isposinf(clear).all() and (near == -1).all() and clear.shape == (3,)


def test_odd_inputs():
    x = np.array([[0.0, 0.0, 0.3], [np.nan, 0.0, 0.0]])
    ci = np.array([[np.nan, 1.0, 0.1], [1.0, np.inf, 0.1], [2.0, 0.0, -0.5], [2.0, 0.0, 0.5], [3.0, 0.0, np.nan]])
    clear, near = workload.clearance(x, ci, 1)
    assert near.tolist() == [2, -1] and np.isposinf(clear[1])  # the tie of circles 2 and 3: the lower index
    pos, _ = workload.clearance(x, ci[3:4], 1)
    assert clear[0] == pos[0]
