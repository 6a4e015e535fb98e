"""The configuration-corner cases (tests/config_corner_cases.py) on the CPU: the reference side of
tests/test_gpu_config_corners.py alone meets what the GPU tests rely on. The oracle certifies every
box QP of every case (and all but at most 2 % of a gap case's), and each case shows what it is for,
read off the oracle's own answer. The zero-width cases have a closed form that needs no solver."""
import numpy as np
import pytest

import config_corner_cases as ccc

CASES = ccc.cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_certifies_every_case(oracle, case):
    """Box rows: no UNCERTIFIED QP and every QP SOLVED. Gap rows: at most 2 % UNCERTIFIED (the cap of
    test_gpu_parity.test_fuzz_configs_against_oracle; the scan seeds were chosen for it), most QPs
    SOLVED, and the box screen has both kinds of QP before it."""
    r = ccc.reference(oracle, case)
    unc = int((r["st"] == oracle.UNCERTIFIED).sum())
    if not case.gap:
        assert unc == 0
        assert (r["st"] == oracle.SOLVED).all(), np.unique(r["st"], return_counts=True)
        return
    assert unc <= max(1, 0.02 * ccc.B_REF), unc
    assert (r["st"] == oracle.SOLVED).mean() > 0.5
    w = r["w"]
    _, xb, sb = oracle.solve_batch(r["prm"], w["x0"], w["u_lin"], w["x_ref"])
    clr = ccc.rows_cleared(w["x0"], xb, r["hs"]) & (sb == oracle.SOLVED)
    assert 0 < clr.sum() < ccc.B_REF, int(clr.sum())


def test_lists_cover_what_the_routes_need():
    """Every family at N = 20 and both dt; zero width, no bound and u_des outside at N = 5 and N = 33;
    a u_des-outside case with u_lin outside the box; a general-frame (q0 != q1) corner."""
    for fam in ccc.FAMILIES:
        for dt in ccc.DTS:
            assert ccc.select(families=[fam], horizons=[20]) and any(c.dt == dt for c in ccc.select(families=[fam], horizons=[20]))
    for N in (5, 33):
        assert {"zero_width", "no_bound", "u_des_outside"} <= {ccc.family(c) for c in ccc.select(horizons=[N])}
    gap = {ccc.family(c) for c in ccc.select(gap=True)}
    assert gap == {"zero_width", "u_des_outside", "no_bound", "weights"}
    assert all(c.N == 20 for c in ccc.select(gap=True))
    below = [c for c in CASES if ccc.member(c) == "below" and not c.gap and c.N == 20][0]
    w, _ = ccc.inputs(below)
    lo, hi, ud = ccc.bounds(below)
    assert (w["u_lin"][:, 0] < lo[0]).all() and (np.abs(w["u_lin"][:, 1]) > hi[1]).any()
    assert ud[0] < lo[0] and ud[1] < lo[1]
    assert any(c.over.get("q", [1, 1])[0] != c.over.get("q", [1, 1])[1] for c in CASES)
    assert len({c.name for c in CASES}) == len(CASES)


def test_smaller_batches_are_the_first_qps(oracle):
    """The routes that run 9, 8 or 1 QPs take the first QPs of the case's 96: same inputs."""
    case = CASES[0]
    r = ccc.reference(oracle, case)
    for B in (9, 8, 1):
        w, _ = ccc.inputs(case, B)
        f = ccc.first(r, B)
        for k in w:
            np.testing.assert_array_equal(w[k], f["w"][k])
        assert f["u"].shape[0] == B


@pytest.mark.parametrize("case", [c for c in CASES if not c.gap], ids=[c.name for c in CASES if not c.gap])
def test_case_shows_what_it_is_for(oracle, case):
    r = ccc.reference(oracle, case)
    u = r["u"]
    lo, hi, ud = ccc.bounds(case)
    on_lo, on_hi, free = ccc.face_counts(case, u)
    fam, mem = ccc.family(case), ccc.member(case)
    n = u.shape[0] * u.shape[1]
    if fam == "zero_width":
        for a in range(2):
            if lo[a] == hi[a]:  # on the bound at every stage of every QP
                assert on_lo[a] == n and on_hi[a] == n
                np.testing.assert_array_equal(u[..., a].astype(np.float32), lo[a])
    elif fam == "u_des_outside":
        # both faces active somewhere in the batch, and some input free
        assert on_lo.sum() > 0 and on_hi.sum() > 0 and free.sum() > 0, (on_lo, on_hi, free)
        assert (ud > hi).all() or (ud < lo).all()
    elif fam == "no_bound":
        dl, dh = ccc.DEFAULT_MIN.astype(np.float64), ccc.DEFAULT_MAX.astype(np.float64)
        assert ((u < dl - 1e-3) | (u > dh + 1e-3)).any()
        if mem.startswith("all"):
            assert on_lo.sum() == 0 and on_hi.sum() == 0
    elif fam == "weights":
        assert on_lo.sum() + on_hi.sum() > 0 and free.sum() > 0, (on_lo, on_hi, free)
    elif fam == "quadrant":
        assert (u >= lo.astype(np.float64) - 1e-9).all() and (u <= hi.astype(np.float64) + 1e-9).all()
        assert on_lo.sum() + on_hi.sum() > 0
        if mem == "steer_positive":
            assert (u[..., 1] >= 0.05 - 1e-7).all()
        if mem == "reverse":
            assert (u[..., 0] < 0).all()
        if mem == "straddle":
            assert lo[0] < 0 < hi[0]


@pytest.mark.parametrize("case", [c for c in CASES if ccc.member(c) == "both" and ccc.family(c) == "zero_width"],
                         ids=lambda c: c.name)
def test_zero_width_on_both_inputs_is_a_closed_form(oracle, case):
    """u_min == u_max on both inputs: the feasible set is one point, so u* is the bound itself, bit
    for bit as float32, and x* the roll-out x_{i+1} = A x_i + B u_i + C of the model linearised at
    (theta0, u_lin) (mpc.cpp:244-248): no solver involved."""
    r = ccc.reference(oracle, case)
    lo, hi, _ = ccc.bounds(case)
    np.testing.assert_array_equal(lo, hi)
    assert (r["st"] == oracle.SOLVED).all()
    np.testing.assert_array_equal(r["u"].astype(np.float32), np.broadcast_to(lo, r["u"].shape))
    w = r["w"]
    ub = lo.astype(np.float64)
    for b in range(0, ccc.B_REF, 7):
        A, Bm, Cm = ccc_linearize(oracle, w, b, case.dt)
        x = w["x0"][b].astype(np.float64)
        np.testing.assert_array_equal(r["x"][b, 0], x)
        for i in range(case.N):
            x = A @ x + Bm @ ub + Cm
            np.testing.assert_allclose(r["x"][b, i + 1], x, rtol=0, atol=1e-9 * max(1.0, np.abs(x).max()))


def ccc_linearize(oracle, w, b, dt):
    return oracle.linearize(float(w["x0"][b, 2]), float(w["u_lin"][b, 0]), float(w["u_lin"][b, 1]), dt)
