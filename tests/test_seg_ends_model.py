"""The two-sided segment-end elimination (tests/diag_seg_ends_model.py, the numpy model of step 2 of
csrc/lane_seg_kernel.h's pass at S <= 4) against a dense fp64 solve of the same S-segment boundary
system and against the one-sided ring it replaces, on the CPU.

Bound: the two-sided result's relative difference to the dense solve is no larger than 4 x the
ring's on the same inputs. Both figures are the worst over the same set of inputs (one input alone
can land on the dense solve's own rounding, where a ratio of two such accidents says nothing); the
whole pass (forward sweep from the segment ends against the sequential Riccati) is held to the same
4 x. The mutual difference follows from the two by the triangle inequality (<= 5 x the ring's).

Measured (200 inputs of each kind per S, `python tests/diag_seg_ends_model.py`), two-sided / ring:
  S = 2: random data 2.5e-13 / 7.0e-13, backward-sweep data 8.9e-16 / 1.5e-15, whole pass 1.3e-15 / 1.1e-15
  S = 4: random data 1.0e-13 / 2.0e-12, backward-sweep data 2.8e-15 / 2.8e-15, whole pass 1.2e-15 / 1.2e-15
  S = 8: random data 2.0e-12 / 5.8e-11, backward-sweep data 7.9e-15 / 7.9e-15, whole pass 1.6e-15 / 1.3e-15
(the ring's whole-pass figure over diag_segment_riccati_model.py's own 300 problems is 1.8e-15).
The random data are ill-conditioned on purpose (P up to 10 |A A'|, Phi up to I + 0.7 randn): the
error there is the conditioning of the boundary system, and the shorter chain carries less of it.
"""
import numpy as np
import pytest

import diag_seg_ends_model as model

TRIALS = 200


@pytest.fixture(scope="module", params=[2, 4, 8])
def measured(request):
    S = request.param
    r = model.measure(S, trials=TRIALS)
    print(f"S = {S}: {r}")
    return S, r


@pytest.mark.parametrize("kind", ["rand", "sweep", "whole"])
def test_two_sided_within_four_times_the_ring(measured, kind):
    """rand / sweep: against the dense solve; whole: the pass's (u, x) against the sequential Riccati."""
    S, r = measured
    two, ring = r[kind]
    print(f"S = {S} {kind}: two-sided {two:.3e}, ring {ring:.3e}")
    assert ring > 0.0 and ring < 1e-9  # the inputs exercise the recursion and the ring solves them
    assert two <= 4.0 * ring


def test_two_sided_against_the_ring(measured):
    S, r = measured
    worst_ring = max(r["rand"][1], r["sweep"][1])
    print(f"S = {S}: two-sided against ring {r['mutual']:.3e}, ring against dense {worst_ring:.3e}")
    assert r["mutual"] <= 5.0 * worst_ring


@pytest.mark.parametrize("S", [2, 4, 8])
def test_boundary_lanes_and_structure(S):
    """Segment 0 starts at x = 0, the top segment carries lam = 0, and the result satisfies both
    coupling equations of every segment to rounding."""
    rng = np.random.default_rng(77 + S)
    for _ in range(20):
        seg = model.random_segments(rng, S)
        x, lam = model.two_sided(seg)
        assert (x[0] == 0.0).all() and (lam[S - 1] == 0.0).all()
        scale = max(1.0, np.abs(x).max(), np.abs(lam).max())
        for j in range(S - 1):
            res = x[j + 1] - (seg[j]["Phi"] @ x[j] + seg[j]["psi"] + seg[j]["Gam"] @ lam[j])
            assert np.abs(res).max() <= 1e-9 * scale
        for j in range(1, S):
            res = lam[j - 1] - (seg[j]["P"] @ x[j] + seg[j]["a"] + seg[j]["Phi"].T @ lam[j])
            assert np.abs(res).max() <= 1e-9 * scale


def test_lower_side_is_the_exchanged_upper_step():
    """The lower side's recursion written out (Z~ = I - beta P, ...) equals the shared step on the
    exchanged operands, and beta stays symmetric negative semidefinite."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        seg = model.random_segments(rng, 3)
        be, al = seg[0]["Gam"], seg[0]["psi"]
        for sj in seg[1:]:
            Zi = np.linalg.inv(np.eye(3) - be @ sj["P"])
            Yt = Zi @ be
            Tt, tt = Yt @ sj["Phi"].T, Yt @ sj["a"] + Zi @ al
            be_n, al_n = sj["Gam"] + sj["Phi"] @ Tt, sj["psi"] + sj["Phi"] @ tt
            T, t, M, m = model.step(be, al, *model.ops(sj, True))
            for got, want in ((T, Tt), (t, tt), (M, be_n), (m, al_n)):
                assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
            assert np.abs(M - M.T).max() <= 1e-10 * max(1.0, np.abs(M).max())
            assert np.linalg.eigvalsh(0.5 * (M + M.T)).max() <= 1e-10 * max(1.0, np.abs(M).max())
            be, al = M, m
