"""The CPU oracle and the host mirror against the reference's own compiled tick.

tests/golden/ref_*.npz hold inputs and what oracle/_ref/ref_driver wrote for them: the reference's
unmodified state / input / cost / model / constraints / mpc sources, compiled behind the stand-in
headers of oracle/refshim/ (recorder: tests/golden/make_ref_golden.py). The oracle restates the same
expressions in the same order on the same host libm, so everything is asserted equal, not close
(numerically equal: the sign of a zero is not compared). One exception, named where it applies: the
unqualified cos / sin on a float angle in FindHalfSpaces resolves to the double or to the float
function depending on whether <math.h> is in the include chain, which only roscpp's and Eigen's
own headers could settle; both builds are recorded and each of the oracle's two variants must
equal its build.
"""
import os
import subprocess

import numpy as np
import pytest
import ref_cases as rc
from conftest import GOLDEN, ROOT

QP_KEYS = ("P_colptr", "P_rowind", "P_val", "q", "A_colptr", "A_rowind", "A_val", "l", "u")


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def tick_groups(d):
    for g in d["groups"]:
        name, N, S, pset = str(g).split(":")
        yield name, int(N), int(S), pset


def scans_of(d):
    off = np.r_[0, np.cumsum(d["beams"])]
    return [d["ranges"][off[k]:off[k + 1]] for k in range(len(d["beams"]))]


# ---- freshness: the committed outputs are what the driver writes today ----------------------------

needs_driver = pytest.mark.skipif(not rc.have_driver(), reason="oracle/_ref/ref_driver is not built: the reference "
                                  "checkout is absent (make -C oracle ref)")


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=what)


@needs_driver
def test_fixtures_are_fresh_model_and_halfspace():
    d = load("ref_model")
    o = rc.run_model(d["rows"])
    for k in ("A", "B", "C", "sim"):
        same_bits(o[k], d[k], k)
    r32 = d["rows"].copy()
    r32[:, 3:5] = r32[:, 3:5].astype(np.float32)
    same_bits(rc.run_model(r32)["sim"], d["sim_f32u"], "sim_f32u")
    h = load("ref_halfspace")
    s1, s2 = rc.run_halfspace(h["poses"].astype(np.float32).astype(np.float64), scans_of(h), h["geom"])
    same_bits(s1, h["l1_f32pose"], "l1_f32pose")
    same_bits(s2, h["l2_f32pose"], "l2_f32pose")
    for mathh, suffix in ((False, ""), (True, "_mathh")):
        l1, l2 = rc.run_halfspace(h["poses"], scans_of(h), h["geom"], mathh=mathh)
        same_bits(l1, h["l1" + suffix], "l1" + suffix)
        same_bits(l2, h["l2" + suffix], "l2" + suffix)


@needs_driver
def test_fixtures_are_fresh_tick_and_loop():
    d = load("ref_tick")
    for name, N, S, pset in tick_groups(d):
        for b in range(4):
            calls = [(d[f"{name}_x0"][b, c], d[f"{name}_u_lin"][b, c], d[f"{name}_x_ref"][b, c],
                      d[f"{name}_ranges"][b, c], d[f"{name}_geom"]) for c in range(2)]
            qps = rc.run_tick(N, rc.OVERRIDE_SETS[pset][0], calls)
            for c in range(2):
                for k in QP_KEYS:
                    same_bits(qps[c][k], d[f"{name}_{k}"][b, c], f"{name} {b} {c} {k}")
    lp = load("ref_loop")
    o = rc.run_loop(int(lp["horizon"]), int(lp["ticks"]), lp["x0"], lp["u_lin0"], lp["x_ref"], lp["ranges"], lp["geom"])
    for k in ("x", "u_lin", "plan", "u_applied"):
        same_bits(o[k], lp[k], k)
    same_bits(o["z"], lp["z_oracle"], "z")
    for b in range(4):
        for t in range(int(lp["ticks"])):
            for k in ("q", "A_val", "l", "u"):
                same_bits(o["qp"][b][t][k], lp[k][b, t], f"loop {b} {t} {k}")


# ---- oracle == reference ---------------------------------------------------------------------------

def test_oracle_linearize_equals_reference(oracle):
    d = load("ref_model")
    assert len(d["rows"]) >= 64
    for i, (x, y, ori, v, steer, dt) in enumerate(d["rows"]):
        A, B, C = np.zeros(9), np.zeros(6), np.zeros(3)
        # the C entry point: oracle.linearize() rounds dt to float32, the rows also hold a double 0.01
        oracle.lib().f110o_linearize(ori, v, steer, dt, oracle._ptr(A), oracle._ptr(B), oracle._ptr(C))
        np.testing.assert_array_equal(A.reshape(3, 3), d["A"][i], err_msg=f"A, row {i}")
        np.testing.assert_array_equal(B.reshape(3, 2), d["B"][i], err_msg=f"B, row {i}")
        np.testing.assert_array_equal(C, d["C"][i], err_msg=f"C, row {i}")


def test_oracle_simulate_dynamics_equals_reference(oracle):
    d = load("ref_model")
    for i, (x, y, ori, v, steer, dt) in enumerate(d["rows"]):
        np.testing.assert_array_equal(oracle.simulate_dynamics([x, y, ori], [v, steer], dt), d["sim"][i],
                                      err_msg=f"row {i}")


@pytest.mark.parametrize("float_trig,suffix", [(False, ""), (True, "_mathh")])
def test_oracle_half_spaces_equal_reference(oracle, float_trig, suffix):
    """float_trig=False against the build without <math.h> (cos(float) calls ::cos(double)), True against
    the build with it (the float overload). The gap indices are locals of the reference's function and
    are not recorded (make_ref_golden.py); the rows determine them on these scans."""
    d = load("ref_halfspace")
    th, div, buf = (float(v) for v in d["params"])
    assert d["l1_flipped"].sum() >= 2 and (~d["l1_flipped"]).sum() >= 2
    assert d["l2_flipped"].sum() >= 2 and (~d["l2_flipped"]).sum() >= 2
    for k, r in enumerate(scans_of(d)):
        rcode, l1, l2, lo, hi = oracle.find_half_spaces(d["poses"][k], r, *d["geom"][k], th, div, buf, float_trig=float_trig)
        assert rcode == 0, k
        np.testing.assert_array_equal(l1, d["l1" + suffix][k], err_msg=f"l1, scan {k} ({d['tags'][k]})")
        np.testing.assert_array_equal(l2, d["l2" + suffix][k], err_msg=f"l2, scan {k} ({d['tags'][k]})")


def oracle_tick(oracle, prm, x0, ul, xr, ranges, geom):
    rcode, l1, l2, _, _ = oracle.find_half_spaces(x0, ranges, *geom)
    assert rcode == 0
    return oracle.assemble(prm, x0, ul, xr, np.stack([l1, l2]), gap_active=False)


def test_oracle_assembly_equals_reference(oracle):
    """Both calls of every pair: the first goes through data()->set*, the second through update*, and
    what the solver holds after it equals a fresh assembly at the second inputs. Explicit zeros, the
    stage-0 ones block that UpdateLinearConstraintMatrix never overwrites, the terminal gradient on
    x_ref[N-1] and the float bounds widened to double are all part of the equality."""
    d = load("ref_tick")
    seen = set()
    for name, N, S, pset in tick_groups(d):
        prm = oracle.params(N, **rc.OVERRIDE_SETS[pset][1])
        ns = 3 * (N + 1)
        for b in range(4):
            for c in range(2):
                got = oracle_tick(oracle, prm, d[f"{name}_x0"][b, c], d[f"{name}_u_lin"][b, c], d[f"{name}_x_ref"][b, c],
                                  d[f"{name}_ranges"][b, c], d[f"{name}_geom"])
                for k in QP_KEYS:
                    np.testing.assert_array_equal(got[k], d[f"{name}_{k}"][b, c], err_msg=f"{name} {b} call {c}: {k}")
                A = rc.dense(got["A_colptr"], got["A_rowind"], d[f"{name}_A_val"][b, c], 7 * N + 5, 5 * N + 3)
                np.testing.assert_array_equal(A[ns:ns + 2, :3], np.ones((2, 3)))  # stage-0 block
                assert (d[f"{name}_A_val"][b, c] == 0).sum() == (got["A_val"] == 0).sum() > 0
                # 6 off-diagonal zeros per Q block and 2 per R block are stored, plus every q2 = 0
                assert (d[f"{name}_P_val"][b, c] == 0).sum() == 7 * (N + 1) + 2 * N == (got["P_val"] == 0).sum()
        seen.add((N, S, pset))
    assert {(1, 1, "default"), (2, 2, "default"), (5, 5, "default"), (20, 20, "default"), (30, 30, "default"),
            (20, 26, "default"), (20, 20, "unequal")} <= seen


def test_oracle_solve_equals_captured_optimum_ticks(oracle):
    """oracle.solve against the optimum of the captured matrices (scipy BVLS on them, certified by
    the recorder), at the 1e-8 of test_exact_solve_vs_independent_bvls."""
    d = load("ref_tick")
    active = 0
    for name, N, S, pset in tick_groups(d):
        prm = oracle.params(N, **rc.OVERRIDE_SETS[pset][1])
        for b in range(4):
            for c in range(2):
                r = oracle.solve(prm, d[f"{name}_x0"][b, c], d[f"{name}_u_lin"][b, c], d[f"{name}_x_ref"][b, c])
                assert r["status"] == oracle.SOLVED
                np.testing.assert_allclose(r["z"], d[f"{name}_z_star"][b, c], rtol=0, atol=1e-8, err_msg=f"{name} {b} {c}")
                u = d[f"{name}_z_star"][b, c][3 * (N + 1):].reshape(N, 2)
                active += bool(((u <= np.array(prm.u_min[:])) | (u >= np.array(prm.u_max[:]))).any())
    assert active >= 56 / 3  # not vacuous: an input bound is active in a third of the QPs


def test_oracle_solve_equals_captured_optimum_loop(oracle):
    d = load("ref_loop")
    N = int(d["horizon"])
    prm = oracle.params(N)
    np.testing.assert_allclose(d["z_oracle"], d["z_star"], rtol=0, atol=1e-8)
    for b in range(d["x"].shape[0]):
        for t in range(int(d["ticks"])):
            r = oracle.solve(prm, d["x"][b, t], d["u_lin"][b, t], d["x_ref"][b])
            np.testing.assert_array_equal(r["z"], d["z_oracle"][b, t])
            # The next three lines restate ref_driver.cpp's own glue (next input = plan[1], drive input =
            # float32(plan[0])) and rollout_cases.oracle_loop's: they keep the two models of the callback
            # in step. They pin nothing of the reference: GetNextInput() / inputs_idx_ live in project.cpp,
            # which is not compiled ("not pinned").
            assert d["u_lin"][b, t + 1, 0] == 4.5 and d["u_lin"][b, t + 1, 1] == d["plan"][b, t, 1, 1]
            np.testing.assert_array_equal(d["u_applied"][b, t], d["plan"][b, t, 0].astype(np.float32))
            np.testing.assert_array_equal(oracle.simulate_dynamics(d["x"][b, t], d["u_applied"][b, t], 0.01), d["x"][b, t + 1])
    steer0 = d["z_star"][:2, 0, 3 * (N + 1) + 1::2]
    assert (np.abs(steer0) >= float(np.float32(0.43)) - 1e-12).any(axis=1).all()  # cars 0, 1 start on the steer bound


def test_loop_captured_qps_equal_oracle_assembly(oracle):
    d = load("ref_loop")
    N = int(d["horizon"])
    prm = oracle.params(N)
    for b in range(d["x"].shape[0]):
        for t in range(int(d["ticks"])):
            got = oracle_tick(oracle, prm, d["x"][b, t], d["u_lin"][b, t], d["x_ref"][b], d["ranges"][b], d["geom"])
            for k in ("P_colptr", "P_rowind", "P_val", "A_colptr", "A_rowind"):
                np.testing.assert_array_equal(got[k], d[k])
            for k in ("q", "A_val", "l", "u"):
                np.testing.assert_array_equal(got[k], d[k][b, t], err_msg=f"car {b} tick {t}: {k}")


def test_reference_gap_rows_are_inactive():
    for name in ("ref_tick", "ref_loop"):
        d = load(name)
        assert int(d["gap_rows_active"]) == 0 and "inactive" in str(d["gap_note"])


# ---- host mirror == reference ----------------------------------------------------------------------

def test_host_mirror_equals_reference(tmp_path):
    """f110-mpc_amd/host: Model::Linearize, Model::simulate_dynamics, Constraints::FindHalfSpaces and
    the input bounds Constraints hands to the assembly, on the same fixtures with the same rule. The
    mirror's FindHalfSpaces is f110qp_find_half_spaces (double trig: the build without <math.h>)."""
    host = os.path.join(ROOT, "f110-mpc_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    m, h, tk = load("ref_model"), load("ref_halfspace"), load("ref_tick")
    scans = scans_of(h)
    v = [np.array([float(len(m["rows"]))]), m["rows"].ravel(), np.array([float(len(scans))])]
    for p, r, g in zip(h["poses"], scans, h["geom"]):
        v += [p, rc.pack_scan(r, g)]
    np.concatenate(v).astype(np.float64).tofile(tmp_path / "in.f64")
    subprocess.check_call([os.path.join(host, "bin", "host_demo"), "ref", rc.PARAMS_YAML, str(tmp_path / "in.f64"),
                           str(tmp_path / "out.f64")])
    o = np.fromfile(tmp_path / "out.f64", np.float64)
    n, k = len(m["rows"]), len(scans)
    mo = o[:21 * n].reshape(n, 21)
    np.testing.assert_array_equal(mo[:, :9].reshape(n, 3, 3), m["A"])
    np.testing.assert_array_equal(mo[:, 9:15].reshape(n, 3, 2), m["B"])
    np.testing.assert_array_equal(mo[:, 15:18], m["C"])
    np.testing.assert_array_equal(mo[:, 18:21], m["sim"])
    ho = o[21 * n:21 * n + 7 * k].reshape(k, 7)
    assert (ho[:, 0] == 1).all()
    np.testing.assert_array_equal(ho[:, 1:4], h["l1"])
    np.testing.assert_array_equal(ho[:, 4:7], h["l2"])
    N = 20
    np.testing.assert_array_equal(np.tile(o[-4:-2], N), tk["n20_l"][0, 0][-2 * N:])
    np.testing.assert_array_equal(np.tile(o[-2:], N), tk["n20_u"][0, 0][-2 * N:])
