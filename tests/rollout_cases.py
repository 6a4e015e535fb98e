"""Inputs and CPU references of the closed-loop rollout tests (test_gpu_rollout.py), and the CPU check
that chose the gap-row seed:  python tests/rollout_cases.py [first_seed [count]]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "f110-mpc_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_gpu_dbl import dbl_batch  # noqa: E402
from test_gpu_parity import halfspaces_oracle  # noqa: E402

from f110qp import workload  # noqa: E402

PLANT_DT, CAR_LENGTH, V_LIN, FAIL_U = 0.01, 0.35, 4.5, (0.5, 0.0)
GAP_SEED = 2  # chosen by choose_gap_seed() below


def start(B, N, seed, P=None):
    """float64 (x0, u_lin, x_ref): a workload.make_batch batch with sub-float32-ulp offsets, as
    test_gpu_dbl.dbl_batch builds it (no shift: the cars start within 50 m of the origin)."""
    return dbl_batch(B, N, seed, 0.0, P)


def plant_step(x, u, dt=PLANT_DT, L=CAR_LENGTH):
    """x + dt (v cos(ori), v sin(ori), tan(steer) v / L) in numpy fp64 (src/model.cpp:67-71): x [B,3]
    float64, u [B,2] the applied input (float32 values or the fallback)."""
    x = np.asarray(x, np.float64)
    v, d = np.asarray(u[:, 0], np.float64), np.asarray(u[:, 1], np.float64)
    dyn = np.stack([v * np.cos(x[:, 2]), v * np.sin(x[:, 2]), np.tan(d) * v / L], 1)
    return x + dyn * dt


def gap_case(oracle, seed, B=64, N=20):
    """Start of the gap-row case: (x0, u_lin, x_ref, hs) with the half-spaces of a workload.make_scans
    scan at the tick-0 states, from the oracle, stored as float32."""
    x0, ul, xr = start(B, N, seed)
    ranges, amin, ainc, amax = workload.make_scans(B, seed=seed + 2)
    return x0, ul, xr, halfspaces_oracle(oracle, x0, ranges, (amin, ainc, amax))


def oracle_loop(oracle, x0, ul, xr, hs, N, T, gap):
    """The closed loop with the oracle as its solver and the numpy plant, u rounded to float32 as the
    device applies it. Returns the per-tick start states [T,B,3], inputs [T,B,2], statuses [T,B]."""
    prm = oracle.params(N)
    B = x0.shape[0]
    xs, uls, sts = np.zeros((T, B, 3)), np.zeros((T, B, 2)), np.zeros((T, B), np.int32)
    x, u_lin = x0.copy(), ul.copy()
    for t in range(T):
        xs[t], uls[t] = x, u_lin
        ua = np.zeros((B, 2))
        nxt = np.zeros(B)
        for b in range(B):
            r = oracle.solve(prm, x[b], u_lin[b], xr[b, :N], None if hs is None else hs[b], gap)
            sts[t, b] = r["status"]
            if r["status"] == oracle.SOLVED:
                u32 = r["u"].astype(np.float32)
                ua[b], nxt[b] = u32[0], u32[1 if N > 1 else 0, 1]
            else:
                ua[b], nxt[b] = FAIL_U, FAIL_U[1]
        x = plant_step(x, ua)
        u_lin = np.stack([np.full(B, V_LIN), nxt], 1)
    return xs, uls, sts


def gap_seed_is_robust(oracle, seed, B=64, N=20, T=4, eps=1e-6):
    """No (car, tick) of the oracle-driven loop changes oracle status when its x0 moves by +-eps in
    any coordinate (nor is one left uncertified), and at least half of the pairs are SOLVED."""
    x0, ul, xr, hs = gap_case(oracle, seed, B, N)
    xs, uls, sts = oracle_loop(oracle, x0, ul, xr, hs, N, T, True)
    if (sts == oracle.UNCERTIFIED).any() or (sts == oracle.SOLVED).mean() < 0.5:
        return False, sts
    prm = oracle.params(N)
    for t in range(T):
        for b in range(B):
            for k in range(3):
                for sgn in (-eps, eps):
                    x = xs[t, b].copy()
                    x[k] += sgn
                    if oracle.solve(prm, x, uls[t, b], xr[b, :N], hs[b], True)["status"] != sts[t, b]:
                        return False, sts
    return True, sts


def choose_gap_seed(first=1, count=20):
    import oracle

    oracle.build()
    for seed in range(first, first + count):
        ok, sts = gap_seed_is_robust(oracle, seed)
        vals, n = np.unique(sts, return_counts=True)
        print(f"seed {seed}: robust={ok} statuses {dict(zip(vals.tolist(), n.tolist()))}", flush=True)
        if ok and (sts != oracle.SOLVED).any():  # a seed that also takes the failure branch
            return seed
    return None


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    print("chosen:", choose_gap_seed(*a))
