"""Running oracle/_ref/ref_driver (the reference's own compiled tick, see oracle/ref_driver.cpp) and
reading what it writes. Shared by the recorder of tests/golden/ref_*.npz (tests/golden/
make_ref_golden.py) and by the freshness test of tests/test_reference_parity.py. The numpy helpers at
the end (dense, condense_captured, z_star) need no driver; tests/test_gpu_reference.py uses them too."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
DRIVER = os.path.join(REF_DIR, "ref_driver")
DRIVER_MATHH = os.path.join(REF_DIR, "ref_driver_mathh")  # <math.h> in the include chain
PARAMS_YAML = os.path.join(ROOT, "f110-mpc_amd", "config", "params.yaml")

# the parameter sets of the tick fixtures: overrides of params.yaml, as the driver's key=value
# arguments and as oracle.params(...) keywords
OVERRIDE_SETS = {
    "default": ({}, {}),
    "unequal": (dict(q0=3.0, q1=25.0, q2=0.0, r0=0.7, r1=2.0, dt=0.05),
                dict(q=(3.0, 25.0, 0.0), r=(0.7, 2.0), dt=np.float32(0.05))),
}


def have_driver():
    return os.path.exists(DRIVER) and os.path.exists(DRIVER_MATHH)


def run_driver(mode, values, overrides=None, mathh=False):
    """One driver process: `values` (flat float64) in, the flat float64 it writes out."""
    args = [f"{k}={v!r}" if isinstance(v, float) else f"{k}={v}" for k, v in (overrides or {}).items()]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.f64"), os.path.join(tmp, "out.f64")
        np.ascontiguousarray(values, np.float64).tofile(fin)
        subprocess.check_call([DRIVER_MATHH if mathh else DRIVER, mode, fin, fout, PARAMS_YAML] + args)
        return np.fromfile(fout, np.float64)


def pack_scan(ranges, geom):
    amin, ainc, amax = geom
    return np.r_[float(amin), float(ainc), float(amax), float(len(ranges)), np.asarray(ranges, np.float64)]


def run_model(rows):
    """rows [n,6] = (x, y, ori, v, steer, dt) -> dict A [n,3,3], B [n,3,2], C [n,3], sim [n,3]"""
    rows = np.asarray(rows, np.float64)
    o = run_driver("model", np.r_[float(len(rows)), rows.ravel()]).reshape(len(rows), 21)
    return dict(A=o[:, :9].reshape(-1, 3, 3), B=o[:, 9:15].reshape(-1, 3, 2), C=o[:, 15:18], sim=o[:, 18:21])


def run_halfspace(poses, scans, geoms, mathh=False):
    """poses [n,3] float64, scans: list of float32 arrays, geoms [n,3] -> (l1 [n,3], l2 [n,3])"""
    v = [np.array([float(len(scans))])]
    for p, r, g in zip(poses, scans, geoms):
        v += [np.asarray(p, np.float64), pack_scan(r, g)]
    o = run_driver("halfspace", np.concatenate(v), mathh=mathh).reshape(len(scans), 6)
    return o[:, :3].copy(), o[:, 3:].copy()


class _Cursor:
    def __init__(self, a):
        self.a, self.p = a, 0

    def take(self, n):
        v = self.a[self.p:self.p + n]
        assert len(v) == n
        self.p += n
        return v

    def one(self):
        return self.take(1)[0]

    def qp(self):
        d = dict(update_path=int(self.one()), set_calls=int(self.one()), update_calls=int(self.one()))
        n, m = int(self.one()), int(self.one())
        for name in ("P", "A"):
            nnz = int(self.one())
            d[name + "_colptr"] = self.take(n + 1).astype(np.int32)
            d[name + "_rowind"] = self.take(nnz).astype(np.int32)
            d[name + "_val"] = self.take(nnz).copy()
            if name == "P":
                d["q"] = self.take(n).copy()
        d["l"], d["u"] = self.take(m).copy(), self.take(m).copy()
        return d


def run_tick(N, overrides, calls):
    """calls: list of (x0 [3], u_lin [2], x_ref [S,3], ranges, geom) handed to one MPC object in turn
    -> list of captured QPs (dicts as oracle.assemble returns, plus the path counters)"""
    S = len(calls[0][2])
    v = [np.array([float(S), float(len(calls))])]
    for x0, ul, xr, ranges, geom in calls:
        v += [np.asarray(x0, np.float64), np.asarray(ul, np.float64), np.asarray(xr, np.float64).ravel(),
              pack_scan(ranges, geom)]
    c = _Cursor(run_driver("tick", np.concatenate(v), dict(overrides, horizon=N)))
    out = [c.qp() for _ in calls]
    assert c.p == len(c.a)
    return out


def run_loop(N, T, x0, ul0, x_ref, ranges, geom):
    """cars x T ticks -> dict of x [B,T+1,3], u_lin [B,T+1,2], status [B,T], qp [B][T], z [B,T,n],
    plan [B,T,N,2], u_applied [B,T,2]"""
    B, S = len(x0), x_ref.shape[1]
    v = [np.array([float(B), float(T), float(S)])]
    for b in range(B):
        v += [np.asarray(x0[b], np.float64), np.asarray(ul0[b], np.float64), np.asarray(x_ref[b], np.float64).ravel(),
              pack_scan(ranges[b], geom)]
    c = _Cursor(run_driver("loop", np.concatenate(v), dict(horizon=N)))
    n = 5 * N + 3
    o = dict(x=np.zeros((B, T + 1, 3)), u_lin=np.zeros((B, T + 1, 2)), status=np.zeros((B, T), np.int32),
             qp=[[None] * T for _ in range(B)], z=np.zeros((B, T, n)), plan=np.zeros((B, T, N, 2)),
             u_applied=np.zeros((B, T, 2)))
    for b in range(B):
        for t in range(T):
            o["x"][b, t], o["u_lin"][b, t], o["status"][b, t] = c.take(3), c.take(2), int(c.one())
            o["qp"][b][t] = c.qp()
            o["z"][b, t] = c.take(n)
            cnt = int(c.one())
            assert cnt == N, cnt  # UpdateSolvedTrajectory's `i < size()-1; i += 2` loop yields all N inputs
            o["plan"][b, t] = c.take(2 * N).reshape(N, 2)
            o["u_applied"][b, t] = c.take(2)
        o["x"][b, T], o["u_lin"][b, T] = c.take(3), c.take(2)
    assert c.p == len(c.a)
    return o


# ---- the optimum of a captured QP, computed from its matrices alone -------------------------------

def dense(colptr, rowind, val, nrows, ncols):
    M = np.zeros((nrows, ncols))
    for j in range(ncols):
        for p in range(colptr[j], colptr[j + 1]):
            M[rowind[p], j] += val[p]
    return M


def condense_captured(qp, N):
    """Eliminate the states through the captured equality rows: x = G u + f, then the condensed
    (H, g) of 1/2 z'Pz + q'z in u, and the input bounds. numpy fp64, no oracle code."""
    ns, n, m = 3 * (N + 1), 5 * N + 3, 7 * N + 5
    P = dense(qp["P_colptr"], qp["P_rowind"], qp["P_val"], n, n)
    A = dense(qp["A_colptr"], qp["A_rowind"], qp["A_val"], m, n)
    assert np.array_equal(qp["l"][:ns], qp["u"][:ns])
    Ex, Eu = A[:ns, :ns], A[:ns, ns:]
    G = -np.linalg.solve(Ex, Eu)
    f = np.linalg.solve(Ex, qp["l"][:ns])
    Z = np.vstack([G, np.eye(2 * N)])
    z0 = np.r_[f, np.zeros(2 * N)]
    H = Z.T @ P @ Z
    g = Z.T @ (P @ z0 + qp["q"])
    return dict(P=P, A=A, G=G, f=f, H=H, g=g, lo=qp["l"][ns + 2 * (N + 1):], hi=qp["u"][ns + 2 * (N + 1):])


def z_star(qp, N, tol=1e-8):
    """The optimum of the captured (P, q, A, l, u) by bounded least squares (scipy BVLS on the
    condensed problem, the route of tests/test_oracle.py::_independent_box_solve), certified by a
    KKT check on the captured sparse problem at `tol`: primal feasibility of every row, and the
    multipliers that stationarity forces (zero on the inactive gap rows) have the sign of their
    active bound and vanish on inactive input rows. Returns (z, number of active input bounds)."""
    from scipy.optimize import lsq_linear

    ns = 3 * (N + 1)
    c = condense_captured(qp, N)
    assert (np.abs(qp["l"][ns:ns + 2 * (N + 1)]) >= 1e30).all() and (qp["u"][ns:ns + 2 * (N + 1)] >= 1e30).all()
    L = np.linalg.cholesky(c["H"])
    res = lsq_linear(L.T, -np.linalg.solve(L, c["g"]), bounds=(c["lo"], c["hi"]), method="bvls", tol=1e-15)
    u = res.x
    z = np.r_[c["G"] @ u + c["f"], u]
    Az = c["A"] @ z
    primal = np.maximum(np.maximum(qp["l"] - Az, Az - qp["u"]), 0.0).max()
    grad = c["P"] @ z + qp["q"]
    y_eq = -np.linalg.solve(c["A"][:ns, :ns].T, grad[:ns])          # state columns (gap multipliers are 0)
    y_in = -(grad[ns:] + c["A"][:ns, ns:].T @ y_eq)                  # input columns
    at_lo, at_hi = u <= c["lo"] + 1e-12, u >= c["hi"] - 1e-12
    viol = np.where(at_lo, np.maximum(y_in, 0.0), np.where(at_hi, np.maximum(-y_in, 0.0), np.abs(y_in))).max()
    assert primal <= tol and viol <= tol, (primal, viol)
    return z, int((at_lo | at_hi).sum())
