# Host design check (numpy, fp64; not product code — the kernel is csrc/lane_seg_kernel.h, step 2 of
# the pass): the segment-end boundary problem eliminated from both sides at once, against a dense
# solve of the same system and against the one-sided ring of diag_segment_riccati_model.py.
#
# Segment j = 0..S-1 starts at x_j and carries the multiplier lam_j of its end coupling:
#   x_{j+1} = Phi_j x_j + psi_j + Gam_j lam_j            (j <= S-2),   x_0 = 0,
#   lam_{j-1} = P_j x_j + a_j + Phi_j' lam_j             (j >= 1),     lam_{S-1} = 0.
# Upper side (the ring's step): lam_j = M_{j+1} x_{j+1} + m_{j+1} gives
#   Z = I - M_{j+1} Gam_j, Y = Z^-1 M_{j+1}, T_j = Y Phi_j, t_j = Y psi_j + Z^-1 m_{j+1},
#   M_j = P_j + Phi_j' T_j, m_j = a_j + Phi_j' t_j,  from (M, m)_{S-1} = (P, a)_{S-1}.
# Lower side: x_j = alpha_{j-1} + beta_{j-1} lam_{j-1}, (alpha, beta)_0 = (psi, Gam)_0, is the same
# step with the operands exchanged,
#   (Mn, mn, Gam, Phi, psi, P, a) <- (beta_{j-1}, alpha_{j-1}, P_j, Phi_j', a_j, Gam_j, psi_j),
# and gives x_j = T~_j lam_j + t~_j and (beta, alpha)_j in the places of (M, m)_j.
# The sides meet at h = S / 2: with own (O, o) and the other side's (R, r) each side solves
#   y = (I - R O)^-1 (r + R o):  the upper side x_h (O = M_h, R = beta_{h-1}),
#                                the lower side lam_{h-1} (O = beta_{h-1}, R = M_h),
# then S / 2 - 1 back-substitution steps per side, w = T y + t, e = Phi y + psi + Gam w with the
# same exchange (up: w = lam_j, e = x_{j+1}; down: w = x_j, e = lam_{j-1}).
# S / 2 - 1 full steps + the meet + S / 2 - 1 short steps replace the ring's S - 1 + S - 1.
import numpy as np

import diag_segment_riccati_model as seq_model


def adj_inv(Z):
    """3 x 3 inverse by the adjugate, as the kernel forms it."""
    A = np.array([[Z[1, 1] * Z[2, 2] - Z[1, 2] * Z[2, 1], Z[0, 2] * Z[2, 1] - Z[0, 1] * Z[2, 2], Z[0, 1] * Z[1, 2] - Z[0, 2] * Z[1, 1]],
                  [Z[1, 2] * Z[2, 0] - Z[1, 0] * Z[2, 2], Z[0, 0] * Z[2, 2] - Z[0, 2] * Z[2, 0], Z[0, 2] * Z[1, 0] - Z[0, 0] * Z[1, 2]],
                  [Z[1, 0] * Z[2, 1] - Z[1, 1] * Z[2, 0], Z[0, 1] * Z[2, 0] - Z[0, 0] * Z[2, 1], Z[0, 0] * Z[1, 1] - Z[0, 1] * Z[1, 0]]])
    det = Z[0, 0] * A[0, 0] + Z[0, 1] * A[1, 0] + Z[0, 2] * A[2, 0]
    return A / det


def step(Mn, mn, Gam, Phi, psi, P, a):
    """One elimination step (the kernel's): T, t and the next (M, m)."""
    Zi = adj_inv(np.eye(3) - Mn @ Gam)
    Y = Zi @ Mn
    T = Y @ Phi
    t = Y @ psi + Zi @ mn
    return T, t, P + Phi.T @ T, a + Phi.T @ t


def ops(sj, lower):
    """(Gam, Phi, psi, P, a) as the step takes them: the segment's own on the upper side, exchanged
    on the lower side."""
    if lower:
        return sj["P"], sj["Phi"].T, sj["a"], sj["Gam"], sj["psi"]
    return sj["Gam"], sj["Phi"], sj["psi"], sj["P"], sj["a"]


def meet(O, o, R, r):
    return adj_inv(np.eye(3) - R @ O) @ (r + R @ o)


def two_sided(seg):
    """x_j (start states) and lam_j of all segments by the two-sided elimination."""
    S = len(seg)
    h = S // 2
    x = np.zeros((S, 3))
    lam = np.zeros((S, 3))
    T, t = [None] * S, [None] * S
    # the two sides in lockstep: S / 2 - 1 full steps each
    M, m = seg[S - 1]["P"], seg[S - 1]["a"]
    be, al = seg[0]["Gam"], seg[0]["psi"]
    for k in range(h - 1):
        ju, jl = S - 2 - k, 1 + k
        T[ju], t[ju], M, m = step(M, m, *ops(seg[ju], False))
        T[jl], t[jl], be, al = step(be, al, *ops(seg[jl], True))
    # the meet: x_h on the upper side, lam_{h-1} on the lower one
    x[h] = meet(M, m, be, al)
    lam[h - 1] = meet(be, al, M, m)
    # back-substitution, S / 2 - 1 short steps each
    for k in range(h - 1):
        ju, jl = h + k, h - 1 - k
        G, F, s, _, _ = ops(seg[ju], False)
        lam[ju] = T[ju] @ x[ju] + t[ju]
        x[ju + 1] = F @ x[ju] + s + G @ lam[ju]
        G, F, s, _, _ = ops(seg[jl], True)
        x[jl] = T[jl] @ lam[jl] + t[jl]
        lam[jl - 1] = F @ lam[jl] + s + G @ x[jl]
    return x, lam


def ring(seg):
    """The present one-sided recursion (csrc/lane_seg_kernel.h before this model, and
    diag_segment_riccati_model.segmented): S - 1 steps up, S - 1 down."""
    S = len(seg)
    M, m = seg[S - 1]["P"], seg[S - 1]["a"]
    T, t = [None] * S, [None] * S
    for j in range(S - 2, -1, -1):
        T[j], t[j], M, m = step(M, m, *ops(seg[j], False))
    x = np.zeros((S, 3))
    lam = np.zeros((S, 3))
    for j in range(S - 1):
        lam[j] = T[j] @ x[j] + t[j]
        x[j + 1] = seg[j]["Phi"] @ x[j] + seg[j]["psi"] + seg[j]["Gam"] @ lam[j]
    return x, lam


def dense(seg):
    """The same boundary system as one 6 (S - 1) linear solve: unknowns x_1..x_{S-1}, lam_0..lam_{S-2}."""
    S = len(seg)
    n = 3 * (S - 1)
    K = np.zeros((2 * n, 2 * n))
    rhs = np.zeros(2 * n)
    xi = lambda j: slice(3 * (j - 1), 3 * j)          # x_j, j = 1..S-1
    li = lambda j: slice(n + 3 * j, n + 3 * j + 3)    # lam_j, j = 0..S-2
    for j in range(S - 1):  # x_{j+1} - Phi_j x_j - Gam_j lam_j = psi_j
        r = slice(3 * j, 3 * j + 3)
        K[r, xi(j + 1)] = np.eye(3)
        if j > 0:
            K[r, xi(j)] = -seg[j]["Phi"]
        K[r, li(j)] = -seg[j]["Gam"]
        rhs[r] = seg[j]["psi"]
    for j in range(1, S):  # lam_{j-1} - P_j x_j - Phi_j' lam_j = a_j
        r = slice(n + 3 * (j - 1), n + 3 * j)
        K[r, li(j - 1)] = np.eye(3)
        K[r, xi(j)] = -seg[j]["P"]
        if j < S - 1:
            K[r, li(j)] = -seg[j]["Phi"].T
        rhs[r] = seg[j]["a"]
    z = np.linalg.solve(K, rhs)
    x = np.zeros((S, 3))
    lam = np.zeros((S, 3))
    x[1:] = z[:n].reshape(S - 1, 3)
    lam[:S - 1] = z[n:].reshape(S - 1, 3)
    return x, lam


def rel(a, b):
    """Largest difference of a to the reference b relative to max(1, |b|)."""
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def err(sol, ref):
    return max(rel(sol[0], ref[0]), rel(sol[1], ref[1]))


def random_segments(rng, S):
    """Random symmetric P >= 0, Gam <= 0, general Phi, random psi and a."""
    seg = []
    for _ in range(S):
        A = rng.normal(size=(3, 3))
        B = rng.normal(size=(3, int(rng.integers(1, 4)))) * rng.choice([0.1, 1.0])
        seg.append(dict(P=A @ A.T * rng.choice([0.1, 1.0, 10.0]), Gam=-(B @ B.T),
                        Phi=np.eye(3) + rng.normal(size=(3, 3)) * rng.choice([0.1, 0.7]),
                        psi=rng.normal(size=3), a=rng.normal(size=3)))
    return seg


def sweep_problem(rng, N, heading):
    """One pass's fixed-active-set problem as diag_segment_riccati_model.main draws it."""
    Q = np.diag([1.0, 1.0, 0.1])
    R = np.diag([0.1, 0.1])
    ud = np.array([4.5, 0.0])
    A, B, C = seq_model.model(rng, N, heading=heading)
    ref = np.cumsum(rng.normal(0, 0.05, (N, 3)), 0)
    ref[:, 0] += np.arange(1, N + 1) * 0.04
    fixed = rng.random((N, 2)) < rng.choice([0.0, 0.2, 0.6, 1.0])
    bval = np.stack([rng.choice([-1.0, 4.5], N), rng.choice([-0.43, 0.43], N)], 1)
    return A, B, C, Q, R, ud, ref, fixed, bval


def sweep_segments(prob, S):
    """Segment data as the backward sweep generates them (segments of floor(N / S) or one more
    stage, the first N mod S longer, as the kernel splits the horizon)."""
    A, B, C, Q, R, ud, ref, fixed, bval = prob
    N = ref.shape[0]
    q, rem = divmod(N, S)
    seg = []
    for j in range(S):
        s = j * q + min(j, rem)
        e = s + q + (1 if j < rem else 0)
        last = j == S - 1
        P = Q.copy() if last else np.zeros((3, 3))
        p = -Q @ ref[N - 1] if last else np.zeros(3)
        Phi, psi, Gam = np.eye(3), np.zeros(3), np.zeros((3, 3))
        K, k, F = {}, {}, {}
        for i in range(e - 1, s - 1, -1):
            K[i], k[i], Pn, pn, I = seq_model.stage(P, p, A, B, C, Q, R, ud, ref[i], fixed[i], bval[i])
            W = Phi @ B
            F[i] = -I @ W.T
            psi = Phi @ (B @ k[i] + C) + psi
            Gam = Gam + W @ F[i]
            Phi = Phi @ (A + B @ K[i])
            P, p = Pn, pn
        seg.append(dict(s=s, e=e, P=P, a=p, Phi=Phi, psi=psi, Gam=Gam, K=K, k=k, F=F))
    return seg


def rollout(prob, seg, x, lam):
    """The forward sweep of every segment from its (x_j, lam_j): the pass's (u, x)."""
    A, B, C = prob[0], prob[1], prob[2]
    N = prob[6].shape[0]
    us = np.zeros((N, 2))
    xs = np.zeros((N + 1, 3))
    for j, sj in enumerate(seg):
        z = x[j]
        xs[sj["s"]] = z
        for i in range(sj["s"], sj["e"]):
            u = sj["K"][i] @ z + sj["k"][i] + sj["F"][i] @ lam[j]
            z = A @ z + B @ u + C
            us[i] = u
            xs[i + 1] = z
    return us, xs


def measure(S, trials=200, seed=0):
    """Worst errors over `trials` inputs of each kind: (two-sided, ring) against the dense solve on
    random segment data and on backward-sweep data, their largest mutual difference, and (two-sided,
    ring) whole-pass error against the sequential Riccati."""
    rng = np.random.default_rng(seed + S)
    out = dict(rand=[0.0, 0.0], sweep=[0.0, 0.0], mutual=0.0, whole=[0.0, 0.0])
    for trial in range(trials):
        seg = random_segments(rng, S)
        d = dense(seg)
        two, rg = two_sided(seg), ring(seg)
        out["rand"] = [max(out["rand"][0], err(two, d)), max(out["rand"][1], err(rg, d))]
        out["mutual"] = max(out["mutual"], err(two, rg))
        N = int(rng.choice([n for n in (4, 8, 9, 17, 20, 30, 40, 47) if n >= 2 * S]))
        prob = sweep_problem(rng, N, heading=bool(trial % 2))
        seg = sweep_segments(prob, S)
        d = dense(seg)
        two, rg = two_sided(seg), ring(seg)
        out["sweep"] = [max(out["sweep"][0], err(two, d)), max(out["sweep"][1], err(rg, d))]
        out["mutual"] = max(out["mutual"], err(two, rg))
        u1, x1 = seq_model.sequential(*prob)
        for k, sol in enumerate((two, rg)):
            u2, x2 = rollout(prob, seg, *sol)
            out["whole"][k] = max(out["whole"][k], rel(u2, u1), rel(x2, x1))
    return out


def main():
    for S in (2, 4, 8):
        r = measure(S)
        print(f"S = {S}: against the dense solve, two-sided / ring: random data {r['rand'][0]:.2e} / {r['rand'][1]:.2e}, "
              f"sweep data {r['sweep'][0]:.2e} / {r['sweep'][1]:.2e}; two-sided against ring {r['mutual']:.2e}; "
              f"whole pass against the sequential Riccati {r['whole'][0]:.2e} / {r['whole'][1]:.2e}")
    # dependent steps per pass: full elimination steps + meet + short steps
    for S in (2, 4, 8):
        print(f"S = {S}: ring {S - 1} full + {S - 1} short steps; two-sided {S // 2 - 1} full + meet + {S // 2 - 1} short")


if __name__ == "__main__":
    main()
