"""The configuration corners of tests/test_gpu_config_corners.py and tests/test_config_corner_cases.py,
in one place: f110qp_config values that validate_config (csrc/f110qp_api.cpp) accepts and that no other
test creates. Zero-width boxes, u_des (and u_lin) outside the box, boxes away from the usual quadrant,
"no bound" as +-1e30 (OSQP's INFTY, the reference's constraints.cpp:15), +-1e20 and +-inf, and the
weight ratios at both ends of what f110qp_create accepts (max(q) / min(r) = F110QP_MAX_WEIGHT_RATIO =
1e3; q = (1e4, 1e4, 0) with r = (1e-3, 1e-3) is rejected, tests/test_capi.py). Test infrastructure.

A case is (name, over, dt, N, batch, gap): `over` the f110qp_config / oracle.params overrides, `batch`
the workload.make_batch arguments (plus "u_lin_speed": the linearisation speed of every QP, where the
case wants u_lin outside the box; gap cases: "scan_seed" for workload.make_scans), `gap` whether the
QPs carry half-space rows. Every case is generated at B_REF = 96 QPs (one full and one ragged wave);
the routes that run fewer (9, 8, 1) take the first QPs of the same batch, so one oracle solve per case
serves every route (reference()).

What chose the seeds:
    python tests/config_corner_cases.py            # every case: oracle statuses and what it shows
    python tests/config_corner_cases.py gap 1 40   # gap cases: UNCERTIFIED / screen split per scan seed
The box cases keep make_batch(seed=5, heading="true", lateral=1.0, steer_range=0.6), the batch the
oracle was first checked on for these corners: no QP of any of them is UNCERTIFIED. The gap cases'
scan seeds are the first ones (from 1) at which the oracle leaves at most 1 of the 96 QPs UNCERTIFIED
(the 2 % cap of test_gpu_parity.test_fuzz_configs_against_oracle) and the box optimum both keeps the
gap rows of some QPs and violates them for others (the box screen has both to do).
"""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "f110-mpc_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

from f110qp import workload  # noqa: E402

Case = namedtuple("Case", "name over dt N batch gap")

B_REF = 96
BASE = dict(seed=5, heading="true", lateral=1.0, steer_range=0.6)
DTS = (float(np.float32(0.01)), float(np.float32(0.05)))
DEFAULT_MIN = np.float32([3.0, -0.43])  # f110qp_default_config
DEFAULT_MAX = np.float32([4.5, 0.43])
DEFAULT_DES = (4.5, 0.0)
BIG = 1e30  # OSQP's INFTY, what the reference passes for "no bound"
INF = float("inf")

# family -> member -> (over, extra make_batch arguments)
FAMILIES = {
    "zero_width": {
        "speed": (dict(u_min=[4.0, -0.43], u_max=[4.0, 0.43]), {}),
        "steer": (dict(u_min=[3.0, 0.1], u_max=[4.5, 0.1]), {}),
        "both": (dict(u_min=[4.0, 0.1], u_max=[4.0, 0.1]), {}),
    },
    "u_des_outside": {
        "above": (dict(u_des=[6.0, 0.8]), {}),
        # u_lin outside the box as well: linearised at 2 m/s below the speed box [3, 4.5] (and at steers
        # up to +-0.6 beyond +-0.43, as every case here)
        "below": (dict(u_des=[1.0, -0.9]), dict(u_lin_speed=2.0)),
    },
    "quadrant": {
        "steer_positive": (dict(u_min=[3.0, 0.05], u_max=[4.5, 0.43]), {}),
        "reverse": (dict(u_min=[-2.0, -0.43], u_max=[-0.5, 0.43], u_des=[-1.0, 0.0]), {}),
        "straddle": (dict(u_min=[-1.0, -0.43], u_max=[2.0, 0.43], u_des=[1.5, 0.0]), {}),
    },
    "no_bound": {
        "all_1e30": (dict(u_min=[-BIG, -BIG], u_max=[BIG, BIG]), {}),
        "one_sided_1e30": (dict(u_min=[3.0, -BIG], u_max=[BIG, 0.43]), {}),
        # another solver's "infinity": far beyond the inputs, far below OSQP's
        "one_sided_1e20": (dict(u_min=[3.0, -1e20], u_max=[1e20, 0.43]), {}),
        "all_inf": (dict(u_min=[-INF, -INF], u_max=[INF, INF]), {}),
        "one_sided_inf": (dict(u_min=[3.0, -INF], u_max=[INF, 0.43]), {}),
    },
    "weights": {
        # max(q) / min(r) = 1e3, the largest ratio f110qp_create accepts (F110QP_MAX_WEIGHT_RATIO)
        "stiff": (dict(q=[1e2, 1e2, 0.0], r=[0.1, 0.1]), {}),
        "soft": (dict(q=[1e-3, 1e-3, 0.0], r=[1e2, 1e3]), {}),
        "heading_only": (dict(q=[0.0, 0.0, 5.0]), {}),
        # q0 != q1: the general-frame lane kernels (the others run the heading-frame ones), on corners
        # of two other families
        "general_u_des_above": (dict(q=[3.0, 7.0, 2.0], u_des=[6.0, 0.8]), {}),
        "general_zero_width_speed": (dict(q=[3.0, 7.0, 2.0], u_min=[4.0, -0.43], u_max=[4.0, 0.43]), {}),
    },
}
# N = 5 (dt 0.05) and N = 33 (dt 0.01: two register rows on the wave kernel, no segmented kernel)
SHORT_LIST = (("zero_width", "speed"), ("zero_width", "both"), ("u_des_outside", "above"),
              ("u_des_outside", "below"), ("no_bound", "all_1e30"), ("no_bound", "one_sided_inf"))
# gap rows, N = 20: (family, member) -> scan seed per dt (see the module docstring for the choice)
GAP_LIST = {
    ("zero_width", "speed"): (1, 1),
    ("u_des_outside", "above"): (1, 1),
    ("u_des_outside", "below"): (1, 1),
    ("no_bound", "one_sided_1e30"): (1, 1),
    ("no_bound", "one_sided_inf"): (1, 1),
    ("weights", "stiff"): (1, 1),
}


def _case(fam, mem, N, dt, gap=False, **extra):
    over, bk = FAMILIES[fam][mem]
    name = f"{fam}/{mem}/N{N}/dt{dt:.2f}" + ("/gap" if gap else "")
    return Case(name, over, dt, N, dict(BASE, **bk, **extra), gap)


def cases():
    """Every case: each family member at N = 20 and both dt, the short list at N = 5 and N = 33, the
    gap-row list at N = 20 and both dt."""
    out = [_case(f, m, 20, dt) for f in FAMILIES for m in FAMILIES[f] for dt in DTS]
    # (five stages against r1 = 5 reach the upper faces from u_des = (1, -0.9) only for references
    # further off: lateral 3.0 puts 21 inputs of the batch there, lateral 1.0 none)
    out += [_case(f, m, 5, DTS[1], **(dict(lateral=3.0) if m == "below" else {})) for f, m in SHORT_LIST]
    out += [_case(f, m, 33, DTS[0]) for f, m in SHORT_LIST]
    out += [_case(f, m, 20, dt, gap=True, scan_seed=s) for (f, m), ss in GAP_LIST.items() for dt, s in zip(DTS, ss)]
    return out


def family(case):
    return case.name.split("/")[0]


def member(case):
    return case.name.split("/")[1]


def select(gap=False, families=None, horizons=None):
    return [c for c in cases() if c.gap == gap and (families is None or family(c) in families)
            and (horizons is None or c.N in horizons)]


def bounds(case):
    """(u_min, u_max, u_des) of a case as the kernels hold them: float32 bounds, double u_des."""
    lo = np.float32(case.over.get("u_min", DEFAULT_MIN))
    hi = np.float32(case.over.get("u_max", DEFAULT_MAX))
    return lo, hi, np.float64(case.over.get("u_des", DEFAULT_DES))


def inputs(case, B=B_REF):
    """The case's batch of B QPs (the first B of the B_REF the case is defined on): dict(x0, u_lin,
    x_ref) and, for a gap case, (ranges, amin, ainc, amax)."""
    bk = dict(case.batch)
    speed = bk.pop("u_lin_speed", None)
    scan_seed = bk.pop("scan_seed", None)
    w = workload.make_batch(B_REF, case.N, **bk)
    if speed is not None:
        w["u_lin"][:, 0] = np.float32(speed)
    w = {k: np.ascontiguousarray(v[:B]) for k, v in w.items()}
    scans = None
    if case.gap:
        ranges, amin, ainc, amax = workload.make_scans(B_REF, seed=scan_seed)
        scans = (np.ascontiguousarray(ranges[:B]), amin, ainc, amax)
    return w, scans


def halfspaces(oracle, x0, scans):
    ranges, *geom = scans
    hs = np.zeros((x0.shape[0], 2, 3), np.float32)
    for b in range(x0.shape[0]):
        rc, l1, l2, _, _ = oracle.find_half_spaces(x0[b].astype(np.float64), ranges[b], *geom)
        assert rc == 0
        hs[b] = l1, l2
    return hs


_ref = {}


def reference(oracle, case):
    """The oracle's answer for the case's B_REF QPs, computed once and left unchanged: dict(w, hs, u,
    x, st, obj, prm)."""
    if case.name not in _ref:
        w, scans = inputs(case)
        hs = halfspaces(oracle, w["x0"], scans) if case.gap else None
        prm = oracle.params(case.N, dt=case.dt, **case.over)
        u, x, st, obj = oracle.solve_batch(prm, w["x0"], w["u_lin"], w["x_ref"], hs, gap_active=case.gap,
                                           objective=True)
        r = dict(w=w, hs=hs, u=u, x=x, st=st, obj=obj, prm=prm)
        for a in list(w.values()) + [u, x, st, obj] + ([hs] if hs is not None else []):
            a.setflags(write=False)
        _ref[case.name] = r
    return _ref[case.name]


def first(ref, B):
    """The first B QPs of a reference()."""
    out = {k: (None if ref[k] is None else ref[k][:B]) for k in ("hs", "u", "x", "st", "obj")}
    out["w"] = {k: v[:B] for k, v in ref["w"].items()}
    out["prm"] = ref["prm"]
    return out


def face_counts(case, u, tol=1e-9):
    """Of inputs u [B,N,2] (float64): how many sit on the lower bound, on the upper bound, and strictly
    inside (further than 1e-6 from both) per input channel: three [2] arrays."""
    lo, hi, _ = bounds(case)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    on_lo = np.abs(u - lo) <= tol
    on_hi = np.abs(u - hi) <= tol
    free = (u > lo + 1e-6) & (u < hi - 1e-6)
    return on_lo.sum(axis=(0, 1)), on_hi.sum(axis=(0, 1)), free.sum(axis=(0, 1))


def rows_cleared(x0, x, hs, margin=1e-6):
    """The box screen's rule (f110qp_kernels.hip gap_screen_kernel) on states x [B,N+1,3] of a box-only
    optimum: True where every gap row of stages 1..N holds with `margin` of the row's terms and the
    constant stage-0 rows hold."""
    x = np.asarray(x, np.float64)
    ok = np.ones(x.shape[0], bool)
    for h in range(2):
        a, b, c = (hs[:, h, k].astype(np.float64)[:, None] for k in range(3))
        ax, by = a * x[:, 1:, 0], b * x[:, 1:, 1]
        ok &= (ax + by + c >= margin * (1.0 + np.abs(ax) + np.abs(by) + np.abs(c))).all(axis=1)
        ok &= a[:, 0] * np.float64(x0[:, 0]) + b[:, 0] * np.float64(x0[:, 1]) >= -c[:, 0] - 1e-9
    return ok


def _report(oracle, which):
    for c in which:
        r = reference(oracle, c)
        st, cnt = np.unique(r["st"], return_counts=True)
        ok = r["st"] == oracle.SOLVED
        lo, hi, free = face_counts(c, r["u"][ok])
        dl, dh = DEFAULT_MIN.astype(np.float64), DEFAULT_MAX.astype(np.float64)
        beyond = int(((r["u"][ok] < dl - 1e-6) | (r["u"][ok] > dh + 1e-6)).sum())
        print(f"{c.name:55s} status {dict(zip(st.tolist(), cnt.tolist()))} on_lo {lo} on_hi {hi} free {free} "
              f"beyond default box {beyond}")


def _gap_seeds(oracle, first_seed, count):
    for (f, m), _ in GAP_LIST.items():
        for dt in DTS:
            for s in range(first_seed, first_seed + count):
                c = _case(f, m, 20, dt, gap=True, scan_seed=s)
                r = reference(oracle, c)
                box = oracle.solve_batch(r["prm"], r["w"]["x0"], r["w"]["u_lin"], r["w"]["x_ref"])
                clr = rows_cleared(r["w"]["x0"], box[1], r["hs"]) & (box[2] == oracle.SOLVED)
                unc = int((r["st"] == oracle.UNCERTIFIED).sum())
                st, cnt = np.unique(r["st"], return_counts=True)
                good = unc <= 1 and 0 < clr.sum() < B_REF
                print(f"{f}/{m} dt {dt:.2f} scan seed {s}: uncertified {unc} cleared {int(clr.sum())}/{B_REF} "
                      f"status {dict(zip(st.tolist(), cnt.tolist()))}{'  <- first that serves' if good else ''}")
                del _ref[c.name]
                if good:
                    break


if __name__ == "__main__":
    import oracle as _oracle

    _oracle.build()
    if len(sys.argv) > 1 and sys.argv[1] == "gap":
        _gap_seeds(_oracle, int(sys.argv[2]) if len(sys.argv) > 2 else 1, int(sys.argv[3]) if len(sys.argv) > 3 else 40)
    else:
        _report(_oracle, cases())
