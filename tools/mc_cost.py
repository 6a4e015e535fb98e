"""Cost of the Monte Carlo outcomes on one MI355X: clear_traj [201][4,096] (T = 200 ticks), crash_tick [4,096],
status_traj and kind_traj [200][4,096], seeded synthetic arrays (the kernels' work does not depend on the values,
apart from the compare-exchange selects); product library, one process.
  (a) per (M, G) in (16, 1), (256, 1), (256, 16), (4,096, 1): f110qp_mc_fan_dev (Q = 5, count given) and
      f110qp_mc_survival_dev by HIP events on the stream; f110qp_mc_outcomes_dev once (it takes no layout);
  (b) what a caller does today, in the same run: the device-to-host copy of the same arrays (wall clock around
      .cpu(), after a synchronise) followed by the numpy oracle (workload.mc_fan, mc_survival, mc_outcomes), each
      timed on its own, `wall_rounds` rounds; and the device results checked against that oracle bit for bit.
Warm-up first, the routes alternating within a round; medians and [min, max] over `rounds`. No ratio is fixed in
advance: the figures are reported as measured.

usage: python tools/mc_cost.py [rounds [out.json]]   (default profiles/mc/mc_cost.json)
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from f110qp import capi, workload  # noqa: E402
from world_cost import stat, timed  # noqa: E402

B, T = 4096, 200
LAYOUTS = ((16, 1), (256, 1), (256, 16), (4096, 1))
PROB = (0.0, 0.05, 0.5, 0.95, 1.0)
WALL_ROUNDS = 3


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mc", "mc_cost.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(2024)
    clear = rng.normal(1.0, 0.5, (T + 1, B))
    clear[rng.random((T + 1, B)) < 0.01] = np.nan
    crash = np.where(rng.random(B) < 0.3, rng.integers(0, T + 1, B), -1).astype(np.int32)
    kind = rng.choice([0, 0, 0, 1, 2, 3], (T, B)).astype(np.int32)
    status = np.where(kind == 0, rng.choice([1, 1, 1, 2, 4], (T, B)), 0).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    dclear, dcrash, dstatus, dkind = t(clear), t(crash), t(status), t(kind)
    Q = len(PROB)
    mcs = {(M, G): capi.default_mc_config(hypotheses=M, group_size=G, prob=PROB) for M, G in LAYOUTS}
    fans = {k: z((T + 1, B // k[0], Q), torch.float64) for k in LAYOUTS}
    counts = {k: z((T + 1, B // k[0]), torch.int32) for k in LAYOUTS}
    alives = {k: z((T + 1, B // k[0]), torch.int32) for k in LAYOUTS}
    hits = {k: z((B // k[0],), torch.int32) for k in LAYOUTS}
    mn = z((B,), torch.float64)
    recs = [z((B,), torch.int32) for _ in range(4)]

    variants = {}
    for k in LAYOUTS:
        variants[f"fan_M{k[0]}_G{k[1]}"] = lambda k=k: capi.mc_fan_dev(mcs[k], dclear, fans[k], counts[k])
        variants[f"survival_M{k[0]}_G{k[1]}"] = lambda k=k: capi.mc_survival_dev(mcs[k], dcrash, T, alives[k], hits[k])
    variants["outcomes"] = lambda: capi.mc_outcomes_dev(dclear, mn, dstatus, dkind, *recs)
    for fn in variants.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ev[k].append(timed(stream, fn))

    wall = {"copy_clear_traj_ms": [], "copy_crash_status_kind_ms": [], "numpy_outcomes_ms": []}
    wall.update({f"numpy_fan_M{M}_G{G}_ms": [] for M, G in LAYOUTS})
    wall.update({f"numpy_survival_M{M}_G{G}_ms": [] for M, G in LAYOUTS})
    same = True
    eq = lambda a, b: bool((np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all())  # noqa: E731
    for _ in range(WALL_ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hclear = dclear.cpu().numpy()
        t1 = time.perf_counter()
        hcrash, hstatus, hkind = dcrash.cpu().numpy(), dstatus.cpu().numpy(), dkind.cpu().numpy()
        t2 = time.perf_counter()
        rec = workload.mc_outcomes(hclear, hstatus, hkind)
        t3 = time.perf_counter()
        wall["copy_clear_traj_ms"].append((t1 - t0) * 1e3)
        wall["copy_crash_status_kind_ms"].append((t2 - t1) * 1e3)
        wall["numpy_outcomes_ms"].append((t3 - t2) * 1e3)
        same &= eq(mn.cpu().numpy(), rec["min_clear"])
        for r, name in zip(recs, ("min_row", "unsolved", "first_unsolved", "plan_failed")):
            same &= eq(r.cpu().numpy(), rec[name])
        for M, G in LAYOUTS:
            t0 = time.perf_counter()
            f, n = workload.mc_fan(hclear, M, G, PROB)
            t1 = time.perf_counter()
            a, h = workload.mc_survival(hcrash, T, M, G)
            t2 = time.perf_counter()
            wall[f"numpy_fan_M{M}_G{G}_ms"].append((t1 - t0) * 1e3)
            wall[f"numpy_survival_M{M}_G{G}_ms"].append((t2 - t1) * 1e3)
            k = (M, G)
            same &= eq(fans[k].cpu().numpy(), f) and eq(counts[k].cpu().numpy(), n)
            same &= eq(alives[k].cpu().numpy(), a) and eq(hits[k].cpu().numpy(), h)

    res = {"B": B, "T": T, "rows": T + 1, "Q": Q, "rounds": rounds, "wall_rounds": WALL_ROUNDS,
           "bytes": {"clear_traj": clear.nbytes, "crash_status_kind": crash.nbytes + status.nbytes + kind.nbytes},
           "unit": "us by HIP events per call: median, [min, max]; the wall clocks (copies, numpy) in ms",
           "note": "one launch per call; the copies are pageable device-to-host copies through torch's .cpu(), "
                   "what a caller without these calls does before numpy can start",
           **{k: stat(v) for k, v in ev.items()}, **{k: stat(v) for k, v in wall.items()},
           "device_equals_numpy_bits": bool(same)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
