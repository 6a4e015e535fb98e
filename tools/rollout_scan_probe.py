"""Cost per tick of the closed loop whose half-space rows follow the car, N = 20, T = 50 ticks, 1,080
beams, B = 64 / 1,024 / 4,096 (product library, AUTO back end), by HIP events on the stream:
  (a) f110qp_rollout_dev, the rows held (gap_mode INACTIVE: none);
  (b) f110qp_rollout_scan_dev, gap_mode INACTIVE, hs_traj recorded: the QPs of (a) bit for bit, so
      (b) - (a) is the fused geometry plus the two launches in front of the loop;
  (c) the loop a caller would otherwise enqueue: find_half_spaces_dev_dbl, solve_batch_dev_dbl,
      advance_dev per tick;
and at B = 1,024 (b) and (c) once more with gap_mode ACTIVE. One process, warm-up first, the routes
alternating within a round; medians and [min, max] over `rounds`. Writes one JSON object.

usage: python tools/rollout_scan_probe.py [rounds [out.json]]   (default profiles/rollout_scan_probe.json)
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
from f110qp import capi, workload  # noqa: E402

N, T, BEAMS = 20, 50, 1080


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def routes(dev, stream, B, gap):
    """The three routes at one shape as closures, plus the solver to close."""
    sp = C.c_void_p(stream.cuda_stream)
    tp = capi._tp
    w = workload.make_batch(B, N, seed=77)
    x0, ul, xr = (np.ascontiguousarray(w[k].astype(np.float64)) for k in ("x0", "u_lin", "x_ref"))
    ranges, amin, ainc, amax = workload.make_scans(B, seed=79, beams=BEAMS)
    s = capi.Solver(capi.default_config(N, gap_mode=capi.GAP_ACTIVE if gap else capi.GAP_INACTIVE))
    L = s.lib
    rc = capi.default_rollout_config(ticks=T)
    sc = capi.default_scan_config(num_ranges=BEAMS, angle_min=amin, angle_increment=ainc, angle_max=amax)

    def chk(rv):
        if rv != capi.OK:
            raise capi.F110QPError(capi.last_error(L))

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    xrd, rg = torch.from_numpy(xr).to(dev), torch.from_numpy(ranges).to(dev)
    xt, ult = z((T + 1, B, 3), torch.float64), z((T + 1, B, 2), torch.float64)
    ua, stt, hst = z((T, B, 2), torch.float32), z((T, B), torch.int32), z((T, B, 2, 3), torch.float32)
    xt[0], ult[0] = torch.from_numpy(x0).to(dev), torch.from_numpy(ul).to(dev)
    uo, xo, st = z((B, N, 2), torch.float32), z((B, N + 1, 3), torch.float32), z((B,), torch.int32)
    hs = z((B, 2, 3), torch.float32)
    keep = [xrd, rg, xt, ult, ua, stt, hst, uo, xo, st, hs]
    held_args = (s._h, C.byref(rc), B, tp(xrd), None, tp(xt), tp(ult), tp(ua), tp(stt), None, None, None, None, sp)
    scan_args = (s._h, C.byref(rc), C.byref(sc), B, tp(xrd), tp(rg), tp(xt), tp(ult), tp(ua), tp(stt), None, None,
                 None, None, tp(hst), sp)
    hs_args = [(B, tp(xt[t]), tp(rg), BEAMS, amin, ainc, amax, sc.ftg_thresh, sc.divider, sc.buffer, tp(hs), None,
                None, sp) for t in range(T)]
    solve_args = [(s._h, B, tp(xt[t]), tp(ult[t]), tp(xrd), tp(hs) if gap else None, tp(uo), tp(xo), tp(st), None,
                   None, None, sp) for t in range(T)]
    adv_args = [(C.byref(rc), B, N, tp(xt[t]), tp(uo), tp(st), tp(xt[t + 1]), tp(ult[t + 1]), tp(ua[t]), sp)
                for t in range(T)]

    def held():  # (a)
        chk(L.f110qp_rollout_dev(*held_args))

    def scan():  # (b)
        chk(L.f110qp_rollout_scan_dev(*scan_args))

    def unfused():  # (c)
        for t in range(T):
            chk(L.f110qp_find_half_spaces_dev_dbl(*hs_args[t]))
            chk(L.f110qp_solve_batch_dev_dbl(*solve_args[t]))
            chk(L.f110qp_advance_dev(*adv_args[t]))

    out = {"rollout_scan_dev": scan, "unfused_loop": unfused}
    if not gap:
        out = {"rollout_dev": held, **out}
    return out, s, keep, (rc, sc)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "rollout_scan_probe.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    res = {"N": N, "T": T, "beams": BEAMS, "rounds": rounds, "unit": "us per tick by HIP events: median, [min, max]",
           "shapes": []}
    for B, gap in ((64, False), (1024, False), (4096, False), (1024, True)):
        variants, s, keep, cfgs = routes(dev, stream, B, gap)
        for fn in variants.values():  # warm-up: code objects, workspaces
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ev = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                ev[k].append(timed(stream, fn) / T)
        row = {"B": B, "gap_mode": "ACTIVE" if gap else "INACTIVE", "backend_info": list(s.backend_info(B))}
        for k in variants:
            row[k] = {"median": round(float(np.median(ev[k])), 2), "min_max": [round(min(ev[k]), 2), round(max(ev[k]), 2)]}
        s.close()
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
