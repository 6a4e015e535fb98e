"""Cost of the closed loop per tick, 4,096 cars x N = 20, T = 50 ticks (product library, AUTO back end):
  (a) the host round trip: f110qp_solve_batch_dev_dbl, download of u_out and status, the numpy
      Model::simulate_dynamics step and next linearisation input, upload of x0 and u_lin, per tick;
  (b) one f110qp_rollout_dev call for the T ticks;
  (c) the T solves of (b) alone, back to back on the stream, each on the inputs (b) recorded for its
      tick (no plant step), so that (b) - (c) is what the plant-step launch adds to a tick;
and the plant-step kernel by itself, back-to-back launches. Each by HIP events on the stream and by
wall clock around work that ends in a stream synchronise, medians over `rounds` after a warm-up, the
variants alternating within a round. Writes one JSON object.

usage: python tools/rollout_probe.py [rounds [out.json]]     (default profiles/rollout_probe.json)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
from f110qp import capi, workload  # noqa: E402

B, N, T = 4096, 20, 50
INNER = 50  # back-to-back plant-step launches per timed interval


def timed(stream, fn):
    """(event us, wall us) of fn(), which enqueues on `stream`; both end when the stream drains."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0, (time.perf_counter() - t0) * 1e6


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "rollout_probe.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    w = workload.make_batch(B, N, seed=77)
    x0, ul, xr = (np.ascontiguousarray(w[k].astype(np.float64)) for k in ("x0", "u_lin", "x_ref"))
    s = capi.Solver(capi.default_config(N))
    L, tp = s.lib, capi._tp
    rc = capi.default_rollout_config(ticks=T)

    def chk(rv):
        if rv != capi.OK:
            raise capi.F110QPError(capi.last_error(L))

    # device arrays of the rollout (b); (a) keeps its own x0, u_lin, (c) reads the rows (b) recorded
    xrd = torch.from_numpy(xr).to(dev)
    xt = torch.zeros((T + 1, B, 3), dtype=torch.float64, device=dev)
    ult = torch.zeros((T + 1, B, 2), dtype=torch.float64, device=dev)
    ua = torch.zeros((T, B, 2), dtype=torch.float32, device=dev)
    stt = torch.zeros((T, B), dtype=torch.int32, device=dev)
    xt[0], ult[0] = torch.from_numpy(x0).to(dev), torch.from_numpy(ul).to(dev)
    x0d, uld = xt[0].clone(), ult[0].clone()
    uo = torch.zeros((B, N, 2), dtype=torch.float32, device=dev)
    xo = torch.zeros((B, N + 1, 3), dtype=torch.float32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    xn, uln = torch.zeros_like(x0d), torch.zeros_like(uld)
    solve_args = (s._h, B, tp(x0d), tp(uld), tp(xrd), None, tp(uo), tp(xo), tp(st), None, None, None, sp)
    roll_args = (s._h, C.byref(rc), B, tp(xrd), None, tp(xt), tp(ult), tp(ua), tp(stt), None, None, None, None, sp)
    adv_args = (C.byref(rc), B, N, tp(x0d), tp(uo), tp(st), tp(xn), tp(uln), None, sp)
    tick_args = [(s._h, B, tp(xt[t]), tp(ult[t]), tp(xrd), None, tp(uo), tp(xo), tp(st), None, None, None, sp)
                 for t in range(T)]

    def host_loop():  # (a)
        x = x0.copy()
        x0d.copy_(torch.from_numpy(x))
        uld.copy_(torch.from_numpy(ul))
        for _ in range(T):
            chk(L.f110qp_solve_batch_dev_dbl(*solve_args))
            u = uo.cpu().numpy().astype(np.float64)  # (synchronises the stream)
            ok = np.isin(st.cpu().numpy(), (capi.SOLVED, capi.SOLVED_INACCURATE))
            u0 = np.where(ok[:, None], u[:, 0], np.array([0.5, 0.0]))
            x = workload.simulate_dynamics(x, u0, rc.plant_dt)
            nxt = np.stack([np.full(B, rc.v_lin), np.where(ok, u[:, 1, 1], 0.0)], 1)
            x0d.copy_(torch.from_numpy(x))
            uld.copy_(torch.from_numpy(nxt))

    def rollout():  # (b)
        chk(L.f110qp_rollout_dev(*roll_args))

    def solves_only():  # (c)
        for a in tick_args:
            chk(L.f110qp_solve_batch_dev_dbl(*a))

    def advances():
        for _ in range(INNER):
            chk(L.f110qp_advance_dev(*adv_args))

    variants = {"host_round_trip": (host_loop, T), "rollout_dev": (rollout, T), "solves_only": (solves_only, T),
                "advance_kernel": (advances, INNER)}
    for fn, _ in variants.values():  # warm-up: code objects, workspaces, pinned staging of the copies
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    assert (stt.cpu().numpy() == capi.SOLVED).all()
    ev = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, n) in variants.items():
            e, wl = timed(stream, fn)
            ev[k].append(e / n)
            wall[k].append(wl / n)
    info = s.backend_info(B) + (s.lane_segments(B),)
    s.close()
    res = {"B": B, "N": N, "T": T, "rounds": rounds, "backend_info": list(info), "unit": "us per tick, median"}
    for k in variants:
        res[k] = {"event_us": round(float(np.median(ev[k])), 2), "wall_us": round(float(np.median(wall[k])), 2),
                  "event_us_min_max": [round(min(ev[k]), 2), round(max(ev[k]), 2)]}
    res["advance_kernel"]["note"] = f"per launch, {INNER} back-to-back launches"
    res["advance_launch_cost_us"] = round(res["rollout_dev"]["event_us"] - res["solves_only"]["event_us"], 2)
    res["rollout_over_host_wall"] = round(res["rollout_dev"]["wall_us"] / res["host_round_trip"]["wall_us"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
