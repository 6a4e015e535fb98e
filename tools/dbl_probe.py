"""Cost of the double-precision input entry points against their float twins: per shape, the kernel
time of f110qp_solve_batch_dev and f110qp_solve_batch_dev_dbl by HIP events, the two calls
alternating in one process after a warm-up (product library, AUTO back end), and for B = 1 the wall
time of the synchronous calls. A _dbl call reads 12 + 8 + 12 S more bytes per QP (S = x_ref_points).
Prints one JSON line.

usage: python tools/dbl_probe.py [rounds]
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

SHAPES = [(1024, 20), (8192, 40), (65536, 40)]
INNER = 20  # back-to-back launches per timed interval


def buffers(B, N, dev):
    w = workload.make_batch(B, N, seed=77)
    T = lambda a, t: torch.from_numpy(np.ascontiguousarray(a.astype(t))).to(dev)  # noqa: E731
    f = tuple(T(w[k], np.float32) for k in ("x0", "u_lin", "x_ref"))
    d = tuple(T(w[k], np.float64) for k in ("x0", "u_lin", "x_ref"))
    out = (torch.empty(B, N, 2, device=dev), torch.empty(B, N + 1, 3, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev))
    return f, d, out


def launchers(s, f, d, out, stream, sync):
    L = s.lib
    tp, sp = capi._tp, C.c_void_p(stream.cuda_stream)
    B = f[0].shape[0]
    if sync:
        ff, fd = L.f110qp_solve_batch_dev_sync, L.f110qp_solve_batch_dev_sync_dbl
        af = (s._h, B, tp(f[0]), tp(f[1]), tp(f[2]), None, tp(out[0]), tp(out[1]), tp(out[2]), None, sp)
        ad = (s._h, B, tp(d[0]), tp(d[1]), tp(d[2]), None, tp(out[0]), tp(out[1]), tp(out[2]), None, sp)
    else:
        ff, fd = L.f110qp_solve_batch_dev, L.f110qp_solve_batch_dev_dbl
        af = (s._h, B, tp(f[0]), tp(f[1]), tp(f[2]), None, tp(out[0]), tp(out[1]), tp(out[2]), None, sp)
        ad = (s._h, B, tp(d[0]), tp(d[1]), tp(d[2]), None, tp(out[0]), tp(out[1]), tp(out[2]), None, None, None, sp)

    def call(fn, args):
        def go():
            if fn(*args) != capi.OK:
                raise capi.F110QPError(capi.last_error(L))
        return go
    return call(ff, af), call(fd, ad)


def kernel_times(B, N, rounds, dev):
    f, d, out = buffers(B, N, dev)
    s = capi.Solver(capi.default_config(N))
    stream = torch.cuda.current_stream(dev)
    lf, ld = launchers(s, f, d, out, stream, sync=False)
    for _ in range(10):
        lf()
        ld()
    torch.cuda.synchronize()
    assert (out[2].cpu().numpy() == capi.SOLVED).all()
    tf, td = [], []
    for _ in range(rounds):
        for go, acc in ((lf, tf), (ld, td)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(INNER):
                go()
            e1.record(stream)
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) * 1000.0 / INNER)
    info = s.backend_info(B) + (s.lane_segments(B),)
    s.close()
    mf, md = float(np.median(tf)), float(np.median(td))
    extra = 12 + 8 + 12 * N
    return dict(B=B, N=N, backend_info=info, float_us=round(mf, 2), dbl_us=round(md, 2), ratio=round(md / mf, 4),
                float_us_min_max=[round(min(tf), 2), round(max(tf), 2)], dbl_us_min_max=[round(min(td), 2), round(max(td), 2)],
                extra_input_bytes_per_qp=extra, extra_input_mib=round(B * extra / 2**20, 3))


def single_sync(N, reps, dev):
    f, d, out = buffers(1, N, dev)
    s = capi.Solver(capi.default_config(N))
    stream = torch.cuda.current_stream(dev)
    lf, ld = launchers(s, f, d, out, stream, sync=True)
    for _ in range(50):
        lf()
        ld()
    wf, wd = [], []
    for _ in range(reps):
        for go, acc in ((lf, wf), (ld, wd)):
            t0 = time.perf_counter()
            go()
            acc.append((time.perf_counter() - t0) * 1e6)
    s.close()
    pf, pd = float(np.percentile(wf, 50)), float(np.percentile(wd, 50))
    return dict(B=1, N=N, call="dev_sync", float_p50_us=round(pf, 2), dbl_p50_us=round(pd, 2), ratio=round(pd / pf, 4),
                float_p99_us=round(float(np.percentile(wf, 99)), 2), dbl_p99_us=round(float(np.percentile(wd, 99)), 2))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = [kernel_times(B, N, rounds, dev) for B, N in SHAPES]
    rows.append(single_sync(20, 50 * rounds, dev))
    print(json.dumps({"dbl_vs_float": rows}))


if __name__ == "__main__":
    main()
