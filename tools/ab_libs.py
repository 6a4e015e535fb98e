"""Same-process A/B of two builds of libf110qp.so on the lane back end's box-only solve, by HIP events.
Run:  python tools/ab_libs.py PARENT_SO BRANCH_SO OUT_JSON [B:N ...]
Per shape both libraries solve the same batch (make_batch, heading frame) through f110qp_solve_batch_dev;
the builds alternate in ROUNDS rounds of LAUNCHES back-to-back launches between two events, and the
figure of a round is its time per launch. Written per shape: median [min, max] over the rounds in us
for each build, each build's route (segments, fixed segment length, starts), whether status,
iters, u and x of the two builds are bit-identical, the largest absolute difference in u and x over
the QPs both solved, and the number of QPs whose iters differ."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f110-mpc_amd"))
from f110qp import capi, workload  # noqa: E402

ROUNDS, LAUNCHES, WARMUP = 15, 200, 50
parent, branch, out_path = sys.argv[1:4]
shapes = [tuple(int(v) for v in s.split(":")) for s in sys.argv[4:]] or [(1024, 20), (4096, 20), (1, 20), (8192, 40)]
torch.cuda.is_available()
dev = torch.device("cuda", 0)


def solver(path, N):
    capi.LIB_PATH = os.path.abspath(path)  # (capi.load caches per path: both builds stay loaded)
    return capi.Solver(capi.default_config(N, backend=capi.BACKEND_LANE), test_build=False)


res = []
for B, N in shapes:
    w = workload.make_batch(B, N, seed=5, heading="true", lateral=0.6, steer_range=0.4)
    x0, ul, xr = (torch.from_numpy(w[k]).to(dev) for k in ("x0", "u_lin", "x_ref"))
    runs = {}
    for name, path in (("parent", parent), ("branch", branch)):
        s = solver(path, N)
        o = dict(u=torch.empty((B, N, 2), dtype=torch.float32, device=dev),
                 x=torch.empty((B, N + 1, 3), dtype=torch.float32, device=dev),
                 st=torch.empty((B,), dtype=torch.int32, device=dev), it=torch.empty((B,), dtype=torch.int32, device=dev))
        runs[name] = (s, o, [s.lane_segments(B), s.lane_fixed_q(B), s.lane_starts(B)], [])

    def launch(name):
        s, o = runs[name][0], runs[name][1]
        s.solve_dev(x0, ul, xr, None, o["u"], o["x"], o["st"], o["it"])

    for name in runs:
        for _ in range(WARMUP):
            launch(name)
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        for name in ("parent", "branch") if r % 2 == 0 else ("branch", "parent"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                launch(name)
            e1.record()
            e1.synchronize()
            runs[name][3].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    host = {n: {k: v.cpu().numpy() for k, v in runs[n][1].items()} for n in runs}
    same = all(np.array_equal(host["parent"][k], host["branch"][k], equal_nan=True) for k in ("u", "x", "st", "it"))
    # the largest difference in u and x over the QPs both builds solved, and the QPs whose pass counts differ
    ok = (host["parent"]["st"] == 1) & (host["branch"]["st"] == 1)
    du, dx = (float(np.abs(host["parent"][k][ok].astype(np.float64) - host["branch"][k][ok]).max()) if ok.any() else 0.0
              for k in ("u", "x"))
    row = dict(B=B, N=N, rounds=ROUNDS, launches=LAUNCHES, outputs_bit_identical=bool(same),
               status_equal=bool(np.array_equal(host["parent"]["st"], host["branch"]["st"])),
               max_abs_diff_u=du, max_abs_diff_x=dx,
               iters_differ=int((host["parent"]["it"] != host["branch"]["it"]).sum()),
               iters_max=int(host["branch"]["it"].max()))
    for n in runs:
        t = np.array(runs[n][3])
        row[n + "_route"] = runs[n][2]
        row[n + "_us"] = [round(float(np.median(t)), 3), round(float(t.min()), 3), round(float(t.max()), 3)]
        runs[n][0].close()
    print(json.dumps(row), flush=True)
    res.append(row)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
