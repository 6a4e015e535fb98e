"""Every closed-loop family's host-pointer call against its device-pointer call on MI355X, bit for bit.

The host calls (f110qp_rollout, _scan, _replan, _world, _race) stage their arrays through one table
(csrc/api_stage.h) into the context's device buffer, run the family's tick loop on those addresses and copy
the outputs back; the _dev calls run the same loop on the caller's tensors. So from the same start state every
array a host call returns must hold the bits the _dev call wrote, the in / out x_ref and have_path of the
re-planning families included, whichever optional arrays the call carries. "Wrote": a re-planning loop leaves
iters / cost / u_plan / x_plan of a tick without a solve and plan_status / best_traj / best_global of a tick without
a plan untouched (test_gpu_rollout_world.compare), so those are compared on the ticks of their kind; every other
array, and every array of the rollout and scan families, is compared whole.

B = 3, T = 3, N = 5: T*B*4 = 36 bytes is no multiple of 8, so the fields behind status / iters / kind stand on
padding, and row 0 of x_traj / u_lin_traj is the caller's while rows 1..T come back. Scans and worlds are the
existing rollout tests' (workload.make_scans, the loop cars of replan_cases, the track world, make_race_grid).
"""
import numpy as np
import pytest
import replan_cases as rp_
import rollout_scan_cases as rsc_
from test_gpu_rollout import solver
from test_gpu_rollout_race import race_case
from test_gpu_rollout_replan import P
from test_gpu_rollout_scan import scan_config
from test_gpu_rollout_world import GEOM, ON_MPC, ON_PLAN, R, world_case
from world_loop import call_dev

pytestmark = pytest.mark.gpu

B, T, N = 3, 3, 5

# (family, variant): scan_rows for scan / replan, world_rows for world, group_size for race
VARIANTS = [("rollout", 0), ("scan", 1), ("scan", T), ("replan", 1), ("replan", T), ("world", 1), ("world", B),
            ("race", 3)]


def _bits(t):
    import torch

    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _device_twin(cuda, host, x0, ul):
    """Device tensors of the host call's result arrays in their start state: outputs filled with a pattern no
    result holds, row 0 of the trajectories the start, x_ref / have_path as the host wrappers start them."""
    import torch

    d = {}
    for k, v in host.items():
        t = torch.from_numpy(v)
        d[k] = torch.full(t.shape, 77 if t.dtype == torch.int32 else -7.0, dtype=t.dtype, device=cuda)
    d["x_traj"][0], d["u_lin_traj"][0] = torch.from_numpy(x0).to(cuda), torch.from_numpy(ul).to(cuda)
    if "x_ref" in d:
        d["x_ref"].fill_(float("nan"))
        d["have_path"].zero_()
    return d


def _held_rows(capi, s_gap, scan):
    """Half-space rows for the plain rollout with gap rows active: the scan rollout's own rows of tick 0."""
    x0, ul, xr, ranges, geom = scan
    return s_gap.rollout_scan(x0, ul, xr, ranges, scan_config(capi, ranges.shape[-1], geom), 1)["hs_traj"][0]


def _run(capi, cuda, s, family, variant, on):
    """(host result dict, device tensors after the _dev call) of one family with its options all on or off."""
    import torch

    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    rc = capi.default_rollout_config(ticks=T)
    opt = dict(plans=on, objective=on)
    common = lambda d: (d["x_traj"], d["u_lin_traj"], d["u_applied"], d["status"], d["iters"], d.get("cost"),  # noqa: E731
                        d.get("u_plan"), d.get("x_plan"))
    if family in ("rollout", "scan"):
        scan = rsc_.scan_case(rsc_.SCAN_SEED, B, N)
        x0, ul, xr, ranges, geom = scan
        if family == "rollout":
            hs = _held_rows(capi, s, scan) if s.config.gap_mode == capi.GAP_ACTIVE else None
            host = s.rollout(x0, ul, xr, T, halfspace=hs, **opt)
            d = _device_twin(cuda, host, x0, ul)
            s.rollout_dev(rc, dev(xr), dev(hs), *common(d))
        else:
            if variant == T:  # a scan per tick, each tick's a little shorter
                ranges = np.ascontiguousarray(np.stack([ranges * np.float32(1.0 - 0.01 * t) for t in range(T)]))
            sc = scan_config(capi, ranges.shape[-1], geom, scan_rows=variant)
            host = s.rollout_scan(x0, ul, xr, ranges, sc, T, rows=on, **opt)
            d = _device_twin(cuda, host, x0, ul)
            s.rollout_scan_dev(rc, sc, dev(xr), dev(ranges.reshape(variant, B, -1)), *common(d), d.get("hs_traj"))
    else:
        opt["rows"] = on
        if family == "replan":
            x0, ul, ranges, geom, wp = rp_.replan_case(rp_.LOOP_POOL, rp_.LOOP_SEED, cars=rp_.LOOP_CARS[:B],
                                                       T=T if variant == T else None)
            sc = scan_config(capi, ranges.shape[-1], geom, scan_rows=variant)
        else:
            x0, ul, circles, wp = race_case(B, variant) if family == "race" else world_case(B, per_car=variant == B)
            sc = scan_config(capi, R, GEOM)
            opt["scans"] = on
        rp = capi.default_replan_config(num_waypoints=wp.shape[0])
        table = capi.traj_table(rp.plan)
        tail = lambda d: (d.get("hs_traj"), d["kind"], d["plan_status"], d["best_traj"], d["best_global"],  # noqa: E731
                          d["pose_traj"])
        if family == "replan":
            host = s.rollout_replan(x0, ul, ranges, sc, rp, table, wp, T, **opt)
            d = _device_twin(cuda, host, x0, ul)
            s.rollout_replan_dev(rc, sc, rp, dev(table), dev(wp), d["x_ref"], d["have_path"],
                                 dev(ranges.reshape(variant, B, -1)), *common(d), *tail(d))
        else:
            wc = capi.default_world_config(num_circles=circles.shape[-2],
                                           world_rows=1 if circles.ndim == 2 else circles.shape[0])
            race = capi.default_race_config(group_size=variant)
            if family == "race":
                host = s.rollout_race(x0, ul, circles, race, sc, rp, table, wp, T, **opt)
            else:
                host = s.rollout_world(x0, ul, circles, sc, rp, table, wp, T, **opt)
            d = _device_twin(cuda, host, x0, ul)
            call_dev(capi, s, family, dict(rc=rc, sc=sc, rp=rp, wc=wc, race=race), {"circles": dev(circles)}, dev(table),
                     dev(wp), d)
    torch.cuda.synchronize(cuda)
    return host, d


@pytest.mark.parametrize("on", [False, True], ids=["options_off", "options_on"])
@pytest.mark.parametrize("gap", [False, True], ids=["box", "gap"])
@pytest.mark.parametrize("family,variant", VARIANTS, ids=[f"{f}{v or ''}" for f, v in VARIANTS])
def test_host_call_equals_device_call(capi, cuda, family, variant, gap, on):
    import torch

    replanning = family in ("replan", "world", "race")
    s = solver(capi, N, gap=gap, **({"x_ref_points": P} if replanning else {}))
    host, d = _run(capi, cuda, s, family, variant, on)
    s.close()
    want = {"x_traj", "u_lin_traj", "u_applied", "status", "iters"}
    if on:
        want |= {"cost", "u_plan", "x_plan"} | ({"hs_traj"} if family != "rollout" else set())
        want |= {"ranges_traj"} if family in ("world", "race") else set()
    if replanning:
        want |= {"x_ref", "have_path", "kind", "plan_status", "best_traj", "best_global", "pose_traj"}
    assert set(host) == want
    assert (host["status"] != 77).all() and not (host["x_traj"] == -7.0).any()  # the loop ran and came back
    written = {}
    if replanning:
        kind = torch.from_numpy(host["kind"]).to(cuda)
        mpc, plan = kind == rp_.MPC, (kind == rp_.PLAN) | (kind == rp_.PLAN_FAILED)
        assert plan[0].all(), "every car starts without a path"
        written = {**{k: mpc for k in ON_MPC}, **{k: plan for k in ON_PLAN}}
    for k, v in host.items():
        h = torch.from_numpy(v).to(cuda)
        assert h.shape == d[k].shape and h.dtype == d[k].dtype, k
        a, b = (h[written[k]], d[k][written[k]]) if k in written else (h, d[k])
        assert torch.equal(_bits(a), _bits(b)), f"{family} {variant} gap={gap} options={on}: {k} differs"
