"""One Solver.rollout_<family>_dev call for the GPU tests of the eight world families (capi.WORLD_FAMILIES): what
the family takes is read off the table, what varies between the tests is a keyword."""
import world_cases as wc_
from test_gpu_rollout_replan import dev, full, replan_buffers
from test_gpu_rollout_scan import scan_config

R = 1080
GEOM = wc_.geometry(R)
OPTIONAL = ("iters", "cost", "u_plan", "x_plan", "hs_traj", "kind", "plan_status", "best_traj", "best_global",
            "pose_traj", "ranges_traj")


def call_dev(capi, s, family, cfg, world, table, wp, d):
    """s.rollout_<family>_dev, positionally as its signature stands: cfg {argument name: config} and world {array
    name: device tensor or None} hold at least what the family takes, d the device tensors under the host calls'
    keys (an optional one may be missing: NULL)."""
    names = [f.name for f in capi.WORLD_FAMILIES]
    fams = capi.WORLD_FAMILIES[:names.index(family) + 1]
    records = ("clear_traj", "crash_tick", "nearest_traj") if any(f.records for f in fams) else ()
    getattr(s, f"rollout_{family}_dev")(
        cfg["rc"], cfg["sc"], cfg["rp"], *(cfg[f.arg] for f in fams), table, wp, d["x_ref"], d["have_path"],
        *(world[f.array] for f in fams if f.array), d["x_traj"], d["u_lin_traj"], d["u_applied"], d["status"],
        *(d.get(k) for k in records + OPTIONAL))


def rollout_dev(capi, cuda, s, family, case, ticks, group=1, stop=0, margin=0.0, every=0, noise=None, grid=None,
                cfg=None, nearest=True, null=(), segments=True, start=None, scan_rows=1):
    """One rollout_<family>_dev call on fresh device arrays -> every array as numpy. case: (x0, u_lin, circles [C,3],
    [B,C,3] or None[, segments [S,4]], waypoints); null: the optional arrays passed as NULL; segments=False: none
    (S = 0, NULL); grid, cfg: the map and its workload.GridSpec; start: the result of a call to continue."""
    import torch

    x0, ul, circles, *sg, wp = case
    nb = x0.shape[0]
    if start is not None:
        x0, ul = start["x_traj"][-1], start["u_lin_traj"][-1]
    d = replan_buffers(cuda, x0, ul, nb, s.horizon, ticks)
    if start is not None:
        d["x_ref"], d["have_path"] = dev(cuda, start["x_ref"]), dev(cuda, start["have_path"])
    d["ranges_traj"] = full(cuda, (ticks, nb, R), torch.float32, -7.0)
    if family not in ("world", "race"):
        d["clear_traj"] = full(cuda, (ticks + 1, nb), torch.float64, -7.0)
        if nearest:
            d["nearest_traj"] = full(cuda, (ticks + 1, nb), torch.int32, -7)
        d["crash_tick"] = full(cuda, (nb,), torch.int32, -7)
    for k in null:
        del d[k]
    rp = capi.default_replan_config(num_waypoints=wp.shape[0])
    ns = sg[0].shape[0] if sg and segments else 0
    config = dict(rc=capi.default_rollout_config(ticks=ticks), sc=scan_config(capi, R, GEOM, scan_rows=scan_rows), rp=rp,
                  wc=capi.default_world_config(num_circles=0 if circles is None else circles.shape[-2],
                                               world_rows=1 if circles is None or circles.ndim == 2 else circles.shape[0]),
                  race=capi.default_race_config(group_size=group),
                  cc=capi.default_contact_config(stop_on_contact=stop, margin=margin), body=capi.default_body_config(),
                  walls=capi.default_walls_config(num_segments=ns), rf=capi.default_refresh_config(every=every),
                  noise=noise, grid_cfg=None if cfg is None else capi.grid_config_of(cfg))
    world = dict(circles=None if circles is None else dev(cuda, circles), segments=dev(cuda, sg[0]) if ns else None,
                 grid=dev(cuda, grid) if grid is not None and grid.size else None)
    call_dev(capi, s, family, config, world, dev(cuda, capi.traj_table(rp.plan)), dev(cuda, wp), d)
    torch.cuda.synchronize(cuda)
    return {k: v.cpu().numpy() for k, v in d.items()}
