"""ctypes binding of libf110qp.so (include/f110qp.h).

This is the Python-side binding a maintainer would write over the C ABI; the product's
compute path is the HIP kernel behind it. There is no CPU fallback: if the library is
missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# F110QP_LIB selects a diagnostic build (e.g. lib_stamps/); default is the in-tree product library
LIB_PATH = os.environ.get("F110QP_LIB", os.path.join(PKG_ROOT, "lib", "libf110qp.so"))
# the test / measurement build (same kernels; f110qp_create also reads the F110QP_* knobs that force
# kernel variants). Solvers use it while USE_TEST_BUILD is true (the tests' `knob` fixture sets it).
TEST_LIB_PATH = os.environ.get("F110QP_TEST_LIB", os.path.join(PKG_ROOT, "lib_test", "libf110qp.so"))
USE_TEST_BUILD = False

OK = 0
ERR_INVALID = -1
ERR_HIP = -2
ERR_ALLOC = -3
SOLVED = 1
SOLVED_INACCURATE = 2
MAX_ITER = -2
PRIMAL_INFEASIBLE = -3
NUMERICAL = -10
GAP_INACTIVE = 0
GAP_ACTIVE = 1
BACKEND_AUTO = 0
BACKEND_WAVE = 1
BACKEND_LANE = 2
LANE_MIN_BATCH = 1024
LANE_MIN_BATCH_WIDE = 1
LANE_MIN_BATCH_GROUPED = LANE_MIN_BATCH
LANE_MIN_BATCH_GROUPED_WIDE = LANE_MIN_BATCH_WIDE
LANE_MAX_SMALL_BATCH = 8
GAP_SCREEN_MIN_BATCH = 1024
TICK_MPC = 0
TICK_PLAN = 1
TICK_HOLD = 2
TICK_PLAN_FAILED = 3
TICK_CRASHED = 4
NO_SOLVE = 0


def auto_backend(horizon: int, batch: int, gap: bool, grouped: bool = False) -> int:
    """The back end BACKEND_AUTO resolves to (mirrors resolve_backend() in f110qp_api.cpp)."""
    if grouped:
        min_b = LANE_MIN_BATCH_GROUPED if horizon <= 32 else LANE_MIN_BATCH_GROUPED_WIDE
    else:
        min_b = LANE_MIN_BATCH if horizon <= 32 else LANE_MIN_BATCH_WIDE
    small = not grouped and horizon <= 32 and batch <= LANE_MAX_SMALL_BATCH
    return BACKEND_LANE if (not gap and (batch >= min_b or small)) else BACKEND_WAVE


def auto_gap_screen(batch: int, grouped: bool = False, warm_start: bool = False) -> bool:
    """Whether AUTO takes the box screen for a gap-row call (mirrors gap_screen() in f110qp_api.cpp)."""
    return not grouped and not warm_start and batch >= GAP_SCREEN_MIN_BATCH


MAX_HORIZON = 48

# every symbol include/f110qp.h declares
EXPORTED = (
    "f110qp_version",
    "f110qp_last_error",
    "f110qp_default_config",
    "f110qp_create",
    "f110qp_destroy",
    "f110qp_solve_batch",
    "f110qp_solve_batch_dev",
    "f110qp_solve_batch_dev_sync",
    "f110qp_solve_grouped",
    "f110qp_solve_grouped_dev",
    "f110qp_condense_debug_dev",
    "f110qp_qp_dims",
    "f110qp_assemble_debug_dev",
    "f110qp_warm_reset",
    "f110qp_find_half_spaces",
    "f110qp_find_half_spaces_dev",
    "f110qp_default_plan_config",
    "f110qp_traj_table",
    "f110qp_parse_waypoints",
    "f110qp_plan_batch_dev",
    "f110qp_plan_batch",
    "f110qp_solve_batch_ex",
    "f110qp_solve_batch_ex_dev",
    "f110qp_solve_grouped_ex",
    "f110qp_solve_grouped_ex_dev",
    "f110qp_select_dev",
    "f110qp_backend_info",
    "f110qp_lane_segments",
    "f110qp_gap_screen",
    "f110qp_last_recheck_count",
    "f110qp_lane_starts",
    "f110qp_lane_fixed_q",
    "f110qp_warm_hits",
    "f110qp_sync_signals",
    "f110qp_test_build",
    "f110qp_solve_batch_dbl",
    "f110qp_solve_batch_dev_dbl",
    "f110qp_solve_batch_dev_sync_dbl",
    "f110qp_solve_grouped_dbl",
    "f110qp_solve_grouped_dev_dbl",
    "f110qp_default_rollout_config",
    "f110qp_advance_dev",
    "f110qp_rollout_dev",
    "f110qp_rollout",
    "f110qp_find_half_spaces_dev_dbl",
    "f110qp_default_scan_config",
    "f110qp_gap_search_dev",
    "f110qp_half_space_rows_dev",
    "f110qp_advance_scan_dev",
    "f110qp_rollout_scan_dev",
    "f110qp_rollout_scan",
    "f110qp_default_replan_config",
    "f110qp_plan_listed_dev",
    "f110qp_replan_start_dev",
    "f110qp_advance_replan_dev",
    "f110qp_rollout_replan_dev",
    "f110qp_rollout_replan",
    "f110qp_default_world_config",
    "f110qp_cast_scans_dev",
    "f110qp_rollout_world_dev",
    "f110qp_rollout_world",
    "f110qp_default_race_config",
    "f110qp_cast_scans_race_dev",
    "f110qp_rollout_race_dev",
    "f110qp_rollout_race",
    "f110qp_clearance_dev",
    "f110qp_default_contact_config",
    "f110qp_rollout_contact_dev",
    "f110qp_rollout_contact",
    "f110qp_default_body_config",
    "f110qp_clearance_body_dev",
    "f110qp_cast_scans_body_dev",
    "f110qp_rollout_body_dev",
    "f110qp_rollout_body",
    "f110qp_default_walls_config",
    "f110qp_cast_scans_walls_dev",
    "f110qp_clearance_walls_dev",
    "f110qp_rollout_walls_dev",
    "f110qp_rollout_walls",
    "f110qp_default_refresh_config",
    "f110qp_gap_refresh_dev",
    "f110qp_rollout_refresh_dev",
    "f110qp_rollout_refresh",
    "f110qp_default_noise_config",
    "f110qp_cast_scans_noisy_dev",
    "f110qp_rollout_noisy_dev",
    "f110qp_rollout_noisy",
    "f110qp_default_grid_config",
    "f110qp_cast_scans_grid_dev",
    "f110qp_clearance_grid_dev",
    "f110qp_rollout_grid_dev",
    "f110qp_rollout_grid",
    "f110qp_path_lengths",
    "f110qp_progress_dev",
    "f110qp_standings_dev",
    "f110qp_race_standings",
    "f110qp_default_mc_config",
    "f110qp_mc_fan_dev",
    "f110qp_mc_survival_dev",
    "f110qp_mc_outcomes_dev",
    "f110qp_mc_summary",
    "f110qp_grid_distance_dev",
    "f110qp_grid_inflate_dev",
    "f110qp_grid_lookup_dev",
    "f110qp_grid_field",
    "f110qp_wall_distance",
    "f110qp_grid_cast_dev",
    "f110qp_rollout_field_dev",
    "f110qp_rollout_field",
)
FIELD_MAX_SIDE = 32768  # F110QP_FIELD_MAX_SIDE
MC_MAX_HYPOTHESES = 4096  # F110QP_MC_MAX_HYPOTHESES
MC_MAX_PROBS = 8          # F110QP_MC_MAX_PROBS
CAST_CIRCLE_TILE = 256  # F110QP_CAST_CIRCLE_TILE: circles per LDS tile of the ray-cast kernel
SCRATCH_NAMES = {0: "none (wave back end)", 1: "LDS fp64", 2: "LDS fp32", 3: "HBM fp64", 4: "HBM fp32"}


class Config(C.Structure):
    _fields_ = [
        ("horizon", C.c_int),
        ("dt", C.c_float),
        ("q", C.c_double * 3),
        ("r", C.c_double * 2),
        ("u_des", C.c_double * 2),
        ("u_min", C.c_float * 2),
        ("u_max", C.c_float * 2),
        ("gap_mode", C.c_int),
        ("max_iter", C.c_int),
        ("device", C.c_int),
        ("warm_start", C.c_int),
        ("backend", C.c_int),
        ("x_ref_points", C.c_int),
    ]


class PlanConfig(C.Structure):
    _fields_ = [
        ("size", C.c_int),
        ("discrete", C.c_float),
        ("dilation", C.c_float),
        ("lookahead", C.c_float),
        ("speed_max", C.c_double),
        ("steer_max", C.c_double),
        ("steer_discrete", C.c_int),
        ("traj_discrete", C.c_int),
        ("dt", C.c_double),
    ]


class RolloutConfig(C.Structure):
    _fields_ = [
        ("ticks", C.c_int),
        ("plant_dt", C.c_double),
        ("car_length", C.c_double),
        ("v_lin", C.c_double),
        ("fail_u", C.c_double * 2),
    ]


class ScanConfig(C.Structure):
    _fields_ = [
        ("num_ranges", C.c_int),
        ("angle_min", C.c_float),
        ("angle_increment", C.c_float),
        ("angle_max", C.c_float),
        ("ftg_thresh", C.c_float),
        ("divider", C.c_float),
        ("buffer", C.c_float),
        ("scan_rows", C.c_int),
    ]


class ReplanConfig(C.Structure):
    _fields_ = [
        ("replan_dist", C.c_double),
        ("plan", PlanConfig),
        ("num_waypoints", C.c_int),
    ]


class WorldConfig(C.Structure):
    _fields_ = [
        ("num_circles", C.c_int),
        ("world_rows", C.c_int),
        ("lidar_offset", C.c_double),
        ("max_range", C.c_double),
    ]


class RaceConfig(C.Structure):
    _fields_ = [
        ("group_size", C.c_int),
        ("car_radius", C.c_double),
        ("center_offset", C.c_double),
    ]


class ContactConfig(C.Structure):
    _fields_ = [
        ("stop_on_contact", C.c_int),
        ("margin", C.c_double),
    ]


class BodyConfig(C.Structure):
    _fields_ = [
        ("half_length", C.c_double),
        ("half_width", C.c_double),
    ]


class WallsConfig(C.Structure):
    _fields_ = [
        ("num_segments", C.c_int),
        ("wall_rows", C.c_int),
    ]


class RefreshConfig(C.Structure):
    _fields_ = [
        ("every", C.c_int),
    ]


class NoiseConfig(C.Structure):
    _fields_ = [
        ("seed", C.c_ulonglong),
        ("car_base", C.c_longlong),
        ("sigma_abs", C.c_double),
        ("sigma_rel", C.c_double),
        ("dropout", C.c_double),
    ]


class GridConfig(C.Structure):
    _fields_ = [
        ("width", C.c_int),
        ("height", C.c_int),
        ("origin_x", C.c_double),
        ("origin_y", C.c_double),
        ("resolution", C.c_double),
        ("reach", C.c_double),
    ]


class McConfig(C.Structure):
    _fields_ = [
        ("hypotheses", C.c_int),
        ("group_size", C.c_int),
        ("num_probs", C.c_int),
        ("prob", C.c_double * MC_MAX_PROBS),
    ]


# f110qp_gap_record (16 bytes) as a numpy record
GAP_RECORD_DTYPE = np.dtype([("lo", np.int32), ("hi", np.int32), ("r_lo", np.float32), ("r_hi", np.float32)])


class F110QPError(RuntimeError):
    pass


# ---- the world families: the one table behind their bindings, checks and test helpers -------------------
# Each family is the one before it plus one config and, some, one world array and output records. A row says what
# its family adds; a family's entry points take what the rows up to its own add, in the rows' order.

class _Record(NamedTuple):
    name: str       # of the output record, in the ABI's order ([B], or [ticks + 1, B] with per_row)
    dtype: str
    per_row: bool
    optional: bool  # the _dev calls may pass None; the host calls return it on the flag of its name less "_traj"


class _Family(NamedTuple):
    name: str                      # f110qp_rollout_<name>[_dev]
    cfg: type                      # the config it adds ...
    arg: str                       # ... under this public argument name
    array: str | None = None       # the world array it adds behind the earlier ones (None where its count is 0)
    records: tuple = ()            # the output records it adds behind ranges_traj
    cast: str | None = None        # its cast entry point, if it has one
    clearance: str | None = None   # its clearance entry point, if it has one
    skips: tuple = ()              # the kinds of entry point ("cast", "clearance") that do not take cfg
    tick: bool = False             # the casts from here on take `tick` directly behind `batch`


WORLD_FAMILIES = (
    _Family("world", WorldConfig, "wc", array="circles", cast="f110qp_cast_scans_dev"),
    _Family("race", RaceConfig, "race", cast="f110qp_cast_scans_race_dev", clearance="f110qp_clearance_dev"),
    _Family("contact", ContactConfig, "cc", skips=("cast", "clearance"),
            records=(_Record("clear_traj", "f64", True, False), _Record("nearest_traj", "i32", True, True),
                     _Record("crash_tick", "i32", False, False))),
    _Family("body", BodyConfig, "body", cast="f110qp_cast_scans_body_dev", clearance="f110qp_clearance_body_dev"),
    _Family("walls", WallsConfig, "walls", array="segments", cast="f110qp_cast_scans_walls_dev",
            clearance="f110qp_clearance_walls_dev"),
    _Family("refresh", RefreshConfig, "rf", skips=("cast", "clearance")),
    _Family("noisy", NoiseConfig, "noise", cast="f110qp_cast_scans_noisy_dev", skips=("clearance",), tick=True),
    _Family("grid", GridConfig, "grid_cfg", array="grid", cast="f110qp_cast_scans_grid_dev",
            clearance="f110qp_clearance_grid_dev"),
)
_TRAJ = ("x_traj", "u_lin_traj", "u_applied", "status_traj", "iters_traj", "cost_traj", "u_plan", "x_plan")
_REC = ("hs_traj", "kind_traj", "plan_status_traj", "best_traj_traj", "best_global_traj", "pose_traj")
# the ctypes of the parameters that are no array (an array, the context and the stream: c_void_p)
_CTYPES = {"rc": C.POINTER(RolloutConfig), "sc": C.POINTER(ScanConfig), "rp": C.POINTER(ReplanConfig),
           "batch": C.c_int, "rows": C.c_int, "tick": C.c_int, **{f.arg: C.POINTER(f.cfg) for f in WORLD_FAMILIES}}


def _families(upto: str, kind: str = "rollout"):
    """The rows up to family `upto` whose config an entry point of `kind` takes."""
    n = [f.name for f in WORLD_FAMILIES].index(upto) + 1
    return [f for f in WORLD_FAMILIES[:n] if kind not in f.skips]


def _abi(kind: str, upto: str, dev: bool = True, field: bool = False):
    """The parameters of family `upto`'s entry point of `kind` ("rollout", "cast", "clearance") in the ABI's order,
    under their public names (dev: the call takes a stream). field: the grid family's calls through the map's
    distance field (f110qp_grid_cast_dev, f110qp_rollout_field_dev), with d2 behind grid and, the cast, visits behind
    ranges."""
    fams = _families(upto, kind)
    cfgs, arrays = [f.arg for f in fams], [f.array for f in fams if f.array]
    if field:
        arrays.append("d2")
    if kind == "cast":
        return ["sc", *cfgs, "batch", *(["tick"] if any(f.tick for f in fams) else []), "list_", "count", "x", *arrays,
                "ranges", *(["visits"] if field else []), "stream"]
    if kind == "clearance":
        return [*cfgs, "batch", "rows", "x", *arrays, "clearance", "nearest", "stream"]
    return ["ctx", "rc", "sc", "rp", *cfgs, "batch", "table", "waypoints", "x_ref", "have_path", *arrays, *_TRAJ, *_REC,
            "ranges_traj", *(r.name for f in fams for r in f.records), *(["stream"] if dev else [])]


def _abi_args(names, a):
    """The device call's values of the parameters `names` out of the arguments a: a config by reference, an int, the
    context and the stream as they are, a tensor's address."""
    return [a[n] if n in ("ctx", "stream") else int(a[n]) if _CTYPES.get(n) is C.c_int
            else C.byref(a[n]) if n in _CTYPES else _tp(a[n]) for n in names]


def _check_cfgs(fams, a, whole: bool):
    """The type check of the configs of the rows `fams` among the arguments a, in front of everything else. whole:
    the error is the rollout wrappers' sentence over all of them; otherwise it names the first wrong one."""
    wrong = [f for f in fams if not isinstance(a[f.arg], f.cfg)]
    if wrong:
        named = fams if whole else wrong[:1]
        said = [f"{f.arg} {'a' if i else 'must be a'} {f.cfg.__name__}" for i, f in enumerate(named)]
        raise F110QPError(", ".join(said[:-1]) + " and " + said[-1] if said[1:] else said[0])


# ---- the solve entry points: the one table behind their argtypes, the Solver's solve methods and its launchers ------
# A row per C symbol, saying what tells it from the others. Its parameters are ctx, batch, x0, u_lin, x_ref, halfspace,
# then group, num_groups if grouped, then u, x, status, iters, then obj, cost if ex, then stream if dev.

class _Solve(NamedTuple):
    symbol: str
    grouped: bool = False  # takes group, num_groups
    fin: str = "f32"       # the element type of x0 / u_lin / x_ref
    dev: bool = False      # device pointers and a stream (else host arrays, synchronous)
    ex: bool = False       # takes obj, cost
    sync: bool = False     # a device call that returns with the results in device memory


SOLVE_CALLS = (
    _Solve("f110qp_solve_batch"),
    _Solve("f110qp_solve_batch_ex", ex=True),
    _Solve("f110qp_solve_batch_dev", dev=True),
    _Solve("f110qp_solve_batch_ex_dev", dev=True, ex=True),
    _Solve("f110qp_solve_batch_dev_sync", dev=True, sync=True),
    _Solve("f110qp_solve_grouped", grouped=True),
    _Solve("f110qp_solve_grouped_ex", grouped=True, ex=True),
    _Solve("f110qp_solve_grouped_dev", grouped=True, dev=True),
    _Solve("f110qp_solve_grouped_ex_dev", grouped=True, dev=True, ex=True),
    _Solve("f110qp_solve_batch_dbl", fin="f64", ex=True),
    _Solve("f110qp_solve_batch_dev_dbl", fin="f64", dev=True, ex=True),
    _Solve("f110qp_solve_batch_dev_sync_dbl", fin="f64", dev=True, sync=True),
    _Solve("f110qp_solve_grouped_dbl", grouped=True, fin="f64", ex=True),
    _Solve("f110qp_solve_grouped_dev_dbl", grouped=True, fin="f64", dev=True, ex=True),
)
_SOLVE_SYMBOL = {row[1:]: row.symbol for row in SOLVE_CALLS}


def _solve_argtypes(row: _Solve):
    fp = C.c_void_p
    return [fp, C.c_int] + [fp] * 4 + [fp, C.c_int] * row.grouped + [fp] * 4 + [fp, fp] * row.ex + [fp] * row.dev


_libs = {}


def load(test: bool = False):
    """Load libf110qp.so (raises if it is missing: there is no fallback path). test=True: the
    test / measurement build lib_test/libf110qp.so."""
    path = TEST_LIB_PATH if test else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise F110QPError(f"{path} not built: run `make -C {PKG_ROOT}` (hipcc, gfx950)")
    L = C.CDLL(path)
    fp = C.c_void_p
    L.f110qp_version.restype = C.c_int
    L.f110qp_last_error.restype = C.c_char_p
    L.f110qp_default_config.argtypes = [C.POINTER(Config), C.c_int]
    L.f110qp_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Config)]
    L.f110qp_destroy.argtypes = [C.c_void_p]
    for row in SOLVE_CALLS:
        getattr(L, row.symbol).argtypes = _solve_argtypes(row)
    L.f110qp_default_rollout_config.argtypes = [C.POINTER(RolloutConfig)]
    L.f110qp_advance_dev.argtypes = [C.POINTER(RolloutConfig), C.c_int, C.c_int] + [fp] * 7
    L.f110qp_rollout_dev.argtypes = [C.c_void_p, C.POINTER(RolloutConfig), C.c_int] + [fp] * 11
    L.f110qp_rollout.argtypes = [C.c_void_p, C.POINTER(RolloutConfig), C.c_int] + [fp] * 10
    L.f110qp_default_scan_config.argtypes = [C.POINTER(ScanConfig)]
    L.f110qp_find_half_spaces_dev_dbl.argtypes = [C.c_int, fp, fp, C.c_int, C.c_float, C.c_float, C.c_float,
                                                  C.c_float, C.c_float, C.c_float, fp, fp, fp, fp]
    L.f110qp_gap_search_dev.argtypes = [C.POINTER(ScanConfig), C.c_int, fp, fp, fp]
    L.f110qp_half_space_rows_dev.argtypes = [C.POINTER(ScanConfig), C.c_int, fp, fp, fp, fp]
    L.f110qp_advance_scan_dev.argtypes = [C.POINTER(RolloutConfig), C.POINTER(ScanConfig), C.c_int, C.c_int] + [fp] * 9
    L.f110qp_rollout_scan_dev.argtypes = [C.c_void_p, C.POINTER(RolloutConfig), C.POINTER(ScanConfig), C.c_int] + [fp] * 12
    L.f110qp_rollout_scan.argtypes = [C.c_void_p, C.POINTER(RolloutConfig), C.POINTER(ScanConfig), C.c_int] + [fp] * 11
    rp, sp, rop = C.POINTER(ReplanConfig), C.POINTER(ScanConfig), C.POINTER(RolloutConfig)
    L.f110qp_default_replan_config.argtypes = [rp]
    L.f110qp_plan_listed_dev.argtypes = [rp, sp, C.c_int] + [fp] * 11
    L.f110qp_replan_start_dev.argtypes = [rp, sp, C.c_int] + [fp] * 10
    L.f110qp_advance_replan_dev.argtypes = [rop, rp, sp, C.c_int, C.c_int] + [fp] * 20
    L.f110qp_rollout_replan_dev.argtypes = [C.c_void_p, rop, sp, rp, C.c_int] + [fp] * 20
    L.f110qp_rollout_replan.argtypes = [C.c_void_p, rop, sp, rp, C.c_int] + [fp] * 19
    L.f110qp_gap_refresh_dev.argtypes = [sp, C.c_int] + [fp] * 5
    # the world families: every argument list from the table (tests/test_capi_families.py holds them to the header)
    for f in WORLD_FAMILIES:
        getattr(L, f"f110qp_default_{f.cfg.__name__[:-len('Config')].lower()}_config").argtypes = [C.POINTER(f.cfg)]
        for symbol, kind, dev in ((f"f110qp_rollout_{f.name}_dev", "rollout", True), (f.cast, "cast", True),
                                  (f"f110qp_rollout_{f.name}", "rollout", False), (f.clearance, "clearance", True)):
            if symbol:
                getattr(L, symbol).argtypes = [_CTYPES.get(n, fp) for n in _abi(kind, f.name, dev)]
    # the grid family's calls through the map's field: its lists with the one more array (the host call: its own)
    L.f110qp_grid_cast_dev.argtypes = [_CTYPES.get(n, fp) for n in _abi("cast", "grid", field=True)]
    L.f110qp_rollout_field_dev.argtypes = [_CTYPES.get(n, fp) for n in _abi("rollout", "grid", field=True)]
    L.f110qp_rollout_field.argtypes = [_CTYPES.get(n, fp) for n in _abi("rollout", "grid", dev=False)]
    rcp = C.POINTER(RaceConfig)
    L.f110qp_path_lengths.argtypes = [fp, C.c_int, fp]
    L.f110qp_progress_dev.argtypes = [C.c_int, C.c_int, fp, fp, fp, C.c_int] + [fp] * 4
    L.f110qp_standings_dev.argtypes = [rcp, C.c_int, C.c_int, fp, C.c_double] + [fp] * 4
    L.f110qp_race_standings.argtypes = [rcp, C.c_int, C.c_int, fp, fp, C.c_int] + [fp] * 6
    mcp = C.POINTER(McConfig)
    L.f110qp_default_mc_config.argtypes = [mcp]
    L.f110qp_default_mc_config.restype = None
    L.f110qp_mc_fan_dev.argtypes = [mcp, C.c_int, C.c_int] + [fp] * 4
    L.f110qp_mc_survival_dev.argtypes = [mcp, C.c_int, C.c_int] + [fp] * 4
    L.f110qp_mc_outcomes_dev.argtypes = [C.c_int, C.c_int] + [fp] * 9
    L.f110qp_mc_summary.argtypes = [mcp, C.c_int, C.c_int] + [fp] * 13
    gcp = C.POINTER(GridConfig)
    L.f110qp_grid_distance_dev.argtypes = [gcp] + [fp] * 5
    L.f110qp_grid_inflate_dev.argtypes = [gcp, fp, C.c_double, fp, fp]
    L.f110qp_grid_lookup_dev.argtypes = [gcp, fp, fp, C.c_int, C.c_int] + [fp] * 4
    L.f110qp_grid_field.argtypes = [gcp, fp, C.c_double] + [fp] * 3
    L.f110qp_wall_distance.argtypes = [gcp, fp, C.c_int, C.c_int] + [fp] * 3
    L.f110qp_select_dev.argtypes = [C.c_int, fp, C.c_int, fp, fp, fp, fp, fp]
    L.f110qp_backend_info.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3
    L.f110qp_lane_segments.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.f110qp_gap_screen.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.f110qp_last_recheck_count.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.f110qp_lane_starts.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.f110qp_lane_fixed_q.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.f110qp_warm_hits.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.f110qp_sync_signals.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    L.f110qp_test_build.restype = C.c_int
    L.f110qp_condense_debug_dev.argtypes = [C.c_void_p, C.c_int] + [fp] * 6
    L.f110qp_warm_reset.argtypes = [C.c_void_p]
    L.f110qp_qp_dims.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 4
    L.f110qp_assemble_debug_dev.argtypes = [C.c_void_p] + [fp] * 14
    L.f110qp_find_half_spaces.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int,
                                          C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.f110qp_find_half_spaces_dev.argtypes = [C.c_int, fp, fp, C.c_int, C.c_float, C.c_float, C.c_float,
                                              C.c_float, C.c_float, C.c_float, fp, fp, fp, fp]
    L.f110qp_default_plan_config.argtypes = [C.POINTER(PlanConfig)]
    L.f110qp_traj_table.argtypes = [C.POINTER(PlanConfig), fp]
    L.f110qp_parse_waypoints.argtypes = [C.c_char_p, fp, C.c_int, C.POINTER(C.c_int)]
    L.f110qp_plan_batch_dev.argtypes = [C.POINTER(PlanConfig), C.c_int, fp, fp, C.c_int, C.c_float, C.c_float,
                                        C.c_float, fp, fp, C.c_int, fp, fp, fp, fp, fp, fp, fp, fp]
    L.f110qp_plan_batch.argtypes = [C.POINTER(PlanConfig), C.c_int, fp, fp, C.c_int, C.c_float, C.c_float,
                                    C.c_float, fp, fp, C.c_int, fp, fp, fp, fp, fp, fp, fp]
    _libs[path] = L
    return L


def last_error(lib=None) -> str:
    return (lib or load()).f110qp_last_error().decode()


def _check(rc: int, what: str, lib=None):
    if rc != OK:
        raise F110QPError(f"{what} failed ({rc}): {last_error(lib)}")


def default_config(horizon: int, **over) -> Config:
    c = Config()
    load().f110qp_default_config(C.byref(c), horizon)
    for k, v in over.items():
        if k in ("q", "r", "u_des", "u_min", "u_max"):
            arr = getattr(c, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(c, k, v)
    return c


def default_rollout_config(**over) -> RolloutConfig:
    """f110qp_default_rollout_config: ticks 1, plant_dt 0.01, car_length 0.35, v_lin 4.5, fail_u
    (0.5, 0.0)."""
    c = RolloutConfig()
    load().f110qp_default_rollout_config(C.byref(c))
    for k, v in over.items():
        if k == "fail_u":
            c.fail_u[0], c.fail_u[1] = v
        else:
            setattr(c, k, v)
    return c


def default_scan_config(**over) -> ScanConfig:
    """f110qp_default_scan_config: ftg_thresh 3.0, divider 1.5, buffer 3.0, scan_rows 1, the scan's
    geometry (num_ranges, angle_min, angle_increment, angle_max) zero until the caller sets it."""
    c = ScanConfig()
    load().f110qp_default_scan_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def default_replan_config(**over) -> ReplanConfig:
    """f110qp_default_replan_config: replan_dist 1.98, the default plan config, num_waypoints 0. Keys of
    the plan config (size, discrete, ..., traj_discrete) set rp.plan's fields; plan=PlanConfig replaces
    it."""
    c = ReplanConfig()
    load().f110qp_default_replan_config(C.byref(c))
    names = {f[0] for f in PlanConfig._fields_}
    for k, v in over.items():
        if k == "plan":
            C.memmove(C.byref(c.plan), C.byref(v), C.sizeof(PlanConfig))
        elif k in names:
            setattr(c.plan, k, v)
        else:
            setattr(c, k, v)
    return c


def default_world_config(**over) -> WorldConfig:
    """f110qp_default_world_config: world_rows 1, lidar_offset 0.275, max_range 10.0, num_circles 0 (the
    caller's)."""
    c = WorldConfig()
    load().f110qp_default_world_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def default_race_config(**over) -> RaceConfig:
    """f110qp_default_race_config: group_size 1, car_radius 0.3, center_offset 0.1651."""
    c = RaceConfig()
    load().f110qp_default_race_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def default_mc_config(**over) -> McConfig:
    """f110qp_default_mc_config: hypotheses 1, group_size 1, num_probs 3, prob (0, 0.5, 1). prob=(...) sets the
    probabilities and, unless num_probs is given too, their number."""
    c = McConfig()
    load().f110qp_default_mc_config(C.byref(c))
    for k, v in over.items():
        if k == "prob":
            v = [float(p) for p in v]
            if len(v) > MC_MAX_PROBS:
                raise F110QPError(f"at most {MC_MAX_PROBS} probabilities, got {len(v)}")
            for i in range(MC_MAX_PROBS):
                c.prob[i] = v[i] if i < len(v) else 0.0
            if "num_probs" not in over:
                c.num_probs = len(v)
        else:
            setattr(c, k, v)
    return c


def default_contact_config(**over) -> ContactConfig:
    """f110qp_default_contact_config: stop_on_contact 0, margin 0.0."""
    c = ContactConfig()
    load().f110qp_default_contact_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def default_body_config(**over) -> BodyConfig:
    """f110qp_default_body_config: half_length 0.29, half_width 0.155."""
    c = BodyConfig()
    load().f110qp_default_body_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def default_walls_config(**over) -> WallsConfig:
    """f110qp_default_walls_config: num_segments 0 (the caller's), wall_rows 1."""
    c = WallsConfig()
    load().f110qp_default_walls_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def default_refresh_config(**over) -> RefreshConfig:
    """f110qp_default_refresh_config: every 0 (MPC keeps its first scan, the reference)."""
    c = RefreshConfig()
    load().f110qp_default_refresh_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def default_noise_config(**over) -> NoiseConfig:
    """f110qp_default_noise_config: all zero (no noise); seed, car_base, sigma_abs, sigma_rel, dropout."""
    c = NoiseConfig()
    load().f110qp_default_noise_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def default_grid_config(**over) -> GridConfig:
    """f110qp_default_grid_config: zeroes, then resolution 0.05 and reach 1.0; width, height, origin_x, origin_y."""
    c = GridConfig()
    load().f110qp_default_grid_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def grid_config_of(spec) -> GridConfig:
    """The GridConfig of anything with a map's fields (workload.GridSpec, as load_map and make_grid_world give)."""
    return default_grid_config(width=int(spec.width), height=int(spec.height), origin_x=float(spec.origin_x),
                               origin_y=float(spec.origin_y), resolution=float(spec.resolution),
                               reach=float(spec.reach))


def _grid_spec(gc, grid):
    if not isinstance(gc, GridConfig):
        raise F110QPError("grid_cfg must be a GridConfig")
    n = max(int(gc.width), 0) * max(int(gc.height), 0)
    return (grid, "u8", n, "grid", n == 0)


def _field_spec(gc, d2):
    """The _devs spec of the map's distance field d2 [H,W] i32 (None for an empty map)."""
    n = max(int(gc.width), 0) * max(int(gc.height), 0)
    return (d2, "i32", n, "d2", n == 0)


def _wall_spec(walls, segments):
    if not isinstance(walls, WallsConfig):
        raise F110QPError("walls must be a WallsConfig")
    Sn = int(walls.num_segments)
    return (segments, "f64", 4 * max(Sn, 0) * max(int(walls.wall_rows), 0), "segments", Sn <= 0)


def _circle_spec(wc, circles):
    Cn = int(wc.num_circles)
    return (circles, "f64", 3 * max(Cn, 0) * max(int(wc.world_rows), 0), "circles", Cn <= 0)


def _world_specs(fams, a):
    """The _devs specs of the world arrays of the rows `fams`, each sized by its row's config."""
    spec = {"circles": _circle_spec, "segments": _wall_spec, "grid": _grid_spec}
    return [spec[f.array](a[f.arg], a[f.array]) for f in fams if f.array]


def _host_circles(a, B):
    """(world config, circles) of a host rollout: a copy of wc (default: f110qp_default_world_config) with the
    counts of the checked array."""
    circles, wc = a["circles"], a["wc"]
    if not isinstance(circles, np.ndarray) or circles.dtype != np.float64 or circles.ndim not in (2, 3) \
            or circles.shape[-1] != 3:
        raise F110QPError("circles must be a float64 numpy array [C, 3] or [B, C, 3]")
    ci = np.ascontiguousarray(circles)
    w = WorldConfig()
    C.memmove(C.byref(w), C.byref(wc if wc is not None else default_world_config()), C.sizeof(w))
    w.num_circles = ci.shape[-2]
    w.world_rows = 1 if ci.ndim == 2 else ci.shape[0]
    if w.world_rows not in (1, B):
        raise F110QPError(f"circles must hold one world or B = {B} worlds, got {w.world_rows}")
    return w, ci


def _host_segments(a, B):
    """(walls config, segments) of a host rollout, the config built from the checked array."""
    segments = a["segments"]
    if not isinstance(segments, np.ndarray) or segments.dtype != np.float64 or segments.ndim not in (2, 3) \
            or segments.shape[-1] != 4:
        raise F110QPError("segments must be a float64 numpy array [S, 4] or [B, S, 4]")
    sg = np.ascontiguousarray(segments)
    wl = default_walls_config(num_segments=sg.shape[-2], wall_rows=1 if sg.ndim == 2 else sg.shape[0])
    if wl.wall_rows not in (1, B):
        raise F110QPError(f"segments must hold one set or B = {B} sets, got {wl.wall_rows}")
    return wl, sg


def _host_grid(a, B):
    """(grid config, map [H,W] uint8) of a host rollout, the caller's config and the checked array."""
    gc, gm = a["grid_cfg"], np.ascontiguousarray(a["grid"], np.uint8)
    if gm.shape != (int(gc.height), int(gc.width)) and gm.size:
        raise F110QPError(f"grid must be [height, width] = [{gc.height}, {gc.width}], got {gm.shape}")
    return gc, gm


_HOST_WORLD = {"circles": _host_circles, "segments": _host_segments, "grid": _host_grid}


def _check_race(race, B):
    G = int(race.group_size)
    if G < 1 or B % G:
        raise F110QPError(f"group_size must be >= 1 and divide B = {B}, got {G}")


def qp_dims(horizon: int):
    """(n, m, nnz_P, nnz_A) of the reference's OSQP problem (f110qp_qp_dims)."""
    v = [C.c_int() for _ in range(4)]
    _check(load().f110qp_qp_dims(horizon, *[C.byref(x) for x in v]), "f110qp_qp_dims")
    return tuple(x.value for x in v)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _f64(a, shape, name: str):
    """A host input of a *_dbl call: a float64 numpy array, taken as it is (no cast: a float32 array
    here is a caller that has already lost what these entry points exist to keep)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float64:
        got = a.dtype if isinstance(a, np.ndarray) else type(a).__name__
        raise F110QPError(f"{name} must be a float64 numpy array, got {got}")
    return np.ascontiguousarray(a).reshape(shape)


def _f32(a, shape, name: str):
    """A host input of a float32 call: anything numpy casts to float32."""
    return np.ascontiguousarray(a, np.float32).reshape(shape)


def _tp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(t, dtype: str, n: int, name: str, optional: bool = False, where: bool = False):
    """Check a device tensor before its raw pointer crosses the C ABI: a contiguous CUDA (HIP)
    tensor of the ABI's element type with at least n elements (the kernels write / read exactly
    that many; a float32 tensor where the ABI wants float64, or an int64 one where it wants int32,
    would be an out-of-bounds write or a silent misread)."""
    if t is None:
        if optional:
            return
        raise F110QPError(f"{name} is required")
    import torch

    want = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "u8": torch.uint8}[dtype]
    if not isinstance(t, torch.Tensor):
        raise F110QPError(f"{name} must be a torch tensor on the device, got {type(t).__name__}")
    if t.dtype != want:
        raise F110QPError(f"{name} must be {want}, got {t.dtype}")
    if not t.is_contiguous():
        raise F110QPError(f"{name} must be contiguous")
    if t.numel() < n:
        raise F110QPError(f"{name} holds {t.numel()} elements, the call needs {n}")
    if where and t.device.type != "cuda":
        raise F110QPError(f"{name} must be a device (cuda/HIP) tensor, got {t.device}")


def _devs(*specs):
    """_dev over several (tensor, dtype, n, name[, optional]) specs: every type / size check
    first, then the placement of each (so a host-side test sees the type errors)."""
    for sp in specs:
        _dev(*sp)
    for sp in specs:
        _dev(*sp[:4], *(sp[4:] or (False,)), where=True)


class Solver:
    """One f110qp context (device workspace). Mirrors the reference's OsqpEigen::Solver
    member of MPC (include/f110-mpc/mpc.h:63) for B instances at once."""

    def __init__(self, config: Config, test_build: bool | None = None):
        self.lib = load(USE_TEST_BUILD if test_build is None else test_build)
        self.config = config
        h = C.c_void_p()
        self._chk = lambda rc, what: _check(rc, what, self.lib)
        self._chk(self.lib.f110qp_create(C.byref(h), C.byref(config)), "f110qp_create")
        self._h = h

    @property
    def horizon(self) -> int:
        return self.config.horizon

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.f110qp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def backend_info(self, batch: int, grouped: bool = False):
        """(backend, qps_per_wave, scratch) of a solve call of `batch` QPs (f110qp_backend_info)."""
        v = [C.c_int() for _ in range(3)]
        self._chk(self.lib.f110qp_backend_info(self._h, int(batch), int(grouped), *[C.byref(x) for x in v]),
               "f110qp_backend_info")
        return tuple(x.value for x in v)

    def lane_segments(self, batch: int) -> int:
        """Horizon segments per QP of a solve call of `batch` QPs (f110qp_lane_segments): 1, or
        2 / 4 / 8 when the lane back end runs the partitioned Riccati (lane_seg_kernel.h)."""
        v = C.c_int()
        self._chk(self.lib.f110qp_lane_segments(self._h, int(batch), C.byref(v)), "f110qp_lane_segments")
        return v.value

    def lane_starts(self, batch: int) -> int:
        """PDAS starts per QP of a solve call of `batch` QPs (f110qp_lane_starts): 2 with the
        partitioned-horizon kernel's twin start, else 1."""
        v = C.c_int()
        self._chk(self.lib.f110qp_lane_starts(self._h, int(batch), C.byref(v)), "f110qp_lane_starts")
        return v.value

    def lane_fixed_q(self, batch: int) -> int:
        """Stages per segment when a solve call of `batch` QPs runs a partitioned-horizon kernel
        compiled for a fixed segment length (f110qp_lane_fixed_q): 5, else 0."""
        v = C.c_int()
        self._chk(self.lib.f110qp_lane_fixed_q(self._h, int(batch), C.byref(v)), "f110qp_lane_fixed_q")
        return v.value

    def last_recheck_count(self) -> int:
        """QPs the last gap-row call sent to the fp64 re-check (f110qp_last_recheck_count;
        synchronises with that call)."""
        v = C.c_int()
        self._chk(self.lib.f110qp_last_recheck_count(self._h, C.byref(v)), "f110qp_last_recheck_count")
        return v.value

    def warm_hits(self):
        """(traffic_calls, hits) since the previous warm_hits (f110qp_warm_hits)."""
        t, h = C.c_int(), C.c_int()
        self._chk(self.lib.f110qp_warm_hits(self._h, C.byref(t), C.byref(h)), "f110qp_warm_hits")
        return t.value, h.value

    def sync_signals(self) -> int:
        """Synchronous calls on this solver that waited on the kernel's completion word instead of
        synchronising the stream (f110qp_sync_signals)."""
        n = C.c_uint()
        self._chk(self.lib.f110qp_sync_signals(self._h, C.byref(n)), "f110qp_sync_signals")
        return n.value

    @property
    def test_build(self) -> bool:
        return bool(self.lib.f110qp_test_build())

    def gap_screen(self, batch: int) -> bool:
        """Does a gap-row solve call of `batch` QPs take the box screen on the lane back end before
        the wave kernel's GI (f110qp_gap_screen)?"""
        v = C.c_int()
        self._chk(self.lib.f110qp_gap_screen(self._h, int(batch), C.byref(v)), "f110qp_gap_screen")
        return bool(v.value)

    # ---- the solve family: one host body and one device body, both reading SOLVE_CALLS --------------------------

    def _check_dev(self, x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters=None, obj=None, cost=None,
                   group=None, fin="f32"):
        """Shapes, element types and placement of a device call's tensors (see _dev). fin: the
        element type of x0 / u_lin / x_ref ("f64" for the *_dbl calls)."""
        B = int(x0.shape[0])
        N = self.horizon
        S = self.config.x_ref_points or N
        specs = [(x0, fin, 3 * B, "x0"), (u_lin, fin, 2 * B, "u_lin"), (x_ref, fin, 3 * S * B, "x_ref"),
                 (halfspace, "f32", 6 * B, "halfspace", self.config.gap_mode == GAP_INACTIVE),
                 (u_out, "f32", 2 * N * B, "u_out"), (x_out, "f32", 3 * (N + 1) * B, "x_out"),
                 (status, "i32", B, "status"), (iters, "i32", B, "iters", True), (obj, "f64", B, "obj", True),
                 (cost, "f64", B, "cost", True)]
        if group is not None:
            specs.append((group, "i32", B, "group"))
        _devs(*specs)
        return B

    @staticmethod
    def _stream(stream, t):
        """The stream argument of a device call: `stream`, or the current stream of tensor t's device."""
        import torch

        return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(t.device)).cuda_stream)

    def _solve_host(self, fin, x0, u_lin, x_ref, halfspace, objective, grp=None):
        """The body of the four host solves. fin: "f32" casts x0 / u_lin / x_ref, "f64" takes float64 only and always
        calls the symbol with obj / cost (null without objective); grp = (group, num_groups): a grouped call."""
        N = self.horizon
        arr = _f64 if fin == "f64" else _f32
        x0 = arr(x0, (-1, 3), "x0")
        B = x0.shape[0]
        ul = arr(u_lin, (B, 2), "u_lin")
        xr = arr(x_ref, (B, self.config.x_ref_points or N, 3), "x_ref")
        hs = None if halfspace is None else np.ascontiguousarray(halfspace, np.float32).reshape(B, 6)
        groups = []
        if grp is not None:
            g = np.ascontiguousarray(grp[0], np.int32).reshape(B)
            groups = [_p(g), int(g.max()) + 1 if grp[1] is None else int(grp[1])]
        out = [np.empty((B, N, 2), np.float32), np.empty((B, N + 1, 3), np.float32), np.empty(B, np.int32),
               np.empty(B, np.int32)]
        oc = [np.empty(B, np.float64) if objective else None for _ in range(2)]
        ex = bool(objective) or fin == "f64"
        name = _SOLVE_SYMBOL[grp is not None, fin, False, ex, False]
        self._chk(getattr(self.lib, name)(self._h, B, _p(x0), _p(ul), _p(xr), _p(hs), *groups, *map(_p, out),
                                          *map(_p, oc if ex else [])), name)
        return tuple(out + oc) if objective else tuple(out)

    def _solve_dev_call(self, fin, x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters, stream, obj=None,
                        cost=None, grp=None, sync=False):
        """(C function, its name, its converted arguments) of a device solve, the tensors checked. The symbol takes
        obj / cost when one is given and, for fin "f64", always; a sync symbol never does."""
        ex = (fin == "f64" or obj is not None or cost is not None) and not sync
        name = _SOLVE_SYMBOL[grp is not None, fin, True, ex, sync]
        if sync and (obj is not None or cost is not None):
            raise F110QPError(f"{name} has no obj / cost outputs")
        B = self._check_dev(x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters, obj, cost,
                            group=grp[0] if grp is not None else None, fin=fin)
        stream = self._stream(stream, x0)
        args = [self._h, B, _tp(x0), _tp(u_lin), _tp(x_ref), _tp(halfspace)]
        if grp is not None:
            args += [_tp(grp[0]), int(grp[1])]
        args += [_tp(u_out), _tp(x_out), _tp(status), _tp(iters)]
        if ex:
            args += [_tp(obj), _tp(cost)]
        return getattr(self.lib, name), name, (*args, stream)

    def _solve_dev(self, *a, **k):
        """The body of the four device solves: one checked C call."""
        fn, name, args = self._solve_dev_call(*a, **k)
        self._chk(fn(*args), name)

    def _launcher(self, what, *a, **k):
        """The body of the two prepare_*: everything converted here, the closure one C call."""
        fn, _, args = self._solve_dev_call("f32", *a, **k)

        def launch():
            rc = fn(*args)
            if rc != OK:
                _check(rc, what, self.lib)
        return launch

    def solve(self, x0, u_lin, x_ref, halfspace=None, objective=False):
        """Host arrays in, host arrays out (synchronous). Returns (u[B,N,2], x[B,N+1,3],
        status[B], iters[B]) and, with objective=True, also (obj[B], cost[B]) float64
        (f110qp_solve_batch_ex)."""
        return self._solve_host("f32", x0, u_lin, x_ref, halfspace, objective)

    def solve_dbl(self, x0, u_lin, x_ref, halfspace=None, objective=False):
        """solve() on float64 x0 / u_lin / x_ref, passed unrounded (f110qp_solve_batch_dbl); any
        other element type is rejected. Outputs as solve()."""
        return self._solve_host("f64", x0, u_lin, x_ref, halfspace, objective)

    def solve_grouped(self, x0, u_lin, x_ref, group, num_groups=None, halfspace=None, objective=False):
        """Grouped solve on host arrays (f110qp_solve_grouped): group [B] int scenario ids.
        objective=True also returns (obj[B], cost[B]) (f110qp_solve_grouped_ex)."""
        return self._solve_host("f32", x0, u_lin, x_ref, halfspace, objective, (group, num_groups))

    def solve_grouped_dbl(self, x0, u_lin, x_ref, group, num_groups=None, halfspace=None, objective=False):
        """solve_grouped() on float64 x0 / u_lin / x_ref (f110qp_solve_grouped_dbl)."""
        return self._solve_host("f64", x0, u_lin, x_ref, halfspace, objective, (group, num_groups))

    def solve_dev(self, x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters=None, stream=None,
                  obj=None, cost=None):
        """Device (torch) tensors in/out, enqueued on `stream` (torch.cuda stream or None =
        current stream). Asynchronous. obj / cost: optional float64 [B] device tensors
        (f110qp_solve_batch_ex_dev)."""
        self._solve_dev("f32", x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters, stream, obj, cost)

    def solve_dev_dbl(self, x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters=None, stream=None,
                      obj=None, cost=None, sync=False):
        """solve_dev() on float64 device tensors x0 / u_lin / x_ref (f110qp_solve_batch_dev_dbl);
        sync=True: f110qp_solve_batch_dev_sync_dbl (returns with the results in device memory; no
        obj / cost)."""
        self._solve_dev("f64", x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters, stream, obj, cost, sync=sync)

    def solve_grouped_dev(self, x0, u_lin, x_ref, halfspace, group, num_groups, u_out, x_out, status, iters=None,
                          stream=None, obj=None, cost=None):
        """Grouped solve on device (torch) tensors; group [B] int32 on the device; obj / cost
        optional float64 [B] (f110qp_solve_grouped_ex_dev)."""
        self._solve_dev("f32", x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters, stream, obj, cost,
                        (group, num_groups))

    def solve_grouped_dev_dbl(self, x0, u_lin, x_ref, halfspace, group, num_groups, u_out, x_out, status,
                              iters=None, stream=None, obj=None, cost=None):
        """solve_grouped_dev() on float64 device tensors x0 / u_lin / x_ref
        (f110qp_solve_grouped_dev_dbl)."""
        self._solve_dev("f64", x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters, stream, obj, cost,
                        (group, num_groups))

    def prepare_dev(self, x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters=None, stream=None,
                    sync=False):
        """A launcher for repeated f110qp_solve_batch_dev calls on the same device buffers: the
        ctypes arguments are converted once, each call is one C call (what a C++ caller of the ABI
        pays; bench.py's timed steps use it so Python argument marshalling is not the step).
        sync=True: f110qp_solve_batch_dev_sync (returns with the results in device memory)."""
        return self._launcher("f110qp_solve_batch_dev", x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters,
                              stream, sync=sync)

    def prepare_grouped_dev(self, x0, u_lin, x_ref, halfspace, group, num_groups, u_out, x_out, status,
                            iters=None, stream=None):
        """prepare_dev for f110qp_solve_grouped_dev."""
        return self._launcher("f110qp_solve_grouped_dev", x0, u_lin, x_ref, halfspace, u_out, x_out, status, iters,
                              stream, grp=(group, num_groups))

    def assemble_debug(self, x0, u_lin, x_ref, halfspace=None):
        """f110qp_assemble_debug_dev for one instance (host arrays in; the device computes; host
        dict of the CSC arrays out, the oracle.assemble layout)."""
        import torch

        N = self.horizon
        n, m, nzp, nza = qp_dims(N)
        dev = torch.device("cuda", self.config.device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).to(dev)  # noqa: E731
        x0d, uld, xrd = t(x0), t(u_lin), t(x_ref)
        hsd = None if halfspace is None else t(halfspace)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731
        f64 = lambda k: torch.empty(k, dtype=torch.float64, device=dev)  # noqa: E731
        out = {"P_colptr": i32(n + 1), "P_rowind": i32(nzp), "P_val": f64(nzp), "q": f64(n), "A_colptr": i32(n + 1),
               "A_rowind": i32(nza), "A_val": f64(nza), "l": f64(m), "u": f64(m)}
        self._chk(self.lib.f110qp_assemble_debug_dev(self._h, _tp(x0d), _tp(uld), _tp(xrd), _tp(hsd),
                                                     *map(_tp, out.values()), self._stream(None, x0d)),
                  "f110qp_assemble_debug_dev")
        torch.cuda.synchronize(dev)
        return {k: v.cpu().numpy() for k, v in out.items()}

    # ---- the closed-loop families: what their bindings share ------------------------------------------
    # rollout, rollout_scan and rollout_replan (and their _dev calls) use these pieces by hand. The eight world
    # families behind them use them through two bodies, _world_dev and _world_host, which read what a family takes
    # off WORLD_FAMILIES: a new family is a row there and a pair of wrappers that hand their arguments over by name.

    @staticmethod
    def _dev_loop(rc, x_ref, x_traj, scan=None):
        """(T, B) of a rollout_*_dev call, checked: ticks, x_traj's shape and, with scan = (sc, ranges),
        scan_rows and the shape of ranges."""
        T = int(rc.ticks)
        if T < 1:
            raise F110QPError("ticks must be >= 1")
        B = int(x_ref.shape[0])
        if scan is not None:
            sc, ranges = scan
            R, NR = int(sc.scan_rows), int(sc.num_ranges)
            if R not in (1, T):
                raise F110QPError(f"scan_rows must be 1 or ticks = {T}, got {R}")
        if tuple(x_traj.shape) != (T + 1, B, 3):
            raise F110QPError(f"x_traj must be [ticks + 1, B, 3] = {(T + 1, B, 3)}, got {tuple(x_traj.shape)}")
        if scan is not None and tuple(ranges.shape) != (R, B, NR):
            raise F110QPError(f"ranges must be [scan_rows, B, num_ranges] = {(R, B, NR)}, got {tuple(ranges.shape)}")
        return T, B

    def _traj_specs(self, T, B, x_traj, u_lin_traj, u_applied, status_traj, iters_traj, cost_traj, u_plan, x_plan):
        """The _devs specs of the arrays every family records (a new per-tick array: one spec here or in
        _record_specs)."""
        N = self.horizon
        return [(x_traj, "f64", 3 * B * (T + 1), "x_traj"), (u_lin_traj, "f64", 2 * B * (T + 1), "u_lin_traj"),
                (u_applied, "f32", 2 * B * T, "u_applied"), (status_traj, "i32", B * T, "status_traj"),
                (iters_traj, "i32", B * T, "iters_traj", True), (cost_traj, "f64", B * T, "cost_traj", True),
                (u_plan, "f32", 2 * N * B * T, "u_plan", True), (x_plan, "f32", 3 * (N + 1) * B * T, "x_plan", True)]

    @staticmethod
    def _plan_specs(rp, B, table, waypoints, x_ref, have_path):
        """The _devs specs of what a re-planning family reads and carries over."""
        P, Tc, W = int(rp.plan.traj_discrete), int(rp.plan.steer_discrete) + 1, int(rp.num_waypoints)
        return [(table, "f64", 3 * P * Tc, "table"), (waypoints, "f64", 2 * W, "waypoints", W == 0),
                (x_ref, "f64", 3 * P * B, "x_ref"), (have_path, "i32", B, "have_path")]

    @staticmethod
    def _record_specs(T, B, hs_traj, kind_traj, plan_status_traj, best_traj_traj, best_global_traj, pose_traj):
        """The _devs specs of a re-planning family's optional records."""
        return [(hs_traj, "f32", 6 * B * T, "hs_traj", True), (kind_traj, "i32", B * T, "kind_traj", True),
                (plan_status_traj, "i32", B * T, "plan_status_traj", True),
                (best_traj_traj, "i32", B * T, "best_traj_traj", True),
                (best_global_traj, "i32", B * T, "best_global_traj", True),
                (pose_traj, "f64", 4 * B * (T + 1), "pose_traj", True)]

    @staticmethod
    def _host_start(x0, u_lin, ticks):
        """(T, B, x0, u_lin) of a host rollout: float64 x0 [B,3] and u_lin [B,2]."""
        T = int(ticks)
        if T < 1:
            raise F110QPError("ticks must be >= 1")
        x0 = _f64(x0, (-1, 3), "x0")
        return T, x0.shape[0], x0, _f64(u_lin, (x0.shape[0], 2), "u_lin")

    @staticmethod
    def _host_ranges(ranges, sc, T, B):
        R = int(sc.scan_rows)
        if R not in (1, T):
            raise F110QPError(f"scan_rows must be 1 or ticks = {T}, got {R}")
        rg = np.ascontiguousarray(ranges, np.float32)
        if rg.size != R * B * int(sc.num_ranges):
            raise F110QPError(f"ranges must hold [scan_rows, B, num_ranges] = {(R, B, int(sc.num_ranges))} values, "
                              f"got shape {rg.shape}")
        return rg

    @staticmethod
    def _host_plan(rp, B, table, waypoints, x_ref, have_path):
        """(x_ref, have_path, table, waypoints) of a host re-planning rollout: the paths the cars hold (copies:
        the call updates them; default none) and the checked table and waypoints."""
        P, Tc, W = int(rp.plan.traj_discrete), int(rp.plan.steer_discrete) + 1, int(rp.num_waypoints)
        xr = np.full((B, P, 3), np.nan) if x_ref is None else _f64(x_ref, (B, P, 3), "x_ref").copy()
        hv = np.zeros(B, np.int32) if have_path is None else np.array(have_path, np.int32).reshape(B)
        tab = _f64(table, (Tc, P, 3), "table")
        wp = np.ascontiguousarray(np.asarray(waypoints, np.float64)[:, :2])
        if wp.shape[0] != W:
            raise F110QPError(f"waypoints must hold num_waypoints = {W} rows, got {wp.shape[0]}")
        return xr, hv, tab, wp

    @staticmethod
    def _ticks_config(rc, T):
        """A copy of rc (default: f110qp_default_rollout_config) with its ticks replaced."""
        cfg = RolloutConfig()
        C.memmove(C.byref(cfg), C.byref(rc if rc is not None else default_rollout_config()), C.sizeof(cfg))
        cfg.ticks = T
        return cfg

    def _host_out(self, T, B, x0, ul, objective, plans, rows=False, scans=0, paths=None):
        """The result dict of a host rollout, row 0 of the trajectories set. paths = (x_ref, have_path): a
        re-planning family, with its records; scans: num_ranges of ranges_traj, 0 for none."""
        N = self.horizon
        i32 = lambda: np.empty((T, B), np.int32)  # noqa: E731
        out = {"x_traj": np.empty((T + 1, B, 3), np.float64), "u_lin_traj": np.empty((T + 1, B, 2), np.float64),
               "u_applied": np.empty((T, B, 2), np.float32), "status": i32(), "iters": i32()}
        if paths is not None:
            out.update({"x_ref": paths[0], "have_path": paths[1], "kind": i32(), "plan_status": i32(),
                        "best_traj": i32(), "best_global": i32(), "pose_traj": np.empty((T + 1, B, 4), np.float64)})
        out["x_traj"][0], out["u_lin_traj"][0] = x0, ul
        if objective:
            out["cost"] = np.empty((T, B), np.float64)
        if plans:
            out["u_plan"] = np.empty((T, B, N, 2), np.float32)
            out["x_plan"] = np.empty((T, B, N + 1, 3), np.float32)
        if rows:
            out["hs_traj"] = np.empty((T, B, 2, 3), np.float32)
        if scans:
            out["ranges_traj"] = np.empty((T, B, scans), np.float32)
        return out

    @staticmethod
    def _out_args(out):
        """The result dict's arrays in the ABI's order (the nine's seven outputs, then hs_traj and, for a
        re-planning family, its records)."""
        a = [_p(out["x_traj"]), _p(out["u_lin_traj"]), _p(out["u_applied"]), _p(out["status"]), _p(out["iters"]),
             _p(out.get("cost")), _p(out.get("u_plan")), _p(out.get("x_plan"))]
        if "kind" in out:
            a += [_p(out.get("hs_traj")), _p(out["kind"]), _p(out["plan_status"]), _p(out["best_traj"]),
                  _p(out["best_global"]), _p(out["pose_traj"])]
        return a

    def rollout_dev(self, rc: RolloutConfig, x_ref, halfspace, x_traj, u_lin_traj, u_applied, status_traj,
                    iters_traj=None, cost_traj=None, u_plan=None, x_plan=None, stream=None):
        """rc.ticks closed-loop ticks on device (torch) tensors, enqueued on `stream`, asynchronous
        and without a host synchronisation (f110qp_rollout_dev): x_ref [B,S,3] f64 and halfspace
        [B,2,3] f32 held fixed; x_traj [T+1,B,3] / u_lin_traj [T+1,B,2] f64 with row 0 the start;
        u_applied [T,B,2] f32, status_traj [T,B] i32; iters_traj [T,B] i32, cost_traj [T,B] f64,
        u_plan [T,B,N,2] and x_plan [T,B,N+1,3] f32 optional."""
        T, B = self._dev_loop(rc, x_ref, x_traj)
        traj = (x_traj, u_lin_traj, u_applied, status_traj, iters_traj, cost_traj, u_plan, x_plan)
        _devs((x_ref, "f64", 3 * (self.config.x_ref_points or self.horizon) * B, "x_ref"),
              (halfspace, "f32", 6 * B, "halfspace", self.config.gap_mode == GAP_INACTIVE),
              *self._traj_specs(T, B, *traj))
        self._chk(self.lib.f110qp_rollout_dev(self._h, C.byref(rc), B, _tp(x_ref), _tp(halfspace), *map(_tp, traj),
                                              self._stream(stream, x_traj)), "f110qp_rollout_dev")

    def rollout(self, x0, u_lin, x_ref, ticks, halfspace=None, plans=False, objective=False, rc=None):
        """`ticks` closed-loop ticks from float64 host arrays x0 [B,3], u_lin [B,2], x_ref [B,S,3]
        (f110qp_rollout, synchronous). rc: a RolloutConfig whose plant parameters to use (its ticks
        is replaced). Returns a dict of numpy arrays: x_traj [T+1,B,3], u_lin_traj [T+1,B,2],
        u_applied [T,B,2], status [T,B], iters [T,B]; plans=True adds u_plan [T,B,N,2] and x_plan
        [T,B,N+1,3], objective=True adds cost [T,B]."""
        T, B, x0, ul = self._host_start(x0, u_lin, ticks)
        xr = _f64(x_ref, (B, self.config.x_ref_points or self.horizon, 3), "x_ref")
        hs = None if halfspace is None else np.ascontiguousarray(halfspace, np.float32).reshape(B, 6)
        out = self._host_out(T, B, x0, ul, objective, plans)
        self._chk(self.lib.f110qp_rollout(self._h, C.byref(self._ticks_config(rc, T)), B, _p(xr), _p(hs),
                                          *self._out_args(out)), "f110qp_rollout")
        return out

    def rollout_scan_dev(self, rc: RolloutConfig, sc: ScanConfig, x_ref, ranges, x_traj, u_lin_traj, u_applied,
                         status_traj, iters_traj=None, cost_traj=None, u_plan=None, x_plan=None, hs_traj=None,
                         stream=None):
        """rollout_dev with the half-spaces of every tick computed at that tick's pose
        (f110qp_rollout_scan_dev): ranges [sc.scan_rows,B,sc.num_ranges] f32 (scan_rows 1 or ticks)
        replaces halfspace; hs_traj [T,B,2,3] f32 optional, row t the rows tick t solved with."""
        T, B = self._dev_loop(rc, x_ref, x_traj, (sc, ranges))
        traj = (x_traj, u_lin_traj, u_applied, status_traj, iters_traj, cost_traj, u_plan, x_plan)
        _devs((x_ref, "f64", 3 * (self.config.x_ref_points or self.horizon) * B, "x_ref"),
              (ranges, "f32", int(sc.scan_rows) * B * int(sc.num_ranges), "ranges"),
              *self._traj_specs(T, B, *traj), (hs_traj, "f32", 6 * B * T, "hs_traj", True))
        self._chk(self.lib.f110qp_rollout_scan_dev(self._h, C.byref(rc), C.byref(sc), B, _tp(x_ref), _tp(ranges),
                                                   *map(_tp, traj), _tp(hs_traj), self._stream(stream, x_traj)),
                  "f110qp_rollout_scan_dev")

    def rollout_scan(self, x0, u_lin, x_ref, ranges, sc: ScanConfig, ticks, plans=False, objective=False,
                     rows=True, rc=None):
        """rollout() with the half-spaces of every tick computed at that tick's pose
        (f110qp_rollout_scan, synchronous): ranges [B,R] (sc.scan_rows 1) or [ticks,B,R] (sc.scan_rows
        ticks) float32. Returns rollout()'s dict; rows=True adds hs_traj [T,B,2,3]."""
        T, B, x0, ul = self._host_start(x0, u_lin, ticks)
        xr = _f64(x_ref, (B, self.config.x_ref_points or self.horizon, 3), "x_ref")
        rg = self._host_ranges(ranges, sc, T, B)
        out = self._host_out(T, B, x0, ul, objective, plans, rows)
        self._chk(self.lib.f110qp_rollout_scan(self._h, C.byref(self._ticks_config(rc, T)), C.byref(sc), B, _p(xr),
                                               _p(rg), *self._out_args(out), _p(out.get("hs_traj"))),
                  "f110qp_rollout_scan")
        return out

    def rollout_replan_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, table, waypoints, x_ref,
                           have_path, ranges, x_traj, u_lin_traj, u_applied, status_traj, iters_traj=None,
                           cost_traj=None, u_plan=None, x_plan=None, hs_traj=None, kind_traj=None,
                           plan_status_traj=None, best_traj_traj=None, best_global_traj=None, pose_traj=None,
                           stream=None):
        """rc.ticks ticks of the closed loop with re-planning on device tensors (f110qp_rollout_replan_dev),
        asynchronous: rollout_scan_dev's arguments plus table [Tc,P,3] f64, waypoints [W,2] f64, x_ref
        [B,P,3] f64 and have_path [B] i32 (both in/out), and the optional kind_traj, plan_status_traj,
        best_traj_traj, best_global_traj [T,B] i32 and pose_traj [T+1,B,4] f64."""
        T, B = self._dev_loop(rc, x_ref, x_traj, (sc, ranges))
        plan = (table, waypoints, x_ref, have_path)
        traj = (x_traj, u_lin_traj, u_applied, status_traj, iters_traj, cost_traj, u_plan, x_plan)
        rec = (hs_traj, kind_traj, plan_status_traj, best_traj_traj, best_global_traj, pose_traj)
        _devs(*self._plan_specs(rp, B, *plan),
              (ranges, "f32", int(sc.scan_rows) * B * int(sc.num_ranges), "ranges"),
              *self._traj_specs(T, B, *traj), *self._record_specs(T, B, *rec))
        self._chk(self.lib.f110qp_rollout_replan_dev(
            self._h, C.byref(rc), C.byref(sc), C.byref(rp), B, *map(_tp, plan), _tp(ranges), *map(_tp, traj),
            *map(_tp, rec), self._stream(stream, x_traj)), "f110qp_rollout_replan_dev")

    def rollout_replan(self, x0, u_lin, ranges, sc: ScanConfig, rp: ReplanConfig, table, waypoints, ticks,
                       x_ref=None, have_path=None, plans=False, objective=False, rows=True, rc=None):
        """`ticks` ticks of the closed loop with re-planning from host arrays (f110qp_rollout_replan,
        synchronous): x0 [B,3], u_lin [B,2] float64, ranges as rollout_scan, table [Tc,P,3] and waypoints
        [W,2] float64. x_ref [B,P,3] float64 / have_path [B] int32: the paths the cars hold (default: none,
        every car plans on tick 0); copies of both come back updated, so a second call can continue.
        Returns rollout_scan()'s dict plus x_ref, have_path, kind, plan_status, best_traj, best_global
        [T,B] and pose_traj [T+1,B,4]."""
        T, B, x0, ul = self._host_start(x0, u_lin, ticks)
        xr, hv, tab, wp = self._host_plan(rp, B, table, waypoints, x_ref, have_path)
        rg = self._host_ranges(ranges, sc, T, B)
        out = self._host_out(T, B, x0, ul, objective, plans, rows, paths=(xr, hv))
        self._chk(self.lib.f110qp_rollout_replan(
            self._h, C.byref(self._ticks_config(rc, T)), C.byref(sc), C.byref(rp), B, _p(tab),
            _p(wp) if wp.shape[0] else None, _p(xr), _p(hv), _p(rg), *self._out_args(out)), "f110qp_rollout_replan")
        return out

    # ---- the world families: one device body and one host body, both walking WORLD_FAMILIES -----------------------

    def _world_dev(self, family, a, field=False):
        """The body of the eight rollout_<family>_dev; a: the wrapper's arguments by name. field: rollout_field_dev,
        the grid family's body with d2 behind grid."""
        fams = _families(family)
        _check_cfgs(fams[1:], a, whole=True)
        T, B = self._dev_loop(a["rc"], a["x_ref"], a["x_traj"])
        WR = int(a["wc"].world_rows)
        if WR not in (1, B):
            raise F110QPError(f"world_rows must be 1 or B = {B}, got {WR}")
        if fams[1:]:
            _check_race(a["race"], B)
        more = []  # behind ranges_traj, row by row: the records a family adds, then its world array
        for f in fams[1:]:
            more += [(a[r.name], r.dtype, (T + 1) * B if r.per_row else B, r.name, r.optional) for r in f.records]
            more += _world_specs([f], a)
        if field:
            more.append(_field_spec(a["grid_cfg"], a["d2"]))
        _devs(*self._plan_specs(a["rp"], B, a["table"], a["waypoints"], a["x_ref"], a["have_path"]),
              *_world_specs(fams[:1], a), *self._traj_specs(T, B, *(a[n] for n in _TRAJ)),
              *self._record_specs(T, B, *(a[n] for n in _REC)),
              (a["ranges_traj"], "f32", T * B * int(a["sc"].num_ranges), "ranges_traj", True), *more)
        name = "f110qp_rollout_field_dev" if field else f"f110qp_rollout_{family}_dev"
        call = {**a, "ctx": self._h, "batch": B, "stream": self._stream(a["stream"], a["x_traj"])}
        self._chk(getattr(self.lib, name)(*_abi_args(_abi("rollout", family, field=field), call)), name)

    def _world_host(self, family, a, name=None):
        """The body of the eight rollout_<family>; a: the wrapper's arguments by name. The world config's counts and
        the walls config come from the arrays' shapes. name: another symbol with the family's parameter list
        (f110qp_rollout_field)."""
        fams = _families(family)
        _check_cfgs([f for f in fams[1:] if f.array != "segments"], a, whole=True)
        T, B, x0, ul = self._host_start(a["x0"], a["u_lin"], a["ticks"])
        xr, hv, tab, wp = self._host_plan(a["rp"], B, a["table"], a["waypoints"], a["x_ref"], a["have_path"])
        cfgs, world = [], []
        for f in fams:
            cfg = a.get(f.arg)
            if f.array:
                cfg, arr = _HOST_WORLD[f.array](a, B)
                world.append(_p(arr) if arr.size else None)
            if f.name == "race":
                _check_race(cfg, B)
            cfgs.append(C.byref(cfg))
        out = self._host_out(T, B, x0, ul, a["objective"], a["plans"], a["rows"],
                             int(a["sc"].num_ranges) if a["scans"] else 0, (xr, hv))
        records = [r for f in fams for r in f.records]
        for r in records:
            if not r.optional or a[r.name[:-len("_traj")]]:
                out[r.name] = np.empty((T + 1, B) if r.per_row else B, {"f64": np.float64, "i32": np.int32}[r.dtype])
        name = name or f"f110qp_rollout_{family}"
        self._chk(getattr(self.lib, name)(
            self._h, C.byref(self._ticks_config(a["rc"], T)), C.byref(a["sc"]), C.byref(a["rp"]), *cfgs, B, _p(tab),
            _p(wp) if wp.shape[0] else None, _p(xr), _p(hv), *world, *self._out_args(out), _p(out.get("ranges_traj")),
            *(_p(out.get(r.name)) for r in records)), name)
        return out

    def rollout_world_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig, table,
                          waypoints, x_ref, have_path, circles, x_traj, u_lin_traj, u_applied, status_traj,
                          iters_traj=None, cost_traj=None, u_plan=None, x_plan=None, hs_traj=None, kind_traj=None,
                          plan_status_traj=None, best_traj_traj=None, best_global_traj=None, pose_traj=None,
                          ranges_traj=None, stream=None):
        """rollout_replan_dev with every tick's scan cast at that tick's pose (f110qp_rollout_world_dev): wc
        and circles [world_rows,C,3] f64 replace ranges, sc.scan_rows is not read, and the optional
        ranges_traj [T,B,num_ranges] f32 records every car's scan of every tick."""
        self._world_dev("world", locals())

    def rollout_race_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig, race: RaceConfig,
                         table, waypoints, x_ref, have_path, circles, x_traj, u_lin_traj, u_applied, status_traj,
                         iters_traj=None, cost_traj=None, u_plan=None, x_plan=None, hs_traj=None, kind_traj=None,
                         plan_status_traj=None, best_traj_traj=None, best_global_traj=None, pose_traj=None,
                         ranges_traj=None, stream=None):
        """rollout_world_dev with the cars of a race in each other's scans (f110qp_rollout_race_dev): the B cars
        are B / race.group_size races of consecutive cars; every cast reads x_traj row t as the casting poses
        and as the opponents'. circles may be None when wc.num_circles is 0."""
        self._world_dev("race", locals())

    def rollout_contact_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig,
                            race: RaceConfig, cc: ContactConfig, table, waypoints, x_ref, have_path, circles, x_traj,
                            u_lin_traj, u_applied, status_traj, clear_traj, crash_tick, nearest_traj=None, iters_traj=None,
                            cost_traj=None, u_plan=None, x_plan=None, hs_traj=None, kind_traj=None, plan_status_traj=None,
                            best_traj_traj=None, best_global_traj=None, pose_traj=None, ranges_traj=None, stream=None):
        """rollout_race_dev with every row's clearance recorded and, with cc.stop_on_contact, crashed cars parked
        (f110qp_rollout_contact_dev): clear_traj [T+1,B] f64, crash_tick [B] i32, nearest_traj [T+1,B] i32
        optional; a parked car's kind is TICK_CRASHED."""
        self._world_dev("contact", locals())

    def rollout_body_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig, race: RaceConfig,
                         cc: ContactConfig, body: BodyConfig, table, waypoints, x_ref, have_path, circles, x_traj,
                         u_lin_traj, u_applied, status_traj, clear_traj, crash_tick, nearest_traj=None, iters_traj=None,
                         cost_traj=None, u_plan=None, x_plan=None, hs_traj=None, kind_traj=None, plan_status_traj=None,
                         best_traj_traj=None, best_global_traj=None, pose_traj=None, ranges_traj=None, stream=None):
        """rollout_contact_dev with rectangular car bodies in every cast and every clearance
        (f110qp_rollout_body_dev): body follows cc, everything else as there."""
        self._world_dev("body", locals())

    def rollout_walls_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig, race: RaceConfig,
                          cc: ContactConfig, body: BodyConfig, walls: WallsConfig, table, waypoints, x_ref, have_path,
                          circles, segments, x_traj, u_lin_traj, u_applied, status_traj, clear_traj, crash_tick,
                          nearest_traj=None, iters_traj=None, cost_traj=None, u_plan=None, x_plan=None, hs_traj=None,
                          kind_traj=None, plan_status_traj=None, best_traj_traj=None, best_global_traj=None,
                          pose_traj=None, ranges_traj=None, stream=None):
        """rollout_body_dev with straight wall segments next to the circles in every cast and every clearance
        (f110qp_rollout_walls_dev): walls follows body, segments [wall_rows,S,4] f64 (None for S = 0) follows
        circles, everything else as there."""
        self._world_dev("walls", locals())

    def rollout_refresh_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig, race: RaceConfig,
                            cc: ContactConfig, body: BodyConfig, walls: WallsConfig, rf: RefreshConfig, table, waypoints,
                            x_ref, have_path, circles, segments, x_traj, u_lin_traj, u_applied, status_traj, clear_traj,
                            crash_tick, nearest_traj=None, iters_traj=None, cost_traj=None, u_plan=None, x_plan=None,
                            hs_traj=None, kind_traj=None, plan_status_traj=None, best_traj_traj=None,
                            best_global_traj=None, pose_traj=None, ranges_traj=None, stream=None):
        """rollout_walls_dev with the scan MPC holds replaced every rf.every ticks by the scan cast at that tick's
        pose (f110qp_rollout_refresh_dev): rf follows walls, everything else as there; rf.every = 0 is
        rollout_walls_dev."""
        self._world_dev("refresh", locals())

    def rollout_noisy_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig, race: RaceConfig,
                          cc: ContactConfig, body: BodyConfig, walls: WallsConfig, rf: RefreshConfig, noise: NoiseConfig,
                          table, waypoints, x_ref, have_path, circles, segments, x_traj, u_lin_traj, u_applied,
                          status_traj, clear_traj, crash_tick, nearest_traj=None, iters_traj=None, cost_traj=None,
                          u_plan=None, x_plan=None, hs_traj=None, kind_traj=None, plan_status_traj=None,
                          best_traj_traj=None, best_global_traj=None, pose_traj=None, ranges_traj=None, stream=None):
        """rollout_refresh_dev with seeded range noise and dropout on every scan it casts
        (f110qp_rollout_noisy_dev): noise follows rf, everything else as there; the all-zero noise config is
        rollout_refresh_dev."""
        self._world_dev("noisy", locals())

    def rollout_grid_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig, race: RaceConfig,
                         cc: ContactConfig, body: BodyConfig, walls: WallsConfig, rf: RefreshConfig, noise: NoiseConfig,
                         grid_cfg: GridConfig, table, waypoints, x_ref, have_path, circles, segments, grid, x_traj,
                         u_lin_traj, u_applied, status_traj, clear_traj, crash_tick, nearest_traj=None, iters_traj=None,
                         cost_traj=None, u_plan=None, x_plan=None, hs_traj=None, kind_traj=None, plan_status_traj=None,
                         best_traj_traj=None, best_global_traj=None, pose_traj=None, ranges_traj=None, stream=None):
        """rollout_noisy_dev on a raster map (f110qp_rollout_grid_dev): grid_cfg follows noise, grid [H,W] u8 (None
        for an empty map) follows segments, everything else as there."""
        self._world_dev("grid", locals())

    def rollout_field_dev(self, rc: RolloutConfig, sc: ScanConfig, rp: ReplanConfig, wc: WorldConfig, race: RaceConfig,
                          cc: ContactConfig, body: BodyConfig, walls: WallsConfig, rf: RefreshConfig,
                          noise: NoiseConfig, grid_cfg: GridConfig, table, waypoints, x_ref, have_path, circles,
                          segments, grid, d2, x_traj, u_lin_traj, u_applied, status_traj, clear_traj, crash_tick,
                          nearest_traj=None, iters_traj=None, cost_traj=None, u_plan=None, x_plan=None, hs_traj=None,
                          kind_traj=None, plan_status_traj=None, best_traj_traj=None, best_global_traj=None,
                          pose_traj=None, ranges_traj=None, stream=None):
        """rollout_grid_dev with every cast grid_cast_dev's (f110qp_rollout_field_dev, rule F1): d2 [H,W] i32, the
        field grid_distance_dev wrote for grid (None for an empty map), follows grid; the clearances still read
        grid. The same bits in every array."""
        self._world_dev("grid", locals(), field=True)

    def rollout_world(self, x0, u_lin, circles, sc: ScanConfig, rp: ReplanConfig, table, waypoints, ticks,
                      wc: WorldConfig = None, x_ref=None, have_path=None, plans=False, objective=False, rows=True,
                      scans=False, rc=None):
        """rollout_replan() in a world of circles (f110qp_rollout_world, synchronous): circles [C,3] (one world
        for all cars) or [B,C,3] float64 replace ranges; wc defaults to f110qp_default_world_config with
        num_circles and world_rows taken from the array. scans=True adds ranges_traj [T,B,num_ranges]."""
        return self._world_host("world", locals())

    def rollout_race(self, x0, u_lin, circles, race: RaceConfig, sc: ScanConfig, rp: ReplanConfig, table, waypoints,
                     ticks, wc: WorldConfig = None, x_ref=None, have_path=None, plans=False, objective=False,
                     rows=True, scans=False, rc=None):
        """rollout_world() with the cars of a race in each other's scans (f110qp_rollout_race, synchronous):
        circles [C,3] or [B,C,3] float64, C = 0 allowed (the world is then the opponents only)."""
        return self._world_host("race", locals())

    def rollout_contact(self, x0, u_lin, circles, race: RaceConfig, cc: ContactConfig, sc: ScanConfig, rp: ReplanConfig,
                        table, waypoints, ticks, wc: WorldConfig = None, x_ref=None, have_path=None, plans=False,
                        objective=False, rows=True, scans=False, nearest=True, rc=None):
        """rollout_race() with contact (f110qp_rollout_contact, synchronous): adds clear_traj [T+1,B], crash_tick
        [B] and, with nearest=True, nearest_traj [T+1,B]; with cc.stop_on_contact crashed cars park."""
        return self._world_host("contact", locals())

    def rollout_body(self, x0, u_lin, circles, race: RaceConfig, cc: ContactConfig, body: BodyConfig, sc: ScanConfig,
                     rp: ReplanConfig, table, waypoints, ticks, wc: WorldConfig = None, x_ref=None, have_path=None,
                     plans=False, objective=False, rows=True, scans=False, nearest=True, rc=None):
        """rollout_contact() with rectangular car bodies (f110qp_rollout_body, synchronous)."""
        return self._world_host("body", locals())

    def rollout_walls(self, x0, u_lin, circles, segments, race: RaceConfig, cc: ContactConfig, body: BodyConfig,
                      sc: ScanConfig, rp: ReplanConfig, table, waypoints, ticks, wc: WorldConfig = None, x_ref=None,
                      have_path=None, plans=False, objective=False, rows=True, scans=False, nearest=True, rc=None):
        """rollout_body() with straight wall segments [S,4] or [B,S,4] float64 next to the circles
        (f110qp_rollout_walls, synchronous); circles may be an empty [0,3] array."""
        return self._world_host("walls", locals())

    def rollout_refresh(self, x0, u_lin, circles, segments, race: RaceConfig, cc: ContactConfig, body: BodyConfig,
                        rf: RefreshConfig, sc: ScanConfig, rp: ReplanConfig, table, waypoints, ticks,
                        wc: WorldConfig = None, x_ref=None, have_path=None, plans=False, objective=False, rows=True,
                        scans=False, nearest=True, rc=None):
        """rollout_walls() with the scan MPC holds replaced every rf.every ticks (f110qp_rollout_refresh,
        synchronous): rf follows body, everything else as there."""
        return self._world_host("refresh", locals())

    def rollout_noisy(self, x0, u_lin, circles, segments, race: RaceConfig, cc: ContactConfig, body: BodyConfig,
                      rf: RefreshConfig, noise: NoiseConfig, sc: ScanConfig, rp: ReplanConfig, table, waypoints, ticks,
                      wc: WorldConfig = None, x_ref=None, have_path=None, plans=False, objective=False, rows=True,
                      scans=False, nearest=True, rc=None):
        """rollout_refresh() with seeded range noise and dropout on every scan (f110qp_rollout_noisy,
        synchronous): noise follows rf, everything else as there."""
        return self._world_host("noisy", locals())

    def rollout_grid(self, x0, u_lin, circles, segments, grid, grid_cfg: GridConfig, race: RaceConfig, cc: ContactConfig,
                     body: BodyConfig, rf: RefreshConfig, noise: NoiseConfig, sc: ScanConfig, rp: ReplanConfig, table,
                     waypoints, ticks, wc: WorldConfig = None, x_ref=None, have_path=None, plans=False, objective=False,
                     rows=True, scans=False, nearest=True, rc=None):
        """rollout_noisy() on a raster map (f110qp_rollout_grid, synchronous): grid [H,W] uint8 (nonzero occupied)
        and grid_cfg follow segments, everything else as there."""
        return self._world_host("grid", locals())

    def rollout_field(self, x0, u_lin, circles, segments, grid, grid_cfg: GridConfig, race: RaceConfig, cc: ContactConfig,
                      body: BodyConfig, rf: RefreshConfig, noise: NoiseConfig, sc: ScanConfig, rp: ReplanConfig, table,
                      waypoints, ticks, wc: WorldConfig = None, x_ref=None, have_path=None, plans=False, objective=False,
                      rows=True, scans=False, nearest=True, rc=None):
        """rollout_grid() with every cast through the map's distance field (f110qp_rollout_field, synchronous): the
        same arguments and the same bits; the field is computed on the device once, before the first tick."""
        return self._world_host("grid", locals(), "f110qp_rollout_field")

    def warm_reset(self):
        self._chk(self.lib.f110qp_warm_reset(self._h), "f110qp_warm_reset")

    def condense_debug_dev(self, x0, u_lin, x_ref, H_out, g_out, stream=None):
        self._chk(self.lib.f110qp_condense_debug_dev(self._h, x0.shape[0], _tp(x0), _tp(u_lin), _tp(x_ref), _tp(H_out),
                                                     _tp(g_out), self._stream(stream, x0)),
                  "f110qp_condense_debug_dev")


def advance_dev(rc: RolloutConfig, horizon: int, x, u_plan, status, x_next, u_lin_next, u_applied=None, stream=None):
    """One plant step on the device (f110qp_advance_dev): x [B,3] f64, u_plan [B,N,2] f32 and status
    [B] i32 of a solve -> x_next [B,3] f64 (not x itself), u_lin_next [B,2] f64, u_applied [B,2] f32
    (optional). Asynchronous on `stream`."""
    import torch

    B, N = int(x.shape[0]), int(horizon)
    _devs((x, "f64", 3 * B, "x"), (u_plan, "f32", 2 * N * B, "u_plan"), (status, "i32", B, "status"),
          (x_next, "f64", 3 * B, "x_next"), (u_lin_next, "f64", 2 * B, "u_lin_next"),
          (u_applied, "f32", 2 * B, "u_applied", True))
    if stream is None:
        stream = torch.cuda.current_stream(x.device)
    _check(load().f110qp_advance_dev(C.byref(rc), B, N, _tp(x), _tp(u_plan), _tp(status), _tp(x_next),
                                     _tp(u_lin_next), _tp(u_applied), C.c_void_p(stream.cuda_stream)),
           "f110qp_advance_dev")


def advance_scan_dev(rc: RolloutConfig, sc: ScanConfig, horizon: int, x, u_plan, status, gap, x_next, u_lin_next,
                     hs_next, u_applied=None, stream=None):
    """advance_dev plus, in the same launch, the half-space rows at x_next (f110qp_advance_scan_dev):
    gap [B] gap records (gap_search_dev) of the scans the next tick reads -> hs_next [B,2,3] f32."""
    import torch

    B, N = int(x.shape[0]), int(horizon)
    _devs((x, "f64", 3 * B, "x"), (u_plan, "f32", 2 * N * B, "u_plan"), (status, "i32", B, "status"),
          (gap, "i32", 4 * B, "gap"), (x_next, "f64", 3 * B, "x_next"), (u_lin_next, "f64", 2 * B, "u_lin_next"),
          (hs_next, "f32", 6 * B, "hs_next"), (u_applied, "f32", 2 * B, "u_applied", True))
    if stream is None:
        stream = torch.cuda.current_stream(x.device)
    _check(load().f110qp_advance_scan_dev(C.byref(rc), C.byref(sc), B, N, _tp(x), _tp(u_plan), _tp(status), _tp(gap),
                                          _tp(x_next), _tp(u_lin_next), _tp(u_applied), _tp(hs_next),
                                          C.c_void_p(stream.cuda_stream)),
           "f110qp_advance_scan_dev")


def plan_listed_dev(rp: ReplanConfig, sc: ScanConfig, list_, count, pose, ranges, table, waypoints, x_ref,
                    plan_status, best_traj, best_global, stream=None):
    """The planning stage for the cars of a device-side list (f110qp_plan_listed_dev): list_ [B] i32 and
    count [1] i32 on the device, pose [B,4] f64, ranges [B,R] f32 -> per listed car plan_status,
    best_traj, best_global [B] i32 and, on status 0, its path into x_ref [B,P,3] f64."""
    import torch

    B, P, Tc, W = int(pose.shape[0]), int(rp.plan.traj_discrete), int(rp.plan.steer_discrete) + 1, int(rp.num_waypoints)
    _devs((list_, "i32", B, "list"), (count, "i32", 1, "count"), (pose, "f64", 4 * B, "pose"),
          (ranges, "f32", B * int(sc.num_ranges), "ranges"), (table, "f64", 3 * P * Tc, "table"),
          (waypoints, "f64", 2 * W, "waypoints", W == 0), (x_ref, "f64", 3 * P * B, "x_ref"),
          (plan_status, "i32", B, "plan_status"), (best_traj, "i32", B, "best_traj"),
          (best_global, "i32", B, "best_global"))
    if stream is None:
        stream = torch.cuda.current_stream(pose.device)
    _check(load().f110qp_plan_listed_dev(C.byref(rp), C.byref(sc), B, _tp(list_), _tp(count), _tp(pose), _tp(ranges),
                                         _tp(table), _tp(waypoints), _tp(x_ref), _tp(plan_status), _tp(best_traj),
                                         _tp(best_global), C.c_void_p(stream.cuda_stream)), "f110qp_plan_listed_dev")


def _cast_scans(family, a, field=False):
    """The body of the six cast_scans*_dev; a: the wrapper's arguments by name. field: grid_cast_dev, the grid
    family's body with d2 behind grid and visits behind ranges."""
    import torch

    fams = _families(family, "cast")
    _check_cfgs(fams[2:], a, whole=False)  # sc, wc and race are read, not type-checked
    x = a["x"]
    B = int(x.shape[0])
    if fams[1:]:
        _check_race(a["race"], B)
    more = []
    if field:
        more = [_field_spec(a["grid_cfg"], a["d2"]), (a["visits"], "i32", B * int(a["sc"].num_ranges), "visits", True)]
    _devs((x, "f64", 3 * B, "x"), *_world_specs(fams, a), (a["ranges"], "f32", B * int(a["sc"].num_ranges), "ranges"),
          (a["list_"], "i32", B, "list", True), (a["count"], "i32", 1, "count", True), *more)
    stream = a["stream"] if a["stream"] is not None else torch.cuda.current_stream(x.device)
    name = "f110qp_grid_cast_dev" if field else fams[-1].cast
    call = {**a, "batch": B, "stream": C.c_void_p(stream.cuda_stream)}
    _check(getattr(load(), name)(*_abi_args(_abi("cast", family, field=field), call)), name)


def _clearance(family, a):
    """The body of the four clearance*_dev; a: the wrapper's arguments by name."""
    import torch

    fams = _families(family, "clearance")
    _check_cfgs(fams[2:], a, whole=False)  # wc and race are read, not type-checked
    x = a["x"]
    if x.dim() not in (2, 3) or x.shape[-1] != 3:
        raise F110QPError(f"x must be [rows, B, 3] or [B, 3], got {tuple(x.shape)}")
    rows, B = (1, int(x.shape[0])) if x.dim() == 2 else (int(x.shape[0]), int(x.shape[1]))
    if rows < 1:
        raise F110QPError("x must hold at least one row")
    _check_race(a["race"], B)
    _devs((x, "f64", 3 * B * rows, "x"), *_world_specs(fams, a), (a["clearance"], "f64", B * rows, "clearance"),
          (a["nearest"], "i32", B * rows, "nearest", True))
    stream = a["stream"] if a["stream"] is not None else torch.cuda.current_stream(x.device)
    name = fams[-1].clearance
    call = {**a, "batch": B, "rows": rows, "stream": C.c_void_p(stream.cuda_stream)}
    _check(getattr(load(), name)(*_abi_args(_abi("clearance", family), call)), name)


def cast_scans_dev(sc: ScanConfig, wc: WorldConfig, x, circles, ranges, list_=None, count=None, stream=None):
    """The simulated LiDAR (f110qp_cast_scans_dev): x [B,3] f64, circles [world_rows,C,3] f64 (None for
    C = 0) -> ranges [B,num_ranges] f32, for all B cars or, with list_ [B] i32 and count [1] i32 on the
    device, for the listed ones."""
    _cast_scans("world", locals())


def cast_scans_race_dev(sc: ScanConfig, wc: WorldConfig, race: RaceConfig, x, circles, ranges, list_=None, count=None,
                        stream=None):
    """cast_scans_dev with the race-mates in every scan (f110qp_cast_scans_race_dev): the B cars are
    B / race.group_size races of consecutive cars, x [B,3] f64 is both the casting poses and the opponents'."""
    _cast_scans("race", locals())


def clearance_dev(wc: WorldConfig, race: RaceConfig, x, circles, clearance, nearest=None, stream=None):
    """Every car's clearance to its world's circles and its race-mates (f110qp_clearance_dev): x [rows,B,3] f64
    (or [B,3]: one row), circles [world_rows,C,3] f64 (None for C = 0) -> clearance [rows,B] f64 and, optionally,
    nearest [rows,B] i32."""
    _clearance("race", locals())


def cast_scans_body_dev(sc: ScanConfig, wc: WorldConfig, race: RaceConfig, body: BodyConfig, x, circles, ranges,
                        list_=None, count=None, stream=None):
    """cast_scans_race_dev with every race-mate a rectangle (f110qp_cast_scans_body_dev)."""
    _cast_scans("body", locals())


def clearance_body_dev(wc: WorldConfig, race: RaceConfig, body: BodyConfig, x, circles, clearance, nearest=None,
                       stream=None):
    """clearance_dev with the car and its race-mates rectangles (f110qp_clearance_body_dev)."""
    _clearance("body", locals())


def cast_scans_walls_dev(sc: ScanConfig, wc: WorldConfig, race: RaceConfig, body: BodyConfig, walls: WallsConfig, x,
                         circles, segments, ranges, list_=None, count=None, stream=None):
    """cast_scans_body_dev with straight wall segments in every scan (f110qp_cast_scans_walls_dev): segments
    [wall_rows,S,4] f64 = (ax, ay, bx, by), None for S = 0."""
    _cast_scans("walls", locals())


def cast_scans_noisy_dev(sc: ScanConfig, wc: WorldConfig, race: RaceConfig, body: BodyConfig, walls: WallsConfig,
                         noise: NoiseConfig, tick, x, circles, segments, ranges, list_=None, count=None, stream=None):
    """cast_scans_walls_dev with seeded range noise and dropout on every beam (f110qp_cast_scans_noisy_dev, rules
    Z1 and Z2 of f110qp.h): noise follows walls, tick (the t of rule Z1's draw) follows it. The oracle is
    workload.noisy_scan on cast_scans_walls_dev's output."""
    _cast_scans("noisy", locals())


def cast_scans_grid_dev(sc: ScanConfig, wc: WorldConfig, race: RaceConfig, body: BodyConfig, walls: WallsConfig,
                        noise: NoiseConfig, grid_cfg: GridConfig, tick, x, circles, segments, grid, ranges, list_=None,
                        count=None, stream=None):
    """cast_scans_noisy_dev with a raster map under every beam (f110qp_cast_scans_grid_dev, rule G1 of f110qp.h):
    grid_cfg follows noise, grid [H,W] u8 (nonzero occupied, None for an empty map) follows segments. The oracle is
    workload.ray_map folded into the noise-free scan, then workload.noisy_scan."""
    _cast_scans("grid", locals())


def grid_cast_dev(sc: ScanConfig, wc: WorldConfig, race: RaceConfig, body: BodyConfig, walls: WallsConfig,
                  noise: NoiseConfig, grid_cfg: GridConfig, tick, x, circles, segments, grid, d2, ranges, visits=None,
                  list_=None, count=None, stream=None):
    """cast_scans_grid_dev with every beam jumping the free space its cell's distance says is there
    (f110qp_grid_cast_dev, rule F1 of f110qp.h): d2 [H,W] i32, the field grid_distance_dev wrote for grid (None for
    an empty map), follows grid; visits [B,num_ranges] i32 (optional) is the cells of d2 each beam read. The same
    bits in ranges. The oracle is workload.ray_field."""
    _cast_scans("grid", locals(), field=True)


def clearance_grid_dev(wc: WorldConfig, race: RaceConfig, body: BodyConfig, walls: WallsConfig, grid_cfg: GridConfig, x,
                       circles, segments, grid, clearance, nearest=None, stream=None):
    """clearance_walls_dev with the occupied cells of a raster map behind the segments (f110qp_clearance_grid_dev,
    rule G2): cell (i, j) has index C + G + S + j W + i in nearest. The oracle is workload.clearance_grid."""
    _clearance("grid", locals())


def clearance_walls_dev(wc: WorldConfig, race: RaceConfig, body: BodyConfig, walls: WallsConfig, x, circles, segments,
                        clearance, nearest=None, stream=None):
    """clearance_body_dev with straight wall segments behind the circles and the mates
    (f110qp_clearance_walls_dev): segment k has index C + G + k in nearest."""
    _clearance("walls", locals())


def _rows_of(x, last, name):
    """(rows, B) of a [rows,B(,last)] array or tensor, or of one row [B(,last)]."""
    shape = tuple(int(v) for v in x.shape)
    nd = 2 + (last is not None)
    want = "[rows, B, 3]" if last else "[rows, B]"
    if len(shape) not in (nd - 1, nd) or (last is not None and shape[-1] != last):
        raise F110QPError(f"{name} must be {want} or one row of it, got {shape}")
    rows, B = (1, shape[0]) if len(shape) == nd - 1 else shape[:2]
    if rows < 1 or B < 1:
        raise F110QPError(f"{name} must hold at least one row and one car")
    return rows, B


def _path(waypoints):
    wp = _f64(waypoints, (-1, 2), "waypoints")
    if wp.shape[0] < 2:
        raise F110QPError("the path needs at least 2 waypoints")
    return wp


def path_lengths(waypoints):
    """The closed path's cumulative lengths (f110qp_path_lengths, on the host): waypoints [W,2] f64 -> cum [W+1]
    f64, cum[0] = 0 and cum[W] the path's length."""
    wp = _path(waypoints)
    cum = np.empty(wp.shape[0] + 1, np.float64)
    _check(load().f110qp_path_lengths(_p(wp), wp.shape[0], _p(cum)), "f110qp_path_lengths")
    return cum


def progress_dev(x, waypoints, cum, s, seg=None, lateral=None, stream=None):
    """Every pose's place on the closed path (f110qp_progress_dev): x [rows,B,3] f64 (or [B,3]: one row),
    waypoints [W,2] f64, cum [W+1] f64 (path_lengths' array, on the device) -> s [rows,B] f64 and, optionally,
    seg [rows,B] i32 and lateral [rows,B] f64."""
    import torch

    rows, B = _rows_of(x, 3, "x")
    if waypoints.dim() != 2 or waypoints.shape[1] != 2 or waypoints.shape[0] < 2:
        raise F110QPError(f"waypoints must be [W, 2] with W >= 2, got {tuple(waypoints.shape)}")
    W = int(waypoints.shape[0])
    _devs((x, "f64", 3 * B * rows, "x"), (waypoints, "f64", 2 * W, "waypoints"), (cum, "f64", W + 1, "cum"),
          (s, "f64", B * rows, "s"), (seg, "i32", B * rows, "seg", True),
          (lateral, "f64", B * rows, "lateral", True))
    if stream is None:
        stream = torch.cuda.current_stream(x.device)
    _check(load().f110qp_progress_dev(B, rows, _tp(x), _tp(waypoints), _tp(cum), W, _tp(seg), _tp(s), _tp(lateral),
                                      C.c_void_p(stream.cuda_stream)), "f110qp_progress_dev")


def standings_dev(race: RaceConfig, s, path_length: float, dist, rank, lap=None, stream=None):
    """Distance driven, laps and positions inside every race (f110qp_standings_dev): s [rows,B] f64 (or [B]: one
    row) on a path of length path_length -> dist [rows,B] f64, rank [rows,B] i32 and, optionally, lap [rows,B]
    i32."""
    import torch

    rows, B = _rows_of(s, None, "s")
    _check_race(race, B)
    _devs((s, "f64", B * rows, "s"), (dist, "f64", B * rows, "dist"), (rank, "i32", B * rows, "rank"),
          (lap, "i32", B * rows, "lap", True))
    if stream is None:
        stream = torch.cuda.current_stream(s.device)
    _check(load().f110qp_standings_dev(C.byref(race), B, rows, _tp(s), float(path_length), _tp(dist), _tp(lap),
                                       _tp(rank), C.c_void_p(stream.cuda_stream)), "f110qp_standings_dev")


def race_standings(race: RaceConfig, x, waypoints, seg=True, lateral=True, lap=True):
    """Both on host arrays, synchronous (f110qp_race_standings): x [rows,B,3] f64 (or [B,3]), waypoints [W,2] f64
    -> a dict of seg, s, lateral, dist, lap and rank, each [rows,B]; an optional output that is switched off is
    None."""
    x = np.ascontiguousarray(x, np.float64)
    rows, B = _rows_of(x, 3, "x")
    wp = _path(waypoints)
    _check_race(race, B)
    i32 = lambda on: np.empty((rows, B), np.int32) if on else None  # noqa: E731
    f64 = lambda on: np.empty((rows, B), np.float64) if on else None  # noqa: E731
    o = dict(seg=i32(seg), s=f64(True), lateral=f64(lateral), dist=f64(True), lap=i32(lap), rank=i32(True))
    _check(load().f110qp_race_standings(C.byref(race), B, rows, _p(x), _p(wp), wp.shape[0], _p(o["seg"]), _p(o["s"]),
                                        _p(o["lateral"]), _p(o["dist"]), _p(o["lap"]), _p(o["rank"])),
           "f110qp_race_standings")
    return o


def _mc_sets(mc: McConfig, B):
    """K, the sample sets of a batch of B cars; the layout's rules (the C call checks the rest)."""
    M, G, Q = int(mc.hypotheses), int(mc.group_size), int(mc.num_probs)
    if not 1 <= M <= MC_MAX_HYPOTHESES:
        raise F110QPError(f"hypotheses must be in 1..{MC_MAX_HYPOTHESES}, got {M}")
    if G < 1 or B % (M * G):
        raise F110QPError(f"hypotheses x group_size must divide B = {B}, got {M} x {G}")
    if not 1 <= Q <= MC_MAX_PROBS:
        raise F110QPError(f"num_probs must be in 1..{MC_MAX_PROBS}, got {Q}")
    return B // M, Q


def mc_fan_dev(mc: McConfig, v, fan, count=None, stream=None):
    """The quantile fan of every sample set at every row (f110qp_mc_fan_dev): v [rows,B] f64 (or [B]: one row) ->
    fan [rows,K,Q] f64 and, optionally, count [rows,K] i32, K = B / mc.hypotheses."""
    import torch

    rows, B = _rows_of(v, None, "v")
    K, Q = _mc_sets(mc, B)
    _devs((v, "f64", B * rows, "v"), (fan, "f64", rows * K * Q, "fan"), (count, "i32", rows * K, "count", True))
    if stream is None:
        stream = torch.cuda.current_stream(v.device)
    _check(load().f110qp_mc_fan_dev(C.byref(mc), B, rows, _tp(v), _tp(fan), _tp(count),
                                    C.c_void_p(stream.cuda_stream)), "f110qp_mc_fan_dev")


def mc_survival_dev(mc: McConfig, crash_tick, ticks: int, alive, crashed=None, stream=None):
    """How many hypotheses of every set are still running at every row (f110qp_mc_survival_dev): crash_tick [B]
    i32 -> alive [ticks+1,K] i32 and, optionally, crashed [K] i32."""
    import torch

    if crash_tick is None or len(crash_tick.shape) != 1 or crash_tick.shape[0] < 1:
        raise F110QPError("crash_tick must be [B]")
    B, T = int(crash_tick.shape[0]), int(ticks)
    if T < 1:
        raise F110QPError(f"ticks must be >= 1, got {T}")
    K, _ = _mc_sets(mc, B)
    _devs((crash_tick, "i32", B, "crash_tick"), (alive, "i32", (T + 1) * K, "alive"), (crashed, "i32", K, "crashed", True))
    if stream is None:
        stream = torch.cuda.current_stream(crash_tick.device)
    _check(load().f110qp_mc_survival_dev(C.byref(mc), B, T, _tp(crash_tick), _tp(alive), _tp(crashed),
                                         C.c_void_p(stream.cuda_stream)), "f110qp_mc_survival_dev")


def mc_outcomes_dev(clear_traj, min_clear, status_traj=None, kind_traj=None, min_row=None, unsolved=None,
                    first_unsolved=None, plan_failed=None, stream=None):
    """Every car's record (f110qp_mc_outcomes_dev): clear_traj [T+1,B] f64, status_traj and kind_traj [T,B] i32 or
    None -> min_clear [B] f64 and, optionally, min_row, unsolved, first_unsolved and plan_failed [B] i32."""
    import torch

    rows, B = _rows_of(clear_traj, None, "clear_traj")
    if len(clear_traj.shape) != 2 or rows < 2:
        raise F110QPError(f"clear_traj must be [T + 1, B] with T >= 1, got {tuple(clear_traj.shape)}")
    T = rows - 1
    if (unsolved is not None or first_unsolved is not None) and status_traj is None:
        raise F110QPError("unsolved and first_unsolved need status_traj")
    if plan_failed is not None and kind_traj is None:
        raise F110QPError("plan_failed needs kind_traj")
    _devs((clear_traj, "f64", rows * B, "clear_traj"), (status_traj, "i32", T * B, "status_traj", True),
          (kind_traj, "i32", T * B, "kind_traj", True), (min_clear, "f64", B, "min_clear"),
          (min_row, "i32", B, "min_row", True), (unsolved, "i32", B, "unsolved", True),
          (first_unsolved, "i32", B, "first_unsolved", True), (plan_failed, "i32", B, "plan_failed", True))
    if stream is None:
        stream = torch.cuda.current_stream(clear_traj.device)
    _check(load().f110qp_mc_outcomes_dev(B, T, _tp(clear_traj), _tp(status_traj), _tp(kind_traj), _tp(min_clear),
                                         _tp(min_row), _tp(unsolved), _tp(first_unsolved), _tp(plan_failed),
                                         C.c_void_p(stream.cuda_stream)), "f110qp_mc_outcomes_dev")


def mc_summary(mc: McConfig, clear_traj, crash_tick, status_traj=None, kind_traj=None, count=True, crashed=True,
               min_row=True):
    """The three on host arrays, synchronous (f110qp_mc_summary), the fan taken on clear_traj: clear_traj [T+1,B]
    f64, crash_tick [B] i32, status_traj and kind_traj [T,B] i32 or None -> a dict of fan [T+1,K,Q], count
    [T+1,K], alive [T+1,K], crashed [K], min_clear, min_row, unsolved, first_unsolved and plan_failed [B]; an
    optional output that is switched off, or whose input is None, is None."""
    clear = _f64(clear_traj, np.shape(clear_traj), "clear_traj")
    if clear.ndim != 2 or clear.shape[0] < 2 or clear.shape[1] < 1:
        raise F110QPError(f"clear_traj must be [T + 1, B] with T >= 1, got {clear.shape}")
    T, B = clear.shape[0] - 1, clear.shape[1]
    K, Q = _mc_sets(mc, B)

    def ints(a, shape, name):
        if a is None:
            return None
        if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.shape != shape:
            got = (a.dtype, a.shape) if isinstance(a, np.ndarray) else type(a).__name__
            raise F110QPError(f"{name} must be an int32 numpy array of shape {shape}, got {got}")
        return np.ascontiguousarray(a)

    crash = ints(crash_tick, (B,), "crash_tick")
    if crash is None:
        raise F110QPError("crash_tick is required")
    status, kind = ints(status_traj, (T, B), "status_traj"), ints(kind_traj, (T, B), "kind_traj")
    i32 = lambda shape, on: np.empty(shape, np.int32) if on else None  # noqa: E731
    o = dict(fan=np.empty((T + 1, K, Q), np.float64), count=i32((T + 1, K), count), alive=i32((T + 1, K), True),
             crashed=i32((K,), crashed), min_clear=np.empty(B, np.float64), min_row=i32((B,), min_row),
             unsolved=i32((B,), status is not None), first_unsolved=i32((B,), status is not None),
             plan_failed=i32((B,), kind is not None))
    _check(load().f110qp_mc_summary(C.byref(mc), B, T, _p(clear), _p(crash), _p(status), _p(kind), _p(o["fan"]),
                                    _p(o["count"]), _p(o["alive"]), _p(o["crashed"]), _p(o["min_clear"]),
                                    _p(o["min_row"]), _p(o["unsolved"]), _p(o["first_unsolved"]), _p(o["plan_failed"])),
           "f110qp_mc_summary")
    return o


def _field_cells(grid_cfg):
    """W, H and W * H of a map for the distance-field calls (the C call checks the rest of the config)."""
    if not isinstance(grid_cfg, GridConfig):
        raise F110QPError("grid_cfg must be a GridConfig")
    W, H = int(grid_cfg.width), int(grid_cfg.height)
    if not (0 <= W <= FIELD_MAX_SIDE and 0 <= H <= FIELD_MAX_SIDE):
        raise F110QPError(f"grid width and height must be in 0..{FIELD_MAX_SIDE}, got {W} x {H}")
    return W, H, W * H


def grid_distance_dev(grid_cfg: GridConfig, grid, d2, work, nearest=None, stream=None):
    """The map's exact distance transform (f110qp_grid_distance_dev): grid [H,W] u8 -> d2 [H,W] i32 (squared cell
    distance to the nearest occupied cell, INT_MAX on a map without one) and, optionally, nearest [H,W] i32 (that
    cell's linear index, -1 for none); work [H,W] i32 of scratch."""
    import torch

    _, _, n = _field_cells(grid_cfg)
    _devs((grid, "u8", n, "grid", n == 0), (d2, "i32", n, "d2", n == 0), (work, "i32", n, "work", n == 0),
          (nearest, "i32", n, "nearest", True))
    if stream is None:
        stream = torch.cuda.current_stream(d2.device if d2 is not None else None)
    _check(load().f110qp_grid_distance_dev(C.byref(grid_cfg), _tp(grid), _tp(d2), _tp(nearest), _tp(work),
                                           C.c_void_p(stream.cuda_stream)), "f110qp_grid_distance_dev")


def grid_inflate_dev(grid_cfg: GridConfig, d2, radius: float, out, stream=None):
    """The map inflated by radius metres (f110qp_grid_inflate_dev): d2 [H,W] i32 -> out [H,W] u8 of 0 / 1, a map
    for every grid call under the same grid_cfg."""
    import torch

    _, _, n = _field_cells(grid_cfg)
    _devs((d2, "i32", n, "d2", n == 0), (out, "u8", n, "out", n == 0))
    if stream is None:
        stream = torch.cuda.current_stream(out.device if out is not None else None)
    _check(load().f110qp_grid_inflate_dev(C.byref(grid_cfg), _tp(d2), float(radius), _tp(out),
                                          C.c_void_p(stream.cuda_stream)), "f110qp_grid_inflate_dev")


def grid_lookup_dev(grid_cfg: GridConfig, d2, x, dist, nearest=None, cell=None, stream=None):
    """The wall distance at poses (f110qp_grid_lookup_dev): d2 [H,W] i32, x [rows,B,3] f64 (or [B,3]: one row; the
    heading is not read) -> dist [rows,B] f64 in metres, NaN outside the map, and, with nearest [H,W] i32 given,
    cell [rows,B] i32 (the nearest occupied cell's linear index, -1 outside the map or on an empty one)."""
    import torch

    _, _, n = _field_cells(grid_cfg)
    rows, B = _rows_of(x, 3, "x")
    if (nearest is None) != (cell is None):
        raise F110QPError("nearest and cell must be given together")
    _devs((d2, "i32", n, "d2", n == 0), (nearest, "i32", n, "nearest", True), (x, "f64", 3 * B * rows, "x"),
          (dist, "f64", B * rows, "dist"), (cell, "i32", B * rows, "cell", True))
    if stream is None:
        stream = torch.cuda.current_stream(x.device)
    _check(load().f110qp_grid_lookup_dev(C.byref(grid_cfg), _tp(d2), _tp(nearest), B, rows, _tp(x), _tp(dist),
                                         _tp(cell), C.c_void_p(stream.cuda_stream)), "f110qp_grid_lookup_dev")


def _host_map(grid_cfg, grid):
    W, H, _ = _field_cells(grid_cfg)
    if not isinstance(grid, np.ndarray) or grid.dtype != np.uint8 or grid.shape != (H, W):
        got = (grid.dtype, grid.shape) if isinstance(grid, np.ndarray) else type(grid).__name__
        raise F110QPError(f"grid must be a uint8 numpy array [height, width] = [{H}, {W}], got {got}")
    return np.ascontiguousarray(grid)


def grid_field(grid_cfg: GridConfig, grid, nearest=True, radius=None):
    """The transform and the inflation on host arrays, synchronous (f110qp_grid_field): grid [H,W] u8 -> a dict of
    d2 [H,W] i32, nearest [H,W] i32 and inflated [H,W] u8 at `radius`; an optional output that is switched off
    (nearest=False, radius=None) is None."""
    g = _host_map(grid_cfg, grid)
    o = dict(d2=np.empty(g.shape, np.int32), nearest=np.empty(g.shape, np.int32) if nearest else None,
             inflated=np.empty(g.shape, np.uint8) if radius is not None else None)
    _check(load().f110qp_grid_field(C.byref(grid_cfg), _p(g), float(0.0 if radius is None else radius), _p(o["d2"]),
                                    _p(o["nearest"]), _p(o["inflated"])), "f110qp_grid_field")
    return o


def wall_distance(grid_cfg: GridConfig, grid, x, cell=True):
    """The wall distance of poses on host arrays, synchronous (f110qp_wall_distance): grid [H,W] u8, x [rows,B,3]
    f64 (or [B,3]) -> (dist [rows,B] f64, cell [rows,B] i32 or None)."""
    g = _host_map(grid_cfg, grid)
    x = _f64(x, np.shape(x), "x")
    rows, B = _rows_of(x, 3, "x")
    dist = np.empty((rows, B), np.float64)
    c = np.empty((rows, B), np.int32) if cell else None
    _check(load().f110qp_wall_distance(C.byref(grid_cfg), _p(g), B, rows, _p(x), _p(dist), _p(c)),
           "f110qp_wall_distance")
    return dist, c


def replan_start_dev(rp: ReplanConfig, sc, x, have_path, x_ref, gap, pose, kind, list_, count, hs=None, stream=None):
    """The launch in front of the re-planning loop (f110qp_replan_start_dev): x [B,3] f64, have_path [B]
    i32, x_ref [B,P,3] f64 -> pose [B,4] f64, kind [B] i32, the PLAN cars appended to list_ [B] / count
    [1] (zero on entry) and, with hs [B,2,3] f32, the half-space rows at x from gap (sc required)."""
    import torch

    B, P = int(x.shape[0]), int(rp.plan.traj_discrete)
    _devs((x, "f64", 3 * B, "x"), (have_path, "i32", B, "have_path"), (x_ref, "f64", 3 * P * B, "x_ref"),
          (gap, "i32", 4 * B, "gap", hs is None), (pose, "f64", 4 * B, "pose"), (kind, "i32", B, "kind"),
          (list_, "i32", B, "list"), (count, "i32", 1, "count"), (hs, "f32", 6 * B, "hs", True))
    if stream is None:
        stream = torch.cuda.current_stream(x.device)
    _check(load().f110qp_replan_start_dev(C.byref(rp), C.byref(sc) if sc is not None else None, B, _tp(x),
                                          _tp(have_path), _tp(x_ref), _tp(gap), _tp(pose), _tp(kind), _tp(list_),
                                          _tp(count), _tp(hs), C.c_void_p(stream.cuda_stream)),
           "f110qp_replan_start_dev")


def advance_replan_dev(rc: RolloutConfig, rp: ReplanConfig, sc, horizon: int, x, kind, u_plan, status, plan_status,
                       x_ref, u_held, held_len, held_idx, have_path, x_next, u_lin_next, pose_next, u_applied=None,
                       kind_next=None, next_list=None, next_count=None, gap=None, hs_next=None, stream=None):
    """One tick's state machine and plant step (f110qp_advance_replan_dev); see include/f110qp.h."""
    import torch

    B, N, P = int(x.shape[0]), int(horizon), int(rp.plan.traj_discrete)
    _devs((x, "f64", 3 * B, "x"), (kind, "i32", B, "kind"), (u_plan, "f32", 2 * N * B, "u_plan"),
          (status, "i32", B, "status"), (plan_status, "i32", B, "plan_status"), (x_ref, "f64", 3 * P * B, "x_ref"),
          (gap, "i32", 4 * B, "gap", hs_next is None), (u_held, "f32", 2 * N * B, "u_held"),
          (held_len, "i32", B, "held_len"), (held_idx, "i32", B, "held_idx"), (have_path, "i32", B, "have_path"),
          (x_next, "f64", 3 * B, "x_next"), (u_lin_next, "f64", 2 * B, "u_lin_next"),
          (u_applied, "f32", 2 * B, "u_applied", True), (pose_next, "f64", 4 * B, "pose_next"),
          (kind_next, "i32", B, "kind_next", True), (next_list, "i32", B, "next_list", kind_next is None),
          (next_count, "i32", 1, "next_count", kind_next is None), (hs_next, "f32", 6 * B, "hs_next", True))
    if stream is None:
        stream = torch.cuda.current_stream(x.device)
    _check(load().f110qp_advance_replan_dev(
        C.byref(rc), C.byref(rp), C.byref(sc) if sc is not None else None, B, N, _tp(x), _tp(kind), _tp(u_plan),
        _tp(status), _tp(plan_status), _tp(x_ref), _tp(gap), _tp(u_held), _tp(held_len), _tp(held_idx),
        _tp(have_path), _tp(x_next), _tp(u_lin_next), _tp(u_applied), _tp(pose_next), _tp(kind_next),
        _tp(next_list), _tp(next_count), _tp(hs_next), C.c_void_p(stream.cuda_stream)), "f110qp_advance_replan_dev")


def select_dev(group, num_groups, cost, status, winner, best_cost, stream=None):
    """Per-scenario argmin on the device (f110qp_select_dev): group [B] i32, cost [B] f64,
    status [B] i32 -> winner [G] i32 (-1: no solved candidate), best_cost [G] f64."""
    import torch

    B = int(group.shape[0])
    _devs((group, "i32", B, "group"), (cost, "f64", B, "cost"), (status, "i32", B, "status"),
          (winner, "i32", int(num_groups), "winner"), (best_cost, "f64", int(num_groups), "best_cost"))
    if stream is None:
        stream = torch.cuda.current_stream(cost.device)
    _check(load().f110qp_select_dev(int(group.shape[0]), _tp(group), int(num_groups), _tp(cost), _tp(status),
                                    _tp(winner), _tp(best_cost), C.c_void_p(stream.cuda_stream)),
           "f110qp_select_dev")


def find_half_spaces(state, ranges, angle_min, angle_inc, angle_max, thresh=3.0, divider=1.5, buffer=3.0):
    """Constraints::FindHalfSpaces for one scan (host). Returns (l1, l2) or raises when the
    scan has no gap."""
    L = load()
    s = np.ascontiguousarray(state, np.float64)
    r = np.ascontiguousarray(ranges, np.float32)
    l1 = np.zeros(3)
    l2 = np.zeros(3)
    rc = L.f110qp_find_half_spaces(s.ctypes.data_as(C.POINTER(C.c_double)), r.ctypes.data_as(C.POINTER(C.c_float)),
                                   len(r), float(angle_min), float(angle_inc), float(angle_max), float(thresh),
                                   float(divider), float(buffer), l1.ctypes.data_as(C.POINTER(C.c_double)),
                                   l2.ctypes.data_as(C.POINTER(C.c_double)))
    _check(rc, "f110qp_find_half_spaces")
    return l1, l2


def find_half_spaces_dev(states, ranges, angle_min, angle_inc, angle_max, hs_out, gap_lo=None, gap_hi=None,
                         thresh=3.0, divider=1.5, buffer=3.0, stream=None):
    """Batched FindHalfSpaces on torch device tensors: states [B,3] f32, ranges [B,R] f32 ->
    hs_out [B,2,3] f32."""
    import torch

    L = load()
    if stream is None:
        stream = torch.cuda.current_stream(states.device)
    B, R = ranges.shape
    _devs((states, "f32", 3 * B, "states"), (ranges, "f32", B * R, "ranges"), (hs_out, "f32", 6 * B, "hs_out"),
          (gap_lo, "i32", B, "gap_lo", True), (gap_hi, "i32", B, "gap_hi", True))
    _check(L.f110qp_find_half_spaces_dev(B, _tp(states), _tp(ranges), R, float(angle_min), float(angle_inc),
                                         float(angle_max), float(thresh), float(divider), float(buffer),
                                         _tp(hs_out), _tp(gap_lo), _tp(gap_hi), C.c_void_p(stream.cuda_stream)),
           "f110qp_find_half_spaces_dev")


def find_half_spaces_dev_dbl(states, ranges, angle_min, angle_inc, angle_max, hs_out, gap_lo=None, gap_hi=None,
                             thresh=3.0, divider=1.5, buffer=3.0, stream=None):
    """find_half_spaces_dev on float64 states [B,3] (f110qp_find_half_spaces_dev_dbl): x and y enter
    the end points unrounded."""
    import torch

    L = load()
    B, R = ranges.shape
    _devs((states, "f64", 3 * B, "states"), (ranges, "f32", B * R, "ranges"), (hs_out, "f32", 6 * B, "hs_out"),
          (gap_lo, "i32", B, "gap_lo", True), (gap_hi, "i32", B, "gap_hi", True))
    if stream is None:
        stream = torch.cuda.current_stream(states.device)
    _check(L.f110qp_find_half_spaces_dev_dbl(B, _tp(states), _tp(ranges), R, float(angle_min), float(angle_inc),
                                             float(angle_max), float(thresh), float(divider), float(buffer),
                                             _tp(hs_out), _tp(gap_lo), _tp(gap_hi), C.c_void_p(stream.cuda_stream)),
           "f110qp_find_half_spaces_dev_dbl")


def gap_search_dev(sc: ScanConfig, ranges, gap_out, stream=None):
    """The gap search of FindHalfSpaces alone (f110qp_gap_search_dev): ranges [..., sc.num_ranges] f32,
    every leading index a scan -> gap_out, an int32 tensor of 4 words per scan holding the 16-byte
    records (lo, hi as int32, r_lo, r_hi as float32 bits: view the host copy as GAP_RECORD_DTYPE)."""
    import torch

    R = int(sc.num_ranges)
    if ranges.shape[-1] != R:
        raise F110QPError(f"ranges must be [..., num_ranges = {R}], got {tuple(ranges.shape)}")
    count = ranges.numel() // R if R else 0
    _devs((ranges, "f32", count * R, "ranges"), (gap_out, "i32", 4 * count, "gap_out"))
    if stream is None:
        stream = torch.cuda.current_stream(ranges.device)
    _check(load().f110qp_gap_search_dev(C.byref(sc), count, _tp(ranges), _tp(gap_out),
                                        C.c_void_p(stream.cuda_stream)), "f110qp_gap_search_dev")


def half_space_rows_dev(sc: ScanConfig, gap, states, hs_out, stream=None):
    """The end-point geometry of FindHalfSpaces (f110qp_half_space_rows_dev): gap [B] records (an
    int32 tensor of 4 words per car), states [B,3] f64 -> hs_out [B,2,3] f32."""
    import torch

    B = int(states.shape[0])
    _devs((gap, "i32", 4 * B, "gap"), (states, "f64", 3 * B, "states"), (hs_out, "f32", 6 * B, "hs_out"))
    if stream is None:
        stream = torch.cuda.current_stream(states.device)
    _check(load().f110qp_half_space_rows_dev(C.byref(sc), B, _tp(gap), _tp(states), _tp(hs_out),
                                             C.c_void_p(stream.cuda_stream)), "f110qp_half_space_rows_dev")


def gap_refresh_dev(sc: ScanConfig, ranges, states, gap_out, hs_out, stream=None):
    """gap_search_dev and half_space_rows_dev of B cars in one launch (f110qp_gap_refresh_dev): ranges
    [B, sc.num_ranges] f32, states [B,3] f64 -> gap_out (an int32 tensor of 4 words per car) and hs_out
    [B,2,3] f32, both bit-identical to those two calls."""
    import torch

    B, R = int(states.shape[0]), int(sc.num_ranges)
    if ranges.dim() != 2 or tuple(ranges.shape) != (B, R):
        raise F110QPError(f"ranges must be [B = {B}, num_ranges = {R}], got {tuple(ranges.shape)}")
    _devs((ranges, "f32", B * R, "ranges"), (states, "f64", 3 * B, "states"), (gap_out, "i32", 4 * B, "gap_out"),
          (hs_out, "f32", 6 * B, "hs_out"))
    if stream is None:
        stream = torch.cuda.current_stream(states.device)
    _check(load().f110qp_gap_refresh_dev(C.byref(sc), B, _tp(ranges), _tp(states), _tp(gap_out), _tp(hs_out),
                                         C.c_void_p(stream.cuda_stream)), "f110qp_gap_refresh_dev")


# ---- planning stage (plan_kernels.hip) ---------------------------------------------------------

def default_plan_config(**over) -> PlanConfig:
    c = PlanConfig()
    load().f110qp_default_plan_config(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def traj_table(cfg: PlanConfig) -> np.ndarray:
    """Traj_Plan::generate_traj_table (host): [T, P, 3] float64, car frame."""
    t = np.zeros((cfg.steer_discrete + 1, cfg.traj_discrete, 3), np.float64)
    rc = load().f110qp_traj_table(C.byref(cfg), _p(t))
    if rc < 0:
        _check(rc, "f110qp_traj_table")
    return t


def parse_waypoints(text: str, max_n: int = 100000) -> np.ndarray:
    """Trajectory::ReadCSV on CSV text: [n, 3] (x, y, ori)."""
    wp = np.zeros((max_n, 3), np.float64)
    n = C.c_int(0)
    _check(load().f110qp_parse_waypoints(text.encode(), _p(wp), max_n, C.byref(n)), "f110qp_parse_waypoints")
    return wp[: n.value].copy()


def grid_blocks(cfg: PlanConfig) -> int:
    return int(np.float32(cfg.size) / np.float32(cfg.discrete))


def plan_batch_dev(cfg: PlanConfig, pose, ranges, angle_min, angle_inc, angle_max, table, waypoints, x_ref, x0,
                   best_traj, best_global, status, valid=None, grid=None, stream=None):
    """Batched planning stage on torch device tensors: pose [B,4] f64, ranges [B,R] f32, table
    [T,P,3] f64, waypoints [W,2] f64 -> x_ref [B,P,3] f32, x0 [B,3] f32, best_traj / best_global
    / status [B] i32 (valid [B,T] u8 and grid [B,G,G] u8 optional)."""
    import torch

    B = pose.shape[0]
    if stream is None:
        stream = torch.cuda.current_stream(pose.device)
    _check(load().f110qp_plan_batch_dev(C.byref(cfg), B, _tp(pose), _tp(ranges), ranges.shape[1], float(angle_min),
                                        float(angle_inc), float(angle_max), _tp(table), _tp(waypoints),
                                        waypoints.shape[0], _tp(grid), _tp(valid), _tp(best_global), _tp(best_traj),
                                        _tp(x_ref), _tp(x0), _tp(status), C.c_void_p(stream.cuda_stream)),
           "f110qp_plan_batch_dev")


def _host(a, dtype, n: int, name: str, optional: bool = False):
    """Check a host output array before its raw pointer crosses the C ABI: a C-contiguous numpy
    array of the ABI's element type with at least n elements (the call writes exactly n)."""
    if a is None:
        if optional:
            return
        raise F110QPError(f"{name} is required")
    if not isinstance(a, np.ndarray) or a.dtype != dtype:
        got = a.dtype if isinstance(a, np.ndarray) else type(a).__name__
        raise F110QPError(f"{name} must be a {np.dtype(dtype).name} numpy array, got {got}")
    if not a.flags.c_contiguous or not a.flags.writeable:
        raise F110QPError(f"{name} must be C-contiguous and writeable")
    if a.size < n:
        raise F110QPError(f"{name} holds {a.size} elements, the call needs {n}")


def plan_batch(cfg: PlanConfig, pose, ranges, angle_min, angle_inc, angle_max, table, waypoints, x_ref, x0,
               best_traj, best_global, status, valid=None, grid=None):
    """Batched planning stage on host memory (f110qp_plan_batch, synchronous; the library stages
    through grow-only device buffers of the calling thread). Inputs as plan_batch_dev, as numpy
    arrays: pose [B,4], ranges [B,R], table [T,P,3], waypoints [W,2]. The outputs are the caller's
    arrays, of which the first B rows are written: x_ref [>=B,P,3] f32, x0 [>=B,3] f32, best_traj /
    best_global / status [>=B] i32 (valid [>=B,T] u8 and grid [>=B,G,G] u8 optional)."""
    pose = np.ascontiguousarray(pose, np.float64)
    ranges = np.ascontiguousarray(ranges, np.float32)
    table = np.ascontiguousarray(table, np.float64)
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64)[:, :2])
    B, T, P, G = pose.shape[0], cfg.steer_discrete + 1, cfg.traj_discrete, grid_blocks(cfg)
    if pose.shape != (B, 4) or ranges.ndim != 2 or ranges.shape[0] != B:
        raise F110QPError(f"pose must be [B,4] and ranges [B,R], got {pose.shape} and {ranges.shape}")
    if table.shape != (T, P, 3):
        raise F110QPError(f"table must be [{T},{P},3] for this config, got {table.shape}")
    _host(x_ref, np.float32, B * P * 3, "x_ref")
    _host(x0, np.float32, B * 3, "x0")
    _host(best_traj, np.int32, B, "best_traj")
    _host(best_global, np.int32, B, "best_global")
    _host(status, np.int32, B, "status")
    _host(valid, np.uint8, B * T, "valid", True)
    _host(grid, np.uint8, B * G * G, "grid", True)
    _check(load().f110qp_plan_batch(C.byref(cfg), B, _p(pose), _p(ranges), ranges.shape[1], float(angle_min),
                                    float(angle_inc), float(angle_max), _p(table), _p(wp) if wp.shape[0] else None,
                                    wp.shape[0], _p(grid), _p(valid), _p(best_global), _p(best_traj), _p(x_ref),
                                    _p(x0), _p(status)),
           "f110qp_plan_batch")
