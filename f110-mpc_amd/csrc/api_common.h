// api_common.h — what the C ABI's translation units share: f110qp_api.cpp (the context, the solve
// entry points), api_rollout.cpp (the closed loops), api_plan.cpp (half-spaces, planning stage),
// api_standings.cpp (race standings), api_mc.cpp (Monte Carlo outcomes) and api_field.cpp (the map's distance field).
// Everything here is internal to the library (hidden visibility: no new exported symbol).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "f110qp.h"
#include "lane_plan.h"

#pragma GCC visibility push(hidden)

// The message f110qp_last_error returns, one object per thread (defined in f110qp_api.cpp).
extern thread_local std::string g_last_error;

static inline int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

static inline int hip_fail(hipError_t e, const char* what) {
  return fail(F110QP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Device buffer that only grows (freed with its owner).
struct DevBuf {
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// Pinned, device-visible (fine-grained, coherent) host buffer that only grows.
struct HostBuf {
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  void* p = nullptr;  // host address
  void* d = nullptr;  // device address of the same memory
  size_t bytes = 0;
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, n, hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) { p = nullptr; return e; }
    e = hipHostGetDevicePointer(&d, p, 0);
    if (e != hipSuccess) { release(); return e; }
    bytes = n;
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = d = nullptr;
    bytes = 0;
  }
};

#pragma GCC visibility pop

// (default visibility, as the ABI header's declaration of it)
struct f110qp_ctx {
  f110qp_config cfg;
  f110qp::KParams kp;
  HostBuf hin, hout;  // host-pointer entry point: packed pinned staging [x0|u_lin|x_ref|hs], [u|x|st|it]
  DevBuf din, dout;   // their device copies for batches above kZeroCopyMaxBatch
  DevBuf wW, wkey, wact;  // warm-start slot state (config.warm_start)
  int warm_batch = 0;     // batch size the warm state was laid out for
  unsigned warm_calls = 0;  // warm calls since the state was laid out (WarmState::call, wraps)
  unsigned warm_prev[2] = {0u, 0u};  // the counters at the last f110qp_warm_hits
  hipStream_t warm_stream = nullptr;  // stream of the last warm call
  DevBuf gW, gkey, glead;    // grouped mode: W = H^-1, key and leader per group
  DevBuf dgrp;               // host-pointer grouped calls: device copy of the group ids
  DevBuf lscr;               // lane back end: HBM Riccati scratch (when not in LDS)
  DevBuf segtab;             // fixed-length segment kernels: the constant block of their code tables (lane_plan.h),
  hipEvent_t segtab_ev = nullptr;       // filled once on the first stream that needs it; the event later
  bool segtab_done = false;             // calls' streams wait on until it has been seen complete
  DevBuf hand;               // gap rows: counts and lists (f110qp::HandLayout, kHandInts(B) ints)
  DevBuf rplan;              // every rollout: one tick's u_plan | x_plan when the caller keeps neither
  DevBuf rdev;               // every host-pointer rollout: device copies of its arrays (api_stage.h)
  DevBuf rgap;               // scan, re-planning, world and race rollouts: one GapRecord per scan
                             // (scan_rows x B; the world and race rollouts hold one row set)
  DevBuf rhs;                // the same rollouts without hs_traj: the current tick's rows (B x 6 floats)
  DevBuf rscan;              // world rollout without ranges_traj: the current tick's scans (B x num_ranges)
  DevBuf rstate;             // re-planning rollout: held plans, indices, plan counters and list, and the
                             // optional per-tick arrays the caller did not give (ReplanWork)
  int lane_kmax = 16;        // lane back end: PDAS passes before single (least-index) flips
  int lane_mode = 0;         // lane scratch placement (LaneWork::mode)
  int lane_qpw = 0;          // lane QPs per wave (LaneWork::qpw, 0 = auto)
  int lane_rot = 1;          // lane heading-frame kernel when q0 == q1 (LaneWork::rot)
  int lane_dref = 1;         // lane fp64 references in LDS when they fit (LaneWork::dref)
  int lane_seg = 0;          // lane horizon segments per QP (LaneWork::seg: 0 auto, 1 off, 2/4/8)
  int lane_seg32 = 0;        // segmented kernel: force fp32 references + scratch (LaneWork::seg32)
  int lane_twin = 1;         // segmented kernel: twin PDAS starts where they fit (LaneWork::twin)
  int seg_fixedq = 1;        // segmented kernel: the fixed-length kernels where they apply (LaneWork::fixedq)
  int gap_screen = -1;      // gap rows, AUTO: box screen on the lane kernel (-1 by batch, 0 off, 1 on)
  int recheck_all = 0;      // gap rows: every QP of a call through the fp64 re-check alone (test build)
  HostBuf hsig;              // synchronous calls: the completion word they poll (wait_done)
  DevBuf dsig;               // its kernel's wave arrival count (zeroed once, re-zeroed by the kernel)
  unsigned sig_seq = 0;      // number of the last signalled call (the value the kernel publishes)
  int sig_poll = 1;          // 0: synchronous calls synchronise the stream (test build, F110QP_SIG_POLL=0)
  hipStream_t stream = nullptr;
  hipStream_t last_gap_stream = nullptr;  // stream of the last gap-row call (f110qp_last_recheck_count)
  int last_gap_batch = 0;                 // its batch (0: no gap-row call yet)
};

#pragma GCC visibility push(hidden)

static inline bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

// The limits of f110qp_find_half_spaces_dev on a scan config; rows: scan_rows must be 1 or `ticks`.
static inline int check_scan_config(const f110qp_scan_config* sc, bool rows, int ticks) {
  if (!sc) return fail(F110QP_ERR_INVALID, "scan config is NULL");
  if (sc->num_ranges < 1 || sc->num_ranges > 65535)
    return fail(F110QP_ERR_INVALID, "num_ranges must be in 1..65535");
  if (!(sc->angle_increment > 0.f)) return fail(F110QP_ERR_INVALID, "angle_increment must be > 0");
  if (rows && sc->scan_rows != 1 && sc->scan_rows != ticks)
    return fail(F110QP_ERR_INVALID, "scan_rows must be 1 or ticks");
  return F110QP_OK;
}

// The raster map of f110qp_cast_scans_grid_dev, f110qp_clearance_grid_dev and f110qp_rollout_grid[_dev]
// (api_rollout.cpp) and of the distance-field calls (api_field.cpp), checked, into *Gr. obstacles:
// num_circles + group_size + num_segments, which wall_params has checked to fit an int (0 for the field).
static inline int grid_params(const f110qp_grid_config* gc, long long obstacles, const void* grid,
                              f110qp::GridParams* Gr) {
  if (!gc) return fail(F110QP_ERR_INVALID, "grid config is NULL");
  if (gc->width < 0 || gc->height < 0) return fail(F110QP_ERR_INVALID, "grid width and height must be >= 0");
  const long long cells = (long long)gc->width * gc->height;
  if (cells > 0 && !grid) return fail(F110QP_ERR_INVALID, "width * height > 0 needs the grid");
  if (!(gc->resolution > 0.0) || !std::isfinite(gc->resolution))
    return fail(F110QP_ERR_INVALID, "grid resolution must be positive and finite");
  if (!(gc->reach >= 0.0) || !std::isfinite(gc->reach))
    return fail(F110QP_ERR_INVALID, "grid reach must be >= 0 and finite");
  if (!std::isfinite(gc->origin_x) || !std::isfinite(gc->origin_y))
    return fail(F110QP_ERR_INVALID, "grid origin must be finite");
  if (obstacles + cells > 0x7fffffffll)
    return fail(F110QP_ERR_INVALID, "num_circles + group_size + num_segments + width * height does not fit an int");
  Gr->W = gc->width;
  Gr->H = gc->height;
  Gr->ox = gc->origin_x;
  Gr->oy = gc->origin_y;
  Gr->res = gc->resolution;
  Gr->reach = gc->reach;
  return F110QP_OK;
}

// Back end of a call and, for the lane back end (or the gap screen), its workspace and its launch plan
// (f110qp_api.cpp).
int lane_work(f110qp_ctx* c, int batch, hipStream_t s, int* backend, f110qp::LaneWork* lw, f110qp::LanePlan* plan,
              bool grouped = false);

// A plan config's limits, with its grid_blocks into *G (api_plan.cpp).
int validate_plan(const f110qp_plan_config* c, int* G);

#pragma GCC visibility pop
