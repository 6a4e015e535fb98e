// f110qp_api.cpp — the core of the C ABI (include/f110qp.h) over the gfx950 kernels: the context, the
// solve and grouped entry points, the introspection calls and the debug hooks. The closed loops are in
// api_rollout.cpp, the half-space and planning-stage entry points in api_plan.cpp; api_common.h is
// what the three share.
//
// Host-side responsibilities only: argument validation, the device workspace of a context and
// H2D/D2H for the host-pointer entry points. No C++ exception crosses this boundary.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "api_common.h"

thread_local std::string g_last_error = "";

// Host-pointer calls of up to this many QPs (the per-tick call of the host MPC class) let the
// kernel read its inputs from and write its outputs to the pinned staging buffers directly
// (zero-copy over PCIe): one launch and one synchronisation per call, no copy engine.
constexpr int kZeroCopyMaxBatch = 64;

#ifdef F110QP_TEST_HOOKS
// Test / measurement build only (lib_test/libf110qp.so, -DF110QP_TEST_HOOKS): create-time knobs read
// from the environment that force one kernel variant or rule of the dispatch, so the tests reach every
// code path AUTO does not pick at their sizes. The product library (lib/libf110qp.so) reads no
// environment variable: its behaviour is the config alone (the reference's solver settings are fixed
// in code, src/mpc.cpp:98-99).
static int env_int(const char* name, int lo, int hi, int* out) {
  const char* e = std::getenv(name);
  if (!e) return 0;
  const int v = std::atoi(e);
  if (v < lo || v > hi) return 0;
  *out = v;
  return 1;
}

static void test_hooks(f110qp_ctx* c) {
  // PDAS passes of the lane back end before single least-index flips (0: single flips from pass 1)
  env_int("F110QP_LANE_KMAX", 0, 64, &c->lane_kmax);
  // QPs per wave of the lane back end (power of two <= 64)
  int v;
  if (env_int("F110QP_LANE_QPW", 1, 64, &v) && (v & (v - 1)) == 0) c->lane_qpw = v;
  // lane scratch: 1 LDS fp64, 2 LDS fp32, 3 HBM fp64, 4 HBM fp32
  env_int("F110QP_LANE_MODE", 0, 4, &c->lane_mode);
  // 0: general-frame lane kernel even when q0 == q1
  if (env_int("F110QP_LANE_ROT", 0, 1, &v)) c->lane_rot = v;
  // 0: float references in LDS (no fp64 DREF array)
  if (env_int("F110QP_LANE_DREF", 0, 1, &v)) c->lane_dref = v;
  // horizon segments per QP (0 auto, 1 off, 2 / 4 / 8 forced where the horizon and the LDS allow)
  if (env_int("F110QP_LANE_SEG", 0, 8, &v) && (v == 0 || v == 1 || v == 2 || v == 4 || v == 8)) c->lane_seg = v;
  // 1: the segmented kernel's float references and scratch
  if (env_int("F110QP_LANE_SEG_F32", 0, 1, &v)) c->lane_seg32 = v;
  // 0: one PDAS start per QP in the segmented kernel (the twin start off)
  if (env_int("F110QP_LANE_TWIN", 0, 1, &v)) c->lane_twin = v;
  // 0: the run-time-length segmented kernel where the fixed-length one would run
  if (env_int("F110QP_SEG_FIXEDQ", 0, 1, &v)) c->seg_fixedq = v;
  // gap rows: the box screen on (1) / off (0) at every batch size
  if (env_int("F110QP_GAP_SCREEN", 0, 1, &v)) c->gap_screen = v;
  // wave GI: 0 picks gap and box candidates by one ranking
  if (env_int("F110QP_GI_GAPFIRST", 0, 1, &v)) c->kp.gap_first = v;
  // lane kernels: PDAS passes per launch (measurement of the pass distribution: MAX_ITER past it)
  env_int("F110QP_LANE_PASSCAP", 1, 999, &c->kp.pass_cap);
  // wave kernel's box PDAS passes (0: GI from the unconstrained point)
  env_int("F110QP_PDAS_MAX", 0, 64, &c->kp.pdas_max);
  // gap rows: every QP of a call through the fp64 re-check (gi64_kernel.h) alone, no screen and no
  // fp32 GI: the re-check's own answers, for its parity tests
  if (env_int("F110QP_RECHECK_ALL", 0, 1, &v)) c->recheck_all = v;
  // 0: synchronous calls wait with hipStreamSynchronize, not on the kernel's completion word
  if (env_int("F110QP_SIG_POLL", 0, 1, &v)) c->sig_poll = v;
}
#endif

// Synchronous calls whose work is one kernel that raises the completion signal (f110qp::launch_signals:
// the box-only solve on the segmented lane kernel, the per-tick call) wait for that kernel's last
// wave to write the call's number to a pinned host word instead of synchronising the stream: the
// hipStreamSynchronize round trip measured 12.2 us p50 against 6.5 us for the polled word on an
// empty kernel (tools/microbench/flag_latency.hip). Arms the signal in *oo when the
// call's kernels raise it; *armed false: the caller synchronises the stream.
static int arm_signal(f110qp_ctx* c, int batch, int backend, const float* h, const f110qp::LanePlan& plan,
                      hipStream_t s, f110qp::ObjOut* oo, bool* armed) {
  *armed = false;
  if (!c->sig_poll || !f110qp::launch_signals(batch, backend, h, plan)) return F110QP_OK;
  if (!c->hsig.p) {
    hipError_t e = c->hsig.ensure(64);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc completion word");
    if ((e = c->dsig.ensure(64)) != hipSuccess) return hip_fail(e, "hipMalloc arrival count");
    if ((e = hipMemsetAsync(c->dsig.p, 0, 64, s)) != hipSuccess) return hip_fail(e, "hipMemsetAsync arrival count");
    __atomic_store_n((unsigned*)c->hsig.p, c->sig_seq, __ATOMIC_RELEASE);
  }
  oo->sig_host = (unsigned*)c->hsig.d;
  oo->sig_count = (unsigned*)c->dsig.p;
  oo->sig_seq = ++c->sig_seq;
  *armed = true;
  return F110QP_OK;
}

// Waits for the call armed by arm_signal (or synchronises the stream when it was not armed). The
// poll reads only the word (a hipStreamQuery inside the usual 10-15 us wait delayed the answer by
// its own cost and made the call bimodal); after kPollWindow it hands over to hipStreamSynchronize,
// so a stalled call does not keep a core spinning and a kernel that faults (no word) is reported by
// its HIP error (a gap-row call of 256 QPs, ~245 us, lost 7 us when the hand-over came at 200 us).
// A drained stream without the word is an error, not a wait.
constexpr auto kPollWindow = std::chrono::microseconds(1000);
static int wait_done(f110qp_ctx* c, hipStream_t s, bool armed) {
  if (armed) {
    const unsigned seq = c->sig_seq;
    const unsigned* w = (const unsigned*)c->hsig.p;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned k = 1;; k++) {
      if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) return F110QP_OK;
      if ((k & 255u) == 0 && std::chrono::steady_clock::now() - t0 > kPollWindow) break;
      __builtin_ia32_pause();
    }
  }
  const hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
  if (armed && __atomic_load_n((const unsigned*)c->hsig.p, __ATOMIC_ACQUIRE) != c->sig_seq)
    return fail(F110QP_ERR_HIP, "solve kernel finished without its completion signal");
  return F110QP_OK;
}

static int validate_config(const f110qp_config* c) {
  if (!c) return fail(F110QP_ERR_INVALID, "config is NULL");
  if (c->horizon < 1 || c->horizon > F110QP_MAX_HORIZON)
    return fail(F110QP_ERR_INVALID, "horizon must be in [1, 48] (one wave holds 2N inputs in <= 2 register rows)");
  if (!(c->dt > 0.f) || !std::isfinite(c->dt)) return fail(F110QP_ERR_INVALID, "dt must be > 0");
  for (int i = 0; i < 3; i++)
    if (!(c->q[i] >= 0.0) || !std::isfinite(c->q[i])) return fail(F110QP_ERR_INVALID, "Q must be >= 0 and finite");
  for (int i = 0; i < 2; i++) {
    if (!(c->r[i] > 0.0) || !std::isfinite(c->r[i]))
      return fail(F110QP_ERR_INVALID, "R must be > 0 (strictly convex QP) and finite");
    if (!std::isfinite(c->u_des[i])) return fail(F110QP_ERR_INVALID, "u_des must be finite");
    if (std::isnan(c->u_min[i]) || std::isnan(c->u_max[i])) return fail(F110QP_ERR_INVALID, "u_min / u_max is NaN");
    if (!(c->u_min[i] <= c->u_max[i])) return fail(F110QP_ERR_INVALID, "u_min > u_max");
    if (c->u_min[i] == INFINITY || c->u_max[i] == -INFINITY)
      return fail(F110QP_ERR_INVALID, "u_min = +inf / u_max = -inf leaves no input");
  }
  // stiff weights: the wave kernel works on the fp32 inverse of H = R + G'QG, and from
  // max(q) / min(r) = 1e5 (N = 48) it returned points off the optimum as SOLVED; from 1e4 both back
  // ends give up on QPs that have a solution (tests/test_gpu_config_corners.py). Up to 1e3 is tested.
  const double qmax = std::fmax(c->q[0], std::fmax(c->q[1], c->q[2])), rmin = std::fmin(c->r[0], c->r[1]);
  if (qmax > F110QP_MAX_WEIGHT_RATIO * rmin)
    return fail(F110QP_ERR_INVALID, "max(q) / min(r) must be <= 1e3 (the weight ratio limit of f110qp.h)");
  if (c->gap_mode != F110QP_GAP_INACTIVE && c->gap_mode != F110QP_GAP_ACTIVE)
    return fail(F110QP_ERR_INVALID, "gap_mode must be 0 (gap rows inactive) or 1 (active)");
  if (c->max_iter < 0) return fail(F110QP_ERR_INVALID, "max_iter must be >= 0");
  if (c->warm_start != 0 && c->warm_start != 1) return fail(F110QP_ERR_INVALID, "warm_start must be 0 or 1");
  if (c->x_ref_points != 0 && c->x_ref_points < c->horizon)
    return fail(F110QP_ERR_INVALID, "x_ref_points must be 0 (= horizon) or >= horizon");
  if (c->backend < F110QP_BACKEND_AUTO || c->backend > F110QP_BACKEND_LANE)
    return fail(F110QP_ERR_INVALID, "backend must be 0 (auto), 1 (wave) or 2 (lane)");
  return F110QP_OK;
}

static int check_batch_args(f110qp_ctx* c, int batch, const void* x0, const void* ul,
                            const void* xr, const void* hs, const void* uo, const void* xo,
                            const void* st) {
  if (!c) return fail(F110QP_ERR_INVALID, "ctx is NULL");
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (batch == 0) return F110QP_OK;
  if (!x0 || !ul || !xr || !uo || !xo || !st)
    return fail(F110QP_ERR_INVALID, "x0/u_lin/x_ref/u_out/x_out/status must be non-NULL");
  if (c->cfg.gap_mode == F110QP_GAP_ACTIVE && !hs)
    return fail(F110QP_ERR_INVALID, "gap_mode ACTIVE needs the halfspace array");
  if (batch > (1 << 30) / 64) return fail(F110QP_ERR_INVALID, "batch too large");
  return F110QP_OK;
}

// Warm-start slot state for a batch of `batch` QPs (allocated and zeroed on first use and
// whenever the batch size changes; zero keys = no valid entry).
static int warm_state(f110qp_ctx* c, int batch, hipStream_t s, f110qp::WarmState* ws) {
  *ws = f110qp::WarmState();
  if (!c->cfg.warm_start) return F110QP_OK;
  const size_t B = (size_t)batch, nu = 2 * (size_t)c->cfg.horizon;
  const size_t rows = (nu + 63) / 64;  // register rows per lane (act masks: 2 x 64 bits per row)
  hipError_t e;
  // keys (16 B per QP), then the lane back ends' last-hit call (warm_traffic) and the cumulative
  // traffic-call and hit counters (f110qp_warm_hits)
  const size_t wbytes = B * 16 + 16 + 8 * (B + 1);  // keys, last-hit call, per-wave counters
  if ((e = c->wW.ensure(B * nu * nu * 4)) || (e = c->wkey.ensure(wbytes)) ||
      (e = c->wact.ensure(B * 16 * rows)))
    return hip_fail(e, "hipMalloc warm-start state");
  if (c->warm_batch != batch) {
    if ((e = hipMemsetAsync(c->wkey.p, 0, wbytes, s)) || (e = hipMemsetAsync(c->wact.p, 0, B * 16 * rows, s)))
      return hip_fail(e, "hipMemsetAsync warm-start state");
    c->warm_batch = batch;
    c->warm_calls = 0;
    c->warm_prev[0] = c->warm_prev[1] = 0;
  }
  ws->W = (float*)c->wW.p;
  ws->key = (unsigned*)c->wkey.p;
  ws->act = (unsigned long long*)c->wact.p;
  ws->hit_call = (unsigned*)((char*)c->wkey.p + B * 16);
  ws->stats = (unsigned*)((char*)c->wkey.p + B * 16 + 16);  // per wave: hits, traffic calls
  ws->call = ++c->warm_calls;
  c->warm_stream = s;
  return F110QP_OK;
}

// The back end a call of `batch` QPs runs on (what AUTO resolves to). Box rows: the lane back end
// from F110QP_LANE_MIN_BATCH[_WIDE]. Gap rows: the wave kernel's GI (AUTO, WAVE), behind the box
// screen on the lane kernel for AUTO batches >= F110QP_GAP_SCREEN_MIN_BATCH; LANE: the box screen
// on the lane kernel for every batch (GI for the QPs it does not clear).
static int resolve_backend(f110qp_ctx* c, int batch, bool grouped) {
  const bool gap = c->cfg.gap_mode == F110QP_GAP_ACTIVE;
  int be = c->cfg.backend;
  if (gap)  // LANE: the screen path (never grouped or warm-started: those run GI on the wave kernel)
    return be == F110QP_BACKEND_LANE && !grouped && !c->cfg.warm_start ? F110QP_BACKEND_LANE : F110QP_BACKEND_WAVE;
  if (be == F110QP_BACKEND_AUTO) {
    const int min_b = grouped ? (c->cfg.horizon <= 32 ? F110QP_LANE_MIN_BATCH_GROUPED
                                                      : F110QP_LANE_MIN_BATCH_GROUPED_WIDE)
                              : (c->cfg.horizon <= 32 ? F110QP_LANE_MIN_BATCH : F110QP_LANE_MIN_BATCH_WIDE);
    const bool small = !grouped && c->cfg.horizon <= 32 && batch <= F110QP_LANE_MAX_SMALL_BATCH;
    be = (batch >= min_b || small) ? F110QP_BACKEND_LANE : F110QP_BACKEND_WAVE;
  }
  return be;
}

// Gap rows: does the call take the box screen on the lane kernel first (backend LANE, or AUTO from
// F110QP_GAP_SCREEN_MIN_BATCH; ungrouped, no warm-start state)?
static bool gap_screen(const f110qp_ctx* c, int batch, bool grouped) {
  if (c->cfg.gap_mode != F110QP_GAP_ACTIVE || grouped || c->cfg.warm_start) return false;
  if (c->cfg.backend == F110QP_BACKEND_LANE) return true;
  if (c->cfg.backend != F110QP_BACKEND_AUTO || c->gap_screen == 0) return false;
  return c->gap_screen == 1 || batch >= F110QP_GAP_SCREEN_MIN_BATCH;
}

// The lane back end's variant knobs of a context (the defaults, or the test build's F110QP_LANE_*):
// one copy for the launch and for the introspection calls, so that both resolve the same kernel.
static f110qp::LaneWork lane_knobs(const f110qp_ctx* c) {
  f110qp::LaneWork lw;
  lw.kmax = c->lane_kmax;
  lw.mode = c->lane_mode;
  lw.qpw = c->lane_qpw;
  lw.rot = c->lane_rot;
  lw.dref = c->lane_dref;
  lw.seg = c->lane_seg;
  lw.seg32 = c->lane_seg32;
  lw.twin = c->lane_twin;
  lw.fixedq = c->seg_fixedq;
  return lw;
}

// The introspection calls' view of a call of `batch` QPs: its back end, and the plan of its lane launch
// by the same resolve_backend, lane_knobs and lane_plan as the call itself (gap rows: the plan of the
// box screen's lane solve, whose kernels have no fixed-length variant). Not the lane back end: the
// neutral plan (one segment, one QP per wave, one start, no scratch).
static f110qp::LanePlan info_plan(f110qp_ctx* c, int batch, bool grouped, int* be) {
  *be = resolve_backend(c, batch, grouped);
  if (*be != F110QP_BACKEND_LANE) return f110qp::LanePlan();
  return f110qp::lane_plan(c->kp, batch, lane_knobs(c), c->cfg.gap_mode == F110QP_GAP_ACTIVE);
}

// The constant block of the fixed-length segment kernels (lane_plan.h), a function of c->kp's bounds,
// input weights and u_des, which no call changes after f110qp_create: filled on the device by the first
// call that plans such a kernel, on that call's stream and in front of its launch. Later calls
// make their stream wait on the fill's event until one of them has seen it complete; after that a call
// only takes the pointer.
static int seg_tab(f110qp_ctx* c, hipStream_t s, f110qp::LaneWork* lw) {
  hipError_t e;
  if (!c->segtab.p) {
    if (!c->segtab_ev && (e = hipEventCreateWithFlags(&c->segtab_ev, hipEventDisableTiming)) != hipSuccess)
      return hip_fail(e, "hipEventCreate segment tables");
    if ((e = c->segtab.ensure(f110qp::kSegBlockBytes)) != hipSuccess) return hip_fail(e, "hipMalloc segment tables");
    if ((e = f110qp::launch_seg_tab_fill(c->kp, (double*)c->segtab.p, s)) != hipSuccess ||
        (e = hipEventRecord(c->segtab_ev, s)) != hipSuccess) {
      c->segtab.release();  // (the event is kept for the next attempt)
      return hip_fail(e, "segment table fill");
    }
  } else if (!c->segtab_done) {
    // (every stream waits, the fill's own too: a wait on an event of the same stream is a no-op, and no
    // stream handle is compared)
    if (hipEventQuery(c->segtab_ev) == hipSuccess) c->segtab_done = true;
    else if ((e = hipStreamWaitEvent(s, c->segtab_ev, 0)) != hipSuccess)
      return hip_fail(e, "hipStreamWaitEvent segment tables");
  }
  lw->seg_tab = (const double*)c->segtab.p;
  return F110QP_OK;
}

// Back end of a call and, for the lane back end (or the gap screen), its workspace and the plan of its
// lane launch (resolved here, once per call: launch_solve and arm_signal read it).
int lane_work(f110qp_ctx* c, int batch, hipStream_t s, int* backend, f110qp::LaneWork* lw, f110qp::LanePlan* plan,
              bool grouped) {
  *lw = lane_knobs(c);
  *plan = f110qp::LanePlan();
  *backend = resolve_backend(c, batch, grouped) == F110QP_BACKEND_LANE ? f110qp::BACKEND_LANE
                                                                      : f110qp::BACKEND_WAVE;
  hipError_t e;
  if (c->cfg.gap_mode == F110QP_GAP_ACTIVE) {
    // counts and lists of the screen's GI list and of the fp64 re-check
    if ((e = c->hand.ensure(f110qp::kHandInts(batch) * sizeof(int))) != hipSuccess)
      return hip_fail(e, "hipMalloc gap-row lists");
    lw->hand = (int*)c->hand.p;
    lw->recheck_all = c->recheck_all;
    lw->screen = gap_screen(c, batch, grouped) && !c->recheck_all;
    c->last_gap_stream = s;
    c->last_gap_batch = batch;
    if (!lw->screen) return F110QP_OK;
  } else if (*backend == f110qp::BACKEND_WAVE) {
    return F110QP_OK;
  }
  // HBM scratch of ceil(B/L) waves x N stages x 8 values x L lanes (<= (B + 63) x N x 8 doubles)
  const size_t N = (size_t)c->cfg.horizon;
  e = c->lscr.ensure(((size_t)batch + 63) * N * 8 * sizeof(double));
  if (e != hipSuccess) return hip_fail(e, "hipMalloc lane workspace");
  lw->scratch = (double*)c->lscr.p;
  *plan = f110qp::lane_plan(c->kp, batch, *lw, lw->screen != 0);
  return plan->Q > 0 ? seg_tab(c, s, lw) : F110QP_OK;
}

// Per-group W cache of a grouped call (grows only; every call re-fills the slots it uses).
// key_words: unsigned words per group key (f110qp::kGroupKeyWords: 4 for float inputs, 8 for double
// ones, whose key holds all 64 bits of theta0, v and delta).
static int group_state(f110qp_ctx* c, const int* group, int num_groups, f110qp::WarmState* gws,
                       int** leader, int key_words) {
  const size_t G = (size_t)num_groups, nu = 2 * (size_t)c->cfg.horizon;
  hipError_t e;
  if ((e = c->gW.ensure(G * nu * nu * 4)) || (e = c->gkey.ensure(G * 4 * (size_t)key_words)) ||
      (e = c->glead.ensure(G * 4)))
    return hip_fail(e, "hipMalloc group state");
  *gws = f110qp::WarmState();
  gws->W = (float*)c->gW.p;
  gws->key = (unsigned*)c->gkey.p;
  gws->group = group;
  gws->ngroups = num_groups;
  *leader = (int*)c->glead.p;
  return F110QP_OK;
}

static int check_groups(const int* group, int num_groups, int batch) {
  if (!group) return fail(F110QP_ERR_INVALID, "group is NULL");
  (void)batch;
  if (num_groups < 1 || num_groups > (1 << 22)) return fail(F110QP_ERR_INVALID, "num_groups must be in [1, 2^22]");
  return F110QP_OK;
}

// device-pointer solve; sync: wait for it before returning (the completion word where the call's
// kernel raises it, else the stream). IN = float, or double for the *_dbl entry points: the kernels
// read the doubles themselves, and such a call neither reads nor updates the warm-start state (its
// 16-byte slot key holds float bits).
template <typename IN>
static int solve_dev(f110qp_ctx* c, int batch, const IN* x0, const IN* ul, const IN* xr,
                     const float* hs, float* uo, float* xo, int* st, int* it, double* obj,
                     double* cost, hipStream_t s, bool sync) {
  int rc = check_batch_args(c, batch, x0, ul, xr, hs, uo, xo, st);
  if (rc || batch == 0) return rc;
  const float* h = (c->cfg.gap_mode == F110QP_GAP_ACTIVE) ? hs : nullptr;
  f110qp::WarmState ws;
  if (sizeof(IN) == 4) rc = warm_state(c, batch, s, &ws);
  if (rc) return rc;
  int backend;
  f110qp::LaneWork lw;
  f110qp::LanePlan plan;
  rc = lane_work(c, batch, s, &backend, &lw, &plan);
  if (rc) return rc;
  f110qp::ObjOut oo;
  oo.obj = obj;
  oo.cost = cost;
  bool armed = false;
  if (sync && (rc = arm_signal(c, batch, backend, h, plan, s, &oo, &armed))) return rc;
  const f110qp::SolveIO<IN> io{batch, x0, ul, xr, h, uo, xo, st, it};
  hipError_t e = f110qp::launch_solve(c->kp, io, ws, backend, lw, plan, oo, s);
  if (e != hipSuccess) return hip_fail(e, "solve kernel launch");
  return sync ? wait_done(c, s, armed) : F110QP_OK;
}

template <typename IN>
static int solve_grouped_dev(f110qp_ctx* c, int batch, const IN* x0, const IN* ul, const IN* xr,
                             const float* hs, const int* group, int num_groups, float* uo, float* xo,
                             int* st, int* it, double* obj, double* cost, void* stream) {
  int rc = check_batch_args(c, batch, x0, ul, xr, hs, uo, xo, st);
  if (rc || batch == 0) return rc;
  if ((rc = check_groups(group, num_groups, batch))) return rc;
  const float* h = (c->cfg.gap_mode == F110QP_GAP_ACTIVE) ? hs : nullptr;
  f110qp::WarmState gws;
  int* leader;
  if ((rc = group_state(c, group, num_groups, &gws, &leader, f110qp::kGroupKeyWords<IN>))) return rc;
  int backend;
  f110qp::LaneWork lw;
  f110qp::LanePlan plan;
  if ((rc = lane_work(c, batch, (hipStream_t)stream, &backend, &lw, &plan, true))) return rc;
  f110qp::ObjOut oo;
  oo.obj = obj;
  oo.cost = cost;
  const f110qp::SolveIO<IN> io{batch, x0, ul, xr, h, uo, xo, st, it};
  hipError_t e = f110qp::launch_solve_grouped(c->kp, io, gws, leader, backend, lw, plan, oo, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "grouped solve launch");
  return F110QP_OK;
}

template <typename IN>
static int solve_host(f110qp_ctx* c, int batch, const IN* x0, const IN* ul, const IN* xr,
                      const float* hs, const int* group, int num_groups, float* uo, float* xo,
                      int* st, int* it, double* obj, double* cost) {
  int rc = check_batch_args(c, batch, x0, ul, xr, hs, uo, xo, st);
  if (rc || batch == 0) return rc;
  hipError_t e = hipSetDevice(c->cfg.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  if (!c->stream) {
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
  }
  const int N = c->cfg.horizon;
  const bool gap = c->cfg.gap_mode == F110QP_GAP_ACTIVE;
  const size_t B = (size_t)batch;
  const size_t S = (size_t)c->kp.xr_stride;
  const size_t s_x0 = B * 3 * sizeof(IN), s_ul = B * 2 * sizeof(IN), s_xr = B * S * 3 * sizeof(IN), s_hs = B * 6 * 4;
  const size_t s_uo = B * N * 2 * 4, s_xo = B * (N + 1) * 3 * 4, s_st = B * 4;
  // packed layouts (every size a multiple of 4 bytes; with double inputs the three input fields are
  // multiples of 8 bytes from an aligned base, so the doubles stay 8-byte aligned and the float
  // half-spaces follow them): in = x0 | u_lin | x_ref | halfspace,
  // out = u | x | status | iters | obj | cost (the doubles 8-byte aligned)
  const size_t o_ul = s_x0, o_xr = o_ul + s_ul, o_hs = o_xr + s_xr, in_bytes = o_hs + (gap ? s_hs : 0);
  const size_t o_xo = s_uo, o_st = o_xo + s_xo, o_it = o_st + s_st;
  const size_t o_ob = (o_it + s_st + 7) & ~(size_t)7, s_ob = B * 8;
  const size_t o_co = o_ob + (obj ? s_ob : 0);
  const size_t out_bytes = o_co + (cost ? s_ob : 0);
  if ((e = c->hin.ensure(in_bytes)) || (e = c->hout.ensure(out_bytes)))
    return hip_fail(e, "hipHostMalloc staging");
  char* hi = (char*)c->hin.p;
  std::memcpy(hi, x0, s_x0);
  std::memcpy(hi + o_ul, ul, s_ul);
  std::memcpy(hi + o_xr, xr, s_xr);
  if (gap) std::memcpy(hi + o_hs, hs, s_hs);
  hipStream_t s = c->stream;
  const bool zc = batch <= kZeroCopyMaxBatch;
  char* di = (char*)c->hin.d;
  char* dq = (char*)c->hout.d;
  if (!zc) {
    if ((e = c->din.ensure(in_bytes)) || (e = c->dout.ensure(out_bytes)))
      return hip_fail(e, "hipMalloc workspace");
    di = (char*)c->din.p;
    dq = (char*)c->dout.p;
    if ((e = hipMemcpyAsync(di, c->hin.p, in_bytes, hipMemcpyHostToDevice, s)))
      return hip_fail(e, "hipMemcpyAsync H2D");
  }
  int backend;
  f110qp::LaneWork lw;
  f110qp::LanePlan plan;
  f110qp::ObjOut oo;
  bool armed = false;
  oo.obj = obj ? (double*)(dq + o_ob) : nullptr;
  oo.cost = cost ? (double*)(dq + o_co) : nullptr;
  const f110qp::SolveIO<IN> io{batch, (const IN*)di, (const IN*)(di + o_ul), (const IN*)(di + o_xr),
                               gap ? (const float*)(di + o_hs) : nullptr, (float*)dq, (float*)(dq + o_xo),
                               (int*)(dq + o_st), (int*)(dq + o_it)};
  if (group) {
    if ((e = c->dgrp.ensure(B * 4)) || (e = hipMemcpyAsync(c->dgrp.p, group, B * 4, hipMemcpyHostToDevice, s)))
      return hip_fail(e, "group ids H2D");
    f110qp::WarmState gws;
    int* leader;
    if ((rc = group_state(c, (const int*)c->dgrp.p, num_groups, &gws, &leader, f110qp::kGroupKeyWords<IN>))) return rc;
    if ((rc = lane_work(c, batch, s, &backend, &lw, &plan, true))) return rc;
    e = f110qp::launch_solve_grouped(c->kp, io, gws, leader, backend, lw, plan, oo, s);
  } else {
    f110qp::WarmState ws;
    if (sizeof(IN) == 4 && (rc = warm_state(c, batch, s, &ws))) return rc;  // (double inputs: cold)
    if ((rc = lane_work(c, batch, s, &backend, &lw, &plan))) return rc;
    // zero-copy: the kernel's stores are the outputs the host reads, so its completion word ends
    // the wait (staged batches wait for the D2H copy on the stream)
    if (zc && (rc = arm_signal(c, batch, backend, io.hs, plan, s, &oo, &armed))) return rc;
    e = f110qp::launch_solve(c->kp, io, ws, backend, lw, plan, oo, s);
  }
  if (e != hipSuccess) return hip_fail(e, "solve kernel launch");
  if (!zc && (e = hipMemcpyAsync(c->hout.p, dq, out_bytes, hipMemcpyDeviceToHost, s)))
    return hip_fail(e, "hipMemcpyAsync D2H");
  if ((rc = wait_done(c, s, armed))) return rc;
  const char* ho = (const char*)c->hout.p;
  std::memcpy(uo, ho, s_uo);
  std::memcpy(xo, ho + o_xo, s_xo);
  std::memcpy(st, ho + o_st, s_st);
  if (it) std::memcpy(it, ho + o_it, s_st);
  if (obj) std::memcpy(obj, ho + o_ob, s_ob);
  if (cost) std::memcpy(cost, ho + o_co, s_ob);
  return F110QP_OK;
}

extern "C" {

int f110qp_version(void) { return F110QP_API_VERSION; }

const char* f110qp_last_error(void) { return g_last_error.c_str(); }

void f110qp_default_config(f110qp_config* c, int horizon) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->horizon = horizon;  // params.yaml:12 (reference default 30)
  c->dt = 0.01f;         // params.yaml:13
  c->q[0] = 10.0; c->q[1] = 10.0; c->q[2] = 0.0;  // params.yaml:1-3
  c->r[0] = 0.10; c->r[1] = 5.0;                  // params.yaml:5-6
  c->u_des[0] = 4.5; c->u_des[1] = 0.0;           // params.yaml:42-43
  c->u_min[0] = 3.0f; c->u_min[1] = -0.43f;       // params.yaml:47, constraints.cpp:21
  c->u_max[0] = 4.5f; c->u_max[1] = 0.43f;        // params.yaml:46, constraints.cpp:19
  c->gap_mode = F110QP_GAP_INACTIVE;
  c->max_iter = 0;
  c->device = 0;
  c->warm_start = 0;
  c->backend = F110QP_BACKEND_AUTO;
  c->x_ref_points = 0;
}

int f110qp_create(f110qp_ctx** out, const f110qp_config* cfg) {
  if (!out) return fail(F110QP_ERR_INVALID, "ctx out-pointer is NULL");
  *out = nullptr;
  int rc = validate_config(cfg);
  if (rc) return rc;
  f110qp_ctx* c = new (std::nothrow) f110qp_ctx();
  if (!c) return fail(F110QP_ERR_ALLOC, "out of host memory");
  c->cfg = *cfg;
  f110qp::KParams& k = c->kp;
  k.N = cfg->horizon;
  k.dt = cfg->dt;
  for (int i = 0; i < 3; i++) k.q[i] = cfg->q[i];
  for (int i = 0; i < 2; i++) {
    k.r[i] = cfg->r[i];
    k.udes[i] = cfg->u_des[i];
    k.umin[i] = cfg->u_min[i];
    k.umax[i] = cfg->u_max[i];
  }
  k.pdas_max = 10;
#ifdef F110QP_TEST_HOOKS
  test_hooks(c);
#endif
  const int nu = 2 * cfg->horizon;
  k.max_iter = cfg->max_iter > 0 ? cfg->max_iter : 8 * (nu + (cfg->gap_mode ? nu : 0)) + 16;
  k.xr_stride = cfg->x_ref_points > 0 ? cfg->x_ref_points : cfg->horizon;
  *out = c;
  return F110QP_OK;
}

void f110qp_destroy(f110qp_ctx* c) {
  if (!c) return;
  // a synchronous call returns on its completion word while its kernel may still be retiring: let
  // it finish before the word and the arrival count are freed (the caller's stream may be gone)
  if (c->sig_seq) (void)hipDeviceSynchronize();
  c->hsig.release(); c->dsig.release();
  c->hin.release(); c->hout.release(); c->din.release(); c->dout.release();
  c->wW.release(); c->wkey.release(); c->wact.release();
  c->lscr.release();
  c->segtab.release();
  if (c->segtab_ev) (void)hipEventDestroy(c->segtab_ev);
  c->hand.release();
  c->rplan.release(); c->rdev.release();
  c->gW.release(); c->gkey.release(); c->glead.release(); c->dgrp.release();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int f110qp_last_recheck_count(f110qp_ctx* c, int* count) {
  if (!c || !count) return fail(F110QP_ERR_INVALID, "ctx / count is NULL");
  *count = 0;
  if (c->cfg.gap_mode != F110QP_GAP_ACTIVE || c->last_gap_batch == 0 || !c->hand.p) return F110QP_OK;
  hipError_t e = hipStreamSynchronize(c->last_gap_stream);
  if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
  const f110qp::HandLayout H((int*)c->hand.p, c->last_gap_batch);
  if ((e = hipMemcpy(count, H.c_rc, sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess)
    return hip_fail(e, "hipMemcpy re-check count");
  return F110QP_OK;
}

int f110qp_warm_hits(f110qp_ctx* c, int* traffic, int* hits) {
  if (!c || !traffic || !hits) return fail(F110QP_ERR_INVALID, "ctx / traffic / hits is NULL");
  *traffic = 0;
  *hits = 0;
  if (!c->cfg.warm_start || c->warm_batch == 0 || !c->wkey.p) return F110QP_OK;
  hipError_t e = hipStreamSynchronize(c->warm_stream);
  if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
  // per-wave counters (hits, traffic calls) of every wave of the lane launches: every wave of a call
  // counts the same traffic, wave 0 is the call's count; the hits sum over the waves
  const size_t nw = (size_t)c->warm_batch + 1;
  std::vector<unsigned> st(2 * nw);
  if ((e = hipMemcpy(st.data(), (char*)c->wkey.p + (size_t)c->warm_batch * 16 + 16, st.size() * sizeof(unsigned),
                     hipMemcpyDeviceToHost)))
    return hip_fail(e, "hipMemcpy warm-start counters");
  unsigned hsum = 0;
  for (size_t w = 0; w < nw; w++) hsum += st[2 * w];
  *traffic = (int)(st[1] - c->warm_prev[0]);
  *hits = (int)(hsum - c->warm_prev[1]);
  c->warm_prev[0] = st[1];
  c->warm_prev[1] = hsum;
  return F110QP_OK;
}

int f110qp_test_build(void) {
#ifdef F110QP_TEST_HOOKS
  return 1;
#else
  return 0;
#endif
}

int f110qp_sync_signals(f110qp_ctx* c, unsigned* count) {
  if (!c || !count) return fail(F110QP_ERR_INVALID, "ctx / count is NULL");
  *count = c->sig_seq;
  return F110QP_OK;
}

int f110qp_warm_reset(f110qp_ctx* c) {
  if (!c) return fail(F110QP_ERR_INVALID, "ctx is NULL");
  c->warm_batch = 0;  // the next call re-zeroes the slot keys
  return F110QP_OK;
}

int f110qp_solve_batch_dev(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                           const float* xr, const float* hs, float* uo, float* xo, int* st,
                           int* it, void* stream) {
  return f110qp_solve_batch_ex_dev(c, batch, x0, ul, xr, hs, uo, xo, st, it, nullptr, nullptr, stream);
}

int f110qp_solve_batch_dev_dbl(f110qp_ctx* c, int batch, const double* x0, const double* ul,
                               const double* xr, const float* hs, float* uo, float* xo, int* st,
                               int* it, double* obj, double* cost, void* stream) {
  return solve_dev(c, batch, x0, ul, xr, hs, uo, xo, st, it, obj, cost, (hipStream_t)stream, false);
}

int f110qp_solve_batch_dev_sync_dbl(f110qp_ctx* c, int batch, const double* x0, const double* ul,
                                    const double* xr, const float* hs, float* uo, float* xo,
                                    int* st, int* it, void* stream) {
  return solve_dev(c, batch, x0, ul, xr, hs, uo, xo, st, it, nullptr, nullptr, (hipStream_t)stream, true);
}

int f110qp_solve_batch_dev_sync(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                                const float* xr, const float* hs, float* uo, float* xo, int* st,
                                int* it, void* stream) {
  return solve_dev(c, batch, x0, ul, xr, hs, uo, xo, st, it, nullptr, nullptr, (hipStream_t)stream, true);
}

int f110qp_solve_batch_ex_dev(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                              const float* xr, const float* hs, float* uo, float* xo, int* st,
                              int* it, double* obj, double* cost, void* stream) {
  return solve_dev(c, batch, x0, ul, xr, hs, uo, xo, st, it, obj, cost, (hipStream_t)stream, false);
}

int f110qp_solve_grouped_dev(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                             const float* xr, const float* hs, const int* group, int num_groups,
                             float* uo, float* xo, int* st, int* it, void* stream) {
  return f110qp_solve_grouped_ex_dev(c, batch, x0, ul, xr, hs, group, num_groups, uo, xo, st, it,
                                     nullptr, nullptr, stream);
}

int f110qp_solve_grouped_ex_dev(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                                const float* xr, const float* hs, const int* group, int num_groups,
                                float* uo, float* xo, int* st, int* it, double* obj, double* cost,
                                void* stream) {
  return solve_grouped_dev(c, batch, x0, ul, xr, hs, group, num_groups, uo, xo, st, it, obj, cost, stream);
}

int f110qp_solve_grouped_dev_dbl(f110qp_ctx* c, int batch, const double* x0, const double* ul,
                                 const double* xr, const float* hs, const int* group,
                                 int num_groups, float* uo, float* xo, int* st, int* it,
                                 double* obj, double* cost, void* stream) {
  return solve_grouped_dev(c, batch, x0, ul, xr, hs, group, num_groups, uo, xo, st, it, obj, cost, stream);
}

int f110qp_solve_batch_dbl(f110qp_ctx* c, int batch, const double* x0, const double* ul,
                           const double* xr, const float* hs, float* uo, float* xo, int* st,
                           int* it, double* obj, double* cost) {
  return solve_host(c, batch, x0, ul, xr, hs, nullptr, 0, uo, xo, st, it, obj, cost);
}

int f110qp_solve_grouped_dbl(f110qp_ctx* c, int batch, const double* x0, const double* ul,
                             const double* xr, const float* hs, const int* group, int num_groups,
                             float* uo, float* xo, int* st, int* it, double* obj, double* cost) {
  if (batch > 0) {
    const int rc = check_groups(group, num_groups, batch);
    if (rc) return rc;
  }
  return solve_host(c, batch, x0, ul, xr, hs, group, num_groups, uo, xo, st, it, obj, cost);
}

int f110qp_solve_batch(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                       const float* xr, const float* hs, float* uo, float* xo, int* st,
                       int* it) {
  return solve_host(c, batch, x0, ul, xr, hs, nullptr, 0, uo, xo, st, it, nullptr, nullptr);
}

int f110qp_solve_batch_ex(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                          const float* xr, const float* hs, float* uo, float* xo, int* st,
                          int* it, double* obj, double* cost) {
  return solve_host(c, batch, x0, ul, xr, hs, nullptr, 0, uo, xo, st, it, obj, cost);
}

int f110qp_solve_grouped(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                         const float* xr, const float* hs, const int* group, int num_groups,
                         float* uo, float* xo, int* st, int* it) {
  return f110qp_solve_grouped_ex(c, batch, x0, ul, xr, hs, group, num_groups, uo, xo, st, it,
                                 nullptr, nullptr);
}

int f110qp_solve_grouped_ex(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                            const float* xr, const float* hs, const int* group, int num_groups,
                            float* uo, float* xo, int* st, int* it, double* obj, double* cost) {
  if (batch > 0) {
    const int rc = check_groups(group, num_groups, batch);
    if (rc) return rc;
  }
  return solve_host(c, batch, x0, ul, xr, hs, group, num_groups, uo, xo, st, it, obj, cost);
}

int f110qp_backend_info(f110qp_ctx* c, int batch, int grouped, int* backend, int* qps_per_wave,
                        int* scratch) {
  if (!c) return fail(F110QP_ERR_INVALID, "ctx is NULL");
  if (batch < 1) return fail(F110QP_ERR_INVALID, "batch must be >= 1");
  int be;
  const f110qp::LanePlan plan = info_plan(c, batch, grouped != 0, &be);
  if (backend) *backend = be;
  if (qps_per_wave) *qps_per_wave = plan.qpw;
  if (scratch) *scratch = plan.mode;
  return F110QP_OK;
}

int f110qp_lane_segments(f110qp_ctx* c, int batch, int* segments) {
  if (!c || !segments) return fail(F110QP_ERR_INVALID, "ctx / segments is NULL");
  if (batch < 1) return fail(F110QP_ERR_INVALID, "batch must be >= 1");
  int be;
  *segments = info_plan(c, batch, false, &be).S;
  return F110QP_OK;
}

int f110qp_lane_starts(f110qp_ctx* c, int batch, int* starts) {
  if (!c || !starts) return fail(F110QP_ERR_INVALID, "ctx / starts is NULL");
  if (batch < 1) return fail(F110QP_ERR_INVALID, "batch must be >= 1");
  int be;
  *starts = info_plan(c, batch, false, &be).starts;
  return F110QP_OK;
}

int f110qp_lane_fixed_q(f110qp_ctx* c, int batch, int* stages) {
  if (!c || !stages) return fail(F110QP_ERR_INVALID, "ctx / stages is NULL");
  if (batch < 1) return fail(F110QP_ERR_INVALID, "batch must be >= 1");
  int be;
  *stages = info_plan(c, batch, false, &be).Q;
  return F110QP_OK;
}

int f110qp_gap_screen(f110qp_ctx* c, int batch, int* on) {
  if (!c || !on) return fail(F110QP_ERR_INVALID, "ctx / on is NULL");
  if (batch < 1) return fail(F110QP_ERR_INVALID, "batch must be >= 1");
  *on = gap_screen(c, batch, false);
  return F110QP_OK;
}

int f110qp_select_dev(int batch, const int* group, int num_groups, const double* cost,
                      const int* status, int* winner, double* best_cost, void* stream) {
  if (batch < 0 || num_groups < 0) return fail(F110QP_ERR_INVALID, "batch / num_groups < 0");
  if (num_groups == 0) return F110QP_OK;
  if (!winner || !best_cost || (batch > 0 && (!group || !cost || !status)))
    return fail(F110QP_ERR_INVALID, "NULL pointer argument");
  hipError_t e = f110qp::launch_select(batch, group, num_groups, cost, status, winner, best_cost,
                                       (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "select kernel launch");
  return F110QP_OK;
}

int f110qp_condense_debug_dev(f110qp_ctx* c, int batch, const float* x0, const float* ul,
                              const float* xr, double* H, double* g, void* stream) {
  if (!c) return fail(F110QP_ERR_INVALID, "ctx is NULL");
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (batch == 0) return F110QP_OK;
  if (!x0 || !ul || !xr || !H || !g) return fail(F110QP_ERR_INVALID, "NULL pointer argument");
  hipError_t e = f110qp::launch_condense_debug(c->kp, batch, x0, ul, xr, H, g,
                                               (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "condense kernel launch");
  return F110QP_OK;
}

int f110qp_qp_dims(int N, int* n, int* m, int* nnz_P, int* nnz_A) {
  if (N < 1 || N > F110QP_MAX_HORIZON) return fail(F110QP_ERR_INVALID, "horizon must be in [1, 48]");
  if (n) *n = 5 * N + 3;              // 3(N+1) states + 2N inputs (mpc.cpp:26-28)
  if (m) *m = 7 * N + 5;              // dynamics + gap + input rows (mpc.cpp:29)
  if (nnz_P) *nnz_P = 9 * (N + 1) + 4 * N;
  if (nnz_A) *nnz_A = 26 * N + 9;
  return F110QP_OK;
}

int f110qp_assemble_debug_dev(f110qp_ctx* c, const float* x0, const float* ul, const float* xr,
                              const float* hs, int* Pc, int* Pr, double* Pv, double* q, int* Ac,
                              int* Ar, double* Av, double* l, double* u, void* stream) {
  if (!c) return fail(F110QP_ERR_INVALID, "ctx is NULL");
  if (!x0 || !ul || !xr || !Pc || !Pr || !Pv || !q || !Ac || !Ar || !Av || !l || !u)
    return fail(F110QP_ERR_INVALID, "NULL pointer argument");
  const int gap = c->cfg.gap_mode == F110QP_GAP_ACTIVE;
  if (gap && !hs) return fail(F110QP_ERR_INVALID, "gap_mode ACTIVE needs the halfspace array");
  hipError_t e = f110qp::launch_assemble(c->kp, x0, ul, xr, hs, gap, Pc, Pr, Pv, q, Ac, Ar, Av, l, u,
                                         (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "assemble kernel launch");
  return F110QP_OK;
}

}  // extern "C"
