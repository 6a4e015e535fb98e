// f110qp_kernels.h — internal launch interface between the C ABI (f110qp_api.cpp) and the
// gfx950 kernels (f110qp_kernels.hip, halfspace_kernels.hip). Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace f110qp {

// per-QP status ids (== F110QP_* in include/f110qp.h)
constexpr int F110QP_SOLVED_ID = 1;
constexpr int F110QP_SOLVED_INACCURATE_ID = 2;
constexpr int F110QP_MAX_ITER_ID = -2;
constexpr int F110QP_PRIMAL_INFEASIBLE_ID = -3;
constexpr int F110QP_NUMERICAL_ID = -10;

// Kernel-side copy of f110qp_config (passed by value in kernarg memory).
struct KParams {
  int N;          // horizon
  float dt;       // MPC::dt_ (float)
  double q[3];    // diag Q
  double r[2];    // diag R
  double udes[2]; // desired input
  float umin[2];  // input lower bounds
  float umax[2];  // input upper bounds
  int max_iter;   // active-set iteration cap
  int xr_stride;  // points per QP in x_ref (>= N; the reference passes its whole miniPath)
  int pdas_max;   // PDAS passes of the wave kernel's box path before its GI loop takes over
  int pass_cap = 0;  // lane kernels: passes per launch (0: max_iter; measurement knob F110QP_LANE_PASSCAP)
  int gap_first = 1;  // wave GI with gap rows: a violated gap row is added before any box row
  int hs_nan_numerical = 0;  // gap rows: non-finite half-space rows give F110QP_NUMERICAL (the scan
                             // rollout, where they mean a scan without a gap), not PRIMAL_INFEASIBLE
};

// 1 + |lb| + |ub| as it enters the scale of a multiplier (flip) tolerance of the lane kernels,
// gtol = tol (1 + r scale): the bounds stand for the size of the inputs there. A bound far beyond
// the inputs (a "no bound" of 1e30, OSQP's INFTY: constraints.cpp:15; 1e20 or inf elsewhere) does
// not: with u_min = (3, -1e30), u_max = (1e30, 0.43) the plain sum made gtol 1e19, and an input once
// fixed on its finite bound never left it (a wrong point returned as SOLVED). Each |bound| counts
// up to m = 1 + |u_des| + the smaller |bound|, which is where the inputs of such a QP live. Where
// the larger |bound| is within m (the shipped box, every box around or next to u_des) this is
// the plain sum, bit for bit.
__host__ __device__ inline double bound_scale(double lb, double ub, double ud) {
  const double al = fabs(lb), au = fabs(ub);
  const double m = 1.0 + fabs(ud) + fmin(al, au);
  return 1.0 + fmin(al, m) + fmin(au, m);
}

// Warm-start state of a context (all null = cold solve). Per QP slot b of the batch:
//   W[b]   the cached W = H^-1 (2N x 2N, fp32) of the last solve of slot b,
//   key[b] the float bits of (theta0, v_lin, delta_lin) it was built for + a valid flag,
//   act[b] the active bounds at the last solution, per register row r of the lane map
//          (R = ceil(2N/64) rows): bit lane of act[2(R b + r)] lower, act[2(R b + r) + 1] upper.
// H depends only on the linearisation point (model.cpp:30-59), so a key hit reuses W exactly.
// Grouped mode (f110qp_solve_grouped*) reuses W/key as a per-GROUP cache instead: group[b] in
// [0, ngroups) names QP b's scenario, a prepare launch fills W[g]/key[g] from one member of each
// group, and every QP whose (theta0, v_lin, delta_lin) bits match its group's key skips the
// Hessian and the inverse (a QP that does not match builds its own: grouping never changes a
// result, the group's W is bit-identical to the one the QP would build).
struct WarmState {
  float* W = nullptr;
  unsigned* key = nullptr;
  unsigned long long* act = nullptr;
  const int* group = nullptr;
  int ngroups = 0;
  // lane back ends: the context's call counter (from 1) and a device int holding the last call in
  // which a wave saw a key hit (see warm_traffic)
  unsigned* hit_call = nullptr;
  unsigned call = 0;  // wraps after 2^32 calls: compared by unsigned difference only
  // lane back ends: cumulative counters per wave w (f110qp_warm_hits), stats[2w] QPs whose key hit,
  // stats[2w + 1] calls that moved warm traffic; read and written by the wave itself, only in a
  // call that moves the traffic
  unsigned* stats = nullptr;
};

// Whether a lane-back-end wave moves warm-start traffic in this call (loads its QPs' keys and masks,
// writes them back). On the closed-loop stream (configs[4]) theta0 changes every tick, so no key
// ever hits, and that traffic measured 0.7 us per call (0.55 the write-back, 0.15 the key loads:
// C5 kernel 29.2 against 28.5 cold). It runs while a hit was seen within the last kWarmRecent
// calls, and on two probe calls in every kWarmProbe (the first writes keys, the second can hit),
// so a stream whose linearisation points repeat turns it back on within kWarmProbe calls. Without
// hit_call (grouped / wave paths): always.
constexpr int kWarmRecent = 2, kWarmProbe = 32;
__device__ __forceinline__ unsigned warm_last_hit(const WarmState& ws) {  // load early, test late
  return ws.hit_call ? __builtin_nontemporal_load(ws.hit_call) : 0u;
}
__device__ __forceinline__ bool warm_traffic(const WarmState& ws, unsigned last) {
  if (!ws.act || !ws.key) return false;
  if (!ws.hit_call) return true;
  return ws.call - last <= (unsigned)kWarmRecent || ws.call % (unsigned)kWarmProbe <= 1u;
}

// LaneWork::hand for a call of B gap-row QPs: kHandInts(B) = 3 B + 4 ints, the two counts first
// (padded to four ints), then three B-int arrays.
struct HandLayout {
  int* c_list;  // [0] the screen's GI list count
  int* c_rc;    // [1] the fp64 re-check's count (the wave kernel appends its non-SOLVED QPs)
  int* list;    // [4, 4 + B) the screen's GI list, heavy first
  int* prio;    // [4 + B, 4 + 2B) screen: GI priority per QP
  int* rc;      // [4 + 2B, 4 + 3B) the re-check list
  HandLayout(int* h, int B)
      : c_list(h), c_rc(h + 1), list(h + 4), prio(h + 4 + (size_t)B), rc(h + 4 + 2 * (size_t)B) {}
};
constexpr size_t kHandInts(int B) { return 3 * (size_t)B + 4; }

// Workspace of the lane-per-QP kernel (lane_kernel.h): the HBM Riccati scratch when it does
// not stay in LDS (ceil(B/L) x N x 8 x L doubles at most, L QPs per wave <= 64).
struct LaneWork {
  double* scratch = nullptr;
  int kmax = 16;  // PDAS passes (all violations flip) before single flips (least index)
  int mode = 0;   // scratch: 0 auto, 1 LDS fp64, 2 LDS fp32, 3 HBM fp64, 4 HBM fp32 (workspace)
  int qpw = 0;    // QPs per wave: 0 auto (lane_plan.h), else a power of two <= 64
  int rot = 1;    // 1: heading-frame kernel when q0 == q1 (lane_kernel.h ROT); 0: general frame
  int dref = 1;   // 1: fp64 references in LDS when the resident waves fit (DREF); 0: float
  int seg = 0;    // horizon segments per QP (lane_seg_kernel.h): 0 auto, 1 off, 2 / 4 / 8 forced
  int seg32 = 0;  // segmented kernel: 1 forces float references and Riccati scratch in LDS
  int twin = 1;   // segmented kernel: two PDAS starts per QP where the grid leaves SIMDs idle
  int fixedq = 1; // segmented kernel: the fixed-length kernels (five-stage segments) where they apply
  const double* seg_tab = nullptr;  // their code tables: the solver's constant block (lane_plan.h)
  int* hand = nullptr;  // gap rows: counts + per-QP lists (HandLayout, kHandInts(B) ints)
  int screen = 0;       // gap rows: box solve on the lane kernel first, GI only for the QPs whose
                        // box optimum violates a gap row (f110qp_kernels.hip)
  int recheck_all = 0;  // gap rows, test build only: every QP through the fp64 re-check alone
};

// Optional per-QP objective outputs (fp64, computed in the kernels' output sweeps from the fp64
// solution): obj[b] = OSQP's objective 1/2 z'Pz + q'z of the reference QP (mpc.cpp:208-229;
// OSQP drops the constant), cost[b] = the same plus that constant
// 1/2 sum_i r_i'Q r_i + N/2 u_des'R u_des, i.e. sum 1/2|x_i - r_i|_Q^2 + 1/2|u_i - u_des|_R^2 >= 0.
struct ObjOut {
  double* obj = nullptr;
  double* cost = nullptr;
  // gap-row box screen fused into the segmented lane kernel's output sweep (f110qp_kernels.hip):
  // the half-spaces, and per QP the GI priority it writes (0: the box optimum stands; else 1 + the
  // gap rows it violates; null: no screen)
  const float* scr_hs = nullptr;
  int* scr_prio = nullptr;
  // wave kernel, gap rows: QPs it does not report SOLVED are appended here for the fp64 re-check
  // (count + list; null: the re-check flags them itself)
  int* rc_count = nullptr;
  int* rc_list = nullptr;
  // completion signal of a synchronous call, raised by its last kernel (signal_call_done): every
  // workgroup arrives on sig_count once its stores are visible at system scope; the last one
  // re-zeroes the count and writes sig_seq to sig_host (the pinned host word the calling thread
  // polls). null: none
  unsigned* sig_host = nullptr;
  unsigned* sig_count = nullptr;
  unsigned sig_seq = 0;
};

// The launch plan of a lane back end call (lane_plan.h).
struct LanePlan;

// whether launch_solve's kernels for this call raise ObjOut's completion signal (every ungrouped
// call: its last kernel is a lane, wave or re-check kernel that signals); the caller synchronises
// the stream otherwise
bool launch_signals(int B, int backend, const float* hs, const LanePlan& plan);

// The completion signal at the very end of a call's last kernel (ObjOut::sig_*): every wave's
// stores visible at system scope (zero-copy outputs in pinned host memory; device outputs written
// back from this XCD's L2), then one arrival per workgroup (after a barrier when it has several
// waves); the last arrival re-zeroes the count for the next call and publishes the call's number
// to the host word the caller polls (f110qp_api.cpp wait_done). Every workgroup must reach it; one
// that stored nothing (wrote = false: a re-check workgroup past the list) skips the fence, whose L2
// write-back walk is what makes a burst of them costly.
__device__ __forceinline__ void signal_call_done(const ObjOut& oo, bool wrote = true) {
  if (!oo.sig_host) return;
  if (wrote) __threadfence_system();
  if (blockDim.x > 64) __syncthreads();
  if (threadIdx.x != 0) return;
  if (gridDim.x == 1) {  // one workgroup: no arrival count to go through
    __hip_atomic_store(oo.sig_host, oo.sig_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const unsigned arrived = __hip_atomic_fetch_add(oo.sig_count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (arrived + 1u == gridDim.x) {
    __hip_atomic_store(oo.sig_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(oo.sig_host, oo.sig_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// IN in the launch functions below: the input scalar of x0, u_lin and x_ref, float or double (the
// *_dbl entry points of include/f110qp.h); both are instantiated in the kernels' objects.
// The arrays of one solve call of B QPs, from the ABI down to the kernel launch (the kernels take
// them as loose parameters).
template <typename IN>
struct SolveIO {
  int B;
  const IN* x0;
  const IN* u_lin;
  const IN* x_ref;
  const float* hs;  // the half-space rows, or null (box rows alone)
  float* u_out;
  float* x_out;
  int* status;
  int* iters;
};

// fp64 re-check of the gap-row QPs the wave kernel did not report SOLVED (its certificate
// failed, or GI ended infeasible / at its cap): the fp64 Goldfarb-Idnani of gi64_kernel.h over
// the device-side list (count, list: HandLayout c_rc / rc), every listed QP, its outputs rewritten.
template <typename IN>
hipError_t launch_gap_recheck(const KParams& P, const SolveIO<IN>& io, const int* list, const int* count,
                              const ObjOut& oo, hipStream_t stream);

enum Backend { BACKEND_WAVE = 0, BACKEND_LANE = 1 };

// The per-group key of a grouped call (gws.key) holds kGroupKeyWords<IN> unsigned words per group.
template <typename IN>
constexpr int kGroupKeyWords = sizeof(IN) == 8 ? 8 : 4;

// Solve B QPs. hs == nullptr -> box-only kernels (gap rows inactive). backend LANE: box rows, the
// lane-per-QP Riccati/PDAS kernel alone (one launch, no hand-over). Gap rows: lw.screen, the box
// solve on the lane kernel, GI for the QPs whose box optimum violates a gap row; else GI for every
// QP; then the fp64 re-check of what GI did not certify. plan: lane_plan(P, io.B, lw, lw.screen)
// where a lane kernel runs (backend LANE on box rows, lw.screen on gap rows; not read otherwise),
// resolved once by the caller, which arms the completion signal from the same record.
template <typename IN>
hipError_t launch_solve(const KParams& P, const SolveIO<IN>& io, const WarmState& warm, int backend,
                        const LaneWork& lw, const LanePlan& plan, const ObjOut& oo, hipStream_t stream);

// The lane-per-QP kernel alone (box rows): the instance and launch parameters plan names.
template <typename IN>
hipError_t launch_lane(const KParams& P, const SolveIO<IN>& io, const WarmState& warm, const LaneWork& lw,
                       const LanePlan& plan, const ObjOut& oo, hipStream_t stream);

// Grouped solve: leader (smallest member) of every group, W = H^-1 per group from its leader,
// then the solve (wave back end; the lane back end has no factor to share and ignores groups).
// ws.W/ws.key hold ngroups slots, leader ngroups ints.
template <typename IN>
hipError_t launch_solve_grouped(const KParams& P, const SolveIO<IN>& io, const WarmState& gws, int* leader,
                                int backend, const LaneWork& lw, const LanePlan& plan, const ObjOut& oo,
                                hipStream_t stream);

// Per-scenario selection (the argmin of src/project.cpp:125-136 taken over the
// QP costs): winner[g] = the smallest b with group[b] == g, status[b] == SOLVED and the minimal
// cost[b]; -1 when the group has no solved member. best[g] = that cost (+inf if none).
hipError_t launch_select(int B, const int* group, int G, const double* cost, const int* status,
                         int* winner, double* best, hipStream_t stream);

// Plant step of the closed loop (rollout_kernels.hip): kernel-side copy of f110qp_rollout_config
// without its tick count.
struct AdvanceParams {
  double plant_dt;    // Euler step of Model::simulate_dynamics
  double car_length;  // CAR_LENGTH of src/model.cpp:2
  double v_lin;       // v of the next linearisation input (src/project.cpp:170)
  double fail_u[2];   // Input of GetNextInput() without a solution (src/project.cpp:215)
};

// One Euler step of B cars on the first input of their plans u_plan [B][N][2] (a solve's u_out,
// 8-byte aligned), and the next linearisation input: x [B][3] -> x_next [B][3], u_lin_next [B][2],
// u_applied [B][2] (float32, 8-byte aligned, may be null). A car whose status is not SOLVED /
// SOLVED_INACCURATE (its plan is NaN) takes fail_u. One thread per car, one launch.
hipError_t launch_advance(const AdvanceParams& P, int B, int N, const double* x, const float* u_plan,
                          const int* status, double* x_next, double* u_lin_next, float* u_applied,
                          hipStream_t stream);

// Dump the condensed H (B x 2N x 2N) and g (B x 2N) as built by the solve kernel.
hipError_t launch_condense_debug(const KParams& P, int B, const float* x0, const float* u_lin,
                                 const float* x_ref, double* H, double* g, hipStream_t stream);

// One instance's (P, q, A, l, u) in the reference's CSC layout (assemble_kernel.hip).
hipError_t launch_assemble(const KParams& P, const float* x0, const float* u_lin, const float* x_ref,
                           const float* hs, int gap_active, int* Pc, int* Pr, double* Pv, double* q,
                           int* Ac, int* Ar, double* Av, double* l, double* u, hipStream_t stream);

// Planning stage (plan_kernels.hip): grid size, candidate count / length, float params.
struct PlanKParams {
  int G;            // grid_blocks_ = size_ / discrete_
  int T;            // candidates (steer_discrete + 1)
  int P;            // points per candidate (traj_discrete)
  float discrete;   // occ_discrete
  float dilation;   // occ_dilation
  float lookahead;  // Trajectory::lookahead
};

hipError_t launch_plan(const PlanKParams& K, int B, const double* pose, const float* ranges,
                       int nr, float angle_min, float angle_inc, float angle_max,
                       const double* table, const double* wp, int W, unsigned char* grid_out,
                       unsigned char* valid_out, int* best_global, int* best_traj, float* x_ref,
                       float* x0, int* status, hipStream_t stream);

// Batched FindHalfSpaces (constraints.cpp:116-265), one wave per scan. ST: the scalar of states,
// float or double (both instantiated in halfspace_kernels.hip).
template <typename ST>
hipError_t launch_half_spaces(int B, const ST* states, const float* ranges, int num_ranges,
                              float angle_min, float angle_inc, float angle_max, float thresh,
                              float divider, float buffer, float* hs, int* gap_lo, int* gap_hi,
                              hipStream_t stream);

// FindHalfSpaces split at the point where the pose enters (halfspace_geom.h): the gap search of
// `count` scans, one wave each, into one GapRecord per scan (constraints.cpp:118-177) ...
struct GapRecord;
hipError_t launch_gap_search(int count, const float* ranges, int num_ranges, float angle_min,
                             float angle_inc, float angle_max, float thresh, float divider, float buffer,
                             GapRecord* rec, hipStream_t stream);
// ... and the end-point geometry (:179-264) of B cars, one thread each: gap [B], states [B][3]
// double -> hs [B][2][3].
hipError_t launch_half_space_rows(int B, int num_ranges, float angle_min, float angle_inc,
                                  const GapRecord* gap, const double* states, float* hs,
                                  hipStream_t stream);
// Both in one launch, one wave per car (f110qp_gap_refresh_dev): ranges [B][num_ranges] and states
// [B][3] double -> rec [B] and hs [B][2][3], bit-identical to launch_gap_search followed by
// launch_half_space_rows on the same arrays.
hipError_t launch_gap_refresh(int B, const float* ranges, int num_ranges, float angle_min, float angle_inc,
                              float angle_max, float thresh, float divider, float buffer, const double* states,
                              GapRecord* rec, float* hs, hipStream_t stream);

// launch_advance plus that geometry at x_next, written to hs_next [B][2][3] (null: no rows, the plant
// step alone): one launch. Every other output is bit-identical to launch_advance's.
hipError_t launch_advance_scan(const AdvanceParams& P, int B, int N, const double* x, const float* u_plan,
                               const int* status, int num_ranges, float angle_min, float angle_inc,
                               const GapRecord* gap, double* x_next, double* u_lin_next, float* u_applied,
                               float* hs_next, hipStream_t stream);

// ---- closed loop with re-planning (rollout_kernels.hip, plan_kernels.hip) -------------------------
// tick kinds (== F110QP_TICK_* in include/f110qp.h)
constexpr int TICK_MPC = 0, TICK_PLAN = 1, TICK_HOLD = 2, TICK_PLAN_FAILED = 3, TICK_CRASHED = 4;

// launch_plan for the cars of a device-side list: workgroups stride over list[0 .. min(*count, B)),
// at most plan_listed_grid(B) of them; a workgroup past the count exits at its first load. pose is
// the pose row [B][4] (x, y, sin(ori/2), cos(ori/2)), ranges [B][nr]. Per listed car: status,
// best_global, best_traj, and on status 0 its path as doubles (widened floats, ori 0) into x_ref
// [B][P][3]; a car without a path keeps the one it has. Unlisted cars are not touched.
int plan_listed_grid(int B);
hipError_t launch_plan_listed(const PlanKParams& K, int B, const int* list, const int* count,
                              const double* pose, const float* ranges, int nr, float angle_min,
                              float angle_inc, float angle_max, const double* table, const double* wp,
                              int W, int* best_global, int* best_traj, double* x_ref, int* status,
                              hipStream_t stream);

// The per-car OdomCallback state around one plant step (advance_replan_kernel), all [B] unless said.
struct ReplanStep {
  const double* x;         // [B][3] this tick's pose
  int* kind;               // this tick's kind; a PLAN tick whose plan failed is rewritten PLAN_FAILED
  const float* u_plan;     // [B][N][2] this tick's solve (read on MPC ticks)
  int* status;             // the solve's status; set to 0 on ticks that are not MPC ticks
  const int* plan_status;  // the listed plan's status (read on PLAN ticks)
  const double* x_ref;     // [B][P][3] the paths (the end point is read)
  int P;
  double replan_dist;
  float* u_held;           // [B][N][2] the published plan
  int* held_len;           // N or 0
  int* held_idx;           // inputs_idx_
  int* have_path;          // get_mini_path_
  double* x_next;          // [B][3]
  double* u_lin_next;      // [B][2]
  float* u_applied;        // [B][2] or null
  double* pose_next;       // [B][4] the pose row the next tick's plan reads
  int* kind_next;          // the next tick's kind, or null (then no list either)
  int* next_list;          // the cars whose next tick is a PLAN tick, in any order
  int* next_count;         // their count (one atomicAdd per wave; zero on entry)
  const GapRecord* gap;    // the records of the scans the next tick reads (with hs_next)
  float* hs_next;          // [B][2][3] or null
  int nr;
  float angle_min, angle_inc;
  // launch_advance_replan_park only: a car with crash_tick[b] >= 0 parks, and repeats its rows
  const int* crash_tick;   // the first row in contact or -1 (launch_clearance's mark)
  const double* u_lin;     // [B][2] this tick's linearisation input
  const double* pose;      // [B][4] this tick's pose row
};
hipError_t launch_advance_replan(const AdvanceParams& P, int B, int N, const ReplanStep& S,
                                 hipStream_t stream);
// The same with parking (f110qp_rollout_contact[_dev] at stop_on_contact = 1): a car whose crash_tick is
// not -1 takes no action on its state (path flag, held plan and index stay), applies (0, 0), repeats the
// bits of its x, u_lin and pose rows into the next ones, has its kind rewritten TICK_CRASHED and its
// status F110QP_NO_SOLVE, is announced TICK_CRASHED in kind_next and is not appended to the plan list; its
// half-space rows are those of the unchanged pose. Every other car is launch_advance_replan's, bit for
// bit. The kernel is advance_replan_kernel's template with PARK = true; the plain launch is PARK = false.
hipError_t launch_advance_replan_park(const AdvanceParams& P, int B, int N, const ReplanStep& S,
                                      hipStream_t stream);

// The launch in front of the loop: pose row 0, kind 0, list 0 (count zero on entry) and, with hs0,
// the half-space rows of tick 0.
struct ReplanStart {
  const double* x;       // [B][3]
  const int* have_path;
  const double* x_ref;   // [B][P][3]
  int P;
  double replan_dist;
  double* pose;          // [B][4]
  int* kind;
  int* list;
  int* count;
  const GapRecord* gap;
  float* hs;             // [B][2][3] or null
  int nr;
  float angle_min, angle_inc;
};
hipError_t launch_replan_start(int B, const ReplanStart& S, hipStream_t stream);

// ---- the world of a car: what it sees (scan_kernels.hip) and what it touches (contact_kernels.hip) ---
// Circles [world_rows][C][3] = (cx, cy, r) (null when C = 0); car b reads row 0 (world_rows 1) or row b.
// Obstacles are processed kCastCircleTile at a time (== F110QP_CAST_CIRCLE_TILE).
constexpr int kCastCircleTile = 256;
struct CastParams {
  int nr;
  float angle_min, angle_inc;
  int C;
  int world_rows;  // 1 or B
  double lidar_offset, max_range;
};
// Races: the B cars are B / G races of G consecutive cars (B % G == 0), and every car also meets each of
// its G - 1 race-mates as the circle (x_m + center_offset cos(ori_m), y_m + center_offset sin(ori_m),
// car_radius) at the mate's pose in x.
struct RaceParams {
  int G;
  double car_radius, center_offset;
};
// Rectangular bodies (body_geom.h): a car is the rectangle with centre (x + center_offset cos(ori), y +
// center_offset sin(ori)), axes along and across the heading and half extents (hl, hw); Q.car_radius is not read.
struct BodyParams {
  double hl, hw;  // half length, half width
};
// Straight walls (wall_geom.h): S segments (ax, ay, bx, by) behind the circles and the mates, segments
// [wall_rows][S][4] (null when S = 0); car b reads row 0 (wall_rows 1) or row b (wall_rows B).
struct WallParams {
  int S;
  int wall_rows;  // 1 or B
};
// A noisy LiDAR (rules Z1 to Z3 of include/f110qp.h): the walls cast with seeded range noise and dropout on
// every beam it stores. drop24 = floor(dropout * 2^24), taken on the host; tick is rule Z3's t of this launch.
struct NoiseParams {
  unsigned long long seed;
  unsigned long long car_base;  // >= 0: car b draws from stream car_base + b
  double sigma_abs, sigma_rel;
  unsigned drop24;
  int tick;
};
// A raster map (grid_geom.h, rules G1 and G2 of include/f110qp.h): one occupancy grid [H][W] of bytes for all
// cars, nonzero occupied, cell (i, j) the square from (ox + i res, oy + j res); W * H == 0: no map (grid null).
struct GridParams {
  int W, H;
  double ox, oy, res;
  double reach;  // the clearance alone: how far beyond the body it looks
};
// The families, each the one before plus one thing: circles alone (casts only), the race-mates as circles,
// the cars as rectangles (the slab test in the cast, body_sd / body_pair in the clearance), the segments
// (rules W1 and W2), the noise on the scans (the clearance never reads it: it is the walls'), the raster map
// (rules G1 and G2) under the noise.
enum WorldFamily {
  WORLD_CIRCLES = 0,
  WORLD_RACE = 1,
  WORLD_BODY = 2,
  WORLD_WALLS = 3,
  WORLD_NOISY = 4,
  WORLD_GRID = 5
};
// One description of the world for both jobs. A family reads the records up to its own.
struct World {
  WorldFamily family;
  CastParams P;  // the clearance reads C and world_rows alone
  RaceParams Q;
  BodyParams H;
  WallParams Wl;
  NoiseParams Z;  // the casts of WORLD_NOISY and WORLD_GRID alone
  const double* circles;
  const double* segments;
  GridParams Gr;  // WORLD_GRID alone, as is grid
  const unsigned char* grid;
  // the cast alone: rule F1 in place of rule G1 (f110qp_grid_cast_dev). d2 [H][W] is grid's field (null without a
  // map), visits [B][nr] or null the cells of d2 each beam read
  bool field;
  const int* d2;
  int* visits;
};

// Grid caps: one 256-thread workgroup per car, one wave on each of a CU's four SIMDs, up to what the MI355X's
// 256 CUs hold at once; a larger batch strides. From the code-object metadata, not from a sweep
// of caps (none was measured): a SIMD's 512 VGPRs are allocated in granules of eight, so a kernel with v
// VGPRs keeps floor(512 / roundup8(v)) waves per SIMD, a CU as many workgroups, and LDS allows more in
// every row (37,888 B a cast workgroup, 44,032 B with bodies; 512 B and 640 B a clearance workgroup):
//   cast       circles, race 155 -> 3 -> 768 (forcing four waves spills 17 VGPRs to scratch)
//              body 183 (184 allocated), walls 185 (192) -> 2 -> 512
//   clearance  race 127 (the fp64 sincos and the eight poses' running minima) -> 4 -> 1,024
//              body, walls 185 (192) -> 2 -> 512
//              noisy 191 (192) -> 2 -> 512: the walls' caps, and its clearance is the walls instantiation
//   grid       cast 216 -> 2 -> 512, with 65,152 B of LDS (the cast's 44,032 B and the 21,120 B square of cell bits):
//              two workgroups in a CU's 160 KB, the same two; clearance 195 (200) -> 2 -> 512, 640 B
//              the field cast (World::field) 213 (216) -> 2 -> 512, 44,032 B: the grid row's cap
// Nothing spills a VGPR and no kernel has scratch.
constexpr struct {
  int cast, clearance;
} kWorldGrids[6] = {{768, 0}, {768, 1024}, {512, 512}, {512, 512}, {512, 512}, {512, 512}};  // by WorldFamily

// Ray casting, workload._ray_circles on the device: per car the scan of nr beams at pose x [B][3] from the
// LiDAR lidar_offset ahead, ranges [B][nr] float32. At most cast_scans_grid(family, B) workgroups striding over
// all B cars (list and count null) or over list[0 .. min(*count, B)) as launch_plan_listed; unlisted cars
// are not touched.
int cast_scans_grid(WorldFamily family, int B);
hipError_t launch_cast_scans(const World& w, int B, const int* list, const int* count, const double* x, float* ranges,
                             hipStream_t stream);

// The clearance of rows x B poses x [rows][B][3] to everything each car can touch: the C circles of its
// world, the G - 1 mates of its race at the same row of x and (WORLD_WALLS) the S segments, the car's body
// being the race model's circle (WORLD_RACE) or the rectangle. clearance [rows][B], nearest [rows][B] or null
// (the index of the minimum: j, C + i for mate i of the race, C + G + k for segment k, -1 for none). At most
// clearance_grid(family, B) workgroups striding over the cars; one launch. No WORLD_CIRCLES clearance.
// The rollout's crash record, updated by the same launch (crash_tick null: no record): crash_tick[b] is the
// first row whose clearance is <= margin, counted from row0, or -1. init: the launch starts every car
// from -1; otherwise from what crash_tick holds (a car that has crashed keeps its row).
struct ClearParams {
  int C;
  int world_rows;  // 1 or B
};
struct ContactMark {
  int* crash_tick;  // [B] or null
  int row0;         // the row of x_traj that row 0 of this launch is
  int init;
  double margin;
};
int clearance_grid(WorldFamily family, int B);
hipError_t launch_clearance(const World& w, int B, int rows, const double* x, double* clearance, int* nearest,
                            const ContactMark& M, hipStream_t stream);

// ---- standings (standings_kernels.hip) ------------------------------------------------------------
// The projection of rows x B poses x [rows][B][3] onto the closed path wp [W][2] with cumulative lengths
// cum [W+1] (the model of include/f110qp.h): seg [rows][B] or null, s [rows][B], lateral [rows][B] or null.
// One workgroup per car, at most progress_grid(B) of them striding over the cars; one launch.
int progress_grid(int B);
hipError_t launch_progress(int B, int rows, const double* x, const double* wp, const double* cum, int W, int* seg,
                           double* s, double* lateral, hipStream_t stream);
// The standings of the B / G races from s [rows][B] on a path of length L: dist [rows][B], lap [rows][B] or
// null, rank [rows][B]. Two launches on the stream (the accumulation in row order, one thread per car; then
// the ranks, one thread per row and car), nothing between them but the stream's order.
hipError_t launch_standings(int G, int B, int rows, const double* s, double L, double* dist, int* lap, int* rank,
                            hipStream_t stream);

// ---- Monte Carlo outcomes (mc_kernels.hip) ----------------------------------------------------------
// The quantile fan of v [rows][B] (the model of include/f110qp.h): B = S M G, K = B / M sample sets of M values
// at stride G; fan [rows][K][Q], count [rows][K] or null. One launch: the wave kernel when M padded to a power
// of two (mc_fan_padded) is at most 64, the LDS kernel up to F110QP_MC_MAX_HYPOTHESES. mc_fan_grid: the
// workgroups of that launch for rows x K items, at most 2,048 (wave) or 1,024 (LDS), which stride.
int mc_fan_padded(int M);
int mc_fan_grid(int M, long long items);
hipError_t launch_mc_fan(int M, int G, int Q, const double* prob, int B, int rows, const double* v, double* fan,
                         int* count, hipStream_t stream);
// alive [T + 1][K] and crashed [K] or null from crash_tick [B]: one launch, one thread per (row, set).
hipError_t launch_mc_survival(int M, int G, int B, int T, const int* crash_tick, int* alive, int* crashed,
                              hipStream_t stream);
// Every car's record from clear [T + 1][B], status and kind [T][B] (either may be null): one launch, one thread
// per car. Every output but min_clear may be null.
hipError_t launch_mc_outcomes(int B, int T, const double* clear, const int* status, const int* kind,
                              double* min_clear, int* min_row, int* unsolved, int* first_unsolved, int* plan_failed,
                              hipStream_t stream);

// ---- the raster map's distance field (field_kernels.hip) ---------------------------------------------
// Rules D1 and D2 of include/f110qp.h for grid [H][W], W and H in 1..32,768: d2 [H][W], nearest [H][W] or null,
// work [H][W] of scratch. Two launches on the stream (the rows: a wave per row, at most field_rows_grid(H)
// workgroups striding; the columns: one thread per cell), nothing between them but the stream's order.
int field_rows_grid(int H);
hipError_t launch_grid_distance(int W, int H, const unsigned char* grid, int* d2, int* nearest, int* work,
                                hipStream_t stream);
// out [H][W] = rule D3's metres of d2 <= radius: one launch, one thread per cell.
hipError_t launch_grid_inflate(int W, int H, double res, const int* d2, double radius, unsigned char* out,
                               hipStream_t stream);
// Rule D4 at rows x B poses x [rows][B][3]: dist [rows][B], cell [rows][B] or null (nearest is read only with
// it). One launch of at most field_lookup_grid(rows x B) workgroups, which stride. G.reach is not read.
int field_lookup_grid(long long n);
hipError_t launch_grid_lookup(const GridParams& G, const int* d2, const int* nearest, int B, int rows,
                              const double* x, double* dist, int* cell, hipStream_t stream);

}  // namespace f110qp
