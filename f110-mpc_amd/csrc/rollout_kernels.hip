// rollout_kernels.hip — the plant step of the device-resident closed loop (f110qp_advance_dev,
// f110qp_rollout[_dev] of include/f110qp.h), and the plant step fused with the next tick's
// half-space rows (f110qp_advance_scan_dev, f110qp_rollout_scan[_dev]).
//
// One thread per car: Model::simulate_dynamics (reference src/model.cpp:61-75) on the first input of
// a solve's plan, and the next linearisation input as project::OdomCallback forms it (GetNextInput()
// with v forced, src/project.cpp:169-170,210-218). 56 bytes in and 40 (48 with u_applied) out per
// car, three fp64 trig calls: the launch is the cost, so there is no LDS, no cross-lane traffic and
// no atomic in these two. The re-planning loop's step (advance_replan_kernel, below) adds the per-car
// OdomCallback state and one ballot and one atomic per wave for the next tick's plan list; its PARK
// instantiation (advance_replan_park_kernel) parks the cars that contact_kernels.hip has marked crashed.
#include <hip/hip_runtime.h>

#include "f110qp_kernels.h"
#include "halfspace_geom.h"

namespace f110qp {

__global__ __launch_bounds__(256) void advance_kernel(const AdvanceParams P, const int B, const int N,
                                                      const double* __restrict__ x,
                                                      const float* __restrict__ u_plan,
                                                      const int* __restrict__ status,
                                                      double* __restrict__ x_next,
                                                      double* __restrict__ u_lin_next,
                                                      float* __restrict__ u_applied) {
  // the reference's x86 build rounds every product and sum (model.cpp:67-71): no fused multiply-add
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int st = status[b];
  const bool usable = st == F110QP_SOLVED_ID || st == F110QP_SOLVED_INACCURATE_ID;  // u_plan is finite
  // u*_0 and u*_1 as two 8-byte loads: row b starts 8 N bytes into an 8-byte aligned array, which
  // is 16-byte aligned only for even N
  const float2* row = reinterpret_cast<const float2*>(u_plan) + (size_t)b * N;
  const float2 u0 = row[0];
  const float2 u1 = row[N > 1 ? 1 : 0];
  // the applied input is the float32 of the plan (the drive message carries float32), widened
  const double v = usable ? (double)u0.x : P.fail_u[0];
  const double delta = usable ? (double)u0.y : P.fail_u[1];
  const double px = x[3 * (size_t)b], py = x[3 * (size_t)b + 1], th = x[3 * (size_t)b + 2];
  const double d0 = v * cos(th);
  const double d1 = v * sin(th);
  const double d2 = tan(delta) * v / P.car_length;
  x_next[3 * (size_t)b] = px + d0 * P.plant_dt;
  x_next[3 * (size_t)b + 1] = py + d1 * P.plant_dt;
  x_next[3 * (size_t)b + 2] = th + d2 * P.plant_dt;
  // GetNextInput(): the next input of the solved trajectory, Input(0.5, 0) without one; v forced
  u_lin_next[2 * (size_t)b] = P.v_lin;
  u_lin_next[2 * (size_t)b + 1] = usable ? (double)u1.y : P.fail_u[1];
  if (u_applied) reinterpret_cast<float2*>(u_applied)[b] = usable ? u0 : make_float2((float)v, (float)delta);
}

hipError_t launch_advance(const AdvanceParams& P, int B, int N, const double* x, const float* u_plan,
                          const int* status, double* x_next, double* u_lin_next, float* u_applied,
                          hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(advance_kernel, dim3((B + 255) / 256), dim3(256), 0, s, P, B, N, x, u_plan, status,
                     x_next, u_lin_next, u_applied);
  return hipGetLastError();
}

// advance_kernel, then the next tick's half-space rows at the pose it has just formed: the reference
// calls FindHalfSpaces(current_state_, scan_msg_) on every tick (src/mpc.cpp:73-75) with the scan it
// stored once, and only the end-point geometry reads the pose (halfspace_geom.h), about 30 scalar
// operations and two sincos per car on values this thread already holds in registers. The plant step
// is advance_kernel's expressions, so every output but hs_next has advance_kernel's bits. gap [B]: the
// records of the scans the next tick reads; 24 more bytes out and 16 more in per car.
__global__ __launch_bounds__(256) void advance_scan_kernel(const AdvanceParams P, const int B, const int N,
                                                           const double* __restrict__ x,
                                                           const float* __restrict__ u_plan,
                                                           const int* __restrict__ status, const int nr,
                                                           const float angle_min, const float angle_inc,
                                                           const GapRecord* __restrict__ gap,
                                                           double* __restrict__ x_next,
                                                           double* __restrict__ u_lin_next,
                                                           float* __restrict__ u_applied,
                                                           float* __restrict__ hs_next) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int st = status[b];
  const bool usable = st == F110QP_SOLVED_ID || st == F110QP_SOLVED_INACCURATE_ID;
  const float2* row = reinterpret_cast<const float2*>(u_plan) + (size_t)b * N;
  const float2 u0 = row[0];
  const float2 u1 = row[N > 1 ? 1 : 0];
  const GapRecord g = hs_next ? gap[b] : GapRecord{-1, -1, 0.f, 0.f};  // loaded early, used last
  const double v = usable ? (double)u0.x : P.fail_u[0];
  const double delta = usable ? (double)u0.y : P.fail_u[1];
  const double px = x[3 * (size_t)b], py = x[3 * (size_t)b + 1], th = x[3 * (size_t)b + 2];
  const double d0 = v * cos(th);
  const double d1 = v * sin(th);
  const double d2 = tan(delta) * v / P.car_length;
  const double nx = px + d0 * P.plant_dt;
  const double ny = py + d1 * P.plant_dt;
  const double nth = th + d2 * P.plant_dt;
  x_next[3 * (size_t)b] = nx;
  x_next[3 * (size_t)b + 1] = ny;
  x_next[3 * (size_t)b + 2] = nth;
  u_lin_next[2 * (size_t)b] = P.v_lin;
  u_lin_next[2 * (size_t)b + 1] = usable ? (double)u1.y : P.fail_u[1];
  if (u_applied) reinterpret_cast<float2*>(u_applied)[b] = usable ? u0 : make_float2((float)v, (float)delta);
  if (!hs_next) return;
  float o[6];
  half_space_rows(g, nr, nx, ny, nth, angle_min, angle_inc, o);
#pragma unroll
  for (int j = 0; j < 6; j++) hs_next[6 * (size_t)b + j] = o[j];
}

hipError_t launch_advance_scan(const AdvanceParams& P, int B, int N, const double* x, const float* u_plan,
                               const int* status, int nr, float angle_min, float angle_inc,
                               const GapRecord* gap, double* x_next, double* u_lin_next, float* u_applied,
                               float* hs_next, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(advance_scan_kernel, dim3((B + 255) / 256), dim3(256), 0, s, P, B, N, x, u_plan, status,
                     nr, angle_min, angle_inc, gap, x_next, u_lin_next, u_applied, hs_next);
  return hipGetLastError();
}

// ---- closed loop with re-planning -----------------------------------------------------------------
// The next tick's kind at the pose the plant step has just formed (host/src/project.cpp:35,76-82):
// PLAN without a path; with one, HOLD when Transforms::CalcDist(car, path end) < replan_dist, else
// MPC. CalcDist (transforms.cpp:20-22) subtracts in float, squares and adds in double (std::pow of a
// float promotes), takes the double root and narrows it to float; the reference compares that float
// with the double 1.98.
__device__ __forceinline__ int tick_kind(const int have, const double x, const double y, const double ex,
                                         const double ey, const double replan_dist) {
#pragma clang fp contract(off)
  if (!have) return TICK_PLAN;
  const float dx = (float)x - (float)ex, dy = (float)y - (float)ey;
  const float dist = (float)sqrt((double)dx * (double)dx + (double)dy * (double)dy);
  return (double)dist < replan_dist ? TICK_HOLD : TICK_MPC;
}

// Append the cars of this wave whose next tick plans to the next tick's list: one ballot, one vector
// atomicAdd per wave that holds such a car (lane 0, every lane of the wave is still here), the
// position of each car its rank among the wave's set bits. A position past the list (a counter that
// was not zero on entry) is dropped.
__device__ __forceinline__ void append_plan_list(const bool plans, const int b, const int B,
                                                 int* __restrict__ list, int* __restrict__ count) {
  const unsigned long long m = __ballot(plans);
  if (m == 0ull) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(count, __popcll(m));
  base = __shfl(base, 0, 64);
  const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
  if (plans && pos >= 0 && pos < B) list[pos] = b;
}

// A parked car's tick (advance_replan<true>): no action on (u_held, len, idx, have_path); the applied input
// is (0, 0); the next x, u_lin and pose rows repeat this tick's bits; this tick's kind is rewritten CRASHED
// over what the previous tick announced (as PLAN_FAILED is over PLAN) and the next one announced CRASHED;
// the status is F110QP_NO_SOLVE; the half-space rows are those of the unchanged pose.
__device__ __forceinline__ void park_car(const int b, const ReplanStep& S) {
#pragma clang fp contract(off)
  const double px = S.x[3 * (size_t)b], py = S.x[3 * (size_t)b + 1], th = S.x[3 * (size_t)b + 2];
  S.kind[b] = TICK_CRASHED;
  S.status[b] = 0;
  S.x_next[3 * (size_t)b] = px;
  S.x_next[3 * (size_t)b + 1] = py;
  S.x_next[3 * (size_t)b + 2] = th;
  S.u_lin_next[2 * (size_t)b] = S.u_lin[2 * (size_t)b];
  S.u_lin_next[2 * (size_t)b + 1] = S.u_lin[2 * (size_t)b + 1];
  if (S.u_applied) reinterpret_cast<float2*>(S.u_applied)[b] = make_float2(0.f, 0.f);
#pragma unroll
  for (int j = 0; j < 4; j++) S.pose_next[4 * (size_t)b + j] = S.pose[4 * (size_t)b + j];
  if (S.kind_next) S.kind_next[b] = TICK_CRASHED;
  if (S.hs_next) {
    float o[6];
    half_space_rows(S.gap[b], S.nr, px, py, th, S.angle_min, S.angle_inc, o);
#pragma unroll
    for (int j = 0; j < 6; j++) S.hs_next[6 * (size_t)b + j] = o[j];
  }
}

// advance_scan_kernel plus the per-car state machine of Project::OdomCallback + Project::DriveStep
// (host/src/project.cpp:31-100; include/f110qp.h, "closed loop with re-planning"). One thread per car.
// The tick's action on (u_held, len, idx, have_path), DriveStep's input, the plant step in
// advance_kernel's expressions (for the same applied input x_next, u_lin_next, u_applied and hs_next
// have advance_scan_kernel's bits), the pose row of the next tick's plan, the next tick's kind and
// its plan list. The N float2 of a plan move only on a usable MPC tick; every other tick reads at most
// two of the held inputs.
//
// PARK (advance_replan_park_kernel, f110qp_rollout_contact[_dev] at stop_on_contact = 1): a car whose
// crash_tick is not -1 takes park_car instead of the tick. Every parking statement is behind `if constexpr`;
// the plain kernel is the PARK = false instantiation.
template <bool PARK>
__device__ __forceinline__ void advance_replan(const AdvanceParams& P, const int B, const int N, const ReplanStep& S) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  const bool live = b < B;  // no early return: the ballot below wants whole waves
  int knext = TICK_MPC;
  bool parked = false;
  if constexpr (PARK) {
    if (live && S.crash_tick[b] >= 0) {
      parked = true;
      knext = TICK_CRASHED;  // not a PLAN tick: the car is not appended to the list
      park_car(b, S);
    }
  }
  if (live && !parked) {
    int kind = S.kind[b];
    int have = S.have_path[b], len = S.held_len[b], idx = S.held_idx[b];
    const GapRecord g = S.hs_next ? S.gap[b] : GapRecord{-1, -1, 0.f, 0.f};
    const double px = S.x[3 * (size_t)b], py = S.x[3 * (size_t)b + 1], th = S.x[3 * (size_t)b + 2];
    float2* held = reinterpret_cast<float2*>(S.u_held) + (size_t)b * N;
    float2 a0 = make_float2(0.f, 0.f), a1 = a0;  // the inputs at idx and idx + 1 after the action
    bool fresh = false;                          // ... already in registers (a usable MPC tick)
    if (kind == TICK_PLAN) {
      if (S.plan_status[b] == 0) {
        have = 1;
      } else {
        kind = TICK_PLAN_FAILED;
        S.kind[b] = kind;
      }
    } else if (kind == TICK_HOLD) {
      have = 0;  // miniPath_ dropped; MPC::Update keeps its solution, re-published at index 0
      idx = 0;
    } else {
      const int st = S.status[b];
      const bool usable = st == F110QP_SOLVED_ID || st == F110QP_SOLVED_INACCURATE_ID;
      idx = 0;
      len = 0;
      if (usable) {
        const float2* row = reinterpret_cast<const float2*>(S.u_plan) + (size_t)b * N;
        for (int k = 0; k < N; k++) {
          const float2 u = row[k];
          held[k] = u;
          if (k == 0) a0 = u;
          if (k == 1) a1 = u;
        }
        len = N;
        fresh = true;
      }
    }
    if (kind != TICK_MPC) S.status[b] = 0;
    // DriveStep: the input at the index, fail_u past the end; then the index moves
    const bool has0 = idx < len, has1 = idx + 1 < len;
    if (!fresh) {
      if (has0) a0 = held[idx];
      if (has1) a1 = held[idx + 1];
    }
    idx++;
    const double v = has0 ? (double)a0.x : P.fail_u[0];
    const double delta = has0 ? (double)a0.y : P.fail_u[1];
    const double d0 = v * cos(th);
    const double d1 = v * sin(th);
    const double d2 = tan(delta) * v / P.car_length;
    const double nx = px + d0 * P.plant_dt;
    const double ny = py + d1 * P.plant_dt;
    const double nth = th + d2 * P.plant_dt;
    S.x_next[3 * (size_t)b] = nx;
    S.x_next[3 * (size_t)b + 1] = ny;
    S.x_next[3 * (size_t)b + 2] = nth;
    S.u_lin_next[2 * (size_t)b] = P.v_lin;
    S.u_lin_next[2 * (size_t)b + 1] = has1 ? (double)a1.y : P.fail_u[1];
    if (S.u_applied)
      reinterpret_cast<float2*>(S.u_applied)[b] = has0 ? a0 : make_float2((float)v, (float)delta);
    S.have_path[b] = have;
    S.held_len[b] = len;
    S.held_idx[b] = idx;
    // the planar quaternion a simulator's odometry would carry
    double sh, ch;
    sincos(nth * 0.5, &sh, &ch);
    S.pose_next[4 * (size_t)b] = nx;
    S.pose_next[4 * (size_t)b + 1] = ny;
    S.pose_next[4 * (size_t)b + 2] = sh;
    S.pose_next[4 * (size_t)b + 3] = ch;
    if (S.kind_next) {
      const double* end = S.x_ref + ((size_t)b * S.P + (S.P - 1)) * 3;
      knext = tick_kind(have, nx, ny, have ? end[0] : 0.0, have ? end[1] : 0.0, S.replan_dist);
      S.kind_next[b] = knext;
    }
    if (S.hs_next) {
      float o[6];
      half_space_rows(g, S.nr, nx, ny, nth, S.angle_min, S.angle_inc, o);
#pragma unroll
      for (int j = 0; j < 6; j++) S.hs_next[6 * (size_t)b + j] = o[j];
    }
  }
  if (S.kind_next) append_plan_list(live && knext == TICK_PLAN, b, B, S.next_list, S.next_count);
}

__global__ __launch_bounds__(256) void advance_replan_kernel(const AdvanceParams P, const int B, const int N,
                                                             const ReplanStep S) {
  advance_replan<false>(P, B, N, S);
}

__global__ __launch_bounds__(256) void advance_replan_park_kernel(const AdvanceParams P, const int B, const int N,
                                                                  const ReplanStep S) {
  advance_replan<true>(P, B, N, S);
}

hipError_t launch_advance_replan(const AdvanceParams& P, int B, int N, const ReplanStep& S, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(advance_replan_kernel, dim3((B + 255) / 256), dim3(256), 0, s, P, B, N, S);
  return hipGetLastError();
}

hipError_t launch_advance_replan_park(const AdvanceParams& P, int B, int N, const ReplanStep& S, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(advance_replan_park_kernel, dim3((B + 255) / 256), dim3(256), 0, s, P, B, N, S);
  return hipGetLastError();
}

// In front of the loop: the pose row, kind and plan list of tick 0 and (hs) its half-space rows.
__global__ __launch_bounds__(256) void replan_start_kernel(const int B, const ReplanStart S) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  const bool live = b < B;
  int kind = TICK_MPC;
  if (live) {
    const double px = S.x[3 * (size_t)b], py = S.x[3 * (size_t)b + 1], th = S.x[3 * (size_t)b + 2];
    const int have = S.have_path[b];
    double sh, ch;
    sincos(th * 0.5, &sh, &ch);
    S.pose[4 * (size_t)b] = px;
    S.pose[4 * (size_t)b + 1] = py;
    S.pose[4 * (size_t)b + 2] = sh;
    S.pose[4 * (size_t)b + 3] = ch;
    const double* end = S.x_ref + ((size_t)b * S.P + (S.P - 1)) * 3;
    kind = tick_kind(have, px, py, have ? end[0] : 0.0, have ? end[1] : 0.0, S.replan_dist);
    S.kind[b] = kind;
    if (S.hs) {
      float o[6];
      half_space_rows(S.gap[b], S.nr, px, py, th, S.angle_min, S.angle_inc, o);
#pragma unroll
      for (int j = 0; j < 6; j++) S.hs[6 * (size_t)b + j] = o[j];
    }
  }
  append_plan_list(live && kind == TICK_PLAN, b, B, S.list, S.count);
}

hipError_t launch_replan_start(int B, const ReplanStart& S, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(replan_start_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, S);
  return hipGetLastError();
}

}  // namespace f110qp
