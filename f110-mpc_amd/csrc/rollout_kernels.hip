// rollout_kernels.hip — the plant step of the device-resident closed loop (f110qp_advance_dev,
// f110qp_rollout[_dev] of include/f110qp.h), and the plant step fused with the next tick's
// half-space rows (f110qp_advance_scan_dev, f110qp_rollout_scan[_dev]).
//
// One thread per car: Model::simulate_dynamics (reference src/model.cpp:61-75) on the first input of
// a solve's plan, and the next linearisation input as project::OdomCallback forms it (GetNextInput()
// with v forced, src/project.cpp:169-170,210-218). 56 bytes in and 40 (48 with u_applied) out per
// car, three fp64 trig calls: the launch is the cost, so there is no LDS, no cross-lane traffic and
// no atomic here.
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

}  // namespace f110qp
