// rollout_kernels.hip — the plant step of the device-resident closed loop (f110qp_advance_dev,
// f110qp_rollout[_dev] of include/f110qp.h).
//
// One thread per car: Model::simulate_dynamics (reference src/model.cpp:61-75) on the first input of
// a solve's plan, and the next linearisation input as project::OdomCallback forms it (GetNextInput()
// with v forced, src/project.cpp:169-170,210-218). 56 bytes in and 40 (48 with u_applied) out per
// car, three fp64 trig calls: the launch is the cost, so there is no LDS, no cross-lane traffic and
// no atomic here.
#include <hip/hip_runtime.h>

#include "f110qp_kernels.h"

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

}  // namespace f110qp
