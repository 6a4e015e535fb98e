// linearize.h — Model::Linearize on the device, fp64 (reference src/model.cpp:30-59; L = 0.3302f
// at :32; dt is the float MPC::dt_). linearize(): the wave kernel (solve_kernel.h) and the
// assembly-parity hook (assemble_kernel.hip). lane_linearize(): the per-lane form of the lane kernels
// (lane_kernel.h, lane_seg_kernel.h), recentred on theta0 and, ROT, in the heading frame.
#pragma once
#include <hip/hip_runtime.h>

namespace f110qp {

constexpr float kWheelbase = 0.3302f;  // model.cpp:32

struct Lin {
  double th0, a02, a12, b00, b10, b20, b21, c0, c1, c2;
};

__device__ __forceinline__ Lin linearize(double th, double v, double d, float dtf) {
  const double dt = (double)dtf;
  const double L = (double)kWheelbase;
  double sn, cs, sd, cd;
  sincos(th, &sn, &cs);
  sincos(d, &sd, &cd);
  const double sec2 = 1.0 / (cd * cd);  // pow(cos(d), -2)
  Lin M;
  M.th0 = th;
  M.a02 = -1 * v * sn * dt;           // :42
  M.a12 = v * cs * dt;                // :43
  M.b00 = cs * dt;                    // :48
  M.b10 = sn * dt;                    // :49
  M.b20 = (sd / cd) * dt / L;         // :50 tan(d)
  M.b21 = v * sec2 * dt / L;          // :51
  M.c0 = v * th * sn * dt;            // :53
  M.c1 = -1 * v * th * cs * dt;       // :54
  M.c2 = -1 * d * v * sec2 * dt / L;  // :55
  return M;
}

// The lane kernels' model of one QP, with sin / cos of theta0 for the frame changes.
// ROT (q0 == q1, the shipped params.yaml:1-2): the (x, y) offsets are expressed in the frame of the
// heading th0, s = cs dx + sn dy, n = cs dy - sn dx. Q = diag(q0, q0, q2) is invariant under that
// rotation and A = I + E, B become A = I + (v dt) e_n e_th', B = [dt 0; 0 0; b20 b21] (the rotated
// model.cpp:42-51 with cs^2 + sn^2 = 1): four zero entries that drop ~20 fp64 operations of the
// backward Riccati stage and ~6 of the forward one.
// The state is recentred on x0 = (X0, Y0, th0): translation invariance in (x, y) and, for the
// heading, x_{i+1} = x_i + a02 th_i + ... + c0 = x_i + a02 (th_i - th0) + ... + (c0 + a02 th0).
// c0 + a02 th0 is zero up to rounding (model.cpp:42,53); keeping it as computed stays exact.
// (In the rotated frame both are exactly zero in exact arithmetic and dropped.)
struct LaneModel {
  double a02, a12, b00, b10, b20, b21, c0, c1, c2, sn, cs;
};

template <bool ROT>
__device__ __forceinline__ LaneModel lane_linearize(double th0, double v, double d, double dt) {
  const double Lw = (double)kWheelbase;
  LaneModel M;
  double sd, cd;
  sincos(th0, &M.sn, &M.cs);
  sincos(d, &sd, &cd);
  const double sn = M.sn, cs = M.cs, sec2 = 1.0 / (cd * cd);
  M.a02 = ROT ? 0.0 : -1 * v * sn * dt;                              // :42
  M.a12 = ROT ? v * dt : v * cs * dt;                                // :43
  M.b00 = ROT ? dt : cs * dt, M.b10 = ROT ? 0.0 : sn * dt;           // :48-49
  M.b20 = (sd / cd) * dt / Lw, M.b21 = v * sec2 * dt / Lw;           // :50-51
  const double c0r = v * th0 * sn * dt, c1r = -1 * v * th0 * cs * dt;  // :53-54
  M.c2 = -1 * d * v * sec2 * dt / Lw;                                // :55
  M.c0 = ROT ? 0.0 : c0r + M.a02 * th0, M.c1 = ROT ? 0.0 : c1r + M.a12 * th0;
  return M;
}

}  // namespace f110qp
