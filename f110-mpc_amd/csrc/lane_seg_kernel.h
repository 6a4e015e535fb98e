// lane_seg_kernel.h — the lane back end for batches that leave lanes over: ONE QP PER S LANES,
// each lane owning one of S horizon segments (a partitioned, parallel-in-time Riccati).
//
// lane_kernel.h solves L <= 64 QPs per wave and, below 64 QPs per wave, runs 64 / L identical
// copies of each QP to keep EXEC full: a QP's time is its serial chain of N backward Riccati
// stages + N forward stages per PDAS pass (mpc.cpp:244-248 block-tridiagonal KKT walked
// strictly in sequence). Here the S = 64 / L lanes of a QP split the horizon into segments
// [s_j, e_j) of m = N / S stages and every pass runs:
//
// 1. backward, all segments at once: the masked Riccati step of lane_kernel.h over the lane's m
//    stages, with the terminal value V_e(x_e) = lam_j' x_e (lam_j: the multiplier of the coupling
//    x_e^(j) = x_s^(j+1), unknown yet; the last segment keeps the true terminal cost, mpc.cpp:228),
//    and alongside it the affine map of the segment's closed loop x_e = Phi x_s + psi + Gam lam_j:
//      W = Phi_{i+1} B,  F_i = -S_i^-1 W'  (the lam-gain of u_i, S_i^-1 the masked inverse),
//      psi_i = W k_i + Phi_{i+1} C + psi_{i+1},  Gam_i = Gam_{i+1} + W F_i,
//      Phi_i = Phi_{i+1} A + W K_i             (Phi_e = I, psi_e = 0, Gam_e = 0).
//    At the segment start V_s(x) = 1/2 x'P_s x + (a_s + Phi' lam_j)' x + const.
// 2. the segment ends: the coupling conditions x_s^(j+1) = Phi_j x_s^(j) + psi_j + Gam_j lam_j and
//    lam_{j-1} = P_j x_s^(j) + a_j + Phi_j' lam_j (x_s^(0) = 0) are an S-stage LQ two-point
//    boundary problem, solved by a Riccati recursion over the segments, lam_{j-1} = M_j x + m_j:
//      T_j = (I - M_{j+1} Gam_j)^-1 M_{j+1} Phi_j,  t_j = (I - M_{j+1} Gam_j)^-1 (M_{j+1} psi_j + m_{j+1}),
//      M_j = P_j + Phi_j' T_j,  m_j = a_j + Phi_j' t_j,   then lam_j = T_j x_s^(j) + t_j forward.
//    (I - M Gam has eigenvalues >= 1: M is positive definite, Gam negative semidefinite.)
//    S <= 4: eliminated from both ends at once. The lower half of the QP's lanes runs the same
//    step on exchanged operands (x_j = alpha_{j-1} + beta_{j-1} lam_{j-1} from x_s^(0) = 0), the
//    two sides meet in the middle in one 3 x 3 vector solve and hand (x_s, lam) outwards again:
//    S / 2 - 1 full steps, the meet and S / 2 - 1 short steps, one instruction stream.
//    S = 8: every lane runs every step on its own data with its neighbour's (M, m) / x_e from a
//    lane shuffle; the top segment's (Phi, psi, Gam) are zeroed so that its lane reproduces (P, a)
//    and hands x_e = 0 to segment 0 round the ring: S - 1 identical steps each way, no selects.
// 3. refresh, all segments: the lam-part of the feed-forward, p^lam_e = lam_j,
//    k_i += -S_i^-1 B' p^lam_{i+1},  p^lam_i = A' p^lam_{i+1} + K_i' B' p^lam_{i+1}
//    (the p-recursion of the Riccati step restricted to its lam-dependent part).
// 4. forward, all segments: lane_kernel.h's sweep from x_s^(j) with the costate
//    P_s x_s + a_s + p^lam_s: rollout, costate carried forward, PDAS re-guess per stage.
// A pass's result equals the sequential pass's up to rounding (tests/diag_segment_riccati_model.py:
// 1.8e-15 relative on random masks), so the PDAS iterates, the single-flip rule (the first
// violation over the whole horizon: a min over the QP's lanes) and the stopping test are
// lane_kernel.h's. Per pass the chain is m stages of ~(200 + 120 + 30) instructions plus the
// segment ends (S = 8: 2 (S - 1) steps; S <= 4: S - 2 and the meet) instead of N stages of ~255.
//
// Layout (fp64 throughout): lane l = S slot + j works on QP L w + slot, segment j (a QP's segments
// are adjacent lanes: its segment-end exchanges stay inside a quad at S <= 4). LDS per wave,
// lane-major so that every access is one conflict-free 64-lane row: references [3m][64] (recentred,
// rotated), PDAS state [m][64] int, Riccati scratch [m][11][64] (K 6, k 2, S^-1 3); the float
// staging of the references borrows the scratch region.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_common.h"
#include "lane_plan.h"

namespace f110qp {

// Diagnostic build only (-DF110QP_STAMPS on lane_seg_inst.hip): per-wave cycles of the setup, each
// pass phase and the output, read back with f110qp_read_seg_stamps() (the macros: stamps.h).
#ifdef F110QP_STAMPS
constexpr int kSegStampSlots = 16;
__device__ unsigned long long g_sstamps[4096 * kSegStampSlots];
#endif

template <int M>
struct SegMode {
  static constexpr int value = M;
};

// Lane-adjacent segments (lane = S slot + segment): the segment ring of a QP is S consecutive lanes,
// so the segment-end exchanges are DPP moves (VALU) instead of ds_bpermute round trips through the
// LDS crossbar: quad permutes at S <= 4, at S = 8 two row shifts and a select (an 8-lane group is
// half a DPP row). A lane only ever reads lanes of its own QP.
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);  // (an invalid source lane reads 0)
}
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)dpp_i<CTRL>((int)(unsigned)b);
  const unsigned hi = (unsigned)dpp_i<CTRL>((int)(unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// the value of segment + 1 (seg_up) / segment - 1 (seg_dn) of the lane's QP, round the QP's ring
template <int S>
__device__ __forceinline__ double seg_up(double v, int lane) {
  static_assert(S == 2 || S == 4 || S == 8, "segments per QP: 2, 4 or 8");
  if constexpr (S == 2) return dpp_d<0xB1>(v);       // quad_perm [1, 0, 3, 2]
  else if constexpr (S == 4) return dpp_d<0x39>(v);  // quad_perm [1, 2, 3, 0]
  else {  // row_shl:1; the top segment's lane takes 0 instead of the ring's wrap: its own
          // (Phi, psi, Gam) are zero in the segment-end recursion, so what it receives only
          // matters as a non-finite value (a neighbouring QP's lane), and 0 is what it computes
          // with anyway (one DPP move and a select per dword instead of two moves and a select)
    const double b = dpp_d<0x101>(v);
    return (lane & 7) == 7 ? 0.0 : b;
  }
}
template <int S>
__device__ __forceinline__ double seg_dn(double v, int lane) {
  if constexpr (S == 2) return dpp_d<0xB1>(v);
  else if constexpr (S == 4) return dpp_d<0x93>(v);  // quad_perm [3, 0, 1, 2]
  else {  // row_shr:1; segment 0 takes 0: the ring hands it the top segment's x_e, which is 0
    const double b = dpp_d<0x111>(v);
    return (lane & 7) == 0 ? 0.0 : b;
  }
}

// the value of the twin sibling's lane (lane ^ S: the other PDAS start of the QP, same segment). At
// S = 4 the sibling is the neighbouring quad of the lane's DPP row: row_shl:4 reads lane + 4,
// row_shr:4 lane - 4, and bit 2 of the lane says which one is the sibling (two VALU moves and a
// select instead of a ds_bpermute round trip); any other S goes through the permute
template <int S>
__device__ __forceinline__ int seg_sib(int v, int lane) {
  if constexpr (S == 4) {
    const int up = dpp_i<0x104>(v), dn = dpp_i<0x114>(v);
    return (lane & 4) ? dn : up;
  } else {
    return __shfl_xor(v, S, 64);
  }
}

#ifndef F110QP_SEG_NEWTON
#define F110QP_SEG_NEWTON 2  // Newton steps after v_rcp_f64 in the masked 2x2 inverse (knob; 1
                             // measured no change: C5 30.2, C2 27.3, C4 shard 63.7 us)
#endif
// unroll factor of the backward stage loop: 2 lets a stage's closed-loop map (Phi, psi, Gam)
// overlap the next stage's Riccati step; same-box A/B C5 30.2 -> 29.6 us, C2 27.4 -> 26.9 at
// S = 4, C4 shard (S = 8, m = 5) 63.6 -> 64.1, so S = 8 keeps 1 (knob F110QP_SEG_BW_UNROLL)
#ifndef F110QP_SEG_BW_UNROLL
#define F110QP_SEG_BW_UNROLL (S <= 4 ? 2 : 1)
#endif
#ifndef F110QP_SEG_WPE
// waves-per-EU hint: 2 (<= 256 VGPRs; the grid still runs one wave per SIMD or CU) schedules
// better than 1: same-box A/B C5 31.2 -> 30.6 us, C2 on the lane back end 28.3 -> 27.7, C4 shard
// neutral (tools/ab_seg_variant.sh)
#define F110QP_SEG_WPE 2
#endif
#ifndef F110QP_SEG_QWPE
#define F110QP_SEG_QWPE 1
#endif
// IN = float or double: the scalar of x0, u_lin and x_ref in global memory (the *_dbl entry points of
// include/f110qp.h). The raw references are staged as IN and every input is widened to fp64 at its
// first use, so past the conversion to recentred references the two instantiations run the same code.
#define F110QP_SEG_KERNEL_ARGS                                                                  \
  const KParams P, const int B, const IN *__restrict__ x0g, const IN *__restrict__ ulg,         \
      const IN *__restrict__ xrg, float *__restrict__ uout, float *__restrict__ xout,           \
      int *__restrict__ status_out, int *__restrict__ iters_out, const WarmState ws, const int kmax, \
      const ObjOut oo
template <int S, bool ROT, bool FST, typename ST = double, bool SCR = false, bool TWIN = false, bool EVEN = false,
          typename IN = float, int Q = 0>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(F110QP_SEG_WPE, F110QP_SEG_WPE))) void lane_seg_kernel(
    F110QP_SEG_KERNEL_ARGS) {
  static_assert(Q == 0, "the fixed-length kernels: lane_seg_kernel_q");
  constexpr const double* ctab = nullptr;  // (read under Q > 0 only)
#include "lane_seg_body.h"
}

// Segments of Q stages, S | N: the heading frame, lam-gains stored, fp64 scratch, no screen. ctab: the
// solver's constant block (kSegBlockBytes, filled by launch_seg_tab_fill).
template <int S, bool TWIN, typename IN, int Q>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(F110QP_SEG_QWPE, F110QP_SEG_QWPE))) void lane_seg_kernel_q(
    F110QP_SEG_KERNEL_ARGS, const double* __restrict__ ctab) {
  static_assert(Q > 0, "a compile-time segment length");
  constexpr bool ROT = true, FST = true, SCR = false, EVEN = true;
  using ST = double;
#include "lane_seg_body.h"
}
#undef F110QP_SEG_KERNEL_ARGS

// The launch of one call: the instance plan names (lane_plan.h: FST, ST, TWIN, EVEN and Q within this
// S, ROT, SCR), its LDS attribute above 64 KiB, the launch.
template <int S, bool ROT, bool SCR, typename IN>
hipError_t launch_lane_seg_t(const KParams& P, const SolveIO<IN>& io, const WarmState& ws, const LaneWork& lw,
                             const LanePlan& plan, const ObjOut& oo, hipStream_t s) {
  // the fixed-length kernels: the same launch with the solver's constant block behind it
  auto goq = [&](auto kern) -> hipError_t {
    if (!lw.seg_tab) return hipErrorInvalidValue;  // (lane_work fills it for every plan with Q > 0)
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(64), plan.lds, s, P, io.B, io.x0, io.u_lin, io.x_ref, io.u_out,
                       io.x_out, io.status, io.iters, ws, lw.kmax, oo, lw.seg_tab);
    return hipGetLastError();
  };
  auto go1 = [&](auto kern) -> hipError_t {
    if (plan.lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(64), plan.lds, s, P, io.B, io.x0, io.u_lin, io.x_ref, io.u_out,
                       io.x_out, io.status, io.iters, ws, lw.kmax, oo);
    return hipGetLastError();
  };
  const bool twin = plan.starts == 2;
  if constexpr (S == 4 && ROT && !SCR) {
    if (plan.Q == 5)
      return twin ? goq(&lane_seg_kernel_q<4, true, IN, 5>) : goq(&lane_seg_kernel_q<4, false, IN, 5>);
  }
#define F110QP_SEG_GO(FST_, ST_, TWIN_)                                                  \
  (plan.even ? go1(&lane_seg_kernel<S, ROT, FST_, ST_, SCR, TWIN_, true, IN>)            \
             : go1(&lane_seg_kernel<S, ROT, FST_, ST_, SCR, TWIN_, false, IN>))
  if (twin) return F110QP_SEG_GO(true, double, true);
  if (plan.mode == 2) return F110QP_SEG_GO(false, float, false);
  return plan.fst ? F110QP_SEG_GO(true, double, false) : F110QP_SEG_GO(false, double, false);
#undef F110QP_SEG_GO
}

}  // namespace f110qp

#ifdef F110QP_STAMPS
extern "C" int f110qp_read_seg_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(f110qp::g_sstamps),
                                  (size_t)n * f110qp::kSegStampSlots * sizeof(unsigned long long));
}
#endif
