// lane_launch.hip — the lane back end's launch: from the plan of a call (lane_plan.h, where the policy
// lives) to the instantiation of lane_kernel.h (lane_inst.hip) or lane_seg_kernel.h
// (lane_seg_inst.hip) it names. With F110QP_LANE_ALL (the -DF110QP_STAMPS diagnostic build) this one
// file instantiates every variant of lane_kernel.h itself.
#ifdef F110QP_LANE_ALL
#include "lane_kernel.h"
#else
#include <hip/hip_runtime.h>

#include "lane_plan.h"
#endif
#include "seg_tables.h"

namespace f110qp {

// IN below: the input scalar of x0 / u_lin / x_ref, float or double (the *_dbl entry points). The
// plan does not depend on it.
template <int S, bool ROT, bool SCR, typename IN>
hipError_t launch_lane_seg_t(const KParams& P, const SolveIO<IN>& io, const WarmState& ws, const LaneWork& lw,
                             const LanePlan& plan, const ObjOut& oo, hipStream_t s);  // lane_seg_inst.hip
#ifndef F110QP_LANE_ALL
template <typename ST, bool SLDS, int L, bool ROT, bool DREF, typename IN>
hipError_t launch_lane_t(const KParams& P, const SolveIO<IN>& io, const WarmState& ws, const LaneWork& lw,
                         const LanePlan& plan, const ObjOut& oo, hipStream_t s);  // lane_inst.hip
#endif

template <typename IN>
hipError_t launch_lane(const KParams& P, const SolveIO<IN>& io, const WarmState& ws, const LaneWork& lw,
                       const LanePlan& plan, const ObjOut& oo, hipStream_t s) {
  using Fn = hipError_t (*)(const KParams&, const SolveIO<IN>&, const WarmState&, const LaneWork&,
                            const LanePlan&, const ObjOut&, hipStream_t);
  if (plan.S > 1) {
    // segmented: [S = 2, 4, 8][ROT][SCR]; the instance picks FST, ST, TWIN, EVEN and Q itself
#define F110QP_SEG_ROW(S)                                                                      \
  {{&launch_lane_seg_t<S, false, false, IN>, &launch_lane_seg_t<S, false, true, IN>},         \
   {&launch_lane_seg_t<S, true, false, IN>, &launch_lane_seg_t<S, true, true, IN>}}
    static const Fn seg[3][2][2] = {F110QP_SEG_ROW(2), F110QP_SEG_ROW(4), F110QP_SEG_ROW(8)};
#undef F110QP_SEG_ROW
    return seg[plan.S == 2 ? 0 : plan.S == 4 ? 1 : 2][plan.rot][plan.scr](P, io, ws, lw, plan, oo, s);
  }
  // sequential: [scratch mode 1 .. 4 = (ST, SLDS)][log2 L][ROT][DREF]
#define F110QP_LANE_ROW(ST, SLDS, L)                                                           \
  {{&launch_lane_t<ST, SLDS, L, false, false, IN>, &launch_lane_t<ST, SLDS, L, false, true, IN>}, \
   {&launch_lane_t<ST, SLDS, L, true, false, IN>, &launch_lane_t<ST, SLDS, L, true, true, IN>}}
#define F110QP_LANE_MODE(ST, SLDS)                                                             \
  {F110QP_LANE_ROW(ST, SLDS, 1), F110QP_LANE_ROW(ST, SLDS, 2), F110QP_LANE_ROW(ST, SLDS, 4),   \
   F110QP_LANE_ROW(ST, SLDS, 8), F110QP_LANE_ROW(ST, SLDS, 16), F110QP_LANE_ROW(ST, SLDS, 32), \
   F110QP_LANE_ROW(ST, SLDS, 64)}
  static const Fn seq[4][7][2][2] = {F110QP_LANE_MODE(double, true), F110QP_LANE_MODE(float, true),
                                     F110QP_LANE_MODE(double, false), F110QP_LANE_MODE(float, false)};
#undef F110QP_LANE_MODE
#undef F110QP_LANE_ROW
  return seq[plan.mode - 1][__builtin_ctz(plan.qpw)][plan.rot][plan.dref](P, io, ws, lw, plan, oo, s);
}
template hipError_t launch_lane<float>(const KParams&, const SolveIO<float>&, const WarmState&, const LaneWork&,
                                       const LanePlan&, const ObjOut&, hipStream_t);
template hipError_t launch_lane<double>(const KParams&, const SolveIO<double>&, const WarmState&, const LaneWork&,
                                        const LanePlan&, const ObjOut&, hipStream_t);


// The solver's constant block (lane_plan.h): lanes 0 .. 15 write one code's rows of the two tables each,
// by the expressions of the kernels that build theirs in LDS (fp64 scratch: 1e-10 scaled, both pass kinds).
__global__ __launch_bounds__(64) void seg_tab_fill_kernel(const KParams P, double* __restrict__ tab) {
  const int lane = threadIdx.x;
  const double lb0 = (double)P.umin[0], lb1 = (double)P.umin[1];
  const double ub0 = (double)P.umax[0], ub1 = (double)P.umax[1];
  const SegTol t = seg_tolerances(lb0, ub0, lb1, ub1, P.r[0], P.r[1], P.udes[0], P.udes[1], 1e-10, 1e-10);
  if (lane < 16) seg_code_rows<true>(lane, lb0, ub0, lb1, ub1, t, tab + 8 * lane, tab + 16 * 8 + 8 * lane);
}

hipError_t launch_seg_tab_fill(const KParams& P, double* tab, hipStream_t s) {
  hipLaunchKernelGGL(seg_tab_fill_kernel, dim3(1), dim3(64), 0, s, P, tab);
  return hipGetLastError();
}

}  // namespace f110qp
