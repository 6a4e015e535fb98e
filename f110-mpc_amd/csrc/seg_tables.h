// seg_tables.h — the two active-state code tables of the segmented lane kernel and the flip tolerances
// in them, as the fill of a solver's constant block evaluates them (seg_tab_fill_kernel, lane_launch.hip;
// lane_plan.h: kSegBlockBytes): functions of KParams' bounds, input weights and u_des alone. The
// fixed-length kernels copy the block; the run-time-length kernels keep building the tables in every
// wave from the same expressions written in place (lane_seg_body.h): calling these helpers there
// changed the instruction order of every one of them, and they are the reference the fixed-length
// route is held to bit for bit (tests/test_gpu_seg_fixed_part.py, degenerate and far bounds included),
// which is also what keeps the two copies of the text the same. Every helper is inlined.
#pragma once
#include <hip/hip_runtime.h>

#include "f110qp_kernels.h"
#include "lane_plan.h"

namespace f110qp {

// PDAS flip tolerances (pt: the primal one, gt: the dual one, both scaled): the bounds widened by
// pt (1 + |bound|) and the multiplier threshold gt (1 + r scale)
struct SegTol {
  double lbe0, ube0, lbe1, ube1, gtol0, gtol1;
};
__device__ __forceinline__ SegTol seg_tolerances(double lb0, double ub0, double lb1, double ub1, double r0,
                                                 double r1, double ud0, double ud1, double pt, double gt) {
  SegTol t;
  t.lbe0 = lb0 - pt * (1.0 + fabs(lb0));
  t.ube0 = ub0 + pt * (1.0 + fabs(ub0));
  t.lbe1 = lb1 - pt * (1.0 + fabs(lb1));
  t.ube1 = ub1 + pt * (1.0 + fabs(ub1));
  t.gtol0 = gt * (1.0 + r0 * bound_scale(lb0, ub0, ud0));
  t.gtol1 = gt * (1.0 + r1 * bound_scale(lb1, ub1, ud1));
  return t;
}

// Row c of the two tables. Code c holds input a's state (c >> 2a) & 3 (0 free, 1 lower, 2 upper).
// e = btab[c] = (bA0, bA1, fm0, fm1, 1 - fm0, 1 - fm1, fm0 fm1, 0): the fixed inputs' bound values and
// the free masks of the masked 2 x 2 solve (products with 0 / 1 instead of ~20 selects per backward
// stage; the first four are read a stage ahead). f = ftab[c] (fp64 scratch only, FT): per input
// (lo, hi, fm, 1 - fm), the re-guess tests y = fm u - (1 - fm) g against y < lo (lower) and y > hi
// (upper); free: y = u in (lbe, ube); at the lower bound: y = -g, stays while -g < gtol; at the upper:
// y = -g, stays while -g > -gtol
template <bool FT>
__device__ __forceinline__ void seg_code_rows(int c, double lb0, double ub0, double lb1, double ub1,
                                              const SegTol& t, double* e, double* f) {
  const int cA = c & 3, cB = (c >> 2) & 3;
  const double fA = cA == 0 ? 1.0 : 0.0, fB = cB == 0 ? 1.0 : 0.0;
  e[0] = cA == 0 ? 0.0 : (cA == 1 ? lb0 : ub0);
  e[1] = cB == 0 ? 0.0 : (cB == 1 ? lb1 : ub1);
  e[2] = fA; e[3] = fB; e[4] = 1.0 - fA; e[5] = 1.0 - fB; e[6] = fA * fB; e[7] = 0.0;
  if constexpr (FT) {
    const double inf = __builtin_inf();
    f[0] = cA == 0 ? t.lbe0 : (cA == 1 ? t.gtol0 : -inf); f[1] = cA == 0 ? t.ube0 : (cA == 2 ? -t.gtol0 : inf);
    f[2] = fA; f[3] = 1.0 - fA;
    f[4] = cB == 0 ? t.lbe1 : (cB == 1 ? t.gtol1 : -inf); f[5] = cB == 0 ? t.ube1 : (cB == 2 ? -t.gtol1 : inf);
    f[6] = fB; f[7] = 1.0 - fB;
  }
}

}  // namespace f110qp
