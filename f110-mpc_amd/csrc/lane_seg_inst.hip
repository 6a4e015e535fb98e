// lane_seg_inst.hip — instantiations of the segmented lane kernel (lane_seg_kernel.h): S = 2, 4, 8
// horizon segments per QP (64 / S QPs per wave), heading frame and general frame. Compiled twice
// (Makefile): F110QP_SEG_SCR = 0 the box-only kernels, 1 the variants with the gap-row screen in
// the output sweep (f110qp_kernels.hip), as two objects that build in parallel; F110QP_SEG_ALL
// (the stamps build) instantiates both here.
#include "lane_seg_kernel.h"

#ifndef F110QP_SEG_SCR
#define F110QP_SEG_SCR 0
#endif

namespace f110qp {
// F110QP_IN: the input scalar of x0 / u_lin / x_ref (float; double in the *_dbl objects)
#ifndef F110QP_IN
#define F110QP_IN float
#endif
#define F110QP_SEG_INST_IN(S, ROT, SCR, IN)                                                          \
  template hipError_t launch_lane_seg_t<S, ROT, SCR, IN>(const KParams&, const SolveIO<IN>&, const WarmState&, \
                                                         const LaneWork&, const LanePlan&, const ObjOut&,       \
                                                         hipStream_t);
#ifdef F110QP_SEG_ALL
#define F110QP_SEG_INST(S, ROT, SCR) F110QP_SEG_INST_IN(S, ROT, SCR, float) F110QP_SEG_INST_IN(S, ROT, SCR, double)
#else
#define F110QP_SEG_INST(S, ROT, SCR) F110QP_SEG_INST_IN(S, ROT, SCR, F110QP_IN)
#endif
#define F110QP_SEG_INST_ALL(SCR) \
  F110QP_SEG_INST(2, true, SCR)  \
  F110QP_SEG_INST(2, false, SCR) \
  F110QP_SEG_INST(4, true, SCR)  \
  F110QP_SEG_INST(4, false, SCR) \
  F110QP_SEG_INST(8, true, SCR)  \
  F110QP_SEG_INST(8, false, SCR)
#if defined(F110QP_SEG_ALL) || F110QP_SEG_SCR == 0
F110QP_SEG_INST_ALL(false)
#endif
#if defined(F110QP_SEG_ALL) || F110QP_SEG_SCR == 1
F110QP_SEG_INST_ALL(true)
#endif
#undef F110QP_SEG_INST_ALL
#undef F110QP_SEG_INST
}  // namespace f110qp
