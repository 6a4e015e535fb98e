// solve_inst.hip — explicit instantiations of the solve kernel (solve_kernel.h).
//
// The Makefile compiles this file once per (NUM, GAP) pair (-DF110QP_NUM=.. -DF110QP_GAP=..)
// and once more per pair for the double-input kernels, so the instantiations build in parallel; the diagnostic stamps build compiles it once with
// -DF110QP_ALL_INST (the per-wave stamp buffer must live in a single translation unit).
#include "solve_kernel.h"

// F110QP_IN: the input scalar of x0 / u_lin / x_ref (float; double in the *_dbl objects, which the
// Makefile builds from this file with -DF110QP_IN=double). F110QP_ALL_INST instantiates both.
#ifndef F110QP_IN
#define F110QP_IN float
#endif
#define F110QP_INSTANTIATE_IN(NUM, GAP, IN)                                                    \
  template hipError_t f110qp::launch_t<NUM, GAP, IN>(const KParams&, const SolveIO<IN>&, double*, double*, \
                                                     const WarmState&, const int*, const int*,            \
                                                     const ObjOut&, hipStream_t);                         \
  template hipError_t f110qp::launch_prep_t<NUM, GAP, IN>(const KParams&, const SolveIO<IN>&,             \
                                                          const WarmState&, const int*, hipStream_t);
#ifdef F110QP_ALL_INST
#define F110QP_INSTANTIATE(NUM, GAP) F110QP_INSTANTIATE_IN(NUM, GAP, float) F110QP_INSTANTIATE_IN(NUM, GAP, double)
#else
#define F110QP_INSTANTIATE(NUM, GAP) F110QP_INSTANTIATE_IN(NUM, GAP, F110QP_IN)
#endif

#ifdef F110QP_ALL_INST
#define F110QP_BOTH(NUM) F110QP_INSTANTIATE(NUM, false) F110QP_INSTANTIATE(NUM, true)
F110QP_BOTH(8) F110QP_BOTH(16) F110QP_BOTH(24) F110QP_BOTH(32) F110QP_BOTH(40)
F110QP_BOTH(48) F110QP_BOTH(56) F110QP_BOTH(64) F110QP_BOTH(80) F110QP_BOTH(96)
#else
F110QP_INSTANTIATE(F110QP_NUM, F110QP_GAP)
#endif

#ifdef F110QP_STAMPS
extern "C" int f110qp_read_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(f110qp::g_stamps),
                                  (size_t)n * f110qp::kStampSlots * sizeof(unsigned long long));
}
#endif
