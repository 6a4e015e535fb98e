// lane_common.h — what the two lane kernels (lane_kernel.h, lane_seg_kernel.h) share: the per-lane
// model (lane_linearize, linearize.h), the stamp macros of the diagnostic build (stamps.h) and the
// stage's state code below. Every helper is inlined; the kernels' instruction streams are those of
// the code written out in place.
#pragma once
#include <hip/hip_runtime.h>

#include "linearize.h"
#include "stamps.h"

namespace f110qp {

// A stage's 4-bit state code (2 bits per input: 0 free, 1 lower bound, 2 upper bound) from the low
// two bits of the warm masks' lower and upper words (bit a: input a; the lower bound wins)
__device__ __forceinline__ unsigned pdas_code(unsigned lw, unsigned hw) {
  const unsigned l2 = lw & 3u, h2 = hw & 3u & ~l2;
  return (l2 & 1u) | ((h2 & 1u) << 1) | ((l2 & 2u) << 1) | ((h2 & 2u) << 2);
}

}  // namespace f110qp
