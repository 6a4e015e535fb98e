// halfspace_geom.h — the pose-dependent half of Constraints::FindHalfSpaces (reference
// src/constraints.cpp:179-264) for one car on one thread.
//
// FindHalfSpaces is a gap search that reads only the scan (:118-177: window, threshold, first
// longest run, buffer inflation) followed by an end-point geometry that reads the pose (:179-264).
// The search (halfspace_kernels.hip, one wave per scan) leaves one GapRecord per scan; this function
// maps a record and an fp64 pose to the six floats of the ABI's half-space layout. It is the wave
// kernel's tail written for one thread (that tail evaluates the two sincos on an even and an odd lane
// and stays as it is): the same float / double types in the same order, sincos(double), no fused
// multiply-add, so the two are bit-equal on the device (tests/test_gpu_rollout_scan.py).
#pragma once
#include <hip/hip_runtime.h>

namespace f110qp {

// What the gap search keeps of a scan (16 bytes): (lo, hi) after the buffer inflation, exactly the
// wave kernel's gap_lo / gap_hi (-1 and out-of-range values included), and ranges[lo], ranges[hi]
// (NaN where lo or hi is no beam of the scan: the reference reads ranges[-1] there).
struct GapRecord {
  int lo, hi;
  float r_lo, r_hi;
};

// hs[0..5] = (a1, b1, c1 + 0.5, a2, b2, c2 + 0.5); six NaNs for a record without a gap
// (lo or hi outside [0, nr)).
__device__ __forceinline__ void half_space_rows(const GapRecord g, const int nr, const double poseX,
                                                const double poseY, const double ori,
                                                const float angle_min, const float angle_inc,
                                                float* __restrict__ o) {
#pragma clang fp contract(off)
  if (g.lo < 0 || g.hi < 0 || g.lo >= nr || g.hi >= nr) {
    const float nanv = __int_as_float(0x7fc00000);
    for (int j = 0; j < 6; j++) o[j] = nanv;
    return;
  }
  const float cur = (float)ori;  // float current_angle = state.ori()
  const float ang1 = angle_min + (float)g.lo * angle_inc + cur;  // :179-180
  const float ang2 = angle_min + (float)g.hi * angle_inc + cur;
  double s1, c1d, s2, c2d;
  sincos((double)ang1, &s1, &c1d);
  sincos((double)ang2, &s2, &c2d);
  const float p1x = (float)((double)g.r_lo * c1d + poseX);  // :181-185
  const float p1y = (float)((double)g.r_lo * s1 + poseY);
  const float p2x = (float)((double)g.r_hi * c2d + poseX);
  const float p2y = (float)((double)g.r_hi * s2 + poseY);
  const float px = (float)poseX, py = (float)poseY;
  float a1 = py - p1y, b1 = p1x - px;  // :233-253
  float c1 = px * p1y - py * p1x;
  if (a1 * p2x + b1 * p2y + c1 < 0.f) {
    a1 = -a1; b1 = -b1; c1 = -c1;
  }
  float a2 = py - p2y, b2 = p2x - px;
  float c2 = px * p2y - py * p2x;
  if (a2 * p1x + b2 * p1y + c2 < 0.f) {
    a2 = -a2; b2 = -b2; c2 = -c2;
  }
  o[0] = a1; o[1] = b1; o[2] = (float)((double)c1 + 0.5);  // :255-264
  o[3] = a2; o[4] = b2; o[5] = (float)((double)c2 + 0.5);
}

}  // namespace f110qp
