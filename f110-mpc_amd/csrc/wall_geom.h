// wall_geom.h — straight wall segments (include/f110qp.h "straight walls"), written once for the ray cast
// (scan_kernels.hip, rule W1) and the clearance kernel (contact_kernels.hip, rule W2).
//
// A wall is the segment from a to b, without thickness, seen from both sides. All fp64, FP contraction off in
// every function (no fused multiply-add), the correctly rounded square root and division; the expression order
// here is the specification's and workload.ray_segments / workload.segment_body repeat it. min and max below
// are fmin and fmax: of a NaN and a number they give the number.
#pragma once
#include <hip/hip_runtime.h>

#include "body_geom.h"
#include "f110qp_kernels.h"  // BodyParams

namespace f110qp {

// Rule W1. The beam from the LiDAR along (dx, dy) against the segment whose ends are A = a - o and B = b - o
// from the LiDAR: ca and cb are the ends' sides of the beam's line, ta and tb their distances along it. A hit
// when the ends straddle the line (a zero counts for either side, so two segments that share a vertex's bits
// cannot both miss a beam that passes between their outer ends), den != 0 and th > 0. Any NaN fails a compare.
#pragma clang fp contract(off)
__device__ __forceinline__ bool wall_hit(const double ax, const double ay, const double bx, const double by,
                                         const double dx, const double dy, double& th) {
  const double ca = dx * ay - dy * ax;
  const double cb = dx * by - dy * bx;
  const double ta = ax * dx + ay * dy;
  const double tb = bx * dx + by * dy;
  const double den = ca - cb;
  if (!((ca <= 0.0 && cb >= 0.0) || (ca >= 0.0 && cb <= 0.0)) || !(den != 0.0)) return false;
  th = ta + (tb - ta) * (ca / den);
  return th > 0.0;
}

// Rule 1 from au on, in the body's own frame: the signed distance of the point (u, w).
#pragma clang fp contract(off)
__device__ __forceinline__ double wall_sd(const double u, const double w, const BodyParams& H) {
  const double au = fabs(u) - H.hl, aw = fabs(w) - H.hw;
  if (au <= 0.0 && aw <= 0.0) return fmax(au, aw);
  const double ex = au < 0.0 ? 0.0 : au, ey = aw < 0.0 ? 0.0 : aw;
  return __dsqrt_rn(ex * ex + ey * ey);
}

// The distance of the corner (cx, cy) to the segment from (ua, wa) along (ex, ey), ee = e.e.
#pragma clang fp contract(off)
__device__ __forceinline__ double wall_corner(const double cx, const double cy, const double ua, const double wa,
                                              const double ex, const double ey, const double ee) {
  const double gx = cx - ua, gy = cy - wa;
  double s = (gx * ex + gy * ey) / ee;
  s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
  if (ee == 0.0) s = 0.0;
  const double rx = gx - s * ex, ry = gy - s * ey;
  return __dsqrt_rn(rx * rx + ry * ry);
}

// Rule W2. The body (qx, qy, c, s) against the segment from (ax, ay) to (bx, by): both ends into the body's
// frame (rule 1's u and w), the slab test of rule 5 along the segment with the window [0, 1], then the least
// signed distance of the ends capped at 0 (crossing or touching) or at the least corner distance (apart).
// ee NaN or +inf (a NaN or infinite field or pose): +inf, which no compare takes.
#pragma clang fp contract(off)
__device__ __forceinline__ double wall_body(const double ax, const double ay, const double bx, const double by,
                                            const double qx, const double qy, const double c, const double s,
                                            const BodyParams& H) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double dax = ax - qx, day = ay - qy, dbx = bx - qx, dby = by - qy;
  const double ua = dax * c + day * s, wa = day * c - dax * s;
  const double ub = dbx * c + dby * s, wb = dby * c - dbx * s;
  const double ex = ub - ua, ey = wb - wa;
  const double ee = ex * ex + ey * ey;
  if (!(ee < inf)) return inf;
  double lo_f, hi_f, lo_l, hi_l;
  body_slab_axis(ua, ex, H.hl, lo_f, hi_f);
  body_slab_axis(wa, ey, H.hw, lo_l, hi_l);
  const double m = fmin(wall_sd(ua, wa, H), wall_sd(ub, wb, H));
  if (fmax(fmax(lo_f, lo_l), 0.0) <= fmin(fmin(hi_f, hi_l), 1.0)) return fmin(m, 0.0);
  const double k0 = wall_corner(H.hl, H.hw, ua, wa, ex, ey, ee);
  const double k1 = wall_corner(H.hl, -H.hw, ua, wa, ex, ey, ee);
  const double k2 = wall_corner(-H.hl, H.hw, ua, wa, ex, ey, ee);
  const double k3 = wall_corner(-H.hl, -H.hw, ua, wa, ex, ey, ee);
  return fmin(m, fmin(fmin(k0, k1), fmin(k2, k3)));
}

}  // namespace f110qp
