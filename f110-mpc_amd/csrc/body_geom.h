// body_geom.h — the rectangular car body (include/f110qp.h "rectangular car bodies"), written once for the
// clearance kernel (contact_kernels.hip) and the ray cast (scan_kernels.hip).
//
// A body is the rectangle with centre q, axes f = (c, s) and l = (-s, c) and half extents (hl, hw). All fp64,
// FP contraction off in every function (no fused multiply-add), the correctly rounded square root; the
// expression order here is the specification's and workload.clearance_body / workload.ray_bodies repeat it.
// min and max below are fmin and fmax: of a NaN and a number they give the number. Where a NaN has to survive
// (body_sd's ex, ey) the select is written out.
#pragma once
#include <hip/hip_runtime.h>

#include "f110qp_kernels.h"  // BodyParams

namespace f110qp {

// Signed distance of the point (px, py) to the body (qx, qy, c, s): negative inside.
//   d = p - q, u = d.f, w = d.l, au = |u| - hl, aw = |w| - hw
//   au <= 0 and aw <= 0: max(au, aw); else sqrt(ex ex + ey ey), ex = au < 0 ? 0 : au, ey likewise
// A NaN au or aw fails the first test and stays in ex or ey: a NaN in gives a NaN out.
#pragma clang fp contract(off)
__device__ __forceinline__ double body_sd(const double px, const double py, const double qx, const double qy,
                                          const double c, const double s, const BodyParams& H) {
  const double dx = px - qx, dy = py - qy;
  const double u = dx * c + dy * s;
  const double w = dy * c - dx * s;
  const double au = fabs(u) - H.hl, aw = fabs(w) - H.hw;
  if (au <= 0.0 && aw <= 0.0) return fmax(au, aw);
  const double ex = au < 0.0 ? 0.0 : au, ey = aw < 0.0 ? 0.0 : aw;
  return __dsqrt_rn(ex * ex + ey * ey);
}

// The least body_sd of the four corners q ± hl f ± hw l of body A against body B.
#pragma clang fp contract(off)
__device__ __forceinline__ double body_corner_min(const double ax, const double ay, const double ac, const double as,
                                                  const double bx, const double by, const double bc, const double bs,
                                                  const BodyParams& H) {
  const double fx = H.hl * ac, fy = H.hl * as;  // hl f
  const double lx = H.hw * as, ly = H.hw * ac;  // hw l = (-lx, ly)
  const double v0 = body_sd((ax + fx) - lx, (ay + fy) + ly, bx, by, bc, bs, H);
  const double v1 = body_sd((ax + fx) + lx, (ay + fy) - ly, bx, by, bc, bs, H);
  const double v2 = body_sd((ax - fx) - lx, (ay - fy) + ly, bx, by, bc, bs, H);
  const double v3 = body_sd((ax - fx) + lx, (ay - fy) - ly, bx, by, bc, bs, H);
  return fmin(fmin(v0, v1), fmin(v2, v3));
}

// Body b against body m: the largest separating-axis gap g over f_b, l_b, f_m, l_m when g <= 0 (overlap: -g
// is the penetration depth), otherwise the least of the eight corner distances (the exact distance of two
// disjoint rectangles). With d = q_m - q_b, cc = f_b.f_m = l_b.l_m and cr = l_m.f_b = -(l_b.f_m):
//   gap on f_x = (|d.f_x| - hl) - (hl |cc| + hw |cr|),  gap on l_x = (|d.l_x| - hw) - (hl |cr| + hw |cc|)
// Swapping b and m negates d and cr exactly and leaves cc's two products and their sum as they are, so the
// four gaps are the same four numbers; the corner terms are body_corner_min(m, b) and (b, m), whose minimum
// does not see the order either: the value is the same bits in both directions.
#pragma clang fp contract(off)
__device__ __forceinline__ double body_pair(const double bx, const double by, const double bc, const double bs,
                                            const double mx, const double my, const double mc, const double ms,
                                            const BodyParams& H) {
  const double dx = mx - bx, dy = my - by;
  const double cc = fabs(bc * mc + bs * ms);
  const double cr = fabs(mc * bs - ms * bc);
  const double el = H.hl * cc + H.hw * cr;  // the other body's extent on an f axis
  const double ew = H.hl * cr + H.hw * cc;  // and on an l axis
  const double gfb = (fabs(dx * bc + dy * bs) - H.hl) - el;
  const double glb = (fabs(dy * bc - dx * bs) - H.hw) - ew;
  const double gfm = (fabs(dx * mc + dy * ms) - H.hl) - el;
  const double glm = (fabs(dy * mc - dx * ms) - H.hw) - ew;
  const double g = fmax(fmax(gfb, gfm), fmax(glb, glm));
  if (g <= 0.0) return g;
  return fmin(body_corner_min(mx, my, mc, ms, bx, by, bc, bs, H), body_corner_min(bx, by, bc, bs, mx, my, mc, ms, H));
}

// One axis of the slab test: the beam o' + t d' is within [-h, h] for t in [lo, hi]. d' == 0: every t when
// |o'| <= h, none otherwise (lo = +inf, hi = -inf); no 0 / 0 arises.
#pragma clang fp contract(off)
__device__ __forceinline__ void body_slab_axis(const double o, const double d, const double h, double& lo,
                                               double& hi) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  if (d != 0.0) {
    const double t1 = (-h - o) / d, t2 = (h - o) / d;
    lo = fmin(t1, t2);
    hi = fmax(t1, t2);
  } else if (fabs(o) <= h) {
    lo = -inf;
    hi = inf;
  } else {
    lo = inf;
    hi = -inf;
  }
}

// A beam from the LiDAR along (dx, dy) against the body whose centre is p = q_m - o from the LiDAR and whose
// axes are (c, s): o' = (-p.f, -p.l) = (of, ol), d' = (d.f, d.l). Returns the entry parameter th and whether
// it counts: th <= the least exit and th > 0 (a LiDAR inside the body sees through it).
#pragma clang fp contract(off)
__device__ __forceinline__ bool body_slab(const double of, const double ol, const double c, const double s,
                                          const double dx, const double dy, const BodyParams& H, double& th) {
  double lo_f, hi_f, lo_l, hi_l;
  body_slab_axis(of, dx * c + dy * s, H.hl, lo_f, hi_f);
  body_slab_axis(ol, dy * c - dx * s, H.hw, lo_l, hi_l);
  th = fmax(lo_f, lo_l);
  return th <= fmin(hi_f, hi_l) && th > 0.0;
}

}  // namespace f110qp
