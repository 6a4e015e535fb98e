// scan_kernels.hip — the simulated LiDAR of the closed loop: 2-D ray casting against circles.
//
// The project's world model (f110qp/workload.py, _ray_circles: every scan of make_scenes, drive_stream,
// the tests and bench.py) on the device, so that a rollout can take tick t's scan at tick t's pose.
// Per car: the LiDAR origin o = (x + off cos(ori), y + off sin(ori)) (occupancy_grid.cpp:63-64), beam
// i along ori + ((double)angle_min + (double)angle_increment i), and per circle (c, r)
//   p = c - o, t = p.d, d2 = p.p - t t, hit: d2 <= r^2 && t > 0, th = t - sqrt(max(r^2 - d2, 0)),
// which counts when th > 0; range = (float)min(min over circles of th, max_range). All fp64 in the
// numpy expression order with FP contraction off, sincos(double) and the correctly rounded sqrt: per
// (beam, circle) pair the value is fixed by the beam's direction, so the minimum does not depend on
// the order the circles are visited in (or on which thread visits them).
//
// Mapping: one 256-thread workgroup per car, striding over the cars (all B, or a device-side list as
// plan_listed_kernel). Brute force is C x R pair tests per car; here the work is circle-parallel
// behind a cull. Per beam tile (kCastBeamTile beams: their directions and running minima in LDS) and
// per circle tile (kCastCircleTile circles, one per thread):
//   A  thread j reads circle j, drops it when |p| - |r| is past max_range (a NaN or inf field fails or
//      passes that compare like any other number: no branch looks for it), and turns it into a beam
//      interval: the circle subtends atan2(p) -+ asin(|r| / |p|), a beam can hit it only inside that
//      arc, so the beams are floor(f_lo) - 1 .. floor(f_lo) + ceil(2w / inc) + 2 with f_lo the arc's
//      low edge in beam units: at least one beam more than the arc at either end, repeated every
//      2 pi / inc beams for a scan that wraps. The LiDAR inside (or on) a circle, an arc that with its
//      margin closes the turn, or an increment too small for the margin: every beam. The low edge
//      atan2(p) - ori - angle_min - w carries a few ulp(|ori| + |angle_min| + pi) of rounding against
//      that one-beam margin: the interval is safe while this ulp is far below one increment. For the
//      1,080-beam scan (5.8e-3 rad a beam) it reaches a thousandth of a beam at |ori| ~ 2.6e10 rad
//      (1.2e-10 rad at 1e6 rad), where the beam directions ori + angle are quantised just as coarsely.
//   B  eight lanes per kept circle run the exact test above on its beams only and fold th into the
//      beam's minimum with an unsigned 64-bit LDS atomic min (positive doubles order as their bits).
// A beam outside an interval cannot hit, one inside is decided by the exact test, so the interval
// changes the work and not the result.
//
// Races (RACE, cast_scans_race_kernel): the B cars are B / G races of G consecutive cars, and car b also
// sees each race-mate m as the circle (x_m + off cos(ori_m), y_m + off sin(ori_m), car_radius), the
// LiDAR origin's own expressions. The mates are a virtual tail of the circle list: index j in
// [C, C + G - 1) is mate k = j - C of the race, stepped over the car's own slot, built by the thread
// that takes j in phase A with one sincos; from there on it is a circle like any other (the same
// cull, inside test, interval and phase B), so what holds per circle holds per opponent: a non-finite
// pose fails the range compare and hits nothing, and the minimum is the same for every order of the
// race's cars. The tile loop runs to C + G - 1: no cap on G. The plain kernel is the RACE = false
// instantiation; every race statement is behind `if constexpr`.
//
// Walls (WALLS, cast_scans_walls_kernel): the body cast with S straight segments (wall_geom.h, rule W1)
// as a third stretch of the list, index j in [C + G - 1, C + G - 1 + S). Phase A culls a segment by its
// distance from the LiDAR and gives it the beams of the arc between atan2(A) and atan2(B) the short way, with
// the circle path's margin and wrap rule; an arc that is not safely below pi (the LiDAR on or next to the
// segment), or an increment below the margin threshold: every beam. A beam outside the arc cannot meet the
// segment at th > 0, so here too the interval changes the work and not the result. Every wall statement is
// behind `if constexpr`.
//
// Noise (NOISE, cast_scans_noisy_kernel): the walls cast with rules Z1 and Z2 of include/f110qp.h in the loop
// that converts a tile's minima to float and stores them: a counter-based hash of (seed, car, tick, beam), a
// dropout draw and a bounded bell curve from four 16-bit fields, integers up to the one fp64 expression of
// Z2. The car's and the tick's keys are folded once per car (uniform over the workgroup); a beam costs two
// mixes. No LDS, no launch and no pass over HBM is added. Every noise statement is behind `if constexpr`.
//
// A raster map (GRID, cast_scans_grid_kernel): the noisy cast with rule G1 of include/f110qp.h (grid_geom.h)
// between the last obstacle tile and the store loop of every beam tile. Once per car the workgroup packs the
// square of cells its beams can reach (max_range to every side of the LiDAR's cell) into LDS, one bit a cell;
// then thread i walks beams i, i + 256, ... cell by cell, reading bits from LDS, up to the minimum the beam
// already holds (the parameter only grows along a walk, so a hit behind that minimum cannot count), and folds
// its hit into the minimum with a plain store: a beam has one walker. A square that does not fit
// kGridWinWords is not packed and the walk reads the map's bytes from global memory (L2): the same walk, the
// same bits. No launch is added. Every grid statement is behind `if constexpr`.
//
// The map through its field (FIELD, grid_cast_kernel): the grid cast with rule F1 in place of rule G1. A beam's
// walker reads d2 where it stands and jumps isqrt(d2 - 1) cells, no cell of which can be occupied, so its cost
// follows the free space and not the beam's length. The cells are d2's ints from global memory (L2): no square is
// packed and the 21 KB of LDS come back. Beams of a wave jump different lengths; the loop runs until the last is
// done. Every field statement is behind `if constexpr`.
#include <hip/hip_runtime.h>

#include "body_geom.h"
#include "f110qp_kernels.h"
#include "grid_geom.h"
#include "wall_geom.h"

namespace f110qp {

namespace {

constexpr int kCastThreads = 256;
constexpr int kCastBeamTile = 1152;  // beams per LDS tile (a 1,080-beam scan is one tile)
constexpr int kCastLanes = 8;        // lanes that share one circle's interval
constexpr int kCastGroups = kCastThreads / kCastLanes;
static_assert(kCastCircleTile == kCastThreads, "phase A: one circle per thread");

constexpr double kTwoPi = 6.283185307179586476925286766559;
// relative slack of the two culls (range and inside-the-circle) and absolute slack of the arc: far
// above the rounding of dist, asin and atan2, far below a beam
constexpr double kCastRel = 1.000001;
constexpr double kCastArcSlack = 1e-9;
// below this increment the one-beam margin is not safely above the rounding of the arc: every beam
constexpr double kCastMinInc = 1e-9;
// a segment's arc at or above this is too close to pi for "the short way" to be trusted: every beam
constexpr double kCastWallArc = 3.1415;

// A circle of the current tile as phase B reads it. nd: beams per interval less one (0: culled, < 0:
// every beam of the scan).
struct CastSlot {
  double px, py, r2, flo, nd;
};
// The body instantiation's slot: a mate is culled and given its beam interval through its circumscribed
// circle (the fields above), and phase B runs the slab test on the rectangle with axes (c, s).
struct CastBodySlot {
  double px, py, r2, flo, nd;
  double c, s;
  int mate;  // 0: a static circle (cast_beams), 1: a race-mate's rectangle (cast_beams_body), 2 (WALLS): a
             // segment with A = (px, py) and B = (c, s) from the LiDAR (cast_beams_wall)
};
template <bool BODY>
struct SlotOf {
  using type = CastSlot;
};
template <>
struct SlotOf<true> {
  using type = CastBodySlot;
};

// The exact hit test of circle (px, py, pp, r2) on beams lo .. hi of the scan (clipped to the beam tile
// [cb, cb + nb)), lanes striding by kCastLanes.
#pragma clang fp contract(off)
__device__ __forceinline__ void cast_beams(const double px, const double py, const double pp, const double r2,
                                           int lo, int hi, const int cb, const int nb, const int sub,
                                           const double* s_dx, const double* s_dy,
                                           unsigned long long* s_min) {
  lo = max(lo, cb) - cb;
  hi = min(hi, cb + nb - 1) - cb;
  for (int i = lo + sub; i <= hi; i += kCastLanes) {
    const double t = px * s_dx[i] + py * s_dy[i];
    const double d2 = pp - t * t;
    if (d2 <= r2 && t > 0.0) {
      const double th = t - __dsqrt_rn(fmax(r2 - d2, 0.0));
      if (th > 0.0) atomicMin(&s_min[i], (unsigned long long)__double_as_longlong(th));
    }
  }
}

// The slab test of body_geom.h on beams lo .. hi of the scan for the mate whose centre is (px, py) from the
// LiDAR and whose axes are (c, s): the beams and the fold are cast_beams'.
#pragma clang fp contract(off)
__device__ __forceinline__ void cast_beams_body(const double px, const double py, const double c, const double s,
                                                const BodyParams& H, int lo, int hi, const int cb, const int nb,
                                                const int sub, const double* s_dx, const double* s_dy,
                                                unsigned long long* s_min) {
  lo = max(lo, cb) - cb;
  hi = min(hi, cb + nb - 1) - cb;
  const double of = -(px * c + py * s), ol = -(py * c - px * s);
  for (int i = lo + sub; i <= hi; i += kCastLanes) {
    double th;
    if (body_slab(of, ol, c, s, s_dx[i], s_dy[i], H, th))
      atomicMin(&s_min[i], (unsigned long long)__double_as_longlong(th));
  }
}

// Rule W1 (wall_geom.h) on beams lo .. hi of the scan for the segment whose ends are (ax, ay) and (bx, by) from
// the LiDAR: the beams and the fold are cast_beams'.
#pragma clang fp contract(off)
__device__ __forceinline__ void cast_beams_wall(const double ax, const double ay, const double bx, const double by,
                                                int lo, int hi, const int cb, const int nb, const int sub,
                                                const double* s_dx, const double* s_dy, unsigned long long* s_min) {
  lo = max(lo, cb) - cb;
  hi = min(hi, cb + nb - 1) - cb;
  for (int i = lo + sub; i <= hi; i += kCastLanes) {
    double th;
    if (wall_hit(ax, ay, bx, by, s_dx[i], s_dy[i], th))
      atomicMin(&s_min[i], (unsigned long long)__double_as_longlong(th));
  }
}

// Phase A of a segment (WALLS): sg = (ax, ay, bx, by) into the slot with A = (px, py) and B = (c, s) from the
// LiDAR (ox, oy). Culled when the segment's nearest point is past max_range (a NaN field fails the compare: it
// hits nothing anyway); otherwise the beams of the arc from atan2(A) to atan2(B) the short way.
#pragma clang fp contract(off)
__device__ __forceinline__ void wall_slot(const double* __restrict__ sg, const double ox, const double oy,
                                          const double ori, const double amin, const double ainc,
                                          const double max_range, CastBodySlot& sl) {
  const double ax = sg[0] - ox, ay = sg[1] - oy, bx = sg[2] - ox, by = sg[3] - oy;
  const double ex = bx - ax, ey = by - ay, ee = ex * ex + ey * ey;
  double t = -(ax * ex + ay * ey) / ee;  // the nearest point of the segment: A + t e, t in [0, 1]
  t = ee > 0.0 ? fmin(fmax(t, 0.0), 1.0) : 0.0;
  const double nx = ax + t * ex, ny = ay + t * ey;
  if (!(__dsqrt_rn(nx * nx + ny * ny) <= max_range * kCastRel)) return;
  sl.px = ax;
  sl.py = ay;
  sl.c = bx;
  sl.s = by;
  sl.mate = 2;
  const double aa = atan2(ay, ax);
  double da = atan2(by, bx) - aa;  // to B the short way: in [-pi, pi]
  da -= kTwoPi * rint(da / kTwoPi);
  const double w = fabs(da) + 2.0 * kCastArcSlack;
  if (w < kCastWallArc && w + 4.0 * ainc < kTwoPi && ainc >= kCastMinInc) {
    double rel = (aa + fmin(da, 0.0)) - ori - amin - kCastArcSlack;  // the arc's low edge from beam 0
    rel -= kTwoPi * floor(rel / kTwoPi);
    sl.flo = rel / ainc;
    sl.nd = ceil(w / ainc) + 3.0;
  } else {
    sl.nd = -1.0;
  }
}

// Rule Z1's mix and rule Z2 on one beam: r the noise-free float32 range, kt the (car, tick) key, i the beam's
// index in the whole scan.
constexpr unsigned long long kNoiseK = 0x9E3779B97F4A7C15ull;
constexpr double kNoiseU = 0x1.bb67ae86627e8p-16;  // the double nearest to sqrt(3 / (2^32 - 1))
__device__ __forceinline__ unsigned long long noise_mix(unsigned long long z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
#pragma clang fp contract(off)
__device__ __forceinline__ float noise_beam(const float r, const unsigned long long kt, const int i,
                                            const NoiseParams& Z, const double max_range) {
  const float mr = (float)max_range;
  if (r == mr) return r;  // no return: untouched
  const unsigned long long h = noise_mix(kt + kNoiseK * (unsigned long long)(i + 1));
  const unsigned long long h2 = noise_mix(h + kNoiseK);
  if ((unsigned)(h2 >> 40) < Z.drop24) return mr;
  const int g = (int)(h & 0xffffull) + (int)((h >> 16) & 0xffffull) + (int)((h >> 32) & 0xffffull) +
                (int)(h >> 48) - 131070;
  const double q = (double)r;
  const double sigma = Z.sigma_abs + Z.sigma_rel * q;
  const double e = (sigma * (double)g) * kNoiseU;
  return (float)fmin(fmax(q + e, 0.0), max_range);
}

#pragma clang fp contract(off)
template <bool RACE, bool BODY, bool WALLS, bool NOISE, bool GRID = false, bool FIELD = false>
__device__ __forceinline__ void cast_one(const CastParams& P, const RaceParams& Q, const BodyParams& H,
                                         const WallParams& Wl, const NoiseParams& Z, const int b,
                                         const double* __restrict__ x,
                                         const double* __restrict__ circles, const double* __restrict__ segments,
                                         float* __restrict__ ranges, double* s_dx, double* s_dy,
                                         unsigned long long* s_min, typename SlotOf<BODY>::type* s_slot,
                                         const GridParams& Gp = GridParams{},
                                         const unsigned char* __restrict__ grid = nullptr,
                                         unsigned* s_win = nullptr, const int* __restrict__ d2 = nullptr,
                                         int* __restrict__ visits = nullptr) {
  static_assert(RACE || !BODY, "bodies are the race-mates'");
  static_assert(BODY || !WALLS, "walls come with the body cast");
  static_assert(WALLS || !NOISE, "the noise comes with the walls cast");
  static_assert(NOISE || !GRID, "the raster map comes with the noisy cast");
  static_assert(GRID || !FIELD, "the field is the raster map's");
  using Slot = typename SlotOf<BODY>::type;
  const int tid = threadIdx.x;
  const double ori = x[(size_t)b * 3 + 2];
  double so, co;
  sincos(ori, &so, &co);
  const double ox = x[(size_t)b * 3 + 0] + P.lidar_offset * co;
  const double oy = x[(size_t)b * 3 + 1] + P.lidar_offset * so;
  const double amin = (double)P.angle_min, ainc = (double)P.angle_inc;
  const double per = kTwoPi / ainc;  // beams per turn
  const double* cw = circles + (P.world_rows == 1 ? (size_t)0 : (size_t)b * (size_t)P.C * 3);
  const int nr = P.nr;
  const double last = (double)(nr - 1);
  int nc = P.C;  // the circles and, in a race, the G - 1 mates behind them
  int own = 0, first = 0;
  if constexpr (RACE) {
    nc += Q.G - 1;
    own = b % Q.G;
    first = b - own;
  }
  const int ns = nc;  // the first segment's index
  const double* sw = nullptr;
  if constexpr (WALLS) {
    nc += Wl.S;
    sw = segments + (Wl.wall_rows == 1 ? (size_t)0 : (size_t)b * (size_t)Wl.S * 4);
  }
  unsigned long long kt = 0;  // the key of (car, tick): uniform over the workgroup
  if constexpr (NOISE) {
    const unsigned long long kc = noise_mix(Z.seed + kNoiseK * (Z.car_base + (unsigned long long)b + 1ull));
    kt = noise_mix(kc + kNoiseK * ((unsigned long long)Z.tick + 1ull));
  }
  GridStart gs{};  // rule G1's start and the LDS square of this car: uniform over the workgroup
  GridWindow gw{};
  int d0 = 0;  // FIELD: d2 at the start cell
  if constexpr (FIELD) {
    if (d2) gs = grid_field_start(Gp, d2, ox, oy, d0);
  } else if constexpr (GRID) {
    if (grid) gs = grid_start(Gp, grid, ox, oy);
    gw.bits = s_win;
    if (gs.state == 2) {
      grid_window_shape(Gp, gs, P.max_range, gw);
      for (int k = tid; k < gw.side * gw.stride; k += kCastThreads) s_win[k] = grid_window_word(Gp, grid, gw, k);
    }
    // the barrier behind the first beam tile's directions orders these writes before the walks
  }
  for (int cb = 0; cb < nr; cb += kCastBeamTile) {
    const int nb = min(kCastBeamTile, nr - cb);
    for (int i = tid; i < nb; i += kCastThreads) {
      double sa, ca;
      sincos(ori + (amin + ainc * (double)(cb + i)), &sa, &ca);
      s_dx[i] = ca;
      s_dy[i] = sa;
      s_min[i] = (unsigned long long)__double_as_longlong(P.max_range);
    }
    __syncthreads();
    for (int c0 = 0; c0 < nc; c0 += kCastCircleTile) {
      {  // A: circle c0 + tid -> slot tid
        Slot sl{};
        const int j = c0 + tid;
        bool wall = false;
        if constexpr (WALLS) wall = j >= ns && j < nc;
        if constexpr (WALLS) {
          if (wall) wall_slot(sw + (size_t)(j - ns) * 4, ox, oy, ori, amin, ainc, P.max_range, sl);
        }
        if (!wall && j < nc) {
          double cx, cy, r;
          bool mate = false;
          if constexpr (RACE) mate = j >= P.C;
          if (mate) {  // mate k of the race, stepped over the own slot
            const int k = j - P.C;
            const double* xm = x + (size_t)(first + k + (k >= own ? 1 : 0)) * 3;
            double sm, cm;
            sincos(xm[2], &sm, &cm);
            cx = xm[0] + Q.center_offset * cm;
            cy = xm[1] + Q.center_offset * sm;
            if constexpr (BODY) {  // the circumscribed circle, for the culls and the interval only
              r = __dsqrt_rn(H.hl * H.hl + H.hw * H.hw) * kCastRel;
              sl.c = cm;
              sl.s = sm;
              sl.mate = 1;
            } else {
              r = Q.car_radius;
            }
          } else {
            r = cw[(size_t)j * 3 + 2];
            cx = cw[(size_t)j * 3 + 0];
            cy = cw[(size_t)j * 3 + 1];
          }
          const double px = cx - ox, py = cy - oy;
          const double ra = fabs(r), dist = __dsqrt_rn(px * px + py * py);
          if (dist - ra <= P.max_range * kCastRel) {
            sl.px = px;
            sl.py = py;
            sl.r2 = r * r;
            const double w = asin(fmin(ra / dist, 1.0)) + kCastArcSlack;
            const bool arc = dist > ra * kCastRel && 2.0 * w + 4.0 * ainc < kTwoPi && ainc >= kCastMinInc;
            if (arc) {
              double rel = atan2(py, px) - ori - amin - w;  // the arc's low edge from beam 0
              rel -= kTwoPi * floor(rel / kTwoPi);
              sl.flo = rel / ainc;
              sl.nd = ceil(2.0 * w / ainc) + 3.0;
            } else {
              sl.nd = -1.0;
            }
          }
        }
        s_slot[tid] = sl;
      }
      __syncthreads();
      {  // B: kCastLanes lanes per kept circle
        const int nt = min(kCastCircleTile, nc - c0), sub = tid % kCastLanes;
        for (int j = tid / kCastLanes; j < nt; j += kCastGroups) {
          const Slot sl = s_slot[j];
          if (sl.nd == 0.0) continue;
          const double pp = sl.px * sl.px + sl.py * sl.py;
          // the exact test of the slot on beams lo .. hi: the slab test on a mate's rectangle
          auto test = [&](const int lo, const int hi) {
            if constexpr (WALLS) {
              if (sl.mate == 2) {
                cast_beams_wall(sl.px, sl.py, sl.c, sl.s, lo, hi, cb, nb, sub, s_dx, s_dy, s_min);
                return;
              }
            }
            if constexpr (BODY) {
              if (sl.mate) {
                cast_beams_body(sl.px, sl.py, sl.c, sl.s, H, lo, hi, cb, nb, sub, s_dx, s_dy, s_min);
                return;
              }
            }
            cast_beams(sl.px, sl.py, pp, sl.r2, lo, hi, cb, nb, sub, s_dx, s_dy, s_min);
          };
          if (sl.nd < 0.0) {
            test(0, nr - 1);
            continue;
          }
          // the interval and its copies a turn apart; the first starts below beam 0 (flo < per)
          for (double k = -1.0;; k += 1.0) {
            const double s = floor(sl.flo + k * per) - 1.0;
            if (!(s <= last)) break;
            const double lo = fmax(s, 0.0), hi = fmin(s + sl.nd, last);
            if (lo <= hi) test((int)lo, (int)hi);
          }
        }
      }
      __syncthreads();
    }
    if constexpr (FIELD) {  // rule F1: one walker a beam, as below; visits is the walker's own store too
      int* vis = visits ? visits + (size_t)b * (size_t)nr + cb : nullptr;
      if (gs.state != 2) {
        for (int i = tid; i < nb; i += kCastThreads) {
          if (gs.state == 1) s_min[i] = 0ull;
          if (vis) vis[i] = gs.state;  // 0 reads outside the map, 1 in an occupied cell
        }
      } else {
        for (int i = tid; i < nb; i += kCastThreads) {
          const double cur = __longlong_as_double((long long)s_min[i]);
          double th;
          int v;
          if (grid_field_walk(Gp, d2, gs, d0, s_dx[i], s_dy[i], cur, th, v) && th < cur)
            s_min[i] = (unsigned long long)__double_as_longlong(th);
          if (vis) vis[i] = v;
        }
      }
    } else if constexpr (GRID) {  // rule G1: one walker a beam, behind the last tile's barrier (or the directions')
      if (gs.state == 1) {
        for (int i = tid; i < nb; i += kCastThreads) s_min[i] = 0ull;
      } else if (gs.state == 2) {
        for (int i = tid; i < nb; i += kCastThreads) {
          const double cur = __longlong_as_double((long long)s_min[i]);
          double th;
          if (grid_walk(Gp, grid, gw, gs, s_dx[i], s_dy[i], cur, th) && th < cur)
            s_min[i] = (unsigned long long)__double_as_longlong(th);
        }
      }
      // thread i stores the beams it walked: no barrier
    }
    float* out = ranges + (size_t)b * (size_t)nr + cb;
    if constexpr (NOISE) {
      for (int i = tid; i < nb; i += kCastThreads)
        out[i] = noise_beam((float)__longlong_as_double((long long)s_min[i]), kt, cb + i, Z, P.max_range);
    } else {
      for (int i = tid; i < nb; i += kCastThreads) out[i] = (float)__longlong_as_double((long long)s_min[i]);
    }
    __syncthreads();  // the next tile (or car) resets the minima
  }
}

// Workgroup w takes cars w, w + nwg, ... below B, or with a list the cars list[w], list[w + nwg], ...
// below min(*count, B) (plan_listed_kernel's rule: one past the count leaves at that load).
template <bool RACE, bool BODY = false, bool WALLS = false, bool NOISE = false, bool GRID = false, bool FIELD = false>
__device__ __forceinline__ void cast_scans(const CastParams& P, const RaceParams& Q, const BodyParams& H, const int B,
                                           const int nwg, const int* __restrict__ list,
                                           const int* __restrict__ count, const double* __restrict__ x,
                                           const double* __restrict__ circles, float* __restrict__ ranges,
                                           const WallParams& Wl = WallParams{},
                                           const double* __restrict__ segments = nullptr,
                                           const NoiseParams& Z = NoiseParams{},
                                           const GridParams& Gp = GridParams{},
                                           const unsigned char* __restrict__ grid = nullptr,
                                           const int* __restrict__ d2 = nullptr, int* __restrict__ visits = nullptr) {
  __shared__ double s_dx[kCastBeamTile];
  __shared__ double s_dy[kCastBeamTile];
  __shared__ unsigned long long s_min[kCastBeamTile];
  __shared__ typename SlotOf<BODY>::type s_slot[kCastCircleTile];
  unsigned* s_win = nullptr;
  if constexpr (GRID && !FIELD) {
    __shared__ unsigned s_bits[kGridWinWords];
    s_win = s_bits;
  }
  const int n = list ? min(*count, B) : B;
  for (int k = blockIdx.x; k < n; k += nwg) {
    const int b = list ? list[k] : k;
    if (b >= 0 && b < B) {  // uniform over the workgroup
      if constexpr (FIELD)
        cast_one<RACE, BODY, WALLS, NOISE, true, true>(P, Q, H, Wl, Z, b, x, circles, segments, ranges, s_dx, s_dy,
                                                       s_min, s_slot, Gp, nullptr, nullptr, d2, visits);
      else if constexpr (GRID)
        cast_one<RACE, BODY, WALLS, NOISE, true>(P, Q, H, Wl, Z, b, x, circles, segments, ranges, s_dx, s_dy, s_min,
                                                 s_slot, Gp, grid, s_win);
      else
        cast_one<RACE, BODY, WALLS, NOISE>(P, Q, H, Wl, Z, b, x, circles, segments, ranges, s_dx, s_dy, s_min, s_slot);
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kCastThreads) void cast_scans_kernel(const CastParams P, const int B, const int nwg,
                                                                  const int* __restrict__ list,
                                                                  const int* __restrict__ count,
                                                                  const double* __restrict__ x,
                                                                  const double* __restrict__ circles,
                                                                  float* __restrict__ ranges) {
  cast_scans<false>(P, RaceParams{}, BodyParams{}, B, nwg, list, count, x, circles, ranges);
}

// The same with the race-mates of every car behind its circles (x is also the opponents' poses).
__global__ __launch_bounds__(kCastThreads) void cast_scans_race_kernel(
    const CastParams P, const RaceParams Q, const int B, const int nwg, const int* __restrict__ list,
    const int* __restrict__ count, const double* __restrict__ x, const double* __restrict__ circles,
    float* __restrict__ ranges) {
  cast_scans<true>(P, Q, BodyParams{}, B, nwg, list, count, x, circles, ranges);
}

// The race cast with every mate the rectangle of body_geom.h in place of the race circle (BODY; Q.car_radius
// is not read): phase A's slot is the mate's circumscribed circle, phase B's test the slab test.
__global__ __launch_bounds__(kCastThreads) void cast_scans_body_kernel(
    const CastParams P, const RaceParams Q, const BodyParams H, const int B, const int nwg,
    const int* __restrict__ list, const int* __restrict__ count, const double* __restrict__ x,
    const double* __restrict__ circles, float* __restrict__ ranges) {
  cast_scans<true, true>(P, Q, H, B, nwg, list, count, x, circles, ranges);
}

// The body cast with the straight walls of wall_geom.h behind the circles and the mates (WALLS).
__global__ __launch_bounds__(kCastThreads) void cast_scans_walls_kernel(
    const CastParams P, const RaceParams Q, const BodyParams H, const WallParams Wl, const int B, const int nwg,
    const int* __restrict__ list, const int* __restrict__ count, const double* __restrict__ x,
    const double* __restrict__ circles, const double* __restrict__ segments, float* __restrict__ ranges) {
  cast_scans<true, true, true>(P, Q, H, B, nwg, list, count, x, circles, ranges, Wl, segments);
}

// The walls cast with rules Z1 and Z2 on every beam it stores (NOISE).
__global__ __launch_bounds__(kCastThreads) void cast_scans_noisy_kernel(
    const CastParams P, const RaceParams Q, const BodyParams H, const WallParams Wl, const NoiseParams Z, const int B,
    const int nwg, const int* __restrict__ list, const int* __restrict__ count, const double* __restrict__ x,
    const double* __restrict__ circles, const double* __restrict__ segments, float* __restrict__ ranges) {
  cast_scans<true, true, true, true>(P, Q, H, B, nwg, list, count, x, circles, ranges, Wl, segments, Z);
}

// The noisy cast with the raster map of grid_geom.h under every beam (GRID, rule G1).
__global__ __launch_bounds__(kCastThreads) void cast_scans_grid_kernel(
    const CastParams P, const RaceParams Q, const BodyParams H, const WallParams Wl, const NoiseParams Z,
    const GridParams Gp, const int B, const int nwg, const int* __restrict__ list, const int* __restrict__ count,
    const double* __restrict__ x, const double* __restrict__ circles, const double* __restrict__ segments,
    const unsigned char* __restrict__ grid, float* __restrict__ ranges) {
  cast_scans<true, true, true, true, true>(P, Q, H, B, nwg, list, count, x, circles, ranges, Wl, segments, Z, Gp, grid);
}

// The grid cast with rule F1 on the map's field d2 in place of rule G1 on its bytes (FIELD); visits [B][nr] or null.
__global__ __launch_bounds__(kCastThreads) void grid_cast_kernel(
    const CastParams P, const RaceParams Q, const BodyParams H, const WallParams Wl, const NoiseParams Z,
    const GridParams Gp, const int B, const int nwg, const int* __restrict__ list, const int* __restrict__ count,
    const double* __restrict__ x, const double* __restrict__ circles, const double* __restrict__ segments,
    const int* __restrict__ d2, float* __restrict__ ranges, int* __restrict__ visits) {
  cast_scans<true, true, true, true, true, true>(P, Q, H, B, nwg, list, count, x, circles, ranges, Wl,
                                                 segments, Z, Gp, nullptr, d2, visits);
}

int cast_scans_grid(WorldFamily family, int B) {
  const int cap = kWorldGrids[family].cast;
  return B < cap ? B : cap;
}

hipError_t launch_cast_scans(const World& w, int B, const int* list, const int* count, const double* x, float* ranges,
                             hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const int nwg = cast_scans_grid(w.family, B);
  const dim3 grid(nwg), block(kCastThreads);
  if (w.family == WORLD_GRID && w.field)
    hipLaunchKernelGGL(grid_cast_kernel, grid, block, 0, s, w.P, w.Q, w.H, w.Wl, w.Z, w.Gr, B, nwg, list, count, x,
                       w.circles, w.segments, w.Gr.W > 0 && w.Gr.H > 0 ? w.d2 : nullptr, ranges, w.visits);
  else if (w.family == WORLD_GRID)
    hipLaunchKernelGGL(cast_scans_grid_kernel, grid, block, 0, s, w.P, w.Q, w.H, w.Wl, w.Z, w.Gr, B, nwg, list, count,
                       x, w.circles, w.segments, w.Gr.W > 0 && w.Gr.H > 0 ? w.grid : nullptr, ranges);
  else if (w.family == WORLD_NOISY)
    hipLaunchKernelGGL(cast_scans_noisy_kernel, grid, block, 0, s, w.P, w.Q, w.H, w.Wl, w.Z, B, nwg, list, count, x,
                       w.circles, w.segments, ranges);
  else if (w.family == WORLD_WALLS)
    hipLaunchKernelGGL(cast_scans_walls_kernel, grid, block, 0, s, w.P, w.Q, w.H, w.Wl, B, nwg, list, count, x,
                       w.circles, w.segments, ranges);
  else if (w.family == WORLD_BODY)
    hipLaunchKernelGGL(cast_scans_body_kernel, grid, block, 0, s, w.P, w.Q, w.H, B, nwg, list, count, x, w.circles,
                       ranges);
  else if (w.family == WORLD_RACE)
    hipLaunchKernelGGL(cast_scans_race_kernel, grid, block, 0, s, w.P, w.Q, B, nwg, list, count, x, w.circles, ranges);
  else
    hipLaunchKernelGGL(cast_scans_kernel, grid, block, 0, s, w.P, B, nwg, list, count, x, w.circles, ranges);
  return hipGetLastError();
}

}  // namespace f110qp
