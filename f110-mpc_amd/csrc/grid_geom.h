// grid_geom.h — the raster map (include/f110qp.h "occupancy-grid maps"), written once for the ray cast
// (scan_kernels.hip, rule G1) and the clearance kernel (contact_kernels.hip, rule G2).
//
// The map is [H][W] bytes, nonzero occupied, cell (i, j) the square from (ox + i res, oy + j res); outside the
// map is free space. All fp64, FP contraction off in every function (no fused multiply-add), the correctly
// rounded division; the expression order here is the specification's and workload.ray_grid /
// workload.clearance_grid repeat it.
#pragma once
#include <hip/hip_runtime.h>

#include "f110qp_kernels.h"  // GridParams, BodyParams
#include "wall_geom.h"

namespace f110qp {

// The LDS copy of the cells a car's beams can reach: the square of `side` cells from cell (x0, y0), one bit a
// cell, rows of `stride` 32-bit words; a cell of the square outside the map is a clear bit. side == 0: no copy,
// every cell is read from global memory. A cell outside the square is read from global memory too, so the
// square's size decides the cost of a walk and never its result.
constexpr int kGridWinWords = 5280;  // 405 rows of 13 words: max_range 10 m at 0.05 m a cell, and a cell to spare
struct GridWindow {
  const unsigned* bits;
  int x0, y0, side, stride;
};

// The start of a car's walks, uniform over the workgroup: the LiDAR in cell units and its cell. state 0: the
// grid gives no hit (no map, the LiDAR outside it or not finite), 1: the start cell is occupied (th = 0), 2: walk.
struct GridStart {
  double px, py;
  int ix, iy, state;
};

#pragma clang fp contract(off)
__device__ __forceinline__ GridStart grid_start(const GridParams& G, const unsigned char* __restrict__ grid,
                                                const double ox, const double oy) {
  GridStart s{};
  s.px = (ox - G.ox) / G.res;
  s.py = (oy - G.oy) / G.res;
  // floor(p) in [0, W) is 0 <= p < W, which a NaN or an infinity fails
  if (!(s.px >= 0.0 && s.px < (double)G.W && s.py >= 0.0 && s.py < (double)G.H)) return s;
  s.ix = (int)floor(s.px);
  s.iy = (int)floor(s.py);
  s.state = grid[(size_t)s.iy * (size_t)G.W + (size_t)s.ix] ? 1 : 2;
  return s;
}

// The square of a start for beams of at most max_range: n = ceil(max_range / res) + 1 cells to every side.
// side 0 when it does not fit kGridWinWords.
#pragma clang fp contract(off)
__device__ __forceinline__ void grid_window_shape(const GridParams& G, const GridStart& s, const double max_range,
                                                  GridWindow& w) {
  w.side = 0;
  const double n = ceil(max_range / G.res) + 1.0;
  if (!(n < 4096.0)) return;
  const int ni = (int)n, side = 2 * ni + 1, stride = (side + 31) >> 5;
  if (stride * side > kGridWinWords) return;
  w.x0 = s.ix - ni;
  w.y0 = s.iy - ni;
  w.side = side;
  w.stride = stride;
}

// Word k of the square, packed from the map's bytes (the workgroup's threads stride over the words).
__device__ __forceinline__ unsigned grid_window_word(const GridParams& G, const unsigned char* __restrict__ grid,
                                                     const GridWindow& w, const int k) {
  const int row = k / w.stride, c0 = (k - row * w.stride) << 5;
  const long long j = (long long)w.y0 + row;
  unsigned bits = 0;
  if (j >= 0 && j < G.H) {
    const unsigned char* gr = grid + (size_t)j * (size_t)G.W;
    const int nk = min(32, w.side - c0);
    for (int b = 0; b < nk; b++) {
      const long long i = (long long)w.x0 + c0 + b;
      if (i >= 0 && i < G.W && gr[i]) bits |= 1u << b;
    }
  }
  return bits;
}

// Cell (i, j) of the map, 0 <= i < W and 0 <= j < H: from the square when it holds the cell.
__device__ __forceinline__ bool grid_occupied(const GridParams& G, const unsigned char* __restrict__ grid,
                                              const GridWindow& w, const int i, const int j) {
  const long long c = (long long)i - w.x0, r = (long long)j - w.y0;
  if (c >= 0 && c < w.side && r >= 0 && r < w.side)
    return (w.bits[(int)r * w.stride + ((int)c >> 5)] >> ((int)c & 31)) & 1u;
  return grid[(size_t)j * (size_t)G.W + (size_t)i] != 0;
}

// Rule G1 for one beam of a start in state 2: the walk from cell (ix, iy) along (dx, dy); false: no hit at or
// below `limit` (max_range, or a lower value that the caller's minimum already holds: the parameter only grows
// along the walk). Each boundary's parameter is computed from the integer boundary when the walk reaches the
// cell in front of it, never accumulated.
#pragma clang fp contract(off)
__device__ __forceinline__ bool grid_walk(const GridParams& G, const unsigned char* __restrict__ grid,
                                          const GridWindow& w, const GridStart& s, const double dx, const double dy,
                                          const double limit, double& th) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double gx = dx / G.res, gy = dy / G.res;
  const int sx = dx > 0.0 ? 1 : -1, sy = dy > 0.0 ? 1 : -1;
  const bool mx = dx > 0.0 || dx < 0.0, my = dy > 0.0 || dy < 0.0;
  int ix = s.ix, iy = s.iy;
  double tx = mx ? ((double)(dx > 0.0 ? ix + 1 : ix) - s.px) / gx : inf;
  double ty = my ? ((double)(dy > 0.0 ? iy + 1 : iy) - s.py) / gy : inf;
  for (long long k = (long long)G.W + G.H + 2; k > 0; k--) {
    double t;
    if (tx <= ty) {
      t = tx;
      ix += sx;
      tx = ((double)(dx > 0.0 ? ix + 1 : ix) - s.px) / gx;
    } else {
      t = ty;
      iy += sy;
      ty = ((double)(dy > 0.0 ? iy + 1 : iy) - s.py) / gy;
    }
    if (!(t <= limit)) return false;  // past the range, or NaN
    if (ix < 0 || ix >= G.W || iy < 0 || iy >= G.H) return false;
    if (grid_occupied(G, grid, w, ix, iy)) {
      th = t + 0.0;  // a -0 (0 / g on a boundary, g < 0) becomes +0
      return true;
    }
  }
  return false;
}

// Rule F1's start, uniform over the workgroup: grid_start with the cell's occupancy read from the field, whose
// value at the start cell goes into D (states 1 and 2).
#pragma clang fp contract(off)
__device__ __forceinline__ GridStart grid_field_start(const GridParams& G, const int* __restrict__ d2,
                                                      const double ox, const double oy, int& D) {
  GridStart s{};
  s.px = (ox - G.ox) / G.res;
  s.py = (oy - G.oy) / G.res;
  if (!(s.px >= 0.0 && s.px < (double)G.W && s.py >= 0.0 && s.py < (double)G.H)) return s;
  s.ix = (int)floor(s.px);
  s.iy = (int)floor(s.py);
  D = d2[(size_t)s.iy * (size_t)G.W + (size_t)s.ix];
  s.state = D <= 0 ? 1 : 2;
  return s;
}

// Is p / g <= q / h (or, with `strict`, <) for the correctly rounded quotients, p / g and q / h both >= 0 and
// finite? The products with the reciprocals are within 2^-51 (relative) of the quotients, so a gap of more than
// 2^-48 between them decides; inside it the quotients themselves are compared.
#pragma clang fp contract(off)
__device__ __forceinline__ bool grid_quot_before(const double p, const double g, const double rg, const double q,
                                                 const double h, const double rh, const bool strict) {
  const double k = 0x1.0000000000010p+0;  // 1 + 2^-48
  const double a = p * rg, b = q * rh;
  if (a * k < b) return true;
  if (b * k < a) return false;
  return strict ? p / g < q / h : p / g <= q / h;
}

// Rule F1 for one beam of a start in state 2 whose cell holds D > 0 in the field: grid_walk's result and bits
// with the cells between two reads of d2 jumped over. After A x-moves and B y-moves the walk's next boundaries
// are X(A) = ((double)(kx + sx A) - px) / gx and Y(B) likewise, rule G1's expressions on the integer boundary, both
// non-decreasing; the walk stands at (A, B) with A + B = n exactly when (A == 0 or X(A - 1) <= Y(B)) and
// (B == 0 or Y(B - 1) < X(A)), and the parameter of its last move is max(X(A - 1), Y(B - 1)). A jump estimates A
// from the real-valued crossing counts, moves it by one while a condition fails (kGridJumpFix times at most:
// the estimate is a move or two off at worst), and past that takes the m moves singly. visits counts the
// reads of d2, the start cell's among them.
constexpr int kGridJumpFix = 4;
#pragma clang fp contract(off)
__device__ __forceinline__ bool grid_field_walk(const GridParams& G, const int* __restrict__ d2, const GridStart& s,
                                                int D, const double dx, const double dy, const double limit,
                                                double& th, int& visits) {
  const double gx = dx / G.res, gy = dy / G.res;
  const int sx = dx > 0.0 ? 1 : -1, sy = dy > 0.0 ? 1 : -1;
  const bool mx = dx > 0.0 || dx < 0.0, my = dy > 0.0 || dy < 0.0;
  const int kx = dx > 0.0 ? s.ix + 1 : s.ix, ky = dy > 0.0 ? s.iy + 1 : s.iy;
  // the numerators of X(k) and Y(l): exact differences of an int and px up to one rounding, as the walk's
  auto nx = [&](const int k) { return (double)(kx + sx * k) - s.px; };
  auto ny = [&](const int l) { return (double)(ky + sy * l) - s.py; };
  visits = 1;
  if (!mx && !my) return false;  // the walk's first step: t = +inf (a direction that is not finite)
  // the estimate's constants: the crossings by parameter t are about (t - X(0)) |gx| + 1 and (t - Y(0)) |gy| + 1
  const double ax = fabs(gx), ay = fabs(gy), rgx = 1.0 / gx, rgy = 1.0 / gy;
  const double x0 = mx ? nx(0) * rgx : 0.0, y0 = my ? ny(0) * rgy : 0.0;
  const double c0 = x0 * ax + y0 * ay, rs = 1.0 / (ax + ay);
  int A = 0, B = 0;
  for (long long left = (long long)G.W + G.H + 2; left > 0;) {
    int m = (int)__dsqrt_rn((double)(D - 1));  // the largest m with m m < D
    m = max(m, 1);
    if ((long long)m > left) m = (int)left;
    left -= m;
    const int n = A + B + m;
    int a;
    if (!mx) {
      a = 0;
    } else if (!my) {
      a = n;
    } else {
      const double te = ((double)(n - 1) + c0) * rs;
      const double ae = floor((te - x0) * ax) + 1.0;
      a = (int)fmin(fmax(ae, (double)A), (double)(A + m));
      int fix = 0;
      for (; fix < kGridJumpFix; fix++) {
        const int b = n - a;
        if (a > 0 && !grid_quot_before(nx(a - 1), gx, rgx, ny(b), gy, rgy, false)) {
          a--;  // the last x-move comes after the next y-move: one x-move too many
        } else if (b > 0 && !grid_quot_before(ny(b - 1), gy, rgy, nx(a), gx, rgx, true)) {
          a++;  // the last y-move does not come before the next x-move: one y-move too many
        } else {
          break;
        }
      }
      if (fix == kGridJumpFix) {  // the m moves singly, from (A, B)
        a = A;
        int b = B;
        for (int k = 0; k < m; k++) {
          if (nx(a) / gx <= ny(b) / gy)
            a++;
          else
            b++;
        }
      }
    }
    A = a;
    B = n - a;
    const double tx = A > 0 ? nx(A - 1) / gx : 0.0, ty = B > 0 ? ny(B - 1) / gy : 0.0;
    const double t = A > 0 && B > 0 ? fmax(tx, ty) : A > 0 ? tx : ty;
    if (!(t <= limit)) return false;  // past the range, or NaN
    const long long ix = (long long)s.ix + (long long)sx * A, iy = (long long)s.iy + (long long)sy * B;
    if (ix < 0 || ix >= G.W || iy < 0 || iy >= G.H) return false;
    D = d2[(size_t)iy * (size_t)G.W + (size_t)ix];
    visits++;
    if (D <= 0) {
      th = t + 0.0;  // a -0 (0 / g on a boundary, g < 0) becomes +0
      return true;
    }
  }
  return false;
}

// Rule G2 for one occupied cell (i, j) against the body (qx, qy, c, s): the least of rule W2 over the cell's four
// edges in the rule's order, and 0 at most when the body's centre is in the cell.
#pragma clang fp contract(off)
__device__ __forceinline__ double grid_cell_body(const GridParams& G, const int i, const int j, const double qx,
                                                 const double qy, const double c, const double s,
                                                 const BodyParams& H) {
  const double x0 = G.ox + (double)i * G.res, x1 = G.ox + (double)(i + 1) * G.res;
  const double y0 = G.oy + (double)j * G.res, y1 = G.oy + (double)(j + 1) * G.res;
  double v = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll 1
  for (int e = 0; e < 4; e++) {  // (x0,y0)-(x1,y0), (x1,y0)-(x1,y1), (x1,y1)-(x0,y1), (x0,y1)-(x0,y0)
    const double ax = (e == 0 || e == 3) ? x0 : x1, ay = e < 2 ? y0 : y1;
    const double bx = e < 2 ? x1 : x0, by = (e == 0 || e == 3) ? y0 : y1;
    v = fmin(v, wall_body(ax, ay, bx, by, qx, qy, c, s, H));
  }
  if (x0 <= qx && qx < x1 && y0 <= qy && qy < y1) v = fmin(v, 0.0);
  return v;
}

// Rule G2's window for the body centre (qx, qy): cells i0 .. i1 by j0 .. j1, clipped to the map; false: no cell
// (a pose that is not finite, or a window beside the map).
#pragma clang fp contract(off)
__device__ __forceinline__ bool grid_body_window(const GridParams& G, const BodyParams& H, const double qx,
                                                 const double qy, int& i0, int& i1, int& j0, int& j1) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  if (!(fabs(qx) < inf && fabs(qy) < inf)) return false;
  const double R = __dsqrt_rn(H.hl * H.hl + H.hw * H.hw) + G.reach;
  const double li = fmax(floor((qx - R - G.ox) / G.res), 0.0), hi = fmin(floor((qx + R - G.ox) / G.res), (double)G.W - 1.0);
  const double lj = fmax(floor((qy - R - G.oy) / G.res), 0.0), hj = fmin(floor((qy + R - G.oy) / G.res), (double)G.H - 1.0);
  if (!(li <= hi && lj <= hj)) return false;
  i0 = (int)li;
  i1 = (int)hi;
  j0 = (int)lj;
  j1 = (int)hj;
  return true;
}

}  // namespace f110qp
