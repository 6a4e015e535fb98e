// contact_kernels.hip — contact in the closed loop's world of circles: every car's clearance to the static
// circles and to its race-mates (f110qp_clearance_dev, f110qp_rollout_contact[_dev] of include/f110qp.h).
//
// The body of a car is the race model's circle: centre q = (x + off cos(ori), y + off sin(ori)) with
// off = center_offset, radius R = car_radius. Per pose and obstacle, all fp64 with FP contraction off and the
// correctly rounded square root (the cast kernel's discipline):
//   static circle j = (cx, cy, r):  dx = cx - qx, dy = cy - qy, d = sqrt(dx dx + dy dy), v = (d - |r|) - R
//   race-mate m (centre q_m built as q is, at the same row of x):   dx = q_m.x - qx, ...,  v = (d - R) - R
// clearance = the minimum of the v, nearest = its index (j, or C + i for the mate with index i inside the
// race), the lowest index on equal values. A candidate replaces the running (best, idx) only when v < best, or
// v == best with a lower index, from the start (+inf, -1): a NaN v never passes a compare, so a NaN circle or
// mate is never chosen and a car with a non-finite pose keeps the start value. Per pair the value depends on
// nothing else, and the (value, index) minimum is associative and commutative: the result does not depend on
// which thread visits which obstacle, or on the order of the list.
//
// Mapping: one 256-thread workgroup per car, striding over the cars; the car's rows in passes of
// kClearPoses. Per pass the first threads build the body centres into LDS (one sincos each), then the
// obstacle list is walked kCastCircleTile at a time, one obstacle per thread: the thread reads its circle
// once (or, in the virtual tail behind the C circles as in cast_one<RACE>, builds mate k of the race at every
// pose's row, stepped over the own slot) and tests it against every pose of the pass, (best, idx) per pose
// in registers. A car's circles are read once per pass straight from global memory, 24 contiguous bytes a
// thread: there is no reuse inside a pass that an LDS copy would serve. The pass ends with a lexicographic
// (value, index) minimum over xor shuffles inside each wave and over the four waves' results in LDS. Every
// loop bound is uniform over the workgroup, so whole waves reach every shuffle and barrier. No atomic. No cull:
// every pair takes its square root (clearances are negative on contact, so a cheaper sign test has nothing
// to stand on), and the result is the exact minimum by construction. No cap on C or G.
//
// That is the WORLD_RACE instantiation of the one kernel below. What the other two families change, each
// behind `if constexpr` as in cast_one; index, update rule, start value, NaN rule, mapping, passes, reduction
// and crash record are the same text for all three:
//   WORLD_BODY (f110qp_clearance_body_dev, f110qp_rollout_body[_dev]): the body is the rectangle of
//     body_geom.h, centre q as above, axes (cos, sin) of the heading, half extents H; Q.car_radius is not
//     read. A static circle gives v = body_sd(c; body) - |r|, a mate v = body_pair(own, mate), the same bits
//     from either side. LDS holds (cos, sin) per pose next to q, and a mate's frame is built by the thread that
//     takes it, one sincos per pose. The mate loop is not unrolled (one body_pair in the code instead of
//     eight, its value folded into the pose's registers by an unrolled select), which is what keeps the
//     instantiation's registers down.
//   WORLD_WALLS (f110qp_clearance_walls_dev, f110qp_rollout_walls[_dev]): WORLD_BODY with the S segments of
//     wall_geom.h as a third stretch of the obstacle list: index j in [C + G - 1, C + G - 1 + S) is segment
//     k = j - (C + G - 1), index C + G + k in nearest. The thread reads its segment once per pass (32
//     contiguous bytes) and tests it against every pose of the pass with wall_body (rule W2); like the mate
//     loop, the pose loop is not unrolled, so there is one wall_body in the code.
//   WORLD_GRID (f110qp_clearance_grid_dev, f110qp_rollout_grid[_dev]): WORLD_WALLS with the occupied cells of
//     the raster map (grid_geom.h, rule G2) as a fourth stretch, cell (i, j) at index C + G + S + j W + i in
//     nearest. It is walked per pose behind the obstacle tiles: the threads stride over the cells of the pose's
//     window (the body's circumscribed circle plus `reach`, clipped to the map), read each cell's byte and test
//     an occupied one with grid_cell_body, one copy in the code. The window is uniform over the workgroup.
#include <hip/hip_runtime.h>

#include "body_geom.h"
#include "f110qp_kernels.h"
#include "grid_geom.h"
#include "wall_geom.h"

namespace f110qp {

namespace {

constexpr int kClearThreads = 256;
constexpr int kClearWaves = kClearThreads / 64;
constexpr int kClearPoses = 8;  // poses (rows of one car) per pass
static_assert(kCastCircleTile == kClearThreads, "one obstacle of the tile per thread");

// (v, i) into (best, idx): the update rule above.
__device__ __forceinline__ void take_min(double& best, int& idx, const double v, const int i) {
  if (v < best || (v == best && i < idx)) {
    best = v;
    idx = i;
  }
}

// The first and the second pointer of the kernel's pack (the segments, the map).
template <typename A, typename... R>
__device__ __forceinline__ A* pack_first(A* a, R*...) {
  return a;
}
template <typename A, typename G>
__device__ __forceinline__ G* pack_second(A*, G* g) {
  return g;
}

}  // namespace

// The configs a family's instantiation reads, its first kernel argument. Each instantiation keeps the
// argument list its family's own kernel had, and with it that kernel's instruction stream: an
// argument that a family does not read still moves the kernarg loads and, through them, the SGPR spills. So
// the record grows with the family, and the segments pointer (WORLD_WALLS) and the map behind it (WORLD_GRID) are
// a parameter pack.
template <WorldFamily FAM>
struct ClearCfg {
  ClearParams P;
  RaceParams Q;
};
template <>
struct ClearCfg<WORLD_BODY> {
  ClearParams P;
  RaceParams Q;
  BodyParams H;
};
template <>
struct ClearCfg<WORLD_WALLS> {
  ClearParams P;
  RaceParams Q;
  BodyParams H;
  WallParams Wl;
};
template <>
struct ClearCfg<WORLD_GRID> {
  ClearParams P;
  RaceParams Q;
  BodyParams H;
  WallParams Wl;
  GridParams Gr;
};

#pragma clang fp contract(off)
// Seg: `const double` for WORLD_WALLS, `const double, const unsigned char` for WORLD_GRID, empty otherwise
template <WorldFamily FAM, typename... Seg>
__global__ __launch_bounds__(kClearThreads) void clearance_kernel(
    const ClearCfg<FAM> W, const int B, const int rows, const int nwg, const double* __restrict__ x,
    const double* __restrict__ circles, Seg* __restrict__... segments, double* __restrict__ clearance,
    int* __restrict__ nearest, const ContactMark M) {
  static_assert(FAM >= WORLD_RACE && FAM != WORLD_NOISY &&
                    sizeof...(Seg) == (FAM == WORLD_GRID ? 2 : FAM == WORLD_WALLS ? 1 : 0),
                "segments come with the walls, the map with the grid");
  constexpr bool BODY = FAM >= WORLD_BODY, WALLS = FAM >= WORLD_WALLS, GRID = FAM == WORLD_GRID;
  const ClearParams& P = W.P;
  const RaceParams& Q = W.Q;
  __shared__ double s_qx[kClearPoses], s_qy[kClearPoses];
  __shared__ double s_c[kClearPoses], s_s[kClearPoses];  // BODY: the frame's axes (not allocated otherwise)
  __shared__ double s_best[kClearWaves][kClearPoses];
  __shared__ int s_idx[kClearWaves][kClearPoses];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const int ns = P.C + Q.G - 1;  // the circles and the G - 1 mates behind them, then (WALLS) the segments
  int nc = ns;
  if constexpr (WALLS) nc += W.Wl.S;
  for (int b = blockIdx.x; b < B; b += nwg) {
    const double* cw = circles + (P.world_rows == 1 ? (size_t)0 : (size_t)b * (size_t)P.C * 3);
    const double* sw = nullptr;
    if constexpr (WALLS) sw = pack_first(segments...) + (W.Wl.wall_rows == 1 ? (size_t)0 : (size_t)b * (size_t)W.Wl.S * 4);
    const int own = b % Q.G, first = b - own;
    int crash = -1;  // thread 0: the first row at or under the margin
    if (M.crash_tick && !M.init && tid == 0) crash = M.crash_tick[b];
    for (int r0 = 0; r0 < rows; r0 += kClearPoses) {
      const int np = min(kClearPoses, rows - r0);
      if (tid < np) {  // the body centre (BODY: frame) of pose tid of the pass
        const double* xp = x + ((size_t)(r0 + tid) * (size_t)B + (size_t)b) * 3;
        double so, co;
        sincos(xp[2], &so, &co);
        s_qx[tid] = xp[0] + Q.center_offset * co;
        s_qy[tid] = xp[1] + Q.center_offset * so;
        if constexpr (BODY) {
          s_c[tid] = co;
          s_s[tid] = so;
        }
      }
      __syncthreads();
      double best[kClearPoses];
      int idx[kClearPoses];
#pragma unroll
      for (int p = 0; p < kClearPoses; p++) {
        best[p] = inf;
        idx[p] = -1;
      }
      for (int c0 = 0; c0 < nc; c0 += kCastCircleTile) {
        const int j = c0 + tid;
        if (j < P.C) {
          const double cx = cw[(size_t)j * 3 + 0], cy = cw[(size_t)j * 3 + 1];
          const double ra = fabs(cw[(size_t)j * 3 + 2]);
#pragma unroll
          for (int p = 0; p < kClearPoses; p++) {
            if (p < np) {
              if constexpr (BODY) {
                take_min(best[p], idx[p], body_sd(cx, cy, s_qx[p], s_qy[p], s_c[p], s_s[p], W.H) - ra, j);
              } else {
                const double dx = cx - s_qx[p], dy = cy - s_qy[p];
                const double d = __dsqrt_rn(dx * dx + dy * dy);
                take_min(best[p], idx[p], (d - ra) - Q.car_radius, j);
              }
            }
          }
        } else if (j < ns) {  // mate k of the race, stepped over the own slot: index i inside the race
          const int k = j - P.C, i = k + (k >= own ? 1 : 0);
          if constexpr (BODY) {
#pragma unroll 1
            for (int p = 0; p < np; p++) {
              const double* xm = x + ((size_t)(r0 + p) * (size_t)B + (size_t)(first + i)) * 3;
              double sm, cm;
              sincos(xm[2], &sm, &cm);
              const double mx = xm[0] + Q.center_offset * cm, my = xm[1] + Q.center_offset * sm;
              const double v = body_pair(s_qx[p], s_qy[p], s_c[p], s_s[p], mx, my, cm, sm, W.H);
#pragma unroll
              for (int q = 0; q < kClearPoses; q++)
                if (q == p) take_min(best[q], idx[q], v, P.C + i);
            }
          } else {
#pragma unroll
            for (int p = 0; p < kClearPoses; p++) {
              if (p < np) {
                const double* xm = x + ((size_t)(r0 + p) * (size_t)B + (size_t)(first + i)) * 3;
                double sm, cm;
                sincos(xm[2], &sm, &cm);
                const double mx = xm[0] + Q.center_offset * cm, my = xm[1] + Q.center_offset * sm;
                const double dx = mx - s_qx[p], dy = my - s_qy[p];
                const double d = __dsqrt_rn(dx * dx + dy * dy);
                take_min(best[p], idx[p], (d - Q.car_radius) - Q.car_radius, P.C + i);
              }
            }
          }
        } else if (WALLS && j < nc) {  // segment j - ns
          if constexpr (WALLS) {
            const double* sg = sw + (size_t)(j - ns) * 4;
            const double ax = sg[0], ay = sg[1], bx = sg[2], by = sg[3];
            const int i = P.C + Q.G + (j - ns);
#pragma unroll 1
            for (int p = 0; p < np; p++) {
              const double v = wall_body(ax, ay, bx, by, s_qx[p], s_qy[p], s_c[p], s_s[p], W.H);
#pragma unroll
              for (int q = 0; q < kClearPoses; q++)
                if (q == p) take_min(best[q], idx[q], v, i);
            }
          }
        }
      }
      if constexpr (GRID) {  // the occupied cells of every pose's window
        const unsigned char* gm = pack_second(segments...);
        if (gm) {
#pragma unroll 1
          for (int p = 0; p < np; p++) {
            int i0, i1, j0, j1;
            if (!grid_body_window(W.Gr, W.H, s_qx[p], s_qy[p], i0, i1, j0, j1)) continue;  // uniform
            const int ni = i1 - i0 + 1;
            const long long cells = (long long)ni * (long long)(j1 - j0 + 1);
            for (long long k = tid; k < cells; k += kClearThreads) {
              const int j = j0 + (int)(k / ni), i = i0 + (int)(k % ni);
              const size_t at = (size_t)j * (size_t)W.Gr.W + (size_t)i;
              if (!gm[at]) continue;
              const double v = grid_cell_body(W.Gr, i, j, s_qx[p], s_qy[p], s_c[p], s_s[p], W.H);
#pragma unroll
              for (int q = 0; q < kClearPoses; q++)
                if (q == p) take_min(best[q], idx[q], v, nc + 1 + (int)at);
            }
          }
        }
      }
      // the wave's (value, index) minimum per pose, then the four waves' through LDS
#pragma unroll
      for (int p = 0; p < kClearPoses; p++) {
        if (p < np) {  // uniform
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(best[p], m, 64);
            const int oi = __shfl_xor(idx[p], m, 64);
            take_min(best[p], idx[p], ov, oi);
          }
          if (lane == 0) {
            s_best[wave][p] = best[p];
            s_idx[wave][p] = idx[p];
          }
        }
      }
      __syncthreads();
      if (tid < np) {
        double v = s_best[0][tid];
        int i = s_idx[0][tid];
#pragma unroll
        for (int w = 1; w < kClearWaves; w++) take_min(v, i, s_best[w][tid], s_idx[w][tid]);
        const size_t o = (size_t)(r0 + tid) * (size_t)B + (size_t)b;
        clearance[o] = v;
        if (nearest) nearest[o] = i;
        s_best[0][tid] = v;  // for the mark below (read by thread 0 behind the barrier)
      }
      if (M.crash_tick) {  // uniform
        __syncthreads();
        if (tid == 0)
          for (int p = 0; p < np; p++)
            if (crash < 0 && s_best[0][p] <= M.margin) crash = M.row0 + r0 + p;
      }
      __syncthreads();  // the next pass (or car) rewrites the centres and the waves' results
    }
    if (M.crash_tick && tid == 0) M.crash_tick[b] = crash;
  }
}

int clearance_grid(WorldFamily family, int B) {
  const int cap = kWorldGrids[family].clearance;
  return B < cap ? B : cap;
}

hipError_t launch_clearance(const World& w, int B, int rows, const double* x, double* clearance, int* nearest,
                            const ContactMark& M, hipStream_t s) {
  if (w.family < WORLD_RACE) return hipErrorInvalidValue;  // contact is between the cars of a race
  if (B <= 0 || rows <= 0) return hipSuccess;
  const int nwg = clearance_grid(w.family, B);
  const dim3 grid(nwg), block(kClearThreads);
  const ClearParams P{w.P.C, w.P.world_rows};
  if (w.family == WORLD_GRID)
    hipLaunchKernelGGL((clearance_kernel<WORLD_GRID, const double, const unsigned char>), grid, block, 0, s,
                       ClearCfg<WORLD_GRID>{P, w.Q, w.H, w.Wl, w.Gr}, B, rows, nwg, x, w.circles, w.segments,
                       w.Gr.W > 0 && w.Gr.H > 0 ? w.grid : nullptr, clearance, nearest, M);
  else if (w.family >= WORLD_WALLS)  // WORLD_NOISY: the clearance never reads the noise
    hipLaunchKernelGGL((clearance_kernel<WORLD_WALLS, const double>), grid, block, 0, s,
                       ClearCfg<WORLD_WALLS>{P, w.Q, w.H, w.Wl}, B, rows, nwg, x, w.circles, w.segments, clearance,
                       nearest, M);
  else if (w.family == WORLD_BODY)
    hipLaunchKernelGGL(clearance_kernel<WORLD_BODY>, grid, block, 0, s, ClearCfg<WORLD_BODY>{P, w.Q, w.H}, B, rows,
                       nwg, x, w.circles, clearance, nearest, M);
  else
    hipLaunchKernelGGL(clearance_kernel<WORLD_RACE>, grid, block, 0, s, ClearCfg<WORLD_RACE>{P, w.Q}, B, rows, nwg, x,
                       w.circles, clearance, nearest, M);
  return hipGetLastError();
}

}  // namespace f110qp
