// standings_kernels.hip — who is ahead: every pose's progress along the closed path, and from it the distance
// driven, the laps and the positions inside each race (f110qp_progress_dev, f110qp_standings_dev and
// f110qp_race_standings of include/f110qp.h, which holds the model).
//
// progress_kernel. Per pose p = (x, y) and segment j = (a = wp[j], b = wp[(j + 1) % W]), all fp64 with FP
// contraction off (contact_kernels.hip's discipline; the divide and the square root are the correctly rounded
// ones):
//   e = b - a, w = p - a, ee = ex ex + ey ey, t = clamp((wx ex + wy ey) / ee) or 0 when ee == 0,
//   c = a + t e, d = p - c, d2 = dx dx + dy dy
// seg = the j of the minimum d2, the lowest j on equal values, under the clearance kernel's replace rule from
// (+inf, -1): a NaN d2 passes no compare, so a segment with a non-finite end is never chosen and a non-finite
// pose keeps -1. Per pair the value depends on nothing else and the (value, index) minimum is associative and
// commutative: the result does not depend on which thread visits which segment.
//
// Mapping: clearance_kernel's. One 256-thread workgroup per car, striding over the cars; the car's rows in
// passes of kProgPoses. Per pass the first threads copy the poses' (x, y) into LDS, then the path is walked
// kProgThreads segments at a time, one segment per thread: the thread reads its two waypoints once (32 bytes,
// of which 16 are its neighbour's: the path is read from L2 whatever the layout, 8 KB at W = 500), forms e and
// ee once and tests every pose of the pass, (best, idx) per pose in registers. The pass ends with a
// lexicographic (d2, j) minimum over xor shuffles inside each wave and over the four waves' results in LDS:
// plain stores and a barrier, no atomic. Every loop bound is uniform over the workgroup, so whole waves reach
// every shuffle and barrier. The winner's t does not travel with it: thread p of the pass recomputes it from j
// in the same expressions (the same bits), with w and e, which the sign of lateral needs anyway. Carrying t
// would cost two more registers and a second conditional-move pair per pose in the inner loop, and two more
// shuffles per pose and step of the reduction; recomputing costs one divide per pose. No cull and no cap on W.
//
// standings_dist_kernel: one thread per car, the sums in row order (the order is part of the specification);
// s is read and dist, lap written [row][car], so a wave's accesses are contiguous. standings_rank_kernel: one
// thread per (row, car) counts the cars of its race ahead of it, walking the race's G values of its row.
#include <hip/hip_runtime.h>

#include <climits>

#include "f110qp_kernels.h"

namespace f110qp {

namespace {

constexpr int kProgThreads = 256;
constexpr int kProgWaves = kProgThreads / 64;
constexpr int kProgPoses = 8;  // poses (rows of one car) per pass
constexpr int kStandThreads = 256;

// (v, i) into (best, idx): contact_kernels.hip's update rule.
__device__ __forceinline__ void take_min(double& best, int& idx, const double v, const int i) {
  if (v < best || (v == best && i < idx)) {
    best = v;
    idx = i;
  }
}

// t of p on the segment from a along e (ee = e.e), clamped.
__device__ __forceinline__ double seg_t(const double wx, const double wy, const double ex, const double ey,
                                        const double ee) {
#pragma clang fp contract(off)
  if (ee == 0.0) return 0.0;
  const double t = (wx * ex + wy * ey) / ee;
  return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
}

__device__ __forceinline__ double wrap_len(const double v, const double L, const double half) {
#pragma clang fp contract(off)
  return v > half ? v - L : (v <= -half ? v + L : v);
}

}  // namespace

__global__ __launch_bounds__(kProgThreads) void progress_kernel(const int B, const int rows, const int nwg,
                                                                const int W, const double* __restrict__ x,
                                                                const double* __restrict__ wp,
                                                                const double* __restrict__ cum,
                                                                int* __restrict__ seg, double* __restrict__ s,
                                                                double* __restrict__ lateral) {
#pragma clang fp contract(off)
  __shared__ double s_px[kProgPoses], s_py[kProgPoses];
  __shared__ double s_best[kProgWaves][kProgPoses];
  __shared__ int s_idx[kProgWaves][kProgPoses];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int b = blockIdx.x; b < B; b += nwg) {
    for (int r0 = 0; r0 < rows; r0 += kProgPoses) {
      const int np = min(kProgPoses, rows - r0);
      if (tid < np) {
        const double* xp = x + ((size_t)(r0 + tid) * (size_t)B + (size_t)b) * 3;
        s_px[tid] = xp[0];
        s_py[tid] = xp[1];
      }
      __syncthreads();
      double best[kProgPoses];
      int idx[kProgPoses];
#pragma unroll
      for (int p = 0; p < kProgPoses; p++) {
        best[p] = inf;
        idx[p] = -1;
      }
      for (int j0 = 0; j0 < W; j0 += kProgThreads) {
        const int j = j0 + tid;
        if (j < W) {
          const int jn = j + 1 == W ? 0 : j + 1;
          const double ax = wp[(size_t)j * 2 + 0], ay = wp[(size_t)j * 2 + 1];
          const double ex = wp[(size_t)jn * 2 + 0] - ax, ey = wp[(size_t)jn * 2 + 1] - ay;
          const double ee = ex * ex + ey * ey;
#pragma unroll
          for (int p = 0; p < kProgPoses; p++) {
            if (p < np) {
              const double px = s_px[p], py = s_py[p];
              const double t = seg_t(px - ax, py - ay, ex, ey, ee);
              const double dx = px - (ax + t * ex), dy = py - (ay + t * ey);
              take_min(best[p], idx[p], dx * dx + dy * dy, j);
            }
          }
        }
      }
      // the wave's (d2, j) minimum per pose, then the four waves' through LDS
#pragma unroll
      for (int p = 0; p < kProgPoses; p++) {
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
        int j = s_idx[0][tid];
#pragma unroll
        for (int w = 1; w < kProgWaves; w++) take_min(v, j, s_best[w][tid], s_idx[w][tid]);
        double sv = nan, lat = nan;
        if (j >= 0) {  // the winner's t again, in the pass's expressions: the same bits
          const int jn = j + 1 == W ? 0 : j + 1;
          const double ax = wp[(size_t)j * 2 + 0], ay = wp[(size_t)j * 2 + 1];
          const double ex = wp[(size_t)jn * 2 + 0] - ax, ey = wp[(size_t)jn * 2 + 1] - ay;
          const double wx = s_px[tid] - ax, wy = s_py[tid] - ay;
          const double t = seg_t(wx, wy, ex, ey, ex * ex + ey * ey);
          const double c0 = cum[j];
          sv = c0 + t * (cum[j + 1] - c0);
          const double d = __dsqrt_rn(v);
          lat = ex * wy - ey * wx >= 0.0 ? d : -d;
        }
        const size_t o = (size_t)(r0 + tid) * (size_t)B + (size_t)b;
        if (seg) seg[o] = j;
        s[o] = sv;
        if (lateral) lateral[o] = lat;
      }
      __syncthreads();  // the next pass (or car) rewrites the poses and the waves' results
    }
  }
}

__global__ __launch_bounds__(kStandThreads) void standings_dist_kernel(const int G, const int B, const int rows,
                                                                       const double L,
                                                                       const double* __restrict__ s,
                                                                       double* __restrict__ dist,
                                                                       int* __restrict__ lap) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * kStandThreads + threadIdx.x;
  if (b >= B) return;
  const double half = 0.5 * L;
  const double s0 = s[b - b % G];
  double prev = s[b];
  double d = s0 + wrap_len(prev - s0, L, half);
  const double d0 = d;
  for (int r = 0;;) {
    const size_t o = (size_t)r * (size_t)B + (size_t)b;
    dist[o] = d;
    if (lap) lap[o] = d == d ? (int)floor((d - d0) / L) : INT_MIN;
    if (++r == rows) break;
    const double cur = s[(size_t)r * (size_t)B + (size_t)b];
    d = d + wrap_len(cur - prev, L, half);
    prev = cur;
  }
}

__global__ __launch_bounds__(kStandThreads) void standings_rank_kernel(const int G, const int B,
                                                                       const long long n,
                                                                       const double* __restrict__ dist,
                                                                       int* __restrict__ rank) {
  const long long o = (long long)blockIdx.x * kStandThreads + threadIdx.x;
  if (o >= n) return;
  const int b = (int)(o % B), own = b % G;
  const double* dr = dist + (o - own);  // the race's G values of this row
  const double d = dr[own];
  const bool num = d == d;
  int ahead = 0;
  for (int m = 0; m < G; m++) {
    const double dm = dr[m];
    // a NaN car is behind every car with a number; among NaN cars, and on equal values, the lower index leads
    const bool a = num ? (dm > d || (dm == d && m < own)) : (dm == dm || m < own);
    ahead += a ? 1 : 0;
  }
  rank[o] = ahead;
}

// Grid: one workgroup per car up to 1,024. The kernel holds 102 VGPRs (the code-object metadata, DESIGN.md
// 2i: the compiler keeps the eight poses' fp64 divides in flight together, which sets that figure, not the 24
// registers of the running minima), allocated as 104, so a SIMD keeps floor(512 / 104) = 4 of its waves; a
// workgroup is one wave on each of a CU's four SIMDs and 512 B of LDS, so a CU holds four workgroups and the
// MI355X's 256 CUs hold 1,024 at once: derived from the occupancy, as clearance_grid's 1,024 is, and not from
// a sweep of caps (none was measured).
constexpr int kProgMaxGrid = 1024;
int progress_grid(int B) { return B < kProgMaxGrid ? B : kProgMaxGrid; }

hipError_t launch_progress(int B, int rows, const double* x, const double* wp, const double* cum, int W, int* seg,
                           double* s, double* lateral, hipStream_t st) {
  if (B <= 0 || rows <= 0) return hipSuccess;
  const int nwg = progress_grid(B);
  hipLaunchKernelGGL(progress_kernel, dim3(nwg), dim3(kProgThreads), 0, st, B, rows, nwg, W, x, wp, cum, seg, s,
                     lateral);
  return hipGetLastError();
}

hipError_t launch_standings(int G, int B, int rows, const double* s, double L, double* dist, int* lap, int* rank,
                            hipStream_t st) {
  if (B <= 0 || rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(standings_dist_kernel, dim3((B + kStandThreads - 1) / kStandThreads), dim3(kStandThreads), 0,
                     st, G, B, rows, L, s, dist, lap);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long n = (long long)rows * B;
  hipLaunchKernelGGL(standings_rank_kernel, dim3((unsigned)((n + kStandThreads - 1) / kStandThreads)),
                     dim3(kStandThreads), 0, st, G, B, n, dist, rank);
  return hipGetLastError();
}

}  // namespace f110qp
