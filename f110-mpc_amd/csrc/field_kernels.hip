// field_kernels.hip — the raster map's exact Euclidean distance transform, the map inflated by a radius and the
// field read at poses (f110qp_grid_distance_dev, f110qp_grid_inflate_dev, f110qp_grid_lookup_dev of
// include/f110qp.h, rules D1 to D4, which hold the model). The transform is integer arithmetic alone: with W and
// H at most 32,768 every squared cell distance is at most 2 x 32,767^2 < INT_MAX, which stays free as the mark
// of "no occupied cell". The two elementwise kernels touch doubles and keep FP contraction off, with the
// correctly rounded root and quotient (grid_geom.h's discipline).
//
// The transform is separable (rule D2), two launches with `work` [H][W] between them:
//   field_rows_kernel. work[j][i] = the column p of the occupied cell of row j nearest to i, the smaller p on a
//     tie, or -1 for a row without one. A wave per row, striding over the rows; the row in chunks of 64 cells, lane
//     l on cell 64 c + l, so a chunk's bytes are one 64-byte load. The ballot of "occupied" over the chunk is the
//     wave scan: the highest set bit at or below l is the last occupied cell to the left inside the chunk (the
//     max-scan of indices), the lowest at or above l the next to the right (the min-scan). What lies outside the
//     chunk comes in as a carry, which is uniform over the wave: the chunks run right to left with "the first
//     occupied cell of a later chunk" (pass A, which parks the right neighbour in work), then left to right with
//     "the last of an earlier chunk" (pass B, which reads the right neighbour back and writes the nearer). Lane l
//     reads in pass B only what lane l wrote in pass A: no thread reads another's store. A chunk past the row's end
//     has its lanes ballot 0 and store nothing, so a row shorter than a wave and a row that is no multiple of 64
//     take the same path.
//   field_cols_kernel. d2[j][i] = min over q of (i - work[q][i])^2 + (j - q)^2. One thread per cell, a workgroup
//     a tile of 64 columns by 4 rows: the lanes of a wave run along i, so every read work[q][i .. i + 63] is one
//     coalesced 256-byte row segment, and the four waves of a tile read nearly the same rows from L2. The search
//     walks outwards from q = j, four distances (eight rows) to a batch so that the batch's loads are in flight
//     together, and stops before a batch once its first distance d has d^2 > best: every candidate at distance
//     d' >= d is at least d'^2, so none of them can lower the minimum or tie it. Inside a batch no stop is needed
//     for exactness, the compare is total: (value, q) replaces (best, bq) when value < best, or value == best and
//     q < bq, which is rule D2's least q whatever the visiting order (a tie below j found after an equal candidate
//     above j replaces it). Within a row the p is the row pass's, so the result depends on nothing but the map.
//     The cost follows the distance, not H: a cell next to a wall reads a handful of rows. The price is a map, or a
//     column band, with no occupied cell anywhere near: its cells walk to the map's edge (H reads a cell).
//     No LDS, no barrier, no atomic.
// field_inflate_kernel: one thread per cell. field_lookup_kernel: one thread per pose, a grid-stride loop over
// rows x B (the grid cap below).
#include <hip/hip_runtime.h>

#include <climits>

#include "f110qp_kernels.h"

namespace f110qp {

namespace {

constexpr int kFieldThreads = 256;
constexpr int kFieldWaves = kFieldThreads / 64;
constexpr int kColsBatch = 4;  // distances per batch of the column walk: 2 x 4 row reads in flight

// Rule D3: metres from a squared cell distance.
__device__ __forceinline__ double field_metres(const int d2, const double res) {
#pragma clang fp contract(off)
  if (d2 == INT_MAX) return __longlong_as_double(0x7ff0000000000000ll);
  return res * __dsqrt_rn((double)d2);
}

// (v, q, p) into (best, bq, bp): rule D2 down a column.
__device__ __forceinline__ void take_cell(int& best, int& bq, int& bp, const int i, const int j, const int q,
                                          const int p) {
  if (p < 0) return;
  const int dx = i - p, dy = j - q, v = dx * dx + dy * dy;
  if (v < best || (v == best && q < bq)) {
    best = v;
    bq = q;
    bp = p;
  }
}

}  // namespace

__global__ __launch_bounds__(kFieldThreads) void field_rows_kernel(const int W, const int H, const int nwaves,
                                                                   const unsigned char* __restrict__ grid,
                                                                   int* __restrict__ work) {
  typedef unsigned long long u64;
  const int lane = threadIdx.x & 63;
  const int nchunks = (W + 63) >> 6;
  for (int j = blockIdx.x * kFieldWaves + (threadIdx.x >> 6); j < H; j += nwaves) {
    const unsigned char* row = grid + (size_t)j * (size_t)W;
    int* out = work + (size_t)j * (size_t)W;
    int carry = -1;  // pass A: the first occupied cell of the chunks to the right
    for (int c = nchunks - 1; c >= 0; c--) {
      const int i = (c << 6) + lane;
      const bool in = i < W;
      const u64 mask = __ballot(in && row[i] != 0);
      const u64 at_right = mask >> lane;
      if (in) out[i] = at_right ? i + (int)__builtin_ctzll(at_right) : carry;
      if (mask) carry = (c << 6) + (int)__builtin_ctzll(mask);
    }
    carry = -1;  // pass B: the last occupied cell of the chunks to the left
    for (int c = 0; c < nchunks; c++) {
      const int i = (c << 6) + lane;
      const bool in = i < W;
      const u64 mask = __ballot(in && row[i] != 0);
      const u64 at_left = mask & (~0ull >> (63 - lane));
      const int l = at_left ? (c << 6) + 63 - (int)__builtin_clzll(at_left) : carry;
      if (in) {
        const int r = out[i];
        // the nearer of the two, the left one (the smaller p) on a tie; -1 when the row has neither
        out[i] = (r < 0 || (l >= 0 && i - l <= r - i)) ? l : r;
      }
      if (mask) carry = (c << 6) + 63 - (int)__builtin_clzll(mask);
    }
  }
}

__global__ __launch_bounds__(kFieldThreads) void field_cols_kernel(const int W, const int H, const int tiles_x,
                                                                   const int* __restrict__ work,
                                                                   int* __restrict__ d2, int* __restrict__ nearest) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i = (tx << 6) + (threadIdx.x & 63), j = ty * kFieldWaves + (threadIdx.x >> 6);
  if (i >= W || j >= H) return;
  const int* col = work + i;
  int best = INT_MAX, bq = -1, bp = -1;
  take_cell(best, bq, bp, i, j, j, col[(size_t)j * (size_t)W]);
  const int far = max(j, H - 1 - j);  // the last distance with a row of the map on either side
  for (int d = 1; d <= far && d * d <= best; d += kColsBatch) {
    int pa[kColsBatch], pb[kColsBatch];
#pragma unroll
    for (int k = 0; k < kColsBatch; k++) {
      const int qa = j - d - k, qb = j + d + k;
      pa[k] = qa >= 0 ? col[(size_t)qa * (size_t)W] : -1;
      pb[k] = qb < H ? col[(size_t)qb * (size_t)W] : -1;
    }
#pragma unroll
    for (int k = 0; k < kColsBatch; k++) {
      take_cell(best, bq, bp, i, j, j - d - k, pa[k]);
      take_cell(best, bq, bp, i, j, j + d + k, pb[k]);
    }
  }
  const size_t o = (size_t)j * (size_t)W + (size_t)i;
  d2[o] = best;
  if (nearest) nearest[o] = bq < 0 ? -1 : bq * W + bp;
}

__global__ __launch_bounds__(kFieldThreads) void field_inflate_kernel(const int n, const double res,
                                                                      const double radius,
                                                                      const int* __restrict__ d2,
                                                                      unsigned char* __restrict__ out) {
  const int o = blockIdx.x * kFieldThreads + threadIdx.x;
  if (o >= n) return;
  out[o] = field_metres(d2[o], res) <= radius ? 1 : 0;
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(kFieldThreads) void field_lookup_kernel(const GridParams G, const long long n,
                                                                     const long long stride,
                                                                     const int* __restrict__ d2,
                                                                     const int* __restrict__ nearest,
                                                                     const double* __restrict__ x,
                                                                     double* __restrict__ dist,
                                                                     int* __restrict__ cell) {
  for (long long o = (long long)blockIdx.x * kFieldThreads + threadIdx.x; o < n; o += stride) {
    const double px = (x[3 * o + 0] - G.ox) / G.res, py = (x[3 * o + 1] - G.oy) / G.res;
    double v = __longlong_as_double(0x7ff8000000000000ll);
    int c = -1;
    // floor(p) in [0, W) is 0 <= p < W, which a NaN or an infinity fails (grid_geom.h's grid_start)
    if (px >= 0.0 && px < (double)G.W && py >= 0.0 && py < (double)G.H) {
      const size_t k = (size_t)(int)floor(py) * (size_t)G.W + (size_t)(int)floor(px);
      v = field_metres(d2[k], G.res);
      if (cell) c = nearest[k];
    }
    dist[o] = v;
    if (cell) cell[o] = c;
  }
}

// Grids (the figures are the code-object metadata; no cap comes from a sweep). Each of the four
// kernels holds fewer than 64 VGPRs, no LDS and no scratch, so a SIMD keeps its full 8 waves, a CU 32 waves =
// 8 workgroups of 256 threads, and the MI355X's 256 CUs 2,048 workgroups at once: the cap of the two kernels that
// stride (the rows, 4 rows a workgroup; the lookup, 256 poses a workgroup). The columns and the inflation are one
// thread per cell: at most 2^30 cells, 4,194,304 workgroups.
constexpr int kFieldMaxGrid = 2048;

int field_rows_grid(int H) {
  const int wgs = (H + kFieldWaves - 1) / kFieldWaves;
  return wgs < kFieldMaxGrid ? wgs : kFieldMaxGrid;
}

int field_lookup_grid(long long n) {
  const long long wgs = (n + kFieldThreads - 1) / kFieldThreads;
  return (int)(wgs < kFieldMaxGrid ? wgs : kFieldMaxGrid);
}

hipError_t launch_grid_distance(int W, int H, const unsigned char* grid, int* d2, int* nearest, int* work,
                                hipStream_t st) {
  if (W <= 0 || H <= 0) return hipSuccess;
  const int nwg = field_rows_grid(H);
  hipLaunchKernelGGL(field_rows_kernel, dim3(nwg), dim3(kFieldThreads), 0, st, W, H, nwg * kFieldWaves, grid, work);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int tiles_x = (W + 63) >> 6, tiles_y = (H + kFieldWaves - 1) / kFieldWaves;
  hipLaunchKernelGGL(field_cols_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(kFieldThreads), 0, st, W, H,
                     tiles_x, work, d2, nearest);
  return hipGetLastError();
}

hipError_t launch_grid_inflate(int W, int H, double res, const int* d2, double radius, unsigned char* out,
                               hipStream_t st) {
  if (W <= 0 || H <= 0) return hipSuccess;
  const int n = W * H;
  hipLaunchKernelGGL(field_inflate_kernel, dim3((unsigned)((n + kFieldThreads - 1) / kFieldThreads)),
                     dim3(kFieldThreads), 0, st, n, res, radius, d2, out);
  return hipGetLastError();
}

hipError_t launch_grid_lookup(const GridParams& G, const int* d2, const int* nearest, int B, int rows,
                              const double* x, double* dist, int* cell, hipStream_t st) {
  if (B <= 0 || rows <= 0) return hipSuccess;
  const long long n = (long long)rows * B;
  const int nwg = field_lookup_grid(n);
  hipLaunchKernelGGL(field_lookup_kernel, dim3(nwg), dim3(kFieldThreads), 0, st, G, n,
                     (long long)nwg * kFieldThreads, d2, nearest, x, dist, cell);
  return hipGetLastError();
}

}  // namespace f110qp
