// mc_kernels.hip — what a Monte Carlo batch came to: the quantile fan of every sample set at every row, the
// survival counts and every car's record (f110qp_mc_fan_dev, f110qp_mc_survival_dev, f110qp_mc_outcomes_dev and
// f110qp_mc_summary of include/f110qp.h, which holds the model). Every result is a selection or a count: no
// arithmetic touches a value, so there is nothing to round and no contraction to switch off, apart from the one
// product prob * (n - 1) that picks a position.
//
// The fan. A work item is one (row, set): M values of v [rows][B] at stride G from (s M G + g), s = k / G,
// g = k % G. A value's 64 bits u become the key ~u (sign set) or u | 1 << 63, whose unsigned order is the total
// order of the model; a NaN and every padding slot get the key 0xFFFFFFFFFFFFFFFF, which no number maps to (it
// would be the NaN 0x7FFF...F). The keys are sorted ascending on the length P = M padded to a power of two, so
// the first n entries are the samples; n is counted at the load (a ballot, or a sum), never read off the sort.
// A quantile is the key at floor(prob * (n - 1)) turned back into its bits.
//
// Two paths by P, both with loop bounds that are uniform over the wave (the workgroup on the second path), so
// whole waves reach every shuffle and barrier:
//   fan_wave_kernel, P <= 64. 64 / P sets per wave, one key per lane, the items of a wave consecutive. A bitonic
//     network over xor shuffles: log2 P (log2 P + 1) / 2 compare-exchange steps, each two 32-bit shuffles and a
//     64-bit select. No LDS, no barrier. The waves stride over the groups of 64 / P items.
//   fan_lds_kernel, 64 < P <= 4,096. One 256-thread workgroup per item, striding over the items; the keys in LDS
//     (8 P bytes of a static 32 KB), one barrier per compare-exchange step (78 at P = 4,096), each thread P / 512
//     pairs per step. A step's pairs are (i, i + j) with i = 2 t - (t & (j - 1)): at j = 1 the lanes' 8-byte
//     reads are 16 bytes apart, a two-way bank conflict on the 64-bank row; from j = 32 on a half wave reads 32
//     consecutive keys and there is none. The sort is not the cost at the sizes measured: the
//     strided loads are.
// Layout. The members of a set are G doubles apart. At G = 1 the wave path's 64 lanes read 64 consecutive
// doubles (the sets of a wave are neighbours in memory as long as M is P; with M < P the padding lanes load
// nothing) and the LDS path's 256 threads read 2 KB at a time: both coalesce fully. At G > 1 a lane's 8 bytes
// sit in a 64-byte line of which the G - 1 race-mates' sets use the rest: the g of a race are consecutive
// items, so on the wave path with P <= 32 the same wave picks them up, and otherwise the next wave or workgroup
// finds the line in L2. The loads favour G = 1; the layout is the rollout's, which this family does not get to
// choose.
//
// mc_survival_kernel: one thread per (row, set) counts the members still running; the threads of row 0 count the
// crashed ones as well. crash_tick is B ints, read T + 1 times over, from L2. mc_outcomes_kernel: one thread per
// car walks the rows in order; every array is [row][car], so a wave's loads are contiguous.
#include <hip/hip_runtime.h>

#include "f110qp.h"
#include "f110qp_kernels.h"

namespace f110qp {

namespace {

typedef unsigned long long u64;

constexpr int kMcThreads = 256;
constexpr int kMcWaves = kMcThreads / 64;
constexpr u64 kPadKey = 0xFFFFFFFFFFFFFFFFull;
constexpr u64 kSign = 0x8000000000000000ull;
constexpr u64 kNanBits = 0x7ff8000000000000ull;

__device__ __forceinline__ u64 key_of(const u64 u) {
  if ((u & ~kSign) > 0x7ff0000000000000ull) return kPadKey;  // a NaN, either sign, any payload
  return (u & kSign) ? ~u : (u | kSign);
}

__device__ __forceinline__ u64 bits_of(const u64 key) { return (key & kSign) ? (key ^ kSign) : ~key; }

// The position of quantile p among n >= 1 samples: one rounded product, then floor.
__device__ __forceinline__ int quantile_pos(const double p, const int n) {
#pragma clang fp contract(off)
  return (int)floor(p * (double)(n - 1));
}

__device__ __forceinline__ u64 shfl_xor64(const u64 v, const int m) {
  const int lo = __shfl_xor((int)(unsigned)v, m, 64), hi = __shfl_xor((int)(unsigned)(v >> 32), m, 64);
  return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}

__device__ __forceinline__ u64 shfl64(const u64 v, const int src) {
  const int lo = __shfl((int)(unsigned)v, src, 64), hi = __shfl((int)(unsigned)(v >> 32), src, 64);
  return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}

// The first member of item's set in v, and whether the item exists.
__device__ __forceinline__ size_t set_base(const long long item, const int K, const int M, const int G, const int B) {
  const long long r = item / K;
  const int k = (int)(item - r * K);
  const int s = k / G, g = k - s * G;
  return (size_t)r * (size_t)B + (size_t)s * (size_t)M * (size_t)G + (size_t)g;
}

}  // namespace

struct McProbs {
  int Q;
  double p[F110QP_MC_MAX_PROBS];
};

__global__ __launch_bounds__(kMcThreads) void fan_wave_kernel(const int M, const int P, const int G, const int B,
                                                              const int K, const long long items,
                                                              const long long groups, const int nwaves,
                                                              const McProbs pr, const u64* __restrict__ v,
                                                              u64* __restrict__ fan, int* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int spw = 64 / P;            // sets per wave
  const int sub = lane / P, j = lane - sub * P;
  const u64 gmask = (P == 64 ? ~0ull : ((1ull << P) - 1ull)) << (sub * P);
  for (long long grp = (long long)blockIdx.x * kMcWaves + (threadIdx.x >> 6); grp < groups; grp += nwaves) {
    const long long item = grp * spw + sub;
    const bool live = item < items;
    u64 key = kPadKey;
    if (live && j < M) key = key_of(v[set_base(item, K, M, G, B) + (size_t)j * (size_t)G]);
    const int n = __popcll(__ballot(key != kPadKey) & gmask);
    // bitonic network on the P lanes of the set: after it lane j of the set holds the key of position j
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
      for (int d = k2 >> 1; d >= 1; d >>= 1) {
        const u64 other = shfl_xor64(key, d);
        const bool up = (j & k2) == 0, low = (j & d) == 0;  // j < P: the last merge runs upwards in every set
        const u64 mn = key < other ? key : other, mx = key < other ? other : key;
        key = (up == low) ? mn : mx;
      }
    }
    for (int q = 0; q < pr.Q; q++) {
      const int pos = n > 0 ? quantile_pos(pr.p[q], n) : 0;
      const u64 kq = shfl64(key, sub * P + pos);
      if (live && j == (q & (P - 1))) fan[(size_t)item * (size_t)pr.Q + (size_t)q] = n > 0 ? bits_of(kq) : kNanBits;
    }
    if (count && live && j == 0) count[item] = n;
  }
}

__global__ __launch_bounds__(kMcThreads) void fan_lds_kernel(const int M, const int P, const int G, const int B,
                                                             const int K, const long long items, const int nwg,
                                                             const McProbs pr, const u64* __restrict__ v,
                                                             u64* __restrict__ fan, int* __restrict__ count) {
  __shared__ u64 s_key[F110QP_MC_MAX_HYPOTHESES];
  __shared__ int s_n[kMcWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long long item = blockIdx.x; item < items; item += nwg) {
    const u64* vs = v + set_base(item, K, M, G, B);
    int mine = 0;
    for (int i = tid; i < P; i += kMcThreads) {
      const u64 key = i < M ? key_of(vs[(size_t)i * (size_t)G]) : kPadKey;
      mine += key != kPadKey ? 1 : 0;
      s_key[i] = key;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
    if (lane == 0) s_n[wave] = mine;
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int w = 0; w < kMcWaves; w++) n += s_n[w];
    const int half = P >> 1;
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
      for (int d = k2 >> 1; d >= 1; d >>= 1) {
        for (int t = tid; t < half; t += kMcThreads) {
          const int i = 2 * t - (t & (d - 1));
          const u64 a = s_key[i], b = s_key[i + d];
          const bool up = (i & k2) == 0;
          if ((a > b) == up) {
            s_key[i] = b;
            s_key[i + d] = a;
          }
        }
        __syncthreads();
      }
    }
    if (tid < pr.Q)
      fan[(size_t)item * (size_t)pr.Q + (size_t)tid] = n > 0 ? bits_of(s_key[quantile_pos(pr.p[tid], n)]) : kNanBits;
    if (count && tid == 0) count[item] = n;
    __syncthreads();  // the next item rewrites the keys and the waves' counts
  }
}

__global__ __launch_bounds__(kMcThreads) void mc_survival_kernel(const int M, const int G, const int K, const int T,
                                                                 const long long n, const int* __restrict__ crash,
                                                                 int* __restrict__ alive, int* __restrict__ crashed) {
  const long long o = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (o >= n) return;
  const int r = (int)(o / K), k = (int)(o - (long long)r * K);
  const int s = k / G, g = k - s * G;
  const int* c = crash + (size_t)s * (size_t)M * (size_t)G + (size_t)g;
  int up = 0, hit = 0;
#pragma unroll 8  // the loads do not depend on each other: eight in flight
  for (int m = 0; m < M; m++) {
    const int ct = c[(size_t)m * (size_t)G];
    up += (ct < 0 || ct > r) ? 1 : 0;
    hit += (ct >= 0 && ct <= T) ? 1 : 0;
  }
  alive[o] = up;
  if (crashed && r == 0) crashed[k] = hit;
}

__global__ __launch_bounds__(kMcThreads) void mc_outcomes_kernel(
    const int B, const int T, const double* __restrict__ clear, const int* __restrict__ status,
    const int* __restrict__ kind, double* __restrict__ min_clear, int* __restrict__ min_row,
    int* __restrict__ unsolved, int* __restrict__ first_unsolved, int* __restrict__ plan_failed) {
  const int b = blockIdx.x * kMcThreads + threadIdx.x;
  if (b >= B) return;
  double best = __longlong_as_double(0x7ff0000000000000ll);
  int idx = -1;
#pragma unroll 8  // eight rows' loads in flight; the compares stay in row order
  for (int r = 0; r <= T; r++) {  // rows ascend: a later row replaces only when it is smaller
    const double c = clear[(size_t)r * (size_t)B + (size_t)b];
    if (c < best) {
      best = c;
      idx = r;
    }
  }
  min_clear[b] = best;
  if (min_row) min_row[b] = idx;
  if (!status && !kind) return;
  int bad = 0, first = -1, failed = 0;
#pragma unroll 8
  for (int t = 0; t < T; t++) {
    const size_t o = (size_t)t * (size_t)B + (size_t)b;
    const int kd = kind ? kind[o] : F110QP_TICK_MPC;
    failed += kd == F110QP_TICK_PLAN_FAILED ? 1 : 0;
    if (status && kd == F110QP_TICK_MPC) {
      const int st = status[o];
      if (st != F110QP_SOLVED && st != F110QP_SOLVED_INACCURATE) {
        if (first < 0) first = t;
        bad++;
      }
    }
  }
  if (unsolved) unsolved[b] = bad;
  if (first_unsolved) first_unsolved[b] = first;
  if (plan_failed) plan_failed[b] = failed;
}

// Grids (the figures are the code-object metadata; neither cap comes from a sweep).
// fan_wave_kernel holds 31 VGPRs and no LDS: at 64 registers or fewer a SIMD keeps its full 8 waves, a CU
// 32 waves = 8 workgroups of 256 threads, and the MI355X's 256 CUs 2,048 workgroups at once.
// fan_lds_kernel holds 35 VGPRs and 32,784 B of LDS (the keys and the four waves' counts):
// floor(163,840 / 32,784) = 4 workgroups per CU (the registers would allow 8), 1,024 on the device.
constexpr int kFanWaveMaxGrid = 2048;
constexpr int kFanLdsMaxGrid = 1024;

int mc_fan_padded(int M) {
  int P = 1;
  while (P < M) P <<= 1;
  return P;
}

int mc_fan_grid(int M, long long items) {
  const int P = mc_fan_padded(M);
  if (P <= 64) {
    const long long groups = (items + 64 / P - 1) / (64 / P), wgs = (groups + kMcWaves - 1) / kMcWaves;
    return (int)(wgs < kFanWaveMaxGrid ? wgs : kFanWaveMaxGrid);
  }
  return (int)(items < kFanLdsMaxGrid ? items : kFanLdsMaxGrid);
}

hipError_t launch_mc_fan(int M, int G, int Q, const double* prob, int B, int rows, const double* v, double* fan,
                         int* count, hipStream_t st) {
  if (B <= 0 || rows <= 0) return hipSuccess;
  McProbs pr;
  pr.Q = Q;
  for (int q = 0; q < F110QP_MC_MAX_PROBS; q++) pr.p[q] = q < Q ? prob[q] : 0.0;
  const int K = B / M, P = mc_fan_padded(M);
  const long long items = (long long)rows * K;
  const int nwg = mc_fan_grid(M, items);
  if (P <= 64) {
    const long long groups = (items + 64 / P - 1) / (64 / P);
    hipLaunchKernelGGL(fan_wave_kernel, dim3(nwg), dim3(kMcThreads), 0, st, M, P, G, B, K, items, groups,
                       nwg * kMcWaves, pr, (const u64*)v, (u64*)fan, count);
  } else {
    hipLaunchKernelGGL(fan_lds_kernel, dim3(nwg), dim3(kMcThreads), 0, st, M, P, G, B, K, items, nwg, pr,
                       (const u64*)v, (u64*)fan, count);
  }
  return hipGetLastError();
}

hipError_t launch_mc_survival(int M, int G, int B, int T, const int* crash_tick, int* alive, int* crashed,
                              hipStream_t st) {
  if (B <= 0 || T <= 0) return hipSuccess;
  const int K = B / M;
  const long long n = (long long)(T + 1) * K;
  hipLaunchKernelGGL(mc_survival_kernel, dim3((unsigned)((n + kMcThreads - 1) / kMcThreads)), dim3(kMcThreads), 0, st,
                     M, G, K, T, n, crash_tick, alive, crashed);
  return hipGetLastError();
}

hipError_t launch_mc_outcomes(int B, int T, const double* clear, const int* status, const int* kind,
                              double* min_clear, int* min_row, int* unsolved, int* first_unsolved, int* plan_failed,
                              hipStream_t st) {
  if (B <= 0 || T <= 0) return hipSuccess;
  hipLaunchKernelGGL(mc_outcomes_kernel, dim3((B + kMcThreads - 1) / kMcThreads), dim3(kMcThreads), 0, st, B, T,
                     clear, status, kind, min_clear, min_row, unsolved, first_unsolved, plan_failed);
  return hipGetLastError();
}

}  // namespace f110qp
