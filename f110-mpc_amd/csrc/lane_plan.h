// lane_plan.h — the lane back end's launch policy: everything that is decided about one box or
// screened call before its kernel is launched (segments, QPs per wave, twin starts, fixed-length
// variant, scratch placement, stored lam-gains, frame, fp64 references, grid, LDS bytes), decided once
// by lane_plan() into one LanePlan record. The launch (lane_launch.hip, lane_kernel.h,
// lane_seg_kernel.h), the completion signal (f110qp_kernels.hip) and the introspection calls of the
// ABI (f110qp_api.cpp) read that record; none of them re-derives a rule. The LDS-size functions of
// the kernels are here too, in their only copy. No device code: plain host C++ over KParams and
// LaneWork.
#pragma once
#include <stddef.h>

#include "f110qp_kernels.h"

namespace f110qp {

// waves the lane kernel's grid aims for (one per CU of the MI355X's 256)
constexpr int kLaneTargetWaves = 256;
// LDS of a CU
constexpr size_t kCuLdsBytes = 160 * 1024;

// LDS bytes per wave of the segmented kernel for horizon N split into S segments (rows for the
// longest segment, ceil(N / S) stages)
// FST: the scratch keeps the lam-gains F_i (6) instead of S_i^-1 (3): 14 doubles per stage
// F32: references and Riccati scratch held as float (the fp64 arithmetic is unchanged): 60 instead
// of 116 bytes per stage and lane, so 16,384 x N = 40 QPs per GPU fit at S = 4 (DESIGN.md 2b')
// + the per-wave tables of the active-state codes (kSegTabBytes: the backward sweep's bound values
// and free masks, the fp64-scratch forward sweep's re-guess thresholds, 16 codes x 8 doubles each)
constexpr size_t kSegTabBytes = 16 * 8 * 8;
constexpr size_t seg_lds_bytes(int N, int S, bool fst = false, bool f32 = false) {
  return (size_t)((N + S - 1) / S) * 64 * (3 * (f32 ? 4 : 8) + 4 + (fst ? 14 : 11) * (f32 ? 4 : 8)) +
         (f32 ? 1 : 2) * kSegTabBytes;
}

// The fixed-length kernels (lane_seg_kernel<..., Q > 0>: EVEN, FST, fp64 scratch, Q stages per segment)
// keep a lane's references, its PDAS state and all 14 per-stage values (K 6, k 2, the lam-gains F 6) in
// registers, so nothing per stage is left in LDS: the request is the two code tables and the pass loop
// reads LDS for table entries only (measured against 8 of the 14 in registers: DESIGN.md 2b'). The
// rules of lane_plan() below still count the run-time-length kernel's LDS. (The references are not
// staged: every lane loads its own 3 Q scalars from global memory.)
constexpr size_t seg_fixedq_lds_bytes(int /*Q*/) { return 2 * kSegTabBytes; }
// Their tables are a copy of the solver's constant block (LaneWork::seg_tab: btab [16][8] doubles, then
// ftab [16][8], the layout of the LDS copy), a function of KParams' bounds, input weights and u_des
// alone. launch_seg_tab_fill (lane_launch.hip) fills kSegBlockBytes of device memory at tab on stream
// s, one wave, from the functions the run-time-length kernels build their tables with (seg_tables.h);
// the caller orders it before the solver's first fixed-length launch.
constexpr size_t kSegBlockBytes = 2 * kSegTabBytes;
hipError_t launch_seg_tab_fill(const KParams& P, double* tab, hipStream_t s);

// LDS per wave of the sequential kernel (lane_kernel.h) at L QPs per wave: the staged references
// (12 N L B) + PDAS state (4 N L B), + the Riccati scratch (8 N L sizeof(ST)) when it is in LDS, + the
// references converted to fp64 (DREF: 12 N L more)
constexpr size_t lane_lds_base(int N, int L) { return (size_t)N * L * (12 + 4); }
constexpr size_t lane_lds_scratch(int N, int L, bool f32) {
  return (size_t)N * 8 * L * (f32 ? sizeof(float) : sizeof(double));
}
constexpr size_t lane_lds_dref(int N, int L) { return (size_t)N * L * 12; }

// What one call of the lane back end runs.
struct LanePlan {
  int S = 1;       // horizon segments per QP: 1 the sequential kernel (lane_kernel.h, one QP per lane
                   // group of 64 / L identical lanes), 2 / 4 / 8 lane_seg_kernel.h
  int qpw = 1;     // QPs per wave: L of the sequential kernel, 64 / S of the segmented one
  int starts = 1;  // PDAS starts per QP: 2 with the segmented kernel's twin start
  int Q = 0;       // segment length of the fixed-length segmented kernels (5), 0 the run-time-length ones
  int mode = 0;    // scratch. Sequential: 1 LDS fp64, 2 LDS fp32, 3 HBM fp64, 4 HBM fp32. Segmented: 1 LDS
                   // fp64, 2 LDS fp32 (references and scratch as float), 0 if neither fits
  bool fst = false;   // segmented: the lam-gains stored (no refresh sweep)
  bool rot = false;   // the heading-frame kernel (q0 == q1)
  bool dref = false;  // sequential: the references converted once to fp64 in LDS
  bool even = false;  // segmented: equal segments (N % S == 0)
  bool scr = false;   // segmented: the gap-row screen in the output sweep (f110qp_kernels.hip)
  int grid = 0;       // workgroups (one wave each)
  size_t lds = 0;     // dynamic LDS bytes per workgroup
};

// Horizon segments per QP (lane_seg_kernel.h). A batch whose waves leave SIMDs idle (the QPs fit
// in fewer than one wave per SIMD at 64 / S QPs per wave) splits every QP's horizon over S lanes
// instead of running 64 / L identical copies of it. S cuts N into segments of >= 2 stages (of
// floor(N / S) or one more), the grid stays within two waves per SIMD (2,048 waves) and a wave's
// segmented LDS fits the CU (fp64 references and scratch when the whole grid is resident with
// them, else float ones, possibly in more than one dispatch round: 16,384 x N = 40 runs S = 4 on
// fp32 scratch in one round, 32,768 x N = 40 in two, round 4). Among those the launch takes the S with the shortest per-pass chain by the
// instruction model of DESIGN.md 2b': sequential N x ~255 instructions, segmented ceil(N / S) x
// ~350 + the segment ends: at S = 8 (S - 1) x ~230 (the ring's two recursions), at S <= 4 ~140 +
// (S / 2 - 1) x ~260 (the two-sided elimination, from the ISA of the S = 2 / S = 4 kernels against
// their ring versions: operand and result selects ~75, the meet ~65 + 18 DPP moves, a full step ~195
// and a short one ~45 with their exchanges). The cheaper ends put S = 4 ahead of S = 8 at N = 21 ..
// 28 by 5 % of the modelled chain, which is inside the model's error and not measured: where the
// ring's constants chose S = 8, S = 8 stays. A forced QPs-per-wave or scratch placement keeps
// lane_kernel.h.
inline int lane_plan_segments(const KParams& P, int B, const LaneWork& lw) {
  const int N = P.N;
  // dispatch rounds of the segmented grid: waves per CU over the waves the CU's 160 KiB of LDS
  // holds at once (fp64 scratch when the whole grid is resident with it, else float); 0 = no fit
  // the cost multiplier is rounds x resident waves per SIMD (a second wave on a SIMD shares its
  // fp64 issue slots: the kernels are VALU-issue bound)
  auto rounds = [&](int S) -> int {
    if (N / S < 2) return 0;
    const size_t waves = ((size_t)B * S + 63) / 64;
    const size_t per_cu = (waves + 255) / 256;
    if (per_cu > 8) return 0;
    size_t resident = per_cu;
    if (per_cu * seg_lds_bytes(N, S) > kCuLdsBytes) {
      resident = kCuLdsBytes / seg_lds_bytes(N, S, false, true);
      if (resident < 1) return 0;
      if (resident > per_cu) resident = per_cu;
    }
    const size_t r = (per_cu + resident - 1) / resident;
    return (int)(r * ((resident + 3) / 4));
  };
  if (lw.seg == 1) return 1;
  if (lw.seg == 2 || lw.seg == 4 || lw.seg == 8) return rounds(lw.seg) > 0 ? lw.seg : 1;
  if (lw.qpw != 0 || (lw.mode != 0 && lw.mode != 1)) return 1;
  int best = 1, ring_best = 1;  // (ring_best: the choice under the ring's segment-end cost at every S)
  double cbest = 255.0 * N, cring = cbest;
  for (int S = 2; S <= 8; S <<= 1) {
    const int r = rounds(S);
    if (r == 0) continue;
    // per-pass chain x dispatch rounds (the sequential kernel keeps its grid resident: HBM scratch)
    const double stages = 350.0 * ((N + S - 1) / S);
    const double ends = S <= 4 ? 140.0 + 260.0 * (S / 2 - 1) : 230.0 * (S - 1);
    const double c = r * (stages + ends), cr = r * (stages + 230.0 * (S - 1));
    if (c < cbest) {
      best = S;
      cbest = c;
    }
    if (cr < cring) {
      ring_best = S;
      cring = cr;
    }
  }
  return ring_best == 8 ? 8 : best;
}

#ifndef F110QP_TWIN_MAX_WAVES
#define F110QP_TWIN_MAX_WAVES 512  // (measurement builds: tools/build_seg_variant.sh -D...)
#endif
constexpr long kTwinMaxWaves = F110QP_TWIN_MAX_WAVES;

// The plan of a call of B QPs: each decision once, in the order of the launch. scr: the call is the
// box solve of a screened gap-row call (it matters to the segmented kernel alone).
inline LanePlan lane_plan(const KParams& P, int B, const LaneWork& lw, bool scr) {
  LanePlan p;
  const int N = P.N;
  // the heading-frame variant when Q's (x, y) weights are equal (lane_kernel.h, ROT)
  p.rot = lw.rot && P.q[0] == P.q[1];
  p.S = lane_plan_segments(P, B, lw);
  if (p.S > 1) {
    const int S = p.S;
    p.qpw = 64 / S;
    p.scr = scr;
    // waves per CU of a grid of b QPs
    auto per_cu = [&](size_t b) { return ((b * S + 63) / 64 + 255) / 256; };
    // Scratch of the segmented kernel for a batch: 1 fp64 (the lam-gains kept when they fit), 2 fp32
    // (references and scratch as float) when fp64 does not fit the CU's 160 KiB at the grid's waves
    // per CU (the float grid may then take more than one dispatch round), or when forced (lw.seg32:
    // F110QP_LANE_SEG_F32=1); 0 if neither fits.
    auto scratch = [&](size_t b) {
      const bool f64 = per_cu(b) * seg_lds_bytes(N, S, false) <= kCuLdsBytes;
      const bool f32 = seg_lds_bytes(N, S, false, true) <= kCuLdsBytes;  // in one or more rounds
      if (lw.seg32 && f32) return 2;
      return f64 ? 1 : (f32 ? 2 : 0);
    };
    // the lam-gains stored (FST, no refresh sweep: measured C5 30.5 -> see DESIGN.md 2b') when the
    // resident waves' LDS holds 14 doubles per stage, else the refresh sweep (11); lw.dref = 0
    // forces the refresh (test hook, F110QP_LANE_DREF=0)
    auto stored = [&](size_t b) {
      return scratch(b) == 1 && lw.dref && per_cu(b) * seg_lds_bytes(N, S, true) <= kCuLdsBytes;
    };
    // Twin starts (lane_seg_kernel<..., TWIN = true>): each QP solved from the cold start and from the
    // speed bound u_des sits on held over the first half of the horizon, in adjacent slots of one wave.
    // Taken when u_des is on a speed bound (the shipped params.yaml:42,46: des_vel = umax), the doubled
    // grid is at most two waves per CU and the lam-gain (FST) scratch of those waves fits a CU's LDS:
    // C2 (1,024 QPs, 128 waves) 26.4 -> 23.4 us. C5 (4,096, 512 waves, two per CU) measured 28.8 ->
    // 30.9 while the segment ends went through ds_bpermute, and 28.95 -> 28.55 us (cold 28.84 -> 28.3)
    // with the DPP exchanges (same box; its slowest tick's passes 5 -> 4). lw.twin = 0 (test build,
    // F110QP_LANE_TWIN=0) turns it off.
    const bool twin = lw.twin && (P.udes[0] >= (double)P.umax[0] || P.udes[0] <= (double)P.umin[0]) &&
                      (2L * B * S + 63) / 64 <= kTwinMaxWaves &&
                      stored(2 * (size_t)B);  // the FST kernel, all waves resident
    p.starts = twin ? 2 : 1;
    const size_t slots = (size_t)B * p.starts;
    p.grid = (int)((slots + p.qpw - 1) / p.qpw);
    p.mode = scratch(slots);
    p.fst = stored(slots);
    p.even = N % S == 0;  // equal segments: the EVEN instantiation
    // Segment length of the fixed-length kernels a batch runs (lane_seg_kernel<..., Q = 5>), 0 for the
    // run-time-length ones: five-stage segments at S = 4 in the heading frame (C2, C5, the single-QP
    // tick at N = 20), exactly where the EVEN, FST, fp64 kernel would run without the gap-row screen.
    // The rules above are unchanged and still count that kernel's LDS; only the launch's request is
    // the smaller one. lw.fixedq = 0 (test build, F110QP_SEG_FIXEDQ=0) keeps the run-time-length
    // kernel.
    p.Q = (lw.fixedq && S == 4 && p.rot && !scr && N == 5 * S && p.fst) ? 5 : 0;
    p.lds = p.Q ? seg_fixedq_lds_bytes(p.Q) : seg_lds_bytes(N, S, p.fst, p.mode == 2);
    return p;
  }
  // QPs per wave: the smallest power of two (<= 64) that fits the batch in kLaneTargetWaves waves
  // (one per CU).
  int L = lw.qpw;
  if (!(L >= 1 && L <= 64 && (L & (L - 1)) == 0)) {
    L = 1;
    while (L < 64 && (B + L - 1) / L > kLaneTargetWaves) L <<= 1;
  }
  p.qpw = L;
  p.grid = (B + L - 1) / L;
  const size_t per_cu = ((size_t)p.grid + 255) / 256;
  // Scratch placement of the lane kernel for a batch (lane_mode 0 = auto; 1/2/3/4 force LDS fp64 /
  // LDS fp32 / HBM fp64 / HBM fp32): auto puts the scratch in LDS when every wave of the grid is
  // resident with it (waves per CU x its LDS within the CU's 160 KiB): fp64 if that fits, else
  // fp32; otherwise fp32 in the HBM workspace (the waves then stay resident on the 16 N L bytes of
  // references + state alone). With the state recentred on x0 the fp32 gains and trajectories stay
  // within ~1e-7 of the exact optimum (tests/test_gpu_parity.py::test_lane_backend_scratch_modes).
  const size_t base = lane_lds_base(N, L);
  const size_t lds64 = base + lane_lds_scratch(N, L, false), lds32 = base + lane_lds_scratch(N, L, true);
  p.mode = lw.mode;
  if (p.mode == 0) p.mode = per_cu * lds64 <= kCuLdsBytes ? 1 : per_cu * lds32 <= kCuLdsBytes ? 2 : 4;
  if (p.mode == 1 && lds64 > kCuLdsBytes) p.mode = 3;
  if (p.mode == 2 && lds32 > kCuLdsBytes) p.mode = 4;
  p.lds = p.mode == 1 ? lds64 : p.mode == 2 ? lds32 : base;
  // the references converted once to fp64 in LDS (DREF: 12 N L more bytes per wave than the float
  // references) when the grid runs one wave per CU. Measured: C4 shard 8,192 x N=40 195.8 ->
  // 184.6 us, C5 66.9 -> 65.3; at four waves per CU (65,536 x N=20) 107.0 -> 109.1, so not there.
  p.dref = lw.dref && per_cu == 1 && p.lds + lane_lds_dref(N, L) <= kCuLdsBytes;
  if (p.dref) p.lds += lane_lds_dref(N, L);
  return p;
}

}  // namespace f110qp
