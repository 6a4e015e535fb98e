// lane_seg_body.h — the body of the segmented lane kernel, included once into each of its two entries
// (lane_seg_kernel.h): lane_seg_kernel (Q == 0, the run-time-length code) and lane_seg_kernel_q
// (Q > 0), which alone has ctab, the solver's constant block of the two code tables (seg_tables.h), as
// a kernel argument. The text reads the entry's parameters and template parameters by name; no include
// guard, it is not a header of declarations.
  constexpr int twin = TWIN ? 1 : 0;
  constexpr int L = 64 / S;  // QPs per wave
  // the kernel arguments the staging address needs, in SGPRs before anything else: hipcc loads
  // kernel arguments next to their first use, which put two dependent kernarg round trips in
  // front of the staging loads
  // Q > 0: a compile-time segment length, m = mM = q = Q (the launcher's choice). The stage loops unroll
  // fully, the lane's references, PDAS state (one packed word, 4 bits per stage) and a stage's 14
  // values (gr[t][e]: K 0 .. 5, k 6 .. 7, the lam-gains F 8 .. 13) live in registers from the backward
  // sweep to the output sweep; LDS holds the two code tables and nothing per stage. Q == 0: the
  // run-time-length code, references, state and scratch in LDS.
  static_assert(Q == 0 || (EVEN && ROT && FST && !SCR && sizeof(ST) == 8),
                "fixed segment length: EVEN, heading frame, lam-gains stored, fp64 scratch, no screen");
  // Q == 0: scratch doubles per stage: K 6, k 2, then F 6 or S^-1 3
  constexpr int NV = FST ? 14 : 11;
  extern __shared__ __attribute__((aligned(16))) double seg_smem[];
  const int lane = threadIdx.x;
  const int sl = lane / S;         // QP slot of the wave
  const int seg = lane & (S - 1);  // segment: the QP's S segments are S consecutive lanes
  // twin = 1: every QP is solved from two PDAS starts at once, adjacent slots 2b (cold) and 2b + 1
  // (the speed bound nearest u_des active on the first half of the horizon); the QP is done when
  // either start has converged, and the converged one (the cold one on a tie) writes the outputs.
  // Both end at the same exact optimum; the pass count is the smaller one (launch_lane_seg_t)
  const int b0 = blockIdx.x * L;                 // first (virtual) QP of the wave
  const int VB = B << twin;
  const int nq = (VB - b0) < L ? (VB - b0) : L;
  // a missing QP's lanes duplicate QP 0 of the wave (twin: the start of the same parity, so that a
  // duplicate's sibling lane is a duplicate of its sibling start)
  const int slot = sl < nq ? sl : (sl & twin);
  const bool owner0 = sl < nq;         // stores the outputs of its segment's stages ...
  const bool qowner0 = owner0 && seg == 0;
  const int vq = b0 + slot;
  const bool var = (vq & twin) != 0;   // ... if its start is the one that converged (owner below)
  const int b = vq >> twin;
  const int N = P.N;
  // segments of q or q + 1 stages (the first N mod S ones longer); LDS rows for the longest
  // EVEN (S divides N, the launcher's choice): every segment has q stages, so the stage loops run
  // on a wave-uniform count (scalar loop control and LDS strides instead of per-lane ones)
  const int q = Q > 0 ? Q : N / S, rem = EVEN ? 0 : N - q * S;
  const int m = EVEN ? q : q + (seg < rem ? 1 : 0);
  const int s0 = EVEN ? seg * q : seg * q + (seg < rem ? seg : rem);
  const int mM = EVEN ? q : q + (rem > 0 ? 1 : 0);
  const bool top = seg == S - 1;

  STAMP(t_start);
#ifdef F110QP_STAMPS
  unsigned long long acc_bw = 0, acc_dual = 0, acc_ref = 0, acc_fw = 0, t_setup = 0, npass = 0;
  unsigned long long t_out_loop = 0;  // the output sweep's stage loop
#endif
  constexpr bool F32 = sizeof(ST) == 4;
  char* const lbase = reinterpret_cast<char*>(seg_smem);
  const size_t o_ap = Q > 0 ? 0 : (size_t)3 * mM * 64 * sizeof(ST), o_sc = Q > 0 ? 0 : o_ap + (size_t)mM * 64 * 4;
  ST* const r64 = reinterpret_cast<ST*>(lbase) + lane;                     // [3mM][64]
  int* const ap = reinterpret_cast<int*>(lbase + o_ap) + lane;             // [mM][64]
  ST* const sc = reinterpret_cast<ST*>(lbase + o_sc) + lane;               // [mM][NV][64]
  // code tables (wave-uniform base; a lane reads the entry of its own stage's state code)
  double* const btab = reinterpret_cast<double*>(lbase + o_sc + (Q > 0 ? 0 : (size_t)mM * NV * 64 * sizeof(ST)));
  double* const ftab = btab + 16 * 8;  // (ST = double only)

  // per-QP inputs and the warm-start traffic switch (warm_traffic), issued before the staging loads
  const IN fX0 = x0g[3 * b + 0], fY0 = x0g[3 * b + 1], fTH0 = x0g[3 * b + 2];
  const IN fv = ulg[2 * b + 0], fd = ulg[2 * b + 1];
  const unsigned wlast = warm_last_hit(ws);
  // ---- stage the wave's reference paths (IN, [3N][L]) into the scratch region ----
  // (room: (3 N LR + 64) sizeof(IN) bytes, junk row included, at most 24 N 64 / S + 512 for doubles,
  // in a region of mM NV 64 sizeof(ST) >= 44 (N / S) 64 bytes: fits whenever N / S >= 2, which
  // lane_plan_segments requires of every S it returns)
  // Element e = q 3N + c of the wave's nq rows (row stride 3 xr_stride in HBM) goes to
  // stg[c L + q]. (q, c) advance by 64 elements per step without a division, every load reads a
  // valid address (clamped) and every store lands (past the staged rows for e >= tot), so the
  // loop has no EXEC-masked region: ~11 instructions per element instead of ~50 (ISA).
  // (Issuing chunk 0 first and the linearisation under its loads measured no gain: C2 23.4 against
  // 23.1 us, C5 30.9 against 30.4, same box.) Twin starts: row q of the wave is QP (b0 >> 1) + q.
  // Twin starts: the two starts of a QP share its row, staged once ([3N][L / 2] QP rows)
  constexpr int LR = L >> twin;
  // Q > 0: no staging. A lane's 3 Q reference scalars are one contiguous run of its QP's row
  // (elements 3 s0 .. 3 s0 + 3 Q - 1, row stride 3 xr_stride), loaded straight into registers next
  // to x0 and u_lin: a QP's S lanes read 12 Q S contiguous bytes, twin siblings the same addresses,
  // and the lanes of a missing QP those of the valid slot they duplicate. Neither LDS round trip
  // nor the barriers on both sides of it remain.
  IN fr[Q > 0 ? 3 * Q : 1];
  // Q > 0: the lane's 32 B of the solver's 2 KiB constant block (btab, then ftab), in the same round
  // trip; an L2 hit for every wave after the first
  double2 ct0 = make_double2(0.0, 0.0), ct1 = ct0;
  if constexpr (Q > 0) {
    ct0 = reinterpret_cast<const double2*>(ctab)[2 * lane];
    ct1 = reinterpret_cast<const double2*>(ctab)[2 * lane + 1];
    const IN* xrow = xrg + (size_t)b * (3 * (size_t)P.xr_stride) + 3 * s0;
#pragma unroll
    for (int e = 0; e < 3 * Q; e++) fr[e] = xrow[e];
  } else {
    IN* stg = reinterpret_cast<IN*>(lbase + o_sc);
    const int nqr = (nq + twin) >> twin;  // QP rows of the wave (b0 is even with twin starts)
    const int n3 = 3 * N, S3 = 3 * P.xr_stride, tot = nqr * n3;
    const int rb0 = b0 >> twin;
    const IN* src = xrg + (size_t)rb0 * S3;
    const int dq = 64 / n3, dc = 64 - dq * n3;
    int q = lane / n3, c = lane - (lane / n3) * n3;
    const int junk = n3 * LR + lane;                 // inside the scratch rows, never read
    const int last_off = (nqr - 1) * S3 + (n3 - 1);  // a valid element
    // C5 and the C4 shard stage 960 floats per wave, the twin kernels 480: one round trip
    // (doubles: half the elements per chunk, the same bytes in flight and registers held)
    constexpr int kChunk = (TWIN ? 8 : 16) / (int)(sizeof(IN) / 4);
    for (int e0 = 0; e0 < tot; e0 += kChunk * 64) {
      IN vbuf[kChunk];
      int dst[kChunk];
#pragma unroll
      for (int j = 0; j < kChunk; j++) {
        const bool in = e0 + j * 64 + lane < tot;
        dst[j] = in ? c * LR + q : junk;
        vbuf[j] = src[in ? q * S3 + c : last_off];
        q += dq;
        c += dc;
        const bool wrap = c >= n3;
        c -= wrap ? n3 : 0;
        q += wrap ? 1 : 0;
      }
#pragma unroll
      for (int j = 0; j < kChunk; j++) stg[dst[j]] = vbuf[j];
    }
    __syncthreads();
  }
  // the warm-start key, when this call moves warm traffic (its round trip overlaps the staging)
  const bool wt = warm_traffic(ws, wlast);
  unsigned key0 = 0u, key1 = 0u, key2 = 0u, key3 = 0u;
  uint2 wst = make_uint2(0u, 0u);  // this wave's warm counters (f110qp_warm_hits), updated at the end
  if (wt) {
    if (ws.stats) wst = *reinterpret_cast<const uint2*>(ws.stats + 2 * (size_t)blockIdx.x);
    const uint4 k4 = *reinterpret_cast<const uint4*>(ws.key + 4 * (size_t)b);
    key0 = k4.x; key1 = k4.y; key2 = k4.z; key3 = k4.w;
  }

  STAMP(t_stg);
  // ---- per-lane QP data (Model::Linearize, model.cpp:30-59: lane_linearize, linearize.h) ----
  const double X0 = (double)fX0, Y0 = (double)fY0;
  const double th0 = (double)fTH0;
  const double v = (double)fv, d = (double)fd;
  const double dt = (double)P.dt;
  const LaneModel M = lane_linearize<ROT>(th0, v, d, dt);
  const double sn = M.sn, cs = M.cs, a02 = M.a02, a12 = M.a12, b00 = M.b00, b10 = M.b10, b20 = M.b20;
  const double b21 = M.b21, c0 = M.c0, c1 = M.c1, c2 = M.c2;
  const double q0 = P.q[0], q1 = P.q[1], q2 = P.q[2], r0 = P.r[0], r1 = P.r[1];
  const double ud0 = P.udes[0], ud1 = P.udes[1];
  const double lb0 = (double)P.umin[0], lb1 = (double)P.umin[1];
  const double ub0 = (double)P.umax[0], ub1 = (double)P.umax[1];
  // PDAS flip tolerances of lane_kernel.h: fp64 scratch 1e-10 (scaled) in every pass; fp32
  // scratch (gains rounded to ~1e-7) exact compares in the PDAS passes and 1e-6 / 1e-5 in the
  // single-flip passes, where a degenerate bound then settles
  const double ptT = F32 ? 0.0 : 1e-10, gtT = F32 ? 0.0 : 1e-10;
  const double ptL = F32 ? 1e-6 : 1e-10, gtL = F32 ? 1e-5 : 1e-10;
  const double lbe0 = lb0 - ptT * (1.0 + fabs(lb0)), ube0 = ub0 + ptT * (1.0 + fabs(ub0));
  const double lbe1 = lb1 - ptT * (1.0 + fabs(lb1)), ube1 = ub1 + ptT * (1.0 + fabs(ub1));
  const double gtol0 = gtT * (1.0 + r0 * bound_scale(lb0, ub0, ud0));
  const double gtol1 = gtT * (1.0 + r1 * bound_scale(lb1, ub1, ud1));
  const double lbl0 = lb0 - ptL * (1.0 + fabs(lb0)), ubl0 = ub0 + ptL * (1.0 + fabs(ub0));
  const double lbl1 = lb1 - ptL * (1.0 + fabs(lb1)), ubl1 = ub1 + ptL * (1.0 + fabs(ub1));
  const double gtoll0 = gtL * (1.0 + r0 * bound_scale(lb0, ub0, ud0));
  const double gtoll1 = gtL * (1.0 + r1 * bound_scale(lb1, ub1, ud1));

  STAMP(t_lin);
  // references of the lane's stages: recentred (ROT: rotated) fp64, lane-major; a non-finite
  // entry flags the QP (one ballot folded over its segment lanes)
  // (the loop runs to the wave-uniform mM: a lane of a shorter segment converts one stage of the
  // next segment, or of the staging's junk rows on the top segment, into a row it never reads, so
  // the loop has no EXEC-masked exits; its flag only counts stages < m)
  bool nonfin = false;
  // Q > 0: the references, the packed state codes (stage t at bits 4t .. 4t + 3) and the gains kept
  // in registers (constant indices only: every loop over them is fully unrolled)
  double rr[Q > 0 ? 3 * Q : 1];
  double gr[Q > 0 ? Q : 1][Q > 0 ? 14 : 1];
  unsigned apk = 0u;
  {
    const IN* stg = reinterpret_cast<const IN*>(lbase + o_sc);
    const int row = slot >> twin;
    if constexpr (Q > 0) {
#pragma unroll
      for (int t = 0; t < Q; t++) {
        const IN fx = fr[3 * t + 0], fy = fr[3 * t + 1], ft = fr[3 * t + 2];
        nonfin |= !(isfinite(fx) && isfinite(fy) && isfinite(ft));
        const double dx = (double)fx - X0, dy = (double)fy - Y0;
        rr[3 * t + 0] = ROT ? cs * dx + sn * dy : dx;
        rr[3 * t + 1] = ROT ? cs * dy - sn * dx : dy;
        rr[3 * t + 2] = (double)ft - th0;
      }
    } else
    for (int t = 0; t < mM; t++) {
      const int i = s0 + t;
      const IN fx = stg[(3 * i + 0) * LR + row], fy = stg[(3 * i + 1) * LR + row];
      const IN ft = stg[(3 * i + 2) * LR + row];
      nonfin |= (t < m) & !(isfinite(fx) && isfinite(fy) && isfinite(ft));
      const double dx = (double)fx - X0, dy = (double)fy - Y0;
      r64[(3 * t + 0) * 64] = ROT ? cs * dx + sn * dy : dx;
      r64[(3 * t + 1) * 64] = ROT ? cs * dy - sn * dx : dy;
      r64[(3 * t + 2) * 64] = (double)ft - th0;
    }
    // the active-state code tables: code c holds input a's state (c >> 2a) & 3 (0 free, 1 lower,
    // 2 upper). btab[c] = (bA0, bA1, fm0, fm1, 1 - fm0, 1 - fm1, fm0 fm1, 0): the fixed inputs'
    // bound values and the free masks of the masked 2 x 2 solve (products with 0 / 1 instead of
    // ~20 selects per backward stage; the first four are read a stage ahead). ftab[c] = per input
    // (lo, hi, fm, 1 - fm), the forward sweep's re-guess tests y = fm u - (1 - fm) g against y < lo
    // (lower) and y > hi (upper): free: y = u in (lbe, ube); at the lower bound: y = -g, stays while
    // -g < gtol; at the upper: y = -g, stays while -g > -gtol (fp64 scratch: one set of tolerances for
    // both pass kinds). Q > 0: a copy of the solver's constant block, 32 B per lane (seg_tables.h
    // fills it by these expressions); Q == 0: lanes 0 .. 15 build one code's rows each
    if constexpr (Q > 0) {
      reinterpret_cast<double2*>(btab)[2 * lane] = ct0;
      reinterpret_cast<double2*>(btab)[2 * lane + 1] = ct1;
    } else if (lane < 16) {
      const int cA = lane & 3, cB = (lane >> 2) & 3;
      const double fA = cA == 0 ? 1.0 : 0.0, fB = cB == 0 ? 1.0 : 0.0;
      double* e = btab + 8 * lane;
      e[0] = cA == 0 ? 0.0 : (cA == 1 ? lb0 : ub0);
      e[1] = cB == 0 ? 0.0 : (cB == 1 ? lb1 : ub1);
      e[2] = fA; e[3] = fB; e[4] = 1.0 - fA; e[5] = 1.0 - fB; e[6] = fA * fB; e[7] = 0.0;
      if constexpr (!F32) {
        const double inf = __builtin_inf();
        double* f = ftab + 8 * lane;
        f[0] = cA == 0 ? lbe0 : (cA == 1 ? gtol0 : -inf); f[1] = cA == 0 ? ube0 : (cA == 2 ? -gtol0 : inf);
        f[2] = fA; f[3] = 1.0 - fA;
        f[4] = cB == 0 ? lbe1 : (cB == 1 ? gtol1 : -inf); f[5] = cB == 0 ? ube1 : (cB == 2 ? -gtol1 : inf);
        f[6] = fB; f[7] = 1.0 - fB;
      }
    }
    __syncthreads();  // the staging region becomes the Riccati scratch
  }
  STAMP(t_conv);
  // terminal reference x_ref[N-1] (mpc.cpp:228): the last stage of the top segment
  constexpr int kQL = Q > 0 ? 3 * (Q - 1) : 0;  // (Q > 0: the register copy)
  double rNx, rNy, rNt;
  if constexpr (Q > 0) {
    rNx = __shfl(rr[kQL + 0], lane | (S - 1));
    rNy = __shfl(rr[kQL + 1], lane | (S - 1));
    rNt = __shfl(rr[kQL + 2], lane | (S - 1));
  } else {
    rNx = __shfl(r64[(3 * (m - 1) + 0) * 64], lane | (S - 1));
    rNy = __shfl(r64[(3 * (m - 1) + 1) * 64], lane | (S - 1));
    rNt = __shfl(r64[(3 * (m - 1) + 2) * 64], lane | (S - 1));
  }
  STAMP(t_rn);

  // warm start: previous tick's active bounds when the slot's (theta0, v, steer) bits repeat
  const int R = (2 * N + 63) / 64;
  // (IN = double: the *_dbl calls pass no warm state, wt is false; the slot key holds float bits)
  const unsigned kth = __float_as_uint((float)fTH0), kv = __float_as_uint((float)fv), kd = __float_as_uint((float)fd);
  {
    // (seeding from the slot's previous set on any key measured C5 31.2 -> 34.9 us: a stale set costs passes)
    const bool hit = sizeof(IN) == 4 && wt && key3 != 0u && key0 == kth && key1 == kv && key2 == kd;
    unsigned long long lw = 0, hw = 0;
    if (wt) {  // (wave-uniform: a call that moves no warm state skips the mask window)
      if (ws.hit_call && __ballot(hit) != 0ull && lane == 0) *ws.hit_call = ws.call;
      wst.x += (unsigned)__popcll(__ballot(hit && qowner0 && !var));  // hits (one lane per QP)
      unsigned long long lo0 = 0, lo1 = 0, hi0 = 0, hi1 = 0;
      if (hit) {
        lo0 = ws.act[2 * R * b];
        hi0 = ws.act[2 * R * b + 1];
        if (R > 1) {
          lo1 = ws.act[2 * (R * b + 1)];
          hi1 = ws.act[2 * (R * b + 1) + 1];
        }
      }
      // the lane's 2m mask bits start at bit 2 s0 of the 128-bit pair (hi word : lo word)
      const int sh = 2 * s0;
      auto window = [&](unsigned long long w0, unsigned long long w1) {
        return sh >= 64 ? (w1 >> (sh - 64)) : (sh == 0 ? w0 : ((w0 >> sh) | (w1 << (64 - sh))));
      };
      lw = window(lo0, lo1);
      hw = window(hi0, hi1);
    }
    // the twin start: the speed bound u_des sits on, active on the first half of the horizon (on
    // the C2 / C5 workloads the optimum holds the speed on its upper bound over a prefix of the
    // horizon that cold PDAS finds a few stages per pass: numpy model of the kernel's PDAS, the
    // slowest QP's passes 4-5 -> 3-4 over eight C2 batches and six C5 ticks; launch_lane_seg_t
    // enables it only when u_des is on a speed bound)
    const int sv = ud0 >= ub0 ? 2 : (ud0 <= lb0 ? 1 : 0);
    const bool tw = var && !hit;
    // per input: 1 lower, 2 upper, 0 free; the lower bound wins. To the wave-uniform mM (rows
    // t >= m of a shorter segment are never read): no EXEC-masked loop exits
    if constexpr (Q > 0) {
      if (wt) {
#pragma unroll
        for (int t = 0; t < Q; t++) {
          const unsigned a = pdas_code((unsigned)(lw >> (2 * t)), (unsigned)(hw >> (2 * t)));
          apk |= ((tw && 2 * (s0 + t) < N) ? (unsigned)sv : a) << (4 * t);
        }
      } else {
        // a call that moves no warm state (wave-uniform): every code is the twin rule's, sv on the
        // lane's stages t with 2 (s0 + t) < N, that is its first nb = (N + 1) / 2 - s0 (clamped to
        // 0 .. Q), and free elsewhere; one nibble per stage
        const int nh = (N + 1) / 2 - s0;
        const int nb = nh < 0 ? 0 : (nh > Q ? Q : nh);
        apk = tw ? (unsigned)sv * (0x11111111u & ((1u << (4 * nb)) - 1u)) : 0u;
      }
    } else
    for (int t = 0; t < mM; t++) {
      const int a = (int)pdas_code((unsigned)(lw >> (2 * t)), (unsigned)(hw >> (2 * t)));
      ap[t * 64] = (tw && 2 * (s0 + t) < N) ? sv : a;
    }
  }
  STAMP(t_mask);

  // whether any of the lane's QP's S lanes has its bit set in a ballot
  auto qany = [&](unsigned long long mk) { return ((mk >> (sl * S)) & ((1ull << S) - 1ull)) != 0ull; };
  const bool bad = !(isfinite(X0) && isfinite(Y0) && isfinite(th0) && isfinite(v) && isfinite(d)) ||
                   qany(__ballot(nonfin));
  bool done = bad;
  int iters = 0;
  // the segment's start state and terminal multiplier lam_j of the current pass (kept for the
  // output sweep)
  double xs0 = 0.0, xs1 = 0.0, xs2 = 0.0, lm0 = 0.0, lm1 = 0.0, lm2 = 0.0;


  const int max_pass = P.pass_cap > 0 ? P.pass_cap : (P.max_iter > kmax ? P.max_iter : kmax);
  // Q > 0: the register gains are not initialised: the first backward sweep writes every one before
  // anything reads them. Only a wave that runs no pass (no budget, or every QP non-finite) reaches
  // the output sweep without them; it has no solved lane, and its sweep (ran == false, wave-uniform)
  // stores the NaNs without reading a gain
  bool ran = false;
#ifdef F110QP_STAMPS
  t_setup = __builtin_amdgcn_s_memtime() - t_start;
#endif
  for (int pass = 0; pass < max_pass; pass++) {
    // a QP is finished when one of its starts is (twin: the sibling start is S lanes over). The
    // shuffle runs on every lane: under a short-circuit || the done lanes are off in EXEC, and a
    // permute reads nothing from an inactive source lane
    if constexpr (TWIN) {
      const int sib = __shfl_xor((int)done, S, 64);
      if (__ballot(!(done || sib != 0)) == 0ull) break;
    } else {
      if (__ballot(!done) == 0ull) break;
    }
    const bool single = pass >= kmax;
    if constexpr (Q > 0) ran = true;
#ifdef F110QP_STAMPS
    npass++;
#endif
    STAMP(t_bw);
    // ---- 1. backward over the segment: Riccati + the closed-loop map (Phi, psi, Gam) ----
    double P00 = top ? q0 : 0.0, P01 = 0.0, P02 = 0.0, P11 = top ? q1 : 0.0, P12 = 0.0;
    double P22 = top ? q2 : 0.0;
    double p0 = top ? -q0 * rNx : 0.0, p1 = top ? -q1 * rNy : 0.0, p2 = top ? -q2 * rNt : 0.0;
    double F00 = 1.0, F01 = 0.0, F02 = 0.0, F10 = 0.0, F11 = 1.0, F12 = 0.0, F20 = 0.0, F21 = 0.0;
    double F22 = 1.0;  // Phi
    double s0v = 0.0, s1v = 0.0, s2v = 0.0;  // psi
    double G00 = 0.0, G01 = 0.0, G02 = 0.0, G11 = 0.0, G12 = 0.0, G22 = 0.0;  // Gam (symmetric)
    {
      int nst = Q > 0 ? (int)((apk >> (4 * (m - 1))) & 15u) : ap[(m - 1) * 64];
      // the next stage's code-table entry (bA0, bA1, fm0, fm1), read one stage ahead: the masked
      // solve needs it right after H, which the previous stage's P already gives
      double nb0 = btab[8 * nst], nb1 = btab[8 * nst + 1], nf0 = btab[8 * nst + 2], nf1 = btab[8 * nst + 3];
      double rx = Q > 0 ? rr[kQL + 0] : r64[(3 * (m - 1) + 0) * 64], ry = Q > 0 ? rr[kQL + 1] : r64[(3 * (m - 1) + 1) * 64];
      double rt = Q > 0 ? rr[kQL + 2] : r64[(3 * (m - 1) + 2) * 64];
      constexpr int kBwUnroll = Q > 0 ? Q : F110QP_SEG_BW_UNROLL;  // (Q > 0: the whole segment)
#pragma unroll kBwUnroll
      for (int t = m - 1; t >= 0; t--) {
        ST* s = sc + t * NV * 64;
        const double bA0 = nb0, bA1 = nb1, fm0 = nf0, fm1 = nf1;
        const int tn = t > 0 ? t - 1 : 0;
        nst = Q > 0 ? (int)((apk >> (4 * tn)) & 15u) : ap[tn * 64];
        const double rxi = rx, ryi = ry, rti = rt;
        rx = Q > 0 ? rr[3 * tn + 0] : r64[(3 * tn + 0) * 64];
        ry = Q > 0 ? rr[3 * tn + 1] : r64[(3 * tn + 1) * 64];
        rt = Q > 0 ? rr[3 * tn + 2] : r64[(3 * tn + 2) * 64];
        const double g0 = ROT ? P02 * c2 + p0 : P00 * c0 + P01 * c1 + P02 * c2 + p0;
        const double g1 = ROT ? P12 * c2 + p1 : P01 * c0 + P11 * c1 + P12 * c2 + p1;
        const double g2 = ROT ? P22 * c2 + p2 : P02 * c0 + P12 * c1 + P22 * c2 + p2;
        const double pb0 = ROT ? P00 * b00 + P02 * b20 : P00 * b00 + P01 * b10 + P02 * b20;
        const double pb1 = ROT ? P01 * b00 + P12 * b20 : P01 * b00 + P11 * b10 + P12 * b20;
        const double pb2 = ROT ? P02 * b00 + P22 * b20 : P02 * b00 + P12 * b10 + P22 * b20;
        const double pc0 = P02 * b21, pc1 = P12 * b21, pc2 = P22 * b21;
        const double H00 = ROT ? r0 + b00 * pb0 + b20 * pb2 : r0 + b00 * pb0 + b10 * pb1 + b20 * pb2;
        const double H01 = b21 * pb2;
        const double H11 = r1 + b21 * pc2;
        const double X00 = pb0, X01 = pb1;
        const double X02 = ROT ? pb2 + a12 * pb1 : pb2 + a02 * pb0 + a12 * pb1;
        const double X10 = pc0, X11 = pc1;
        const double X12 = ROT ? pc2 + a12 * pc1 : pc2 + a02 * pc0 + a12 * pc1;
        const double h0 = ROT ? -r0 * ud0 + b00 * g0 + b20 * g2
                              : -r0 * ud0 + b00 * g0 + b10 * g1 + b20 * g2;
        const double h1 = -r1 * ud1 + b21 * g2;
        const double e0 = ROT ? P02 + a12 * P01 : P02 + a02 * P00 + a12 * P01;
        const double e1 = ROT ? P12 + a12 * P11 : P12 + a02 * P01 + a12 * P11;
        const double e2 = ROT ? P22 + a12 * P12 : P22 + a02 * P02 + a12 * P12;
        const double Y00 = q0 + P00, Y01 = P01, Y11 = q1 + P11, Y02 = e0, Y12 = e1;
        const double Y22 = ROT ? q2 + e2 + a12 * e1 : q2 + e2 + a02 * e0 + a12 * e1;
        const double hx0 = -q0 * rxi + g0, hx1 = -q1 * ryi + g1;
        const double hx2 = ROT ? g2 - q2 * rti + a12 * g1 : g2 - q2 * rti + a02 * g0 + a12 * g1;
        // the stage's masked 2 x 2 solve from its code's table entry: M = the free block of H with
        // ones on the fixed diagonal, S^-1 rows of the fixed inputs zero (exact: products with 0 / 1)
        {
          const double* tb = btab + 8 * nst;
          nb0 = tb[0]; nb1 = tb[1]; nf0 = tb[2]; nf1 = tb[3];
        }
        const double om0 = 1.0 - fm0, om1 = 1.0 - fm1, fm01 = fm0 * fm1;
        const double M00 = fm0 * H00 + om0, M11 = fm1 * H11 + om1, M01 = fm01 * H01;
        const double det = M00 * M11 - M01 * M01;
        double idet = __builtin_amdgcn_rcp(det);
#pragma unroll
        for (int nt = 0; nt < F110QP_SEG_NEWTON; nt++) idet = fma(idet, fma(-det, idet, 1.0), idet);
        const double I00 = fm0 * (M11 * idet), I11 = fm1 * (M00 * idet);
        const double I01 = -M01 * idet;
        const double K00 = -I00 * X00 - I01 * X10, K01 = -I00 * X01 - I01 * X11;
        const double K02 = -I00 * X02 - I01 * X12;
        const double K10 = -I01 * X00 - I11 * X10, K11 = -I01 * X01 - I11 * X11;
        const double K12 = -I01 * X02 - I11 * X12;
        const double w0 = h0 + H00 * bA0 + H01 * bA1, w1 = h1 + H01 * bA0 + H11 * bA1;
        const double k0 = bA0 - I00 * w0 - I01 * w1, k1 = bA1 - I01 * w0 - I11 * w1;
        if constexpr (Q > 0) {
          gr[t][0] = K00; gr[t][1] = K01; gr[t][2] = K02; gr[t][3] = K10; gr[t][4] = K11;
          gr[t][5] = K12; gr[t][6] = k0; gr[t][7] = k1;
        } else {
          s[0] = K00; s[64] = K01; s[2 * 64] = K02; s[3 * 64] = K10; s[4 * 64] = K11;
          s[5 * 64] = K12; s[6 * 64] = k0; s[7 * 64] = k1;
        }
        if constexpr (!FST) {
          s[8 * 64] = I00; s[9 * 64] = I01; s[10 * 64] = I11;
        }
        P00 = Y00 + X00 * K00 + X10 * K10;
        P01 = Y01 + X00 * K01 + X10 * K11;
        P02 = Y02 + X00 * K02 + X10 * K12;
        P11 = Y11 + X01 * K01 + X11 * K11;
        P12 = Y12 + X01 * K02 + X11 * K12;
        P22 = Y22 + X02 * K02 + X12 * K12;
        p0 = hx0 + X00 * k0 + X10 * k1;
        p1 = hx1 + X01 * k0 + X11 * k1;
        p2 = hx2 + X02 * k0 + X12 * k1;
        // closed-loop map of the segment (Phi = Phi_{i+1} on entry)
        const double W00 = ROT ? F00 * b00 + F02 * b20 : F00 * b00 + F01 * b10 + F02 * b20;  // Phi B
        const double W10 = ROT ? F10 * b00 + F12 * b20 : F10 * b00 + F11 * b10 + F12 * b20;
        const double W20 = ROT ? F20 * b00 + F22 * b20 : F20 * b00 + F21 * b10 + F22 * b20;
        const double W01 = F02 * b21, W11 = F12 * b21, W21 = F22 * b21;
        // lam-gain of u_i: Fl = -S^-1 W'
        // (written as -a b - c d: the negation folds into the fma's source modifiers, where
        // -(a b + c d) cost a v_xor per entry)
        const double L00 = -I00 * W00 - I01 * W01, L01 = -I00 * W10 - I01 * W11;
        const double L02 = -I00 * W20 - I01 * W21;
        const double L10 = -I01 * W00 - I11 * W01, L11 = -I01 * W10 - I11 * W11;
        const double L12 = -I01 * W20 - I11 * W21;
        if constexpr (Q > 0) {
          gr[t][8] = L00; gr[t][9] = L01; gr[t][10] = L02;
          gr[t][11] = L10; gr[t][12] = L11; gr[t][13] = L12;
        } else if constexpr (FST) {
          s[8 * 64] = L00; s[9 * 64] = L01; s[10 * 64] = L02;
          s[11 * 64] = L10; s[12 * 64] = L11; s[13 * 64] = L12;
        }
        // The accumulations below are written acc + a b + c d (left to right: a chain of FMAs on the
        // accumulator), where acc += a b + c d compiled to a multiply, an FMA and an add
        // psi += W k + Phi C
        s0v = ROT ? s0v + W00 * k0 + W01 * k1 + F02 * c2
                  : s0v + W00 * k0 + W01 * k1 + F00 * c0 + F01 * c1 + F02 * c2;
        s1v = ROT ? s1v + W10 * k0 + W11 * k1 + F12 * c2
                  : s1v + W10 * k0 + W11 * k1 + F10 * c0 + F11 * c1 + F12 * c2;
        s2v = ROT ? s2v + W20 * k0 + W21 * k1 + F22 * c2
                  : s2v + W20 * k0 + W21 * k1 + F20 * c0 + F21 * c1 + F22 * c2;
        // Gam += W Fl
        G00 = G00 + W00 * L00 + W01 * L10;
        G01 = G01 + W00 * L01 + W01 * L11;
        G02 = G02 + W00 * L02 + W01 * L12;
        G11 = G11 + W10 * L01 + W11 * L11;
        G12 = G12 + W10 * L02 + W11 * L12;
        G22 = G22 + W20 * L02 + W21 * L12;
        // Phi = Phi A + W K  (A = I + E, E = a02 e_0 e_2' + a12 e_1 e_2')
        const double n02 = (ROT ? F02 + a12 * F01 : F02 + a02 * F00 + a12 * F01) + W00 * K02 + W01 * K12;
        const double n12 = (ROT ? F12 + a12 * F11 : F12 + a02 * F10 + a12 * F11) + W10 * K02 + W11 * K12;
        const double n22 = (ROT ? F22 + a12 * F21 : F22 + a02 * F20 + a12 * F21) + W20 * K02 + W21 * K12;
        F00 = F00 + W00 * K00 + W01 * K10; F01 = F01 + W00 * K01 + W01 * K11;
        F10 = F10 + W10 * K00 + W11 * K10; F11 = F11 + W10 * K01 + W11 * K11;
        F20 = F20 + W20 * K00 + W21 * K10; F21 = F21 + W20 * K01 + W21 * K11;
        F02 = n02; F12 = n12; F22 = n22;
      }
    }
    STAMP_ACC(acc_bw, t_bw);
    STAMP(t_dual);
    // ---- 2. the segment ends: the boundary problem over the segments, eliminated from both ends ----
    // S <= 4: the lower half of a QP's lanes (x_s^(0) = 0 below) and the upper half (the true terminal
    // cost on top) eliminate towards the middle in lockstep, S / 2 - 1 full steps each, and meet in
    // one 3 x 3 vector solve; S / 2 - 1 short steps per side then hand (x_s, lam) outwards. The lower
    // side's recursion x_j = alpha_{j-1} + beta_{j-1} lam_{j-1}, (alpha, beta)_0 = (psi, Gam)_0, is the
    // upper side's step with the operands exchanged,
    //   (Mn, mn, Gam, Phi, psi, P, a) <- (beta_{j-1}, alpha_{j-1}, P_j, Phi_j', a_j, Gam_j, psi_j),
    // so both halves run one instruction stream on operand copies selected once per pass (the
    // forward sweep still needs the lane's own P, a and Phi). beta stays symmetric negative
    // semidefinite and M positive semidefinite: I - beta P, I - M Gam and the meet's I - beta M have
    // eigenvalues >= 1. S = 8 keeps the one-sided ring: the top segment's (Phi, psi, Gam) zeroed so
    // that its lane hands (P, a) up the chain and x_e = 0 round the ring, S - 1 steps each way.
    // (tests/diag_seg_ends_model.py: both against a dense solve of the boundary system)
    lm0 = lm1 = lm2 = 0.0;
    xs0 = xs1 = xs2 = 0.0;
    if constexpr (S > 1) {
      constexpr bool TWO = S <= 4;
      const bool low = TWO && seg < S / 2;
      if constexpr (!TWO) {
        if (top) {
          F00 = F01 = F02 = F10 = F11 = F12 = F20 = F21 = F22 = 0.0;
          s0v = s1v = s2v = 0.0;
          G00 = G01 = G02 = G11 = G12 = G22 = 0.0;
        }
      }
      // the step's operands: the lane's own, exchanged on the lower side (Phi' is a renaming)
      const double gG00 = low ? P00 : G00, gG01 = low ? P01 : G01, gG02 = low ? P02 : G02;
      const double gG11 = low ? P11 : G11, gG12 = low ? P12 : G12, gG22 = low ? P22 : G22;
      const double gF00 = F00, gF11 = F11, gF22 = F22;
      const double gF01 = low ? F10 : F01, gF10 = low ? F01 : F10, gF02 = low ? F20 : F02;
      const double gF20 = low ? F02 : F20, gF12 = low ? F21 : F12, gF21 = low ? F12 : F21;
      const double gs0 = low ? p0 : s0v, gs1 = low ? p1 : s1v, gs2 = low ? p2 : s2v;
      const double gP00 = low ? G00 : P00, gP01 = low ? G01 : P01, gP02 = low ? G02 : P02;
      const double gP11 = low ? G11 : P11, gP12 = low ? G12 : P12, gP22 = low ? G22 : P22;
      const double gp0 = low ? s0v : p0, gp1 = low ? s1v : p1, gp2 = low ? s2v : p2;
      // what the lane hands on: (M, m) upwards, (beta, alpha) on the lower side; before any step
      // the top segment's (P, a) and segment 0's (Gam, psi)
      double M00 = gP00, M01 = gP01, M02 = gP02, M11 = gP11, M12 = gP12, M22 = gP22;
      double m0 = gp0, m1 = gp1, m2 = gp2;
      double T00 = 0, T01 = 0, T02 = 0, T10 = 0, T11 = 0, T12 = 0, T20 = 0, T21 = 0, T22 = 0;
      double t0 = 0, t1 = 0, t2 = 0;
      // one full elimination step with the neighbour's (Mn, mn): T, t and the lane's new (M, m)
      auto step = [&](double N00, double N01, double N02, double N11, double N12, double N22, double n0,
                      double n1, double n2) {
        // Z = I - Mn Gam (the diagonal as FMA chains on the 1)
        const double Z00 = 1.0 - N00 * gG00 - N01 * gG01 - N02 * gG02;
        const double Z01 = -(N00 * gG01 + N01 * gG11 + N02 * gG12);
        const double Z02 = -(N00 * gG02 + N01 * gG12 + N02 * gG22);
        const double Z10 = -(N01 * gG00 + N11 * gG01 + N12 * gG02);
        const double Z11 = 1.0 - N01 * gG01 - N11 * gG11 - N12 * gG12;
        const double Z12 = -(N01 * gG02 + N11 * gG12 + N12 * gG22);
        const double Z20 = -(N02 * gG00 + N12 * gG01 + N22 * gG02);
        const double Z21 = -(N02 * gG01 + N12 * gG11 + N22 * gG12);
        const double Z22 = 1.0 - N02 * gG02 - N12 * gG12 - N22 * gG22;
        // Z^-1 by the adjugate
        const double A00 = Z11 * Z22 - Z12 * Z21, A01 = Z02 * Z21 - Z01 * Z22, A02 = Z01 * Z12 - Z02 * Z11;
        const double A10 = Z12 * Z20 - Z10 * Z22, A11 = Z00 * Z22 - Z02 * Z20, A12 = Z02 * Z10 - Z00 * Z12;
        const double A20 = Z10 * Z21 - Z11 * Z20, A21 = Z01 * Z20 - Z00 * Z21, A22 = Z00 * Z11 - Z01 * Z10;
        const double zdet = Z00 * A00 + Z01 * A10 + Z02 * A20;
        double iz = __builtin_amdgcn_rcp(zdet);
        iz = fma(iz, fma(-zdet, iz, 1.0), iz);
        iz = fma(iz, fma(-zdet, iz, 1.0), iz);
        // Y = Z^-1 Mn is symmetric ((I - N G)^-1 N = N (I - G N)^-1 for symmetric N, G): six
        // entries, then T = Y Phi and t = Y psi + Z^-1 mn (15 fewer fp64 operations per step than
        // T = Z^-1 (Mn Phi))
        const double Y00 = iz * (A00 * N00 + A01 * N01 + A02 * N02);
        const double Y01 = iz * (A00 * N01 + A01 * N11 + A02 * N12);
        const double Y02 = iz * (A00 * N02 + A01 * N12 + A02 * N22);
        const double Y11 = iz * (A10 * N01 + A11 * N11 + A12 * N12);
        const double Y12 = iz * (A10 * N02 + A11 * N12 + A12 * N22);
        const double Y22 = iz * (A20 * N02 + A21 * N12 + A22 * N22);
        T00 = Y00 * gF00 + Y01 * gF10 + Y02 * gF20; T01 = Y00 * gF01 + Y01 * gF11 + Y02 * gF21;
        T02 = Y00 * gF02 + Y01 * gF12 + Y02 * gF22;
        T10 = Y01 * gF00 + Y11 * gF10 + Y12 * gF20; T11 = Y01 * gF01 + Y11 * gF11 + Y12 * gF21;
        T12 = Y01 * gF02 + Y11 * gF12 + Y12 * gF22;
        T20 = Y02 * gF00 + Y12 * gF10 + Y22 * gF20; T21 = Y02 * gF01 + Y12 * gF11 + Y22 * gF21;
        T22 = Y02 * gF02 + Y12 * gF12 + Y22 * gF22;
        const double an0 = A00 * n0 + A01 * n1 + A02 * n2, an1 = A10 * n0 + A11 * n1 + A12 * n2;
        const double an2 = A20 * n0 + A21 * n1 + A22 * n2;
        t0 = Y00 * gs0 + Y01 * gs1 + Y02 * gs2 + iz * an0;
        t1 = Y01 * gs0 + Y11 * gs1 + Y12 * gs2 + iz * an1;
        t2 = Y02 * gs0 + Y12 * gs1 + Y22 * gs2 + iz * an2;
        // M = P + Phi' T, m = a + Phi' t
        M00 = gP00 + gF00 * T00 + gF10 * T10 + gF20 * T20;
        M01 = gP01 + gF00 * T01 + gF10 * T11 + gF20 * T21;
        M02 = gP02 + gF00 * T02 + gF10 * T12 + gF20 * T22;
        M11 = gP11 + gF01 * T01 + gF11 * T11 + gF21 * T21;
        M12 = gP12 + gF01 * T02 + gF11 * T12 + gF21 * T22;
        M22 = gP22 + gF02 * T02 + gF12 * T12 + gF22 * T22;
        m0 = gp0 + gF00 * t0 + gF10 * t1 + gF20 * t2;
        m1 = gp1 + gF01 * t0 + gF11 * t1 + gF21 * t2;
        m2 = gp2 + gF02 * t0 + gF12 * t1 + gF22 * t2;
      };
      // a short step from the lane's unknown y (x_s going up, lam going down): w = T y + t (lam_j
      // up, x_s down) and what the next lane outwards starts from, e = Phi y + psi + Gam w
      // (x_s^(j+1) up; lam_{j-1} = Phi' lam + a + P x_s down)
      auto hand_on = [&](double y0, double y1, double y2, double& w0, double& w1, double& w2, double& e0,
                         double& e1, double& e2) {
        w0 = t0 + T00 * y0 + T01 * y1 + T02 * y2;
        w1 = t1 + T10 * y0 + T11 * y1 + T12 * y2;
        w2 = t2 + T20 * y0 + T21 * y1 + T22 * y2;
        e0 = gs0 + gF00 * y0 + gF01 * y1 + gF02 * y2 + gG00 * w0 + gG01 * w1 + gG02 * w2;
        e1 = gs1 + gF10 * y0 + gF11 * y1 + gF12 * y2 + gG01 * w0 + gG11 * w1 + gG12 * w2;
        e2 = gs2 + gF20 * y0 + gF21 * y1 + gF22 * y2 + gG02 * w0 + gG12 * w1 + gG22 * w2;
      };
      if constexpr (TWO) {
        // quad_perm [1, 0, 3, 2]: segment 1 reads segment 0 and segment 2 segment 3 in one move (the
        // outer lanes run the step on what they receive and drop the result)
        constexpr int kPair = 0xB1;
        if constexpr (S == 4) {
          step(dpp_d<kPair>(M00), dpp_d<kPair>(M01), dpp_d<kPair>(M02), dpp_d<kPair>(M11), dpp_d<kPair>(M12),
               dpp_d<kPair>(M22), dpp_d<kPair>(m0), dpp_d<kPair>(m1), dpp_d<kPair>(m2));
        }
        // the meet: with the other side's (R, r) each middle lane solves for its own unknown,
        //   y = (I - R M)^-1 (r + R m):  x_s^(h) on the upper side (R = beta), lam_{h-1} on the lower
        // (R = M_h; lam = M x + m and x = alpha + beta lam give (I - M beta) lam = m + M alpha).
        // A vector solve: one Z, one adjugate, no Y, T or M. quad_perm [0, 2, 1, 3] at S = 4.
        constexpr int kMeet = S == 2 ? 0xB1 : 0xD8;
        const double R00 = dpp_d<kMeet>(M00), R01 = dpp_d<kMeet>(M01), R02 = dpp_d<kMeet>(M02);
        const double R11 = dpp_d<kMeet>(M11), R12 = dpp_d<kMeet>(M12), R22 = dpp_d<kMeet>(M22);
        const double r0m = dpp_d<kMeet>(m0), r1m = dpp_d<kMeet>(m1), r2m = dpp_d<kMeet>(m2);
        const double Z00 = 1.0 - R00 * M00 - R01 * M01 - R02 * M02;
        const double Z01 = -(R00 * M01 + R01 * M11 + R02 * M12);
        const double Z02 = -(R00 * M02 + R01 * M12 + R02 * M22);
        const double Z10 = -(R01 * M00 + R11 * M01 + R12 * M02);
        const double Z11 = 1.0 - R01 * M01 - R11 * M11 - R12 * M12;
        const double Z12 = -(R01 * M02 + R11 * M12 + R12 * M22);
        const double Z20 = -(R02 * M00 + R12 * M01 + R22 * M02);
        const double Z21 = -(R02 * M01 + R12 * M11 + R22 * M12);
        const double Z22 = 1.0 - R02 * M02 - R12 * M12 - R22 * M22;
        const double A00 = Z11 * Z22 - Z12 * Z21, A01 = Z02 * Z21 - Z01 * Z22, A02 = Z01 * Z12 - Z02 * Z11;
        const double A10 = Z12 * Z20 - Z10 * Z22, A11 = Z00 * Z22 - Z02 * Z20, A12 = Z02 * Z10 - Z00 * Z12;
        const double A20 = Z10 * Z21 - Z11 * Z20, A21 = Z01 * Z20 - Z00 * Z21, A22 = Z00 * Z11 - Z01 * Z10;
        const double zdet = Z00 * A00 + Z01 * A10 + Z02 * A20;
        double iz = __builtin_amdgcn_rcp(zdet);
        iz = fma(iz, fma(-zdet, iz, 1.0), iz);
        iz = fma(iz, fma(-zdet, iz, 1.0), iz);
        const double v0 = r0m + R00 * m0 + R01 * m1 + R02 * m2;
        const double v1 = r1m + R01 * m0 + R11 * m1 + R12 * m2;
        const double v2 = r2m + R02 * m0 + R12 * m1 + R22 * m2;
        const double y0 = iz * (A00 * v0 + A01 * v1 + A02 * v2);
        const double y1 = iz * (A10 * v0 + A11 * v1 + A12 * v2);
        const double y2 = iz * (A20 * v0 + A21 * v1 + A22 * v2);
        if constexpr (S == 2) {
          // segment 0: x_s = 0 and lam_0 = y; the top segment: x_s = y and lam = 0
          xs0 = low ? 0.0 : y0; xs1 = low ? 0.0 : y1; xs2 = low ? 0.0 : y2;
          lm0 = low ? y0 : 0.0; lm1 = low ? y1 : 0.0; lm2 = low ? y2 : 0.0;
        } else {
          // the middle lanes keep (y, w) as their (x_s, lam) (the lower one as (lam, x_s)) and hand
          // e outwards: segment 0 takes lam_0 and keeps x_s = 0, the top one x_s and keeps lam = 0
          double w0, w1, w2, e0, e1, e2;
          hand_on(y0, y1, y2, w0, w1, w2, e0, e1, e2);
          const double f0 = dpp_d<kPair>(e0), f1 = dpp_d<kPair>(e1), f2 = dpp_d<kPair>(e2);
          const bool mid = seg == 1 || seg == 2;
          xs0 = mid ? (low ? w0 : y0) : (low ? 0.0 : f0);
          xs1 = mid ? (low ? w1 : y1) : (low ? 0.0 : f1);
          xs2 = mid ? (low ? w2 : y2) : (low ? 0.0 : f2);
          lm0 = mid ? (low ? y0 : w0) : (low ? f0 : 0.0);
          lm1 = mid ? (low ? y1 : w1) : (low ? f1 : 0.0);
          lm2 = mid ? (low ? y2 : w2) : (low ? f2 : 0.0);
        }
      } else {
#pragma unroll 1
        for (int it = 0; it < S - 1; it++) {
          step(seg_up<S>(M00, lane), seg_up<S>(M01, lane), seg_up<S>(M02, lane), seg_up<S>(M11, lane),
               seg_up<S>(M12, lane), seg_up<S>(M22, lane), seg_up<S>(m0, lane), seg_up<S>(m1, lane),
               seg_up<S>(m2, lane));
        }
        double l0, l1, l2, e0, e1, e2;
#pragma unroll 1
        for (int it = 0; it < S - 1; it++) {
          hand_on(xs0, xs1, xs2, l0, l1, l2, e0, e1, e2);
          xs0 = seg_dn<S>(e0, lane);
          xs1 = seg_dn<S>(e1, lane);
          xs2 = seg_dn<S>(e2, lane);
        }
        lm0 = top ? 0.0 : T00 * xs0 + T01 * xs1 + T02 * xs2 + t0;
        lm1 = top ? 0.0 : T10 * xs0 + T11 * xs1 + T12 * xs2 + t1;
        lm2 = top ? 0.0 : T20 * xs0 + T21 * xs1 + T22 * xs2 + t2;
      }
    }
    STAMP_ACC(acc_dual, t_dual);
    STAMP(t_ref);
    // ---- 3. refresh: the lam-part of the feed-forward, backward over the segment ----
    // (FST: nothing to refresh; the forward sweep adds F_i lam_j to k_i and the costate at the
    // segment start takes p^lam_s = Phi_s' lam_j. The top lane's lam is 0, so its Phi, zeroed by the
    // S = 8 ring and kept at S <= 4, does not matter.)
    double pl0 = lm0, pl1 = lm1, pl2 = lm2;
    if constexpr (FST) {
      pl0 = F00 * lm0 + F10 * lm1 + F20 * lm2;
      pl1 = F01 * lm0 + F11 * lm1 + F21 * lm2;
      pl2 = F02 * lm0 + F12 * lm1 + F22 * lm2;
    }
    if constexpr (S > 1 && !FST) {
      // stage t - 1's values are loaded while stage t computes (clamped: no branch)
      double nr[11];
#pragma unroll
      for (int e = 0; e < 11; e++) nr[e] = sc[((m - 1) * NV + e) * 64];
      for (int t = m - 1; t >= 0; t--) {
        ST* s = sc + t * NV * 64;
        const double K00 = nr[0], K01 = nr[1], K02 = nr[2], K10 = nr[3], K11 = nr[4];
        const double K12 = nr[5], k0 = nr[6], k1 = nr[7];
        const double I00 = nr[8], I01 = nr[9], I11 = nr[10];
        {
          const ST* sn1 = sc + (t > 0 ? t - 1 : 0) * NV * 64;
#pragma unroll
          for (int e = 0; e < 11; e++) nr[e] = sn1[e * 64];
        }
        const double bp0 = ROT ? b00 * pl0 + b20 * pl2 : b00 * pl0 + b10 * pl1 + b20 * pl2;  // B' p
        const double bp1 = b21 * pl2;
        s[6 * 64] = k0 - I00 * bp0 - I01 * bp1;
        s[7 * 64] = k1 - I01 * bp0 - I11 * bp1;
        const double n0 = pl0 + K00 * bp0 + K10 * bp1, n1 = pl1 + K01 * bp0 + K11 * bp1;
        pl2 = (ROT ? pl2 + a12 * pl1 : pl2 + a02 * pl0 + a12 * pl1) + K02 * bp0 + K12 * bp1;
        pl0 = n0; pl1 = n1;
      }
    }
    STAMP_ACC(acc_ref, t_ref);
    STAMP(t_fw);
    // ---- 4. forward over the segment: rollout, costate, PDAS re-guess ----
    // Two instantiations as in lane_kernel.h: plain PDAS passes (MODE 0) store the re-guessed
    // state as it is; single-flip passes (MODE 1) take the segment's first change only and
    // remember it (stage, replaced state) for the min over the QP's lanes below.
    bool changed = false;
    int fi = N;       // single-flip passes: this segment's first flip (stage) ...
    int fold_st = 0;  // ... and the state it replaced
    auto forward = [&](auto mode_tag) {
      constexpr int MODE = decltype(mode_tag)::value;
      double x0 = xs0, x1 = xs1, x2 = xs2;
      double l0 = p0 + pl0 + P00 * x0 + P01 * x1 + P02 * x2;  // costate at x_s
      double l1 = p1 + pl1 + P01 * x0 + P11 * x1 + P12 * x2;
      double l2 = p2 + pl2 + P02 * x0 + P12 * x1 + P22 * x2;
      bool flipped = false;
      // Q > 0, PDAS passes: the re-guessed codes are collected in a word of their own, every test's bit
      // selected at its place in it (the same integers as before), and `changed` is one compare of
      // the two words after the sweep instead of a compare and a mask OR per stage
      constexpr bool kWord = Q > 0 && MODE == 0;
      unsigned npk = 0u;
      double rx = Q > 0 ? rr[0] : r64[0], ry = Q > 0 ? rr[Q > 0 ? 1 : 0] : r64[64], rt = Q > 0 ? rr[Q > 0 ? 2 : 0] : r64[2 * 64];
      int old_n = Q > 0 ? (int)(apk & 15u) : ap[0];
      constexpr int NG = FST ? 14 : 8;
      double ng[NG];  // stage t + 1's gains, loaded while stage t computes
#pragma unroll
      for (int e = 0; e < NG; e++) {
        if constexpr (Q > 0) ng[e] = gr[0][e];
        else ng[e] = (double)sc[e * 64];
      }
      // unrolled by 2: same-box A/B C5 29.6 -> 29.3 us, C2 27.0 -> 26.5, C4 shard neutral
      // (Q > 0: the whole segment; the clamped next-stage indices below become constants and the
      // last stage's prefetch goes away)
      constexpr int kFwUnroll = Q > 0 ? Q : 2;
#pragma unroll kFwUnroll
      for (int t = 0; t < m; t++) {
        const double K00 = ng[0], K01 = ng[1], K02 = ng[2], K10 = ng[3], K11 = ng[4];
        const double K12 = ng[5];
        const double k0 = FST ? ng[6] + ng[8] * lm0 + ng[9] * lm1 + ng[10] * lm2 : ng[6];
        const double k1 = FST ? ng[7] + ng[11] * lm0 + ng[12] * lm1 + ng[13] * lm2 : ng[7];
        {
          const ST* sn1 = sc + (t + 1 < m ? t + 1 : m - 1) * NV * 64;
#pragma unroll
          for (int e = 0; e < NG; e++) {
            if constexpr (Q > 0) ng[e] = gr[t + 1 < m ? t + 1 : m - 1][e];
            else ng[e] = (double)sn1[e * 64];
          }
        }
        // (Q > 0: k + F lam kept in k's place, so that the output sweep reads no lam-gain)
        if constexpr (Q > 0) {
          gr[t][6] = k0; gr[t][7] = k1;
        }
        const int old = old_n;
        const double rxi = rx, ryi = ry, rti = rt;
        {
          const int tn = t + 1 < m ? t + 1 : m - 1;
          old_n = Q > 0 ? (int)((apk >> (4 * tn)) & 15u) : ap[tn * 64];
          rx = Q > 0 ? rr[3 * tn + 0] : r64[(3 * tn + 0) * 64];
          ry = Q > 0 ? rr[3 * tn + 1] : r64[(3 * tn + 1) * 64];
          rt = Q > 0 ? rr[3 * tn + 2] : r64[(3 * tn + 2) * 64];
        }
        const double u0 = k0 + K00 * x0 + K01 * x1 + K02 * x2;  // (an FMA chain on k)
        const double u1 = k1 + K10 * x0 + K11 * x1 + K12 * x2;
        const double w0 = l0 - q0 * (x0 - rxi), w1 = l1 - q1 * (x1 - ryi);
        const double w2 = l2 - q2 * (x2 - rti);
        l0 = w0; l1 = w1; l2 = ROT ? w2 - a12 * w1 : w2 - a02 * w0 - a12 * w1;
        const double g0 = ROT ? r0 * (u0 - ud0) + b00 * l0 + b20 * l2
                              : r0 * (u0 - ud0) + b00 * l0 + b10 * l1 + b20 * l2;
        const double g1 = r1 * (u1 - ud1) + b21 * l2;
        int st = MODE ? old : 0;
        const double* tf = ftab + 8 * old;  // (fp64 scratch) the old state's test thresholds
#pragma unroll
        for (int a = 0; a < 2; a++) {
          const int ca = (old >> (2 * a)) & 3;
          const double u = a ? u1 : u0, g = a ? g1 : g0;
          bool nlo, nhi;
          if constexpr (!F32) {
            // (the two tests exclude each other: lbe < ube, and a bound input has one test)
            const double y = tf[4 * a + 2] * u - tf[4 * a + 3] * g;
            nlo = y < tf[4 * a];
            nhi = y > tf[4 * a + 1];
          } else {
            const double gta = MODE ? (a ? gtoll1 : gtoll0) : (a ? gtol1 : gtol0);
            const double lbx = MODE ? (a ? lbl1 : lbl0) : (a ? lbe1 : lbe0);
            const double ubx = MODE ? (a ? ubl1 : ubl0) : (a ? ube1 : ube0);
            nlo = ((ca == 1) & (g > -gta)) | ((ca == 0) & (u < lbx));
            nhi = !nlo & (((ca == 2) & (g < gta)) | ((ca == 0) & (u > ubx)));
          }
          const int nca = (int)nlo | ((int)nhi << 1);
          if constexpr (kWord) {
            npk |= (nhi ? 2u : (unsigned)nlo) << (4 * t + 2 * a);  // (= nca: the tests exclude each other)
          } else if constexpr (MODE == 0) {
            st |= nca << (2 * a);
          } else {
            const bool take = (nca != ca) & !flipped;
            st = take ? ((st & ~(3 << (2 * a))) | (nca << (2 * a))) : st;
            flipped |= take;
          }
        }
        if constexpr (!kWord) {
          const bool ch = st != old;
          if constexpr (MODE == 1) {
            fi = (ch & (fi == N)) ? s0 + t : fi;
            fold_st = (ch & (fi == s0 + t)) ? old : fold_st;
          }
          changed |= ch;
          if constexpr (Q > 0) apk = (apk & ~(15u << (4 * t))) | ((unsigned)st << (4 * t));
          else ap[t * 64] = st;
        }
        const double nx0 = ROT ? x0 + b00 * u0 : x0 + a02 * x2 + b00 * u0 + c0;
        const double nx1 = ROT ? x1 + a12 * x2 : x1 + a12 * x2 + b10 * u0 + c1;
        const double nx2 = x2 + b20 * u0 + b21 * u1 + c2;
        x0 = nx0; x1 = nx1; x2 = nx2;
      }
      if constexpr (kWord) {
        changed = npk != apk;
        apk = npk;
      }
    };
    if (single) forward(SegMode<1>{});
    else forward(SegMode<0>{});
    // single-flip passes keep only the QP's first flip over the whole horizon
    if (single) {
      int mn = fi;
#pragma unroll
      for (int k = 1; k < S; k <<= 1) {
        const int o = __shfl_xor(mn, k, 64);
        mn = o < mn ? o : mn;
      }
      if (fi < N && fi != mn) {
        if constexpr (Q > 0) apk = (apk & ~(15u << (4 * (fi - s0)))) | ((unsigned)fold_st << (4 * (fi - s0)));
        else ap[(fi - s0) * 64] = fold_st;
        changed = false;
      }
    }
    const bool qchanged = qany(__ballot(changed));
    STAMP_ACC(acc_fw, t_fw);
    if (!qchanged && !done) {
      done = true;
      iters = pass + 1;
    }
  }

  STAMP(t_out);
  // the start whose outputs stand: the one that converged first (a converged start keeps its
  // iteration count while its wave sweeps on), the cold one on a tie or when neither converged
  bool owner = owner0, qowner = qowner0;
  if constexpr (TWIN) {
    // (Q > 0: the sibling's done flag and pass count in one word, one exchange)
    const int sibw = Q > 0 ? seg_sib<S>((iters << 1) | (int)done, lane) : 0;
    const bool sdone = Q > 0 ? (sibw & 1) != 0 : __shfl_xor((int)done, S, 64) != 0;
    const int sibit = Q > 0 ? sibw >> 1 : __shfl_xor(iters, S, 64);
    const bool win = var ? (done && (!sdone || iters < sibit)) : (done ? (!sdone || iters <= sibit) : !sdone);
    owner = owner0 && win;
    qowner = qowner0 && win;
  }
  // ---- output sweep: u* = K x + k from the final gains, x* by the fp64 rollout ----
  const bool solved = done && !bad;
  const float nanv = __int_as_float(0x7fc00000);
  float* uo = uout + (size_t)b * 2 * N;
  float* xo = xout + (size_t)b * 3 * (N + 1);
  if (qowner) {
    xo[0] = solved ? (float)fX0 : nanv;
    xo[1] = solved ? (float)fY0 : nanv;
    xo[2] = solved ? (float)fTH0 : nanv;
    if constexpr (Q > 0) {  // (nothing orders these after the sweep: issued ahead of its arithmetic)
      status_out[b] = bad ? F110QP_NUMERICAL_ID : (done ? F110QP_SOLVED_ID : F110QP_MAX_ITER_ID);
      if (iters_out) iters_out[b] = bad ? 0 : (done ? iters : max_pass);
    }
  }
  const bool want_obj = oo.obj || oo.cost;
  double J = 0.0, Cr = 0.0;
  auto qterm = [&](double rx, double ry, double rt, double e0, double e1, double e2) {
    const double d0 = e0 - rx, d1 = e1 - ry, d2 = e2 - rt;
    J += 0.5 * (q0 * d0 * d0 + q1 * d1 * d1 + q2 * d2 * d2);
    const double wx = (ROT ? cs * rx - sn * ry : rx) + X0, wy = (ROT ? sn * rx + cs * ry : ry) + Y0;
    const double wt = rt + th0;
    Cr += 0.5 * (q0 * wx * wx + q1 * wy * wy + q2 * wt * wt);
  };
  // gap-row box screen (f110qp_kernels.hip, AUTO gap calls): the box optimum is the optimum with
  // the gap rows too when it keeps every row of stages 1..N with a margin of 1e-6 of the row's
  // terms (evaluated here on the fp64 rollout in world coordinates) and the constant stage-0 rows
  // hold; any other QP goes on the list for GI. A template variant (SCR): the box-only kernels
  // keep their code (a runtime test cost C2 26.7 -> 27.5 us, same box)
  double ga0 = 0.0, gb0 = 0.0, gc0 = 0.0, ga1 = 0.0, gb1 = 0.0, gc1 = 0.0;
  if constexpr (SCR) {
    const float* h6 = oo.scr_hs + 6 * (size_t)b;
    ga0 = h6[0]; gb0 = h6[1]; gc0 = h6[2]; ga1 = h6[3]; gb1 = h6[4]; gc1 = h6[5];
  }
  int nviol = 0;  // gap rows of this lane's stages the box optimum violates (or within the margin)
  STAMP(t_ol0);
  {
    double x0 = xs0, x1 = xs1, x2 = xs2;
    if constexpr (Q > 0) {
      // (the last forward sweep left k + F lam in k's place: no lam-gain is read here)
      // The objective test is one wave-uniform branch round two copies of the sweep, every output
      // is selected once (solved or NaN) into registers, and the lane's 5 Q stores go out together
      // under one owner test: a run of 2 Q floats of u and one of 3 Q of x.
      float fu[2 * Q], fx[3 * Q];
      auto sweep = [&](auto obj_tag) {
        constexpr bool OBJ = decltype(obj_tag)::value != 0;
#pragma unroll
        for (int t = 0; t < Q; t++) {
          const double u0 = gr[t][6] + gr[t][0] * x0 + gr[t][1] * x1 + gr[t][2] * x2;
          const double u1 = gr[t][7] + gr[t][3] * x0 + gr[t][4] * x1 + gr[t][5] * x2;
          if constexpr (OBJ) {
            qterm(rr[3 * t], rr[3 * t + 1], rr[3 * t + 2], x0, x1, x2);
            J += 0.5 * (r0 * (u0 - ud0) * (u0 - ud0) + r1 * (u1 - ud1) * (u1 - ud1));
          }
          const double nx0 = x0 + b00 * u0, nx1 = x1 + a12 * x2;  // (ROT)
          x2 = x2 + b20 * u0 + b21 * u1 + c2;
          x0 = nx0; x1 = nx1;
          fu[2 * t] = solved ? (float)u0 : nanv;
          fu[2 * t + 1] = solved ? (float)u1 : nanv;
          fx[3 * t + 0] = solved ? (float)(cs * x0 - sn * x1 + X0) : nanv;
          fx[3 * t + 1] = solved ? (float)(sn * x0 + cs * x1 + Y0) : nanv;
          fx[3 * t + 2] = solved ? (float)(x2 + th0) : nanv;
        }
      };
      if (!ran) {  // no pass ran: nothing is solved (done == bad), the parent's zero gains gave NaN too
#pragma unroll
        for (int e = 0; e < 2 * Q; e++) fu[e] = nanv;
#pragma unroll
        for (int e = 0; e < 3 * Q; e++) fx[e] = nanv;
      } else if (want_obj) sweep(SegMode<1>{});
      else sweep(SegMode<0>{});
      if (owner) {
        float* const ul = uo + 2 * s0;
        float* const xl = xo + 3 * s0 + 3;
#pragma unroll
        for (int e = 0; e < 2 * Q; e++) ul[e] = fu[e];
#pragma unroll
        for (int e = 0; e < 3 * Q; e++) xl[e] = fx[e];
      }
    } else
    for (int t = 0; t < m; t++) {
      const int i = s0 + t;
      const ST* s = sc + t * NV * 64;
      const double K00 = s[0], K01 = s[64], K02 = s[2 * 64], K10 = s[3 * 64], K11 = s[4 * 64];
      const double K12 = s[5 * 64];
      const double k0 = FST ? s[6 * 64] + s[8 * 64] * lm0 + s[9 * 64] * lm1 + s[10 * 64] * lm2 : s[6 * 64];
      const double k1 = FST ? s[7 * 64] + s[11 * 64] * lm0 + s[12 * 64] * lm1 + s[13 * 64] * lm2 : s[7 * 64];
      // fp32 scratch: clamp a free input that sits outside its box by the single-flip tolerance
      const double u0 = F32 ? fmin(fmax(k0 + K00 * x0 + K01 * x1 + K02 * x2, lb0), ub0)
                            : k0 + K00 * x0 + K01 * x1 + K02 * x2;
      const double u1 = F32 ? fmin(fmax(k1 + K10 * x0 + K11 * x1 + K12 * x2, lb1), ub1)
                            : k1 + K10 * x0 + K11 * x1 + K12 * x2;
      if (want_obj) {
        qterm(r64[(3 * t) * 64], r64[(3 * t + 1) * 64], r64[(3 * t + 2) * 64], x0, x1, x2);
        J += 0.5 * (r0 * (u0 - ud0) * (u0 - ud0) + r1 * (u1 - ud1) * (u1 - ud1));
      }
      const double nx0 = ROT ? x0 + b00 * u0 : x0 + a02 * x2 + b00 * u0 + c0;
      const double nx1 = ROT ? x1 + a12 * x2 : x1 + a12 * x2 + b10 * u0 + c1;
      const double nx2 = x2 + b20 * u0 + b21 * u1 + c2;
      x0 = nx0; x1 = nx1; x2 = nx2;
      if constexpr (SCR) {
        const double wx = (ROT ? cs * x0 - sn * x1 : x0) + X0, wy = (ROT ? sn * x0 + cs * x1 : x1) + Y0;
        const double ta0 = ga0 * wx, tb0 = gb0 * wy, ta1 = ga1 * wx, tb1 = gb1 * wy;
        nviol += !(ta0 + tb0 + gc0 >= 1e-6 * (1.0 + fabs(ta0) + fabs(tb0) + fabs(gc0)));
        nviol += !(ta1 + tb1 + gc1 >= 1e-6 * (1.0 + fabs(ta1) + fabs(tb1) + fabs(gc1)));
      }
      if (owner) {
        uo[2 * i] = solved ? (float)u0 : nanv;
        uo[2 * i + 1] = solved ? (float)u1 : nanv;
        const double ox = ROT ? cs * x0 - sn * x1 : x0, oy = ROT ? sn * x0 + cs * x1 : x1;
        xo[3 * i + 3] = solved ? (float)(ox + X0) : nanv;
        xo[3 * i + 4] = solved ? (float)(oy + Y0) : nanv;
        xo[3 * i + 5] = solved ? (float)(x2 + th0) : nanv;
      }
    }
    if (want_obj && top) qterm(rNx, rNy, rNt, x0, x1, x2);  // x_N against x_ref[N-1]
  }
  STAMP_ACC(t_out_loop, t_ol0);
  if (want_obj) {
#pragma unroll
    for (int k = 1; k < S; k <<= 1) {
      J += __shfl_xor(J, k, 64);
      Cr += __shfl_xor(Cr, k, 64);
    }
    const double Cu = 0.5 * (double)N * (r0 * ud0 * ud0 + r1 * ud1 * ud1);
    const double dnan = __longlong_as_double(0x7ff8000000000000ll);
    if (qowner && oo.cost) oo.cost[b] = solved ? J : dnan;
    if (qowner && oo.obj) oo.obj[b] = solved ? J - Cr - Cu : dnan;
  }
  if constexpr (SCR) {
    // the QP's violation count over its S lanes; GI priority 1 + count (the list is ordered by it,
    // heavy first: gap_order_kernel), 1 for a violated stage-0 row or a box solve that failed
#pragma unroll
    for (int k = 1; k < S; k <<= 1) nviol += __shfl_xor(nviol, k, 64);
    const bool ok0 = (ga0 * X0 + gb0 * Y0 >= -gc0 - 1e-9) & (ga1 * X0 + gb1 * Y0 >= -gc1 - 1e-9);
    if (qowner) oo.scr_prio[b] = (!solved || !ok0) ? 1 : (nviol > 0 ? 1 + nviol : 0);
  }
  if constexpr (Q == 0) {
    if (qowner) {
      status_out[b] = bad ? F110QP_NUMERICAL_ID : (done ? F110QP_SOLVED_ID : F110QP_MAX_ITER_ID);
      if (iters_out) iters_out[b] = bad ? 0 : (done ? iters : max_pass);
    }
  }
  if (wt) {  // active set of this solution for the next tick (OR over the segments)
    // the lane's 2m bits (input a of stage t at bit 2t + a), placed at bit 2 s0 of the pair
    unsigned long long lw = 0, hw = 0;
    for (int t = 0; t < m; t++) {
      const unsigned st = Q > 0 ? (apk >> (4 * t)) & 15u : (unsigned)ap[t * 64];
      const unsigned l2 = (st & 1u) | ((st >> 1) & 2u), h2 = ((st >> 1) & 1u) | ((st >> 2) & 2u);
      lw |= (unsigned long long)l2 << (2 * t);
      hw |= (unsigned long long)h2 << (2 * t);
    }
    const int sh = 2 * s0;
    unsigned long long lo0 = sh < 64 ? lw << sh : 0ull, hi0 = sh < 64 ? hw << sh : 0ull;
    unsigned long long lo1 = sh == 0 ? 0ull : (sh < 64 ? lw >> (64 - sh) : lw << (sh - 64));
    unsigned long long hi1 = sh == 0 ? 0ull : (sh < 64 ? hw >> (64 - sh) : hw << (sh - 64));
#pragma unroll
    for (int k = 1; k < S; k <<= 1) {
      lo0 |= __shfl_xor(lo0, k, 64);
      hi0 |= __shfl_xor(hi0, k, 64);
      lo1 |= __shfl_xor(lo1, k, 64);
      hi1 |= __shfl_xor(hi1, k, 64);
    }
    if (qowner) {
      ws.act[2 * R * b] = lo0;
      ws.act[2 * R * b + 1] = hi0;
      if (R > 1) {
        ws.act[2 * (R * b + 1)] = lo1;
        ws.act[2 * (R * b + 1) + 1] = hi1;
      }
      unsigned* key = ws.key + 4 * b;
      key[0] = kth; key[1] = kv; key[2] = kd; key[3] = 2u;
    }
    // the wave's own counters (no atomics on one address: 256 waves x 2 of them measured ~3 us on
    // a stream whose keys hit every call)
    if (ws.stats && lane == 0) {
      *reinterpret_cast<uint2*>(ws.stats + 2 * (size_t)blockIdx.x) = make_uint2(wst.x, wst.y + 1u);
    }
  }
#ifdef F110QP_STAMPS
  if (lane == 0 && blockIdx.x < 4096) {
    unsigned long long* o = g_sstamps + (size_t)blockIdx.x * kSegStampSlots;
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    o[0] = t_setup; o[1] = acc_bw; o[2] = acc_dual; o[3] = acc_ref; o[4] = acc_fw;
    o[5] = t_end - t_out; o[6] = npass; o[7] = t_end - t_start;
    o[8] = t_stg - t_start; o[9] = t_lin - t_stg; o[10] = t_conv - t_lin; o[11] = t_setup - (t_conv - t_start);
    o[12] = t_rn - t_conv; o[13] = t_mask - t_rn; o[14] = t_setup - (t_mask - t_start); o[15] = t_out_loop;
  }
#endif
  signal_call_done(oo);  // a synchronous call's completion word (f110qp_kernels.h)
