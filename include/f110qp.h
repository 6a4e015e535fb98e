/*
 * f110qp.h — C ABI of the MI355X batched MPC/QP solver for the f110-mpc control tick.
 *
 * Drop-in boundary. In the reference the per-tick hot path is
 *   MPC::Update (src/mpc.cpp:69-143)
 *     Model::Linearize            (src/model.cpp:30-59)
 *     Constraints::FindHalfSpaces (src/constraints.cpp:116-265)
 *     MPC::CreateGradientVector / Update{LinearConstraintMatrix,Lower,Upper}Bound
 *                                 (src/mpc.cpp:221-306)
 *     OsqpEigen::Solver::{updateGradient, updateLinearConstraintsMatrix, updateBounds,
 *                         initSolver, solve, getSolution}  (src/mpc.cpp:81-142,
 *                         solver_ member at include/f110-mpc/mpc.h:63)
 * f110qp_solve_batch[_dev] replaces that whole sequence for B ticks/candidates at once:
 * linearisation, condensing, the QP solve and the (u*, x*) extraction of
 * MPC::UpdateSolvedTrajectory (src/mpc.cpp:145-159) run in one HIP launch on gfx950.
 *
 * Conventions
 *  - Plain C: no C++ exceptions cross this boundary; every entry point returns an int
 *    (F110QP_OK = 0, negative = error; details from f110qp_last_error()).
 *  - The caller owns every buffer. *_dev entry points take device pointers and a
 *    hipStream_t (passed as void*) and are asynchronous on that stream; the host-pointer
 *    entry points are synchronous.
 *  - One f110qp_ctx per host thread. A ctx owns its device workspace, so the calls made on
 *    one ctx must be ordered (one stream, or synchronised between streams).
 *  - Layouts (row-major, float32):
 *      x0        [B][3]      (x, y, ori)           State  (include/f110-mpc/state.h:10-45)
 *      u_lin     [B][2]      (v, steer_ang)        Input  (include/f110-mpc/input.h:11-34)
 *      x_ref     [B][S][3]   desired states, S = x_ref_points (default N); states 0..N-1 are
 *                            read (the reference reads the first N of its 50-point mini path;
 *                            stage N reuses x_ref[N-1], mpc.cpp:228)
 *      halfspace [B][2][3]   (l1, l2) = (a, b, c+0.5) from FindHalfSpaces, or NULL
 *      u_out     [B][N][2]   u*_k = z[3(N+1)+2k .. +1]            (mpc.cpp:148-157)
 *      x_out     [B][N+1][3] x*_k = z[3k .. 3k+2]                 (mpc.cpp:167-169)
 *      status    [B]         F110QP_SOLVED / _PRIMAL_INFEASIBLE / _MAX_ITER / _NUMERICAL
 *                            (OSQP codes)
 *      iters     [B]         active-set iterations (may be NULL): box-only QPs on either back end
 *                            count the equality-QP solves of the primal-dual active set including
 *                            the final one that confirms the KKT point (0 would mean none ran);
 *                            QPs the wave back end hands to its Goldfarb-Idnani loop (gap rows,
 *                            or a box PDAS that did not settle) count GI iterations instead
 *      obj       [B] double  (the *_ex entry points; may be NULL) OSQP's objective value
 *                            1/2 z'Pz + q'z of the solved QP (osqp_info::obj_val; P, q of
 *                            mpc.cpp:208-229), computed in fp64 on the device
 *      cost      [B] double  (*_ex; may be NULL) the same objective WITH the constant OSQP drops:
 *                            sum_i 1/2|x_i - x_ref_i|_Q^2 + sum_k 1/2|u_k - u_des|_R^2 >= 0
 *                            (= obj + 1/2 sum_i x_ref_i'Q x_ref_i + N/2 u_des'R u_des). Candidates
 *                            with different references are compared on `cost`: obj carries the
 *                            reference-dependent constant -1/2 sum x_ref'Q x_ref.
 *    On a non-SOLVED status u_out/x_out hold NaN (obj/cost too), as OSQP's solution does on
 *    failure, with one exception: F110QP_SOLVED_INACCURATE returns the finite but uncertified
 *    point (u, x, obj, cost written; see the status below).
 */
#ifndef F110QP_H
#define F110QP_H

#ifdef __cplusplus
extern "C" {
#endif

#define F110QP_API_VERSION 6

/* return codes */
#define F110QP_OK 0
#define F110QP_ERR_INVALID -1     /* bad argument / unsupported configuration */
#define F110QP_ERR_HIP -2         /* HIP runtime error (no device, launch failure, ...) */
#define F110QP_ERR_ALLOC -3

/* per-QP status codes (values follow OSQP's status ids) */
#define F110QP_SOLVED 1
#define F110QP_SOLVED_INACCURATE 2 /* a point whose fp64 certificate failed (box rows: the KKT  */
                                  /* check in primal units; gap rows: the duality-gap bound     */
                                  /* below, also after the fp64 Goldfarb-Idnani re-check): u,   */
                                  /* x, obj, cost                                               */
                                  /* are written but not certified, and f110qp_select_dev never */
                                  /* picks it. Its active set may seed the next warm start (a   */
                                  /* seed is only a first guess; every solve is certified on    */
                                  /* its own).                                                  */
#define F110QP_MAX_ITER -2
#define F110QP_PRIMAL_INFEASIBLE -3
#define F110QP_NUMERICAL -10      /* non-finite data or factorisation breakdown */

/* gap (follow-the-gap half-space) row semantics, src/mpc.cpp:279-300 */
#define F110QP_GAP_INACTIVE 0     /* as shipped: gap rows bounded by +-OsqpEigen::INFTY */
#define F110QP_GAP_ACTIVE 1       /* a*x+b*y >= -(c+0.5) on stages 1..N (mpc.cpp:297-298) */

/* solver back ends (f110qp_config.backend) */
#define F110QP_BACKEND_AUTO 0     /* lane-per-QP for box-only batches >= F110QP_LANE_MIN_BATCH  */
                                  /* or <= F110QP_LANE_MAX_SMALL_BATCH (N <= 32), and >=       */
                                  /* F110QP_LANE_MIN_BATCH_WIDE (N > 32)                       */
#define F110QP_BACKEND_WAVE 1     /* one wavefront per QP: condensed W = H^-1 + PDAS/GI         */
#define F110QP_BACKEND_LANE 2     /* one lane per QP: Riccati/PDAS in fp64; with gap rows the   */
                                  /* box screen at every batch size: the lane solve of the box- */
                                  /* only problem, the wave kernel's GI for the QPs whose box   */
                                  /* optimum violates a gap row (no warm state, ungrouped)      */
/* Gap rows: the wave kernel's GI (AUTO: behind the box screen from
 * F110QP_GAP_SCREEN_MIN_BATCH QPs); GI's final point is certified in fp64, and every QP it does not
 * certify is re-checked in the same call by an fp64 Goldfarb-Idnani with the oracle's rules
 * (SOLVED, PRIMAL_INFEASIBLE, MAX_ITER or SOLVED_INACCURATE from there). What SOLVED certifies on
 * this path: every row holds to 1e-9 (1 + |b| + |u|_inf) in fp64, and |u - u*'|_2 <= 1e-6
 * max(1, |u|_inf) for the exact optimum u*' of the reference QP with each row bound moved by u's own
 * residual on it (a backward error <= that 1e-9 relative, below the float32 rounding of the
 * inputs): the duality gap at the clamped multipliers, rho'W rho / min(R) with rho = Hu + g - N_A mu+,
 * rho'W rho bounded from above in fp64. The distance to the optimum of the unmoved QP also depends
 * on that QP's sensitivity to its bounds, which is not bounded here (tests: within 4e-8 of the
 * oracle's exact optimum on every gap-row case).
 * AUTO thresholds, measured on MI355X (kernel us, DESIGN.md section 6, round 3: the lane back end
 * with the partitioned-horizon kernel below one wave per SIMD, the wave back end with its fp64
 * certification). N = 20 (C2 recipe, cold): wave 27.3 vs lane 30.6 at 512 (before the last
 * segmented-kernel changes), 28.5 vs 27.7 at 1,024, 53.1 vs 36.3 at 2,048, 93.0 vs 37.0 at
 * 3,072. N = 30: 94.8 vs 77.9 at 2,048. N = 40: wave 223 vs lane 45.7 at 256, 365 vs 46.1 at
 * 512, 428 vs 53.7 at 768: the lane back end from one QP on.
 * Grouped calls use the same thresholds: the wave back end's per-group W saves its inverse but
 * its per-QP active-set phase still dominates (C4 candidate sets: 8,192 x N=40 grouped wave
 * 1,041 us vs lane 240 us, round 2). */
#define F110QP_LANE_MIN_BATCH 1024
#define F110QP_LANE_MIN_BATCH_WIDE 1
/* ... and, at N <= 32, batches of at most this many QPs (the single QP of MPC::Update): the
 * partitioned-horizon lane kernel splits each horizon over S = 4 lanes and beats the wave kernel's
 * one-QP chain (round 4, kernel us, N = 20: B = 1 lane 10.3 vs wave 19.3, B = 4 20.5 vs 23.9,
 * B = 16 25.8 vs 25.5, B = 64 30.8 vs 25.2; tools/latency_probe.py) */
#define F110QP_LANE_MAX_SMALL_BATCH 8
/* Gap rows (gap_mode ACTIVE), AUTO, ungrouped, no warm start, batches of at least this many QPs:
 * the box-only problem is solved on the lane back end first, and only the QPs whose box optimum
 * leaves a gap row violated (or within a 1e-6 margin) go to the wave kernel's GI; the others'
 * lane outputs are the optimum with the gap rows as well (round 4: 57% of the C3 batch). Results
 * are the exact optimum either way; the iteration count is the lane PDAS passes for screened QPs. */
#define F110QP_GAP_SCREEN_MIN_BATCH 1024
#define F110QP_LANE_MIN_BATCH_GROUPED F110QP_LANE_MIN_BATCH
#define F110QP_LANE_MIN_BATCH_GROUPED_WIDE F110QP_LANE_MIN_BATCH_WIDE

/* Largest max(q) / min(r) f110qp_create accepts. The wave back end holds the inverse of the condensed
 * Hessian H = R + G'QG in fp32: measured on an MI355X against the exact optimum, it returned points
 * off the optimum as SOLVED from a ratio of 1e5 (N = 48, dt 0.01; from 1e6 at N = 20), and from 1e4
 * both back ends gave up (SOLVED_INACCURATE, NUMERICAL, MAX_ITER) on QPs that have a solution. The
 * shipped weights are at 100; the parity tests reach 1e3. */
#define F110QP_MAX_WEIGHT_RATIO 1e3

#define F110QP_MAX_HORIZON 48  /* 2N <= 96 decision variables: two register rows per lane */

typedef struct f110qp_ctx f110qp_ctx;

typedef struct {
  int horizon;      /* N; params.yaml:12 ("/horizon"), 1..F110QP_MAX_HORIZON (48)     */
  float dt;         /* params.yaml:13, held as float MPC::dt_ (include/f110-mpc/mpc.h:46) */
  double q[3];      /* diag Q: q0,q1,q2 (params.yaml:1-3; mpc.cpp:20-24)                 */
  double r[2];      /* diag R: r0,r1 (params.yaml:5-6)                                    */
  double u_des[2];  /* des_vel, des_steer (params.yaml:42-43; mpc.cpp:18-19)              */
  float u_min[2];   /* (umin, -0.43f) constraints.cpp:21                                  */
  float u_max[2];   /* (umax,  0.43f) constraints.cpp:19                                  */
                    /* q, r and u_des are finite, max(q) <= F110QP_MAX_WEIGHT_RATIO min(r), */
                    /* u_min <= u_max (equal: the input is                                  */
                    /* fixed); u_des and u_lin may lie outside the box. "No bound" is       */
                    /* -+1e30, OSQP's INFTY (constraints.cpp:15), or -+inf, on either side. */
  int gap_mode;     /* F110QP_GAP_INACTIVE | F110QP_GAP_ACTIVE                            */
  int max_iter;     /* active-set iteration cap per QP; 0 = the default 8 * 2N + 16, with   */
                    /* gap rows 8 * (2N + 2N) + 16. A QP the cap stops has status           */
                    /* F110QP_MAX_ITER and NaN outputs, never a point off the optimum; a QP */
                    /* solved under a cap is solved under every larger one (box rows: bit   */
                    /* for bit alike, iters included).                                      */
                    /* What the cap counts depends on the back end a call runs on (AUTO     */
                    /* chooses by batch size, so one context may meet both meanings):       */
                    /*  - wave: one count over the box PDAS passes, the fp64 passes behind  */
                    /*    them and the dual active-set (GI) steps. The first fp32 PDAS      */
                    /*    passes (up to 10) always run: a QP they solve is SOLVED under any */
                    /*    cap, with iters up to 10.                                         */
                    /*  - lane (sequential and partitioned-horizon kernels): PDAS passes,   */
                    /*    and never fewer than the 16 multi-flip passes: the cap in effect  */
                    /*    is max(max_iter, 16).                                             */
                    /* Gap rows: a QP the wave kernel does not certify (stopped by the cap  */
                    /* included) is answered by the fp64 re-check, whose cap is its own,    */
                    /* whatever max_iter says: there a small max_iter costs time, not       */
                    /* answers.                                                             */
  int device;       /* HIP device ordinal used by the host-pointer entry points            */
  int warm_start;   /* 1: keep per-slot state across calls (OsqpEigen setWarmStart(true),   */
                    /*    mpc.cpp:98): the factor W = H^-1 is reused when a slot's          */
                    /*    linearisation point (theta0, v, steer) is bit-identical to its    */
                    /*    previous call's, and the previous active set seeds the solve.    */
                    /*    Slot b of call t+1 continues slot b of call t (same batch size). */
                    /*    The lane back ends move this state only while keys hit (within  */
                    /*    the last 2 calls, or on 2 probe calls in every 32).             */
                    /*    A stream whose linearisation point changes every tick (the      */
                    /*    closed loop of configs[4]: theta0 follows the plant) never hits: */
                    /*    its solves are cold solves (no factor or active set is reused;  */
                    /*    the previous tick's active set measured a worse seed than none, */
                    /*    DESIGN.md 2b). f110qp_warm_hits reports what a call reused.      */
  int backend;      /* F110QP_BACKEND_AUTO | _WAVE | _LANE (both give the exact optimum)    */
  int x_ref_points; /* points per QP in x_ref, >= N (0 = N). MPC::Update receives the whole   */
                    /* miniPath and reads its first N states (mpc.cpp:223-228): pass the      */
                    /* planner's [B][P][3] x_ref with x_ref_points = P                        */
} f110qp_config;

/* Library / ABI version (F110QP_API_VERSION). */
int f110qp_version(void);
/* Message of the last error on this thread (never NULL). */
const char* f110qp_last_error(void);

/* Defaults of params.yaml + constraints.cpp:19,21 for horizon N.
 * Replaces the getParam block of MPC::MPC (src/mpc.cpp:5-24) and Constraints::Constraints
 * (src/constraints.cpp:7-21). */
void f110qp_default_config(f110qp_config* cfg, int horizon);

/* Create a solver context (device workspace). Replaces the lazy OsqpEigen workspace set-up
 * of MPC::Update's first call (src/mpc.cpp:96-131). */
int f110qp_create(f110qp_ctx** ctx, const f110qp_config* cfg);
void f110qp_destroy(f110qp_ctx* ctx);

/* Solve B independent ticks (host pointers, synchronous). Replaces, per instance,
 * MPC::Update's Linearize + gradient/constraint/bound updates + solver_.solve() +
 * getSolution (src/mpc.cpp:69-143) and UpdateSolvedTrajectory (src/mpc.cpp:145-159).
 * Up to 64 QPs the kernel reads the inputs from and writes the outputs to pinned host staging
 * (zero-copy), and the call returns on its last kernel's completion word (f110qp_sync_signals);
 * larger batches are staged through device memory and wait for the stream. */
int f110qp_solve_batch(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                       const float* x_ref, const float* halfspace, float* u_out, float* x_out,
                       int* status, int* iters);

/* Same on device pointers, enqueued on `stream` (a hipStream_t, NULL = default stream). */
int f110qp_solve_batch_dev(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                           const float* x_ref, const float* halfspace, float* u_out,
                           float* x_out, int* status, int* iters, void* stream);

/* f110qp_solve_batch_dev, then a wait until the results are in device memory: one call per
 * control tick for a caller that needs the answer before it returns, as solver_.solve() +
 * getSolution do in MPC::Update (src/mpc.cpp:133-142). When the call's last kernel (lane or wave
 * kernel; for gap rows the fp64 re-check) has at most 256 workgroups, the call waits on the
 * completion word that kernel writes from its last wave or workgroup after a system-scope fence:
 * the outputs are then visible to any stream and to the host, and the kernel may still be retiring
 * on `stream` when this returns. Larger launches synchronise `stream`. */
int f110qp_solve_batch_dev_sync(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                                const float* x_ref, const float* halfspace, float* u_out,
                                float* x_out, int* status, int* iters, void* stream);

/* Grouped solve: the candidates of one control tick share their linearisation point.
 * Model::Linearize depends only on (theta0, v, delta) (src/model.cpp:30-59), so the candidate
 * mini-paths of one pose (src/project.cpp:76-113) share A, B, C, the condensed Hessian H and
 * W = H^-1: only the gradient differs (the proposal's `group` argument, 8(b)).
 *   group [B]   scenario id of each QP in [0, num_groups); ids need not be contiguous or sorted.
 * One W per group is built from its first member; every member whose (x0[b][2], u_lin[b]) bits
 * equal that member's reuses it, any other QP (or an id outside [0, num_groups)) builds its own.
 * Grouping therefore never changes a result: the output is bit-identical to
 * f110qp_solve_batch[_dev] on the wave back end. The lane back end (chosen by AUTO at and above
 * F110QP_LANE_MIN_BATCH_GROUPED[_WIDE]) ignores the groups (only its first, cold pass has
 * group-invariant Riccati matrices: <= ~4% of a C4 launch). Grouped
 * calls neither use nor update the warm-start state. Same layouts and conventions as above. */
int f110qp_solve_grouped(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                         const float* x_ref, const float* halfspace, const int* group,
                         int num_groups, float* u_out, float* x_out, int* status, int* iters);
int f110qp_solve_grouped_dev(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                             const float* x_ref, const float* halfspace, const int* group,
                             int num_groups, float* u_out, float* x_out, int* status, int* iters,
                             void* stream);

/* Same as f110qp_solve_batch[_dev] / f110qp_solve_grouped[_dev], plus the per-QP objective
 * `obj` and `cost` (see Layouts; either may be NULL). The objective is what
 * OsqpEigen::Solver::solve() leaves in osqp_info::obj_val after src/mpc.cpp:133. */
int f110qp_solve_batch_ex(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                          const float* x_ref, const float* halfspace, float* u_out, float* x_out,
                          int* status, int* iters, double* obj, double* cost);
int f110qp_solve_batch_ex_dev(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                              const float* x_ref, const float* halfspace, float* u_out,
                              float* x_out, int* status, int* iters, double* obj, double* cost,
                              void* stream);
int f110qp_solve_grouped_ex(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                            const float* x_ref, const float* halfspace, const int* group,
                            int num_groups, float* u_out, float* x_out, int* status, int* iters,
                            double* obj, double* cost);
int f110qp_solve_grouped_ex_dev(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                                const float* x_ref, const float* halfspace, const int* group,
                                int num_groups, float* u_out, float* x_out, int* status,
                                int* iters, double* obj, double* cost, void* stream);

/* ---- double-precision inputs ------------------------------------------------------------------
 * The reference holds State, Input and the reference path as double (include/f110-mpc/state.h:41-43,
 * include/f110-mpc/input.h:31-32, used unrounded in src/mpc.cpp:225-228,299,305). The *_dbl entry
 * points take x0 [B][3], u_lin [B][2] and x_ref [B][S][3] as double, same row-major shapes; every
 * other argument keeps its type (halfspace float32, as the reference's float pairs; u_out / x_out
 * float32; status, iters, obj, cost unchanged; obj and cost may be NULL). Additive: the float entry
 * points above are unchanged and F110QP_API_VERSION stays 6.
 *  - The kernels read the doubles themselves (double-input instantiations of every kernel family):
 *    nothing is narrowed on the host, no conversion launch runs in front of the solve, and a call
 *    makes the same launches as its float twin. Past the loads the arithmetic is the float call's:
 *    x_ref - x0, theta0, v and delta in fp64. For doubles that are float32 values the outputs are
 *    bit-identical to the float call's, except on the sequential lane kernel with float references
 *    in LDS (scratch modes of large batches, more than one wave per CU): there the _dbl kernel
 *    stages x_ref - x0, subtracted in fp64 and rounded to float32, where the float kernel stages
 *    the absolute float32 reference.
 *  - The launch policy is the float call's: f110qp_backend_info, f110qp_lane_segments,
 *    f110qp_lane_starts and f110qp_gap_screen answer for both.
 *  - The completion-word waits (f110qp_sync_signals) and the <= 64-QP zero-copy staging of the
 *    host-pointer call work as for float; its packed pinned input layout has 8-byte fields for the
 *    three double arrays (8-byte aligned), the float half-spaces behind them.
 *  - Warm start: on a warm_start = 1 context a _dbl call solves cold and neither reads nor updates
 *    the per-slot state (as the grouped calls). The slot key is three float bit patterns in 16
 *    bytes; a key that does not compare all 64 bits of theta0, v and delta could reuse a factor
 *    built for another linearisation point. A wider slot key is not part of this ABI version.
 *    f110qp_warm_hits is not moved by _dbl calls; float calls on the same context hit as before.
 *  - Grouped, wave back end: the per-group key of a _dbl call holds the full doubles of
 *    (x0[b][2], u_lin[b]) (32 bytes per group, allocated per call), so two scenarios whose
 *    linearisation points share their float32 rounding but differ as doubles never share a W.
 *    Results are bit-identical to f110qp_solve_batch_dev_dbl on the wave back end. The lane back
 *    end ignores the groups, as for float.
 *  - x_out is the absolute state in float32: far from the origin it carries the float32 rounding of
 *    the position, up to half an ulp of |x| (6e-5 m at 1 km), and x_out[b][0] is x0 rounded to
 *    float32. u_out, which MPC::Update consumes (src/mpc.cpp:148-157), is not affected.
 *  - The debug hooks f110qp_condense_debug_dev / f110qp_assemble_debug_dev stay float-only. */
int f110qp_solve_batch_dbl(f110qp_ctx* ctx, int batch, const double* x0, const double* u_lin,
                           const double* x_ref, const float* halfspace, float* u_out, float* x_out,
                           int* status, int* iters, double* obj, double* cost);
/* device pointers, asynchronous on `stream` */
int f110qp_solve_batch_dev_dbl(f110qp_ctx* ctx, int batch, const double* x0, const double* u_lin,
                               const double* x_ref, const float* halfspace, float* u_out,
                               float* x_out, int* status, int* iters, double* obj, double* cost,
                               void* stream);
/* as f110qp_solve_batch_dev_sync */
int f110qp_solve_batch_dev_sync_dbl(f110qp_ctx* ctx, int batch, const double* x0,
                                    const double* u_lin, const double* x_ref,
                                    const float* halfspace, float* u_out, float* x_out, int* status,
                                    int* iters, void* stream);
int f110qp_solve_grouped_dbl(f110qp_ctx* ctx, int batch, const double* x0, const double* u_lin,
                             const double* x_ref, const float* halfspace, const int* group,
                             int num_groups, float* u_out, float* x_out, int* status, int* iters,
                             double* obj, double* cost);
int f110qp_solve_grouped_dev_dbl(f110qp_ctx* ctx, int batch, const double* x0, const double* u_lin,
                                 const double* x_ref, const float* halfspace, const int* group,
                                 int num_groups, float* u_out, float* x_out, int* status,
                                 int* iters, double* obj, double* cost, void* stream);

/* ---- closed loop on the device ------------------------------------------------------------------
 * The MPC branch of project::OdomCallback (src/project.cpp:160-198) driven by a simulated car, for B
 * cars and T ticks without a host round trip: per tick the solve of f110qp_solve_batch_dev_dbl on
 * the car's fp64 pose, then one plant-step launch (Model::simulate_dynamics, src/model.cpp:61-75)
 * that also forms the next linearisation input (GetNextInput() with v forced to 4.5,
 * src/project.cpp:169-170,210-218). Additive: F110QP_API_VERSION stays 6. */
typedef struct {
  int    ticks;        /* T >= 1 (f110qp_rollout[_dev]; f110qp_advance_dev ignores it)             */
  double plant_dt;     /* Euler step of the plant; default 0.01 (params.yaml:13 as a double)       */
  double car_length;   /* 0.35, CAR_LENGTH of src/model.cpp:2 (not the 0.3302f of Linearize)       */
  double v_lin;        /* 4.5: v of the next linearisation input, src/project.cpp:170               */
  double fail_u[2];    /* (0.5, 0.0): Input of GetNextInput() without a solution, project.cpp:215  */
} f110qp_rollout_config;

/* ticks = 1 and the defaults above. */
void f110qp_default_rollout_config(f110qp_rollout_config* rc);

/* One plant step of B cars on the first input of their plans (device pointers, asynchronous on
 * `stream`, one launch; replaces Model::simulate_dynamics + GetNextInput() per car):
 *   x [B][3] double, u_plan [B][N][2] float32 (a solve's u_out), status [B] (that solve's)
 *   -> x_next [B][3] double, u_lin_next [B][2] double, u_applied [B][2] float32 (may be NULL).
 * A car is usable when its status is F110QP_SOLVED or F110QP_SOLVED_INACCURATE (the statuses for
 * which u_out is finite). Two modelling choices:
 *  - the applied input is u_plan[b][0], a float32 widened to double (the reference's drive message
 *    carries float32 too), or fail_u when the car is not usable;
 *  - u_lin_next = (v_lin, steer of u_plan[b][1]) (of u_plan[b][0] when N == 1); when not usable
 *    (v_lin, fail_u[1]): after a failed solve solved_trajectory() is empty and GetNextInput()
 *    returns Input(0.5, 0).
 * x_next = x + plant_dt * (v cos(ori), v sin(ori), tan(steer) v / car_length) in fp64, in the
 * reference's expression order, every product and sum rounded (no fused multiply-add).
 * x_next must not alias x; u_plan and u_applied must be 8-byte aligned. rc->ticks is not read;
 * plant_dt and car_length must be positive and finite, v_lin and fail_u finite. */
int f110qp_advance_dev(const f110qp_rollout_config* rc, int batch, int horizon, const double* x,
                       const float* u_plan, const int* status, double* x_next, double* u_lin_next,
                       float* u_applied, void* stream);

/* T closed-loop ticks of B cars (device pointers, asynchronous on `stream`):
 *   x_ref      [B][S][3] double, halfspace [B][2][3] float32 or NULL: held fixed over the T ticks
 *              (the reference passes the same miniPath_ every tick between re-plans,
 *              src/project.cpp:188). Holding the half-spaces is a shortcut of this call, not the
 *              reference's behaviour: MPC::Update recomputes them on every tick from the scan it
 *              holds and the car's current pose (src/mpc.cpp:73-75), so both lines move and turn
 *              with the car. f110qp_rollout_scan[_dev] below does that.
 *   x_traj     [T+1][B][3] double, u_lin_traj [T+1][B][2] double: row 0 holds the start on entry,
 *              row t+1 is written by tick t
 *   u_applied  [T][B][2] float32, status_traj [T][B]
 *   iters_traj [T][B], cost_traj [T][B] double, u_plan [T][B][N][2], x_plan [T][B][N+1][3] float32:
 *              each may be NULL.
 * Tick t is f110qp_solve_batch_dev_dbl on (x_traj[t], u_lin_traj[t], x_ref, halfspace), writing
 * straight into row t of status_traj / iters_traj / cost_traj / u_plan / x_plan (a NULL u_plan or
 * x_plan: into a workspace of the context, sized once), then f110qp_advance_dev into row t+1 of
 * x_traj / u_lin_traj and row t of u_applied. A call makes exactly the launches of T such solve
 * calls plus T plant-step launches, with the solve call's launch policy (f110qp_backend_info,
 * f110qp_lane_segments, ... answer for it) and, as every _dbl call, without reading or updating the
 * warm-start state. It performs no host synchronisation, reads back no device value and allocates
 * nothing inside the tick loop; every argument is checked before the first launch (ticks >= 1,
 * required pointers, the plant parameters as for f110qp_advance_dev). */
int f110qp_rollout_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc, int batch,
                       const double* x_ref, const float* halfspace, double* x_traj,
                       double* u_lin_traj, float* u_applied, int* status_traj, int* iters_traj,
                       double* cost_traj, float* u_plan, float* x_plan, void* stream);

/* Same on host pointers (synchronous): staged through device buffers of the context, one stream
 * synchronisation at the end. It does not wait on a completion word: f110qp_sync_signals does not
 * move. */
int f110qp_rollout(f110qp_ctx* ctx, const f110qp_rollout_config* rc, int batch, const double* x_ref,
                   const float* halfspace, double* x_traj, double* u_lin_traj, float* u_applied,
                   int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                   float* x_plan);

/* Per-scenario selection on the device: the candidate argmin of
 * project::OdomCallback (src/project.cpp:125-136), taken over the QP costs of each scenario's
 * candidates instead of the end-point distance. winner[g] = the smallest b with group[b] == g,
 * status[b] == F110QP_SOLVED and the minimal cost[b] (exact, deterministic), or -1 when the
 * scenario has no solved candidate; best_cost[g] = that cost (+inf if none). group/cost/status
 * [batch], winner/best_cost [num_groups], device pointers, async on stream. Across GPUs, the
 * per-rank (best_cost, winner) pairs reduce with a min-loc all-reduce (f110qp/shard.py). */
int f110qp_select_dev(int batch, const int* group, int num_groups, const double* cost,
                      const int* status, int* winner, double* best_cost, void* stream);

/* The launch a solve call of `batch` QPs on this context makes (grouped != 0: the grouped entry
 * points): backend = F110QP_BACKEND_WAVE or _LANE (what AUTO resolves to), qps_per_wave (lane:
 * QPs per 64-lane wavefront; wave: 1) and scratch (lane: 1 LDS fp64, 2 LDS fp32, 3 HBM fp64,
 * 4 HBM fp32 Riccati gain scratch; the partitioned-horizon kernel uses 1 or 2 (float references
 * and scratch where fp64 does not fit); wave: 0). With gap rows, LANE means the box screen's lane
 * solve (F110QP_BACKEND_LANE). Any pointer may be NULL. */
int f110qp_backend_info(f110qp_ctx* ctx, int batch, int grouped, int* backend, int* qps_per_wave,
                        int* scratch);

/* Horizon segments per QP of that launch: 1, or S = 2 / 4 / 8 when the lane back end splits each
 * QP's horizon over S lanes (partitioned Riccati; batches too small to give every SIMD a wave of
 * distinct QPs; with gap rows on the lane back end: the box screen's solve).
 * The result is the exact optimum either way. */
int f110qp_lane_segments(f110qp_ctx* ctx, int batch, int* segments);

/* PDAS starts per QP of that launch: 2 when the partitioned-horizon kernel solves each QP from two
 * starts at once (the cold one and the speed bound u_des sits on held over the first half of the
 * horizon; taken when u_des is on a speed bound and the doubled grid still leaves no SIMD with
 * two waves), else 1. The first start to converge gives the answer: the same exact optimum, in the
 * smaller of the two pass counts (DESIGN.md 2b'). */
int f110qp_lane_starts(f110qp_ctx* ctx, int batch, int* starts);

/* Stages per segment of that launch when it runs a partitioned-horizon kernel compiled for a fixed
 * segment length (5: box rows, 4 segments of a 20-stage horizon in the heading frame; DESIGN.md
 * 2b'), else 0: the kernels that take the segment length at run time. Same results either way. */
int f110qp_lane_fixed_q(f110qp_ctx* ctx, int batch, int* stages);

/* on = 1 when a gap-row call of `batch` QPs takes the box screen (F110QP_GAP_SCREEN_MIN_BATCH):
 * the lane back end solves the box-only problem, the wave kernel's GI only the QPs whose box
 * optimum does not keep every gap row (an ungrouped solve call; replaces nothing in the reference:
 * a query of this library's dispatch, like f110qp_backend_info). */
int f110qp_gap_screen(f110qp_ctx* ctx, int batch, int* on);

/* Forget the warm-start state of every slot (the next call solves cold). */
int f110qp_warm_reset(f110qp_ctx* ctx);

/* What the solve calls on this context did with the warm-start state (config.warm_start) since
 * the previous f110qp_warm_hits (or since the state was laid out for the batch size): *traffic =
 * the calls that loaded and stored the slots' keys and active sets (the lane back ends skip both
 * while no key hits, see warm_start), *hits = the QPs whose slot key equalled their linearisation
 * point, i.e. that started from the slot's previous active set. Counted by the lane back ends'
 * kernels (the wave back end reports 0); synchronises with the last warm call's stream; both 0
 * without warm_start. */
int f110qp_warm_hits(f110qp_ctx* ctx, int* traffic, int* hits);

/* Gap rows: how many QPs the last gap-row solve call on this context sent to the fp64
 * Goldfarb-Idnani re-check (the QPs whose fp32 GI answer the fp64
 * certificate did not accept). Synchronises with that call's stream; 0 before any gap-row call. */
int f110qp_last_recheck_count(f110qp_ctx* ctx, int* count);

/* How many synchronous calls on this context (f110qp_solve_batch_dev_sync, and the host-pointer
 * calls of at most 64 QPs, whose kernel stores the outputs into pinned host memory) waited on the
 * kernel's completion word instead of synchronising the stream: the calls whose last kernel (lane or
 * wave kernel, for gap rows the fp64 re-check) has at most 256 workgroups, which publishes the
 * call's number to a pinned host word after a system-scope fence (single-QP latency).
 * Larger launches, host-pointer calls of more than 64 QPs and the grouped calls synchronise the
 * stream. */
int f110qp_sync_signals(f110qp_ctx* ctx, unsigned* count);

/* 1 for the test / measurement build (lib_test/libf110qp.so, -DF110QP_TEST_HOOKS), whose
 * f110qp_create also reads create-time F110QP_* knobs from the environment that force kernel
 * variants for the tests; 0 for the product library, which reads no environment variable. */
int f110qp_test_build(void);

/* Debug/parity hook: the condensed Hessian H [B][2N][2N] and gradient g [B][2N] exactly as
 * the solve kernel builds them on the device (float64), for comparison with the CPU oracle's
 * condensing of the reference QP (src/mpc.cpp:208-306). Device pointers, async on stream. */
int f110qp_condense_debug_dev(f110qp_ctx* ctx, int batch, const float* x0, const float* u_lin,
                              const float* x_ref, double* H_out, double* g_out, void* stream);

/* Sizes of the reference's OSQP problem for horizon N (src/mpc.cpp:26-29): n = 5N+3 variables,
 * m = 7N+5 constraints, and the stored nonzeros of P (9(N+1) + 4N) and A (26N + 9), explicit
 * zeros of the dense blocks included. Returns F110QP_OK or F110QP_ERR_INVALID. */
int f110qp_qp_dims(int horizon, int* n, int* m, int* nnz_P, int* nnz_A);

/* Assembly-parity hook: ONE instance's QP exactly as
 * MPC::Update leaves it for OsqpEigen (src/mpc.cpp:77-80, layouts :208-306), computed on the
 * device from x0[3], u_lin[2], x_ref[S][3] (S = x_ref_points) and halfspace[6] (NULL: zeros) with
 * the solve kernels' Model::Linearize: P (CSC: colptr[n+1], rowind/val[nnz_P]), q[n], A (CSC:
 * colptr[n+1], rowind/val[nnz_A]), l[m], u[m]; +-1e30 = OsqpEigen::INFTY. gap_mode INACTIVE gives
 * the shipped rows (stage-0 all-ones placeholder block, +-INFTY bounds), ACTIVE the C3 semantic.
 * Device pointers, async on stream. */
int f110qp_assemble_debug_dev(f110qp_ctx* ctx, const float* x0, const float* u_lin,
                              const float* x_ref, const float* halfspace, int* P_colptr,
                              int* P_rowind, double* P_val, double* q, int* A_colptr, int* A_rowind,
                              double* A_val, double* l, double* u, void* stream);

/* Constraints::FindHalfSpaces (src/constraints.cpp:116-265) for one scan, host code.
 * state[3] = (x, y, ori); writes l1[3], l2[3] = (a, b, c+0.5). Returns F110QP_OK, or
 * F110QP_ERR_INVALID when the scan holds no gap (the reference then reads ranges[-1]). */
int f110qp_find_half_spaces(const double state[3], const float* ranges, int num_ranges,
                            float angle_min, float angle_increment, float angle_max,
                            float ftg_thresh, float divider, float buffer, double l1[3],
                            double l2[3]);

/* Batched FindHalfSpaces on the device, one wavefront per scan (num_ranges <= 65535, angle_increment
 * > 0): scans [B][num_ranges], states [B][3] -> hs [B][2][3]
 * (float32, the f110qp_solve_batch halfspace layout); gap_lo/gap_hi [B] may be NULL. */
int f110qp_find_half_spaces_dev(int batch, const float* states, const float* ranges,
                                int num_ranges, float angle_min, float angle_increment,
                                float angle_max, float ftg_thresh, float divider, float buffer,
                                float* hs_out, int* gap_lo, int* gap_hi, void* stream);

/* Same on double states [B][3]: x and y enter the end points unrounded, as the reference reads
 * poseX / poseY (doubles); ori is narrowed to float where the reference narrows it (float
 * current_angle = state.ori()). For doubles that are float32 values the output is bit-identical to
 * the float call's. */
int f110qp_find_half_spaces_dev_dbl(int batch, const double* states, const float* ranges,
                                    int num_ranges, float angle_min, float angle_increment,
                                    float angle_max, float ftg_thresh, float divider, float buffer,
                                    float* hs_out, int* gap_lo, int* gap_hi, void* stream);

/* ---- closed loop with gap rows: FindHalfSpaces at every tick's pose -----------------------------
 * MPC::Update calls constraints_.FindHalfSpaces(current_state_, scan_msg_) on every tick
 * (src/mpc.cpp:73-75) with the scan MPC::UpdateScan stored on the first scan message
 * (src/project.cpp:45-49) and the car's current pose. FindHalfSpaces splits where the pose enters:
 *   the gap search (src/constraints.cpp:118-177: window, threshold, first longest run, buffer
 *   inflation) reads only the scan: one launch per scan set, one wavefront per scan, one 16-byte
 *   record per scan;
 *   the end-point geometry (:179-264) reads the record and the pose: one thread per car, fused
 *   into the plant-step launch, which holds the car's next pose in registers.
 * Additive: F110QP_API_VERSION stays 6. */
typedef struct {
  int   num_ranges;       /* beams per scan, 1..65535                                               */
  float angle_min;        /* LaserScan.angle_min                                                    */
  float angle_increment;  /* LaserScan.angle_increment, > 0                                         */
  float angle_max;        /* LaserScan.angle_max                                                    */
  float ftg_thresh;       /* 3.0, params.yaml (Constraints::ftg_thresh_)                            */
  float divider;          /* 1.5: the field-of-view window is +-1.571 / divider                     */
  float buffer;           /* 3.0: beams the gap shrinks by at either end                            */
  int   scan_rows;        /* 1: one scan per car, held for the whole call (the reference); T: ranges */
                          /* [T][B][num_ranges], tick t reads row t (recorded or simulated scans)    */
} f110qp_scan_config;

/* Zeroes *sc, then ftg_thresh 3.0, divider 1.5, buffer 3.0 and scan_rows 1 (the scan's geometry is
 * the caller's). */
void f110qp_default_scan_config(f110qp_scan_config* sc);

/* One record of the gap search: (lo, hi) exactly what f110qp_find_half_spaces_dev reports as
 * gap_lo / gap_hi (after the buffer inflation; -1 and out-of-range values included), r_lo / r_hi =
 * ranges[lo], ranges[hi], NaN where lo or hi is no beam of the scan (the rows are NaN then). */
typedef struct {
  int   lo, hi;
  float r_lo, r_hi;
} f110qp_gap_record;

/* The gap search of `count` scans (device pointers, asynchronous, one launch): ranges
 * [count][num_ranges] -> gap_out [count]. sc->scan_rows is not read. */
int f110qp_gap_search_dev(const f110qp_scan_config* sc, int count, const float* ranges,
                          f110qp_gap_record* gap_out, void* stream);

/* The end-point geometry of B cars (one launch, one thread per car): gap [B], states [B][3] double
 * -> hs_out [B][2][3] float32. f110qp_gap_search_dev followed by this call is bit-identical to
 * f110qp_find_half_spaces_dev_dbl. Reads num_ranges, angle_min and angle_increment of sc. */
int f110qp_half_space_rows_dev(const f110qp_scan_config* sc, int batch, const f110qp_gap_record* gap,
                               const double* states, float* hs_out, void* stream);

/* f110qp_advance_dev and, in the same launch, f110qp_half_space_rows_dev at x_next into hs_next
 * [B][2][3]: gap [B] holds the records of the scans the next tick reads. x_next, u_lin_next and
 * u_applied are bit-identical to f110qp_advance_dev's. The argument rules of f110qp_advance_dev
 * apply; gap and hs_next must be non-NULL. */
int f110qp_advance_scan_dev(const f110qp_rollout_config* rc, const f110qp_scan_config* sc, int batch,
                            int horizon, const double* x, const float* u_plan, const int* status,
                            const f110qp_gap_record* gap, double* x_next, double* u_lin_next,
                            float* u_applied, float* hs_next, void* stream);

/* f110qp_rollout_dev with the half-spaces of every tick computed at that tick's pose, as the
 * reference computes them. Arguments as f110qp_rollout_dev, except:
 *   ranges   [scan_rows][B][num_ranges] float32 replaces halfspace (scan_rows = 1 or T; any other
 *            value is F110QP_ERR_INVALID)
 *   hs_traj  [T][B][2][3] float32: row t holds the rows tick t solved with; may be NULL (the rows
 *            then live in one buffer of the context of B rows: in stream order tick t's solve has
 *            read them before tick t's plant step writes the next ones).
 * Launches: in front of the loop one gap search over scan_rows x B scans and one rows launch for
 * tick 0; per tick exactly the launches of f110qp_rollout_dev, the plant step being the fused one
 * (the last tick's the plain one: there is no row T). No host synchronisation, read-back or
 * allocation inside the loop; every argument is checked before the first launch.
 * gap_mode INACTIVE: valid. The rows are computed only when hs_traj is given (the shipped reference
 * computes them and then bounds them by +-INFTY) and the solves ignore them; with hs_traj NULL the
 * call makes exactly f110qp_rollout_dev's launches.
 * A scan without a gap gives NaN rows: the tick's solve returns F110QP_NUMERICAL for that car
 * (non-finite data; in this call only: f110qp_solve_batch* on NaN rows keeps its
 * F110QP_PRIMAL_INFEASIBLE, with the same NaN outputs) and the car applies fail_u, as any car
 * without a usable plan. */
int f110qp_rollout_scan_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc,
                            const f110qp_scan_config* sc, int batch, const double* x_ref,
                            const float* ranges, double* x_traj, double* u_lin_traj, float* u_applied,
                            int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                            float* x_plan, float* hs_traj, void* stream);

/* Same on host pointers (synchronous): ranges staged to and hs_traj copied back from device
 * buffers of the context, one stream synchronisation at the end, as f110qp_rollout. */
int f110qp_rollout_scan(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                        int batch, const double* x_ref, const float* ranges, double* x_traj,
                        double* u_lin_traj, float* u_applied, int* status_traj, int* iters_traj,
                        double* cost_traj, float* u_plan, float* x_plan, float* hs_traj);

/* ---- planning stage in front of MPC::Update (src/project.cpp:73-152) ----------------------- */

typedef struct {
  int size;            /* occ_size, params.yaml:16 (OccGrid::size_ is int)                    */
  float discrete;      /* occ_discrete, params.yaml:17 (float)                                  */
  float dilation;      /* occ_dilation, params.yaml:18 (float)                                  */
  float lookahead;     /* lookahead, params.yaml:63 (Trajectory::lookahead is float)            */
  double speed_max;    /* umax as Traj_Plan reads it, params.yaml:46                            */
  double steer_max;    /* steer_max, params.yaml:60                                             */
  int steer_discrete;  /* params.yaml:59: T = steer_discrete + 1 candidates                     */
  int traj_discrete;   /* params.yaml:61: P points per candidate                               */
  double dt;           /* params.yaml:13 (Traj_Plan::dt is double)                              */
} f110qp_plan_config;

/* params.yaml defaults of the planning stage. */
void f110qp_default_plan_config(f110qp_plan_config* cfg);

/* Traj_Plan::generate_traj_table (src/trajectory_planner.cpp:26-72), host code: table
 * [T][P][3] doubles (car frame). Returns T (> 0) or a negative error code. */
int f110qp_traj_table(const f110qp_plan_config* cfg, double* table);

/* Trajectory::ReadCSV (src/trajectory.cpp:18-55) on CSV text in memory: wp[n][3] = (x, y, ori)
 * with the reference's float parsing and its (0u - 1) % n predecessor of point 0. Writes the
 * count to *n; returns F110QP_OK or F110QP_ERR_INVALID. */
int f110qp_parse_waypoints(const char* text, double* wp, int max_n, int* n);

/* The planning branch of project::OdomCallback (src/project.cpp:73-152) for B scenarios on the
 * device, one workgroup each: OccGrid::FillOccGrid of the scenario's LaserScan
 * (src/occupancy_grid.cpp:55-88), the collision check of the T candidates, the lookahead
 * waypoint (src/trajectory.cpp:81-126) and the nearest valid end point. Device pointers:
 *   pose [B][4] doubles (x, y, qz, qw; planar odometry pose), ranges [B][num_ranges],
 *   table [T][P][3] (f110qp_traj_table), waypoints [W][2] (x, y);
 * outputs: x_ref [B][P][3] = the chosen candidate in the map frame with ori 0 (miniPath_,
 * src/project.cpp:149-152; NaN without a candidate), x0 [B][3] = (x, y, GetCarOrientation)
 * for f110qp_solve_batch_dev, best_traj / best_global [B], status [B] (0 ok, 1 no valid
 * candidate — the reference returns before MPC, 2 no waypoint ahead — the reference throws);
 * valid [B][T] and grid [B][G][G] (G = size / discrete) may be NULL. */
int f110qp_plan_batch_dev(const f110qp_plan_config* cfg, int batch, const double* pose,
                          const float* ranges, int num_ranges, float angle_min,
                          float angle_increment, float angle_max, const double* table,
                          const double* waypoints, int num_waypoints, unsigned char* grid,
                          unsigned char* valid, int* best_global, int* best_traj, float* x_ref,
                          float* x0, int* status, void* stream);

/* Same on host pointers (synchronous; device buffers are cached per host thread). table and
 * waypoints are host arrays too. Used by the ROS-free host mirror for one scenario per tick. */
int f110qp_plan_batch(const f110qp_plan_config* cfg, int batch, const double* pose,
                      const float* ranges, int num_ranges, float angle_min, float angle_increment,
                      float angle_max, const double* table, const double* waypoints,
                      int num_waypoints, unsigned char* grid, unsigned char* valid,
                      int* best_global, int* best_traj, float* x_ref, float* x0, int* status);

/* ---- closed loop with re-planning: project::OdomCallback's per-car state on the device ----------
 * f110qp_rollout[_scan][_dev] hold x_ref for the whole call. The reference does not: a mini path of
 * traj_discrete = 50 points at dt 0.01 and umax 4.5 is 2.205 m long, project::OdomCallback drops it
 * once the car is within 1.98 m of its end (src/project.cpp:180-186), and the next callback plans
 * again (a re-plan about every 0.225 m driven, derived from those parameters). The calls below run
 * that loop for B cars and T ticks on one stream, without a host round trip. Additive:
 * F110QP_API_VERSION stays 6.
 *
 * Specification: per car, one tick is one Project::OdomCallback followed by one Project::DriveStep of
 * the host mirror (f110-mpc_amd/host/src/project.cpp:31-100), including its choice for the tick on
 * which the reference reads an emptied miniPath_: MPC::Update refuses the path, keeps its previous
 * solution, and that solution is re-published with the input index reset to 0.
 * Per-car state: have_path (get_mini_path_), the path x_ref[b] ([P][3] doubles that are widened
 * floats, ori 0, as miniPath_), the published plan u_held[b] ([N][2] float32), its length len (N or
 * 0) and the index idx (inputs_idx_).
 * A tick's kind is decided at the tick's pose:
 *   PLAN  have_path == 0. The planning branch (f110qp_plan_batch_dev's kernel) runs at this pose on
 *         this tick's scan row. Status 0: the path is stored, have_path = 1. Any other status
 *         (reported as F110QP_TICK_PLAN_FAILED): path and flag stay. No solve result is used;
 *         u_held, len, idx are untouched.
 *   HOLD  have_path == 1 and Transforms::CalcDist((float)x, (float)y, path end) < replan_dist (its
 *         float expression, compared as the reference compares a float with the double 1.98):
 *         have_path = 0, idx = 0; no solve result is used.
 *   MPC   have_path == 1 otherwise. The solve's plan is published: a usable status (F110QP_SOLVED,
 *         F110QP_SOLVED_INACCURATE) gives u_held = u*, len = N, idx = 0, any other len = 0, idx = 0
 *         (f110qp_advance_dev's choices).
 * Then, on every tick: DriveStep applies idx < len ? u_held[idx] : fail_u and idx++; the plant step
 * is f110qp_advance_dev's; u_lin_next = (v_lin, idx < len ? u_held[idx].steer : fail_u[1]). On an
 * uninterrupted run of MPC ticks this is f110qp_rollout_scan_dev for N >= 2; the calls below refuse
 * horizon < 2 (f110qp_advance_dev's N = 1 rule has no counterpart in the index model).
 * Modelling choices, next to the two of f110qp_advance_dev: the pose the planner reads is (x, y,
 * sin(ori / 2), cos(ori / 2)), the planar quaternion a simulator's odometry would carry, formed in
 * fp64 by the plant-step launch.
 * The solve runs for all B cars on every tick, unmasked, with the launch policy of
 * f110qp_solve_batch_dev_dbl at batch B (f110qp_backend_info, ... answer for it) and bit-identical to
 * that call (NaN half-space rows keep its F110QP_PRIMAL_INFEASIBLE). On PLAN, PLAN_FAILED and HOLD
 * ticks status_traj holds F110QP_NO_SOLVE and the car's rows of iters_traj, cost_traj, u_plan and
 * x_plan are unspecified (whatever the stale path gave, NaN for a caller's NaN path at tick 0);
 * nothing reads them. plan_status_traj, best_traj_traj and best_global_traj are written on PLAN /
 * PLAN_FAILED ticks only (unspecified elsewhere). */
#define F110QP_TICK_MPC 0
#define F110QP_TICK_PLAN 1
#define F110QP_TICK_HOLD 2
#define F110QP_TICK_PLAN_FAILED 3
#define F110QP_TICK_CRASHED 4     /* f110qp_rollout_contact[_dev] with stop_on_contact only: a parked car */
#define F110QP_NO_SOLVE 0         /* status_traj on a tick whose solve result is not used */

typedef struct {
  double replan_dist;       /* 1.98, src/project.cpp:182; positive and finite                        */
  f110qp_plan_config plan;  /* the planning stage; traj_discrete must equal the context's x_ref_points */
  int num_waypoints;        /* rows of `waypoints`                                                    */
} f110qp_replan_config;

/* replan_dist 1.98, f110qp_default_plan_config, num_waypoints 0 (the caller's). */
void f110qp_default_replan_config(f110qp_replan_config* rp);

/* f110qp_plan_batch_dev for the cars of a device-side list (one launch): list[0 .. min(*count,
 * batch)) names the cars, in any order; count is read on the device. pose is a pose row [B][4]
 * doubles, ranges [B][num_ranges] (sc: num_ranges, angle_min, angle_increment, angle_max). Per listed
 * car: plan_status, best_traj, best_global, and on status 0 the path into x_ref [B][P][3] as doubles
 * (the float32 values f110qp_plan_batch_dev writes, widened). A listed car with another status keeps
 * the path it has (no NaN is written); unlisted cars are not touched; count 0 changes nothing.
 * Workgroups stride over the list, at most min(batch, 768) of them (what the device holds at once);
 * one past the count exits at its first load. */
int f110qp_plan_listed_dev(const f110qp_replan_config* rp, const f110qp_scan_config* sc, int batch,
                           const int* list, const int* count, const double* pose, const float* ranges,
                           const double* table, const double* waypoints, double* x_ref,
                           int* plan_status, int* best_traj, int* best_global, void* stream);

/* The launch in front of the loop: pose [B][4] = (x, y, sin(ori/2), cos(ori/2)) of x [B][3], kind [B]
 * at that pose from have_path [B] and the path ends of x_ref [B][P][3], the cars whose kind is PLAN
 * appended to list [B] (one atomic per wavefront on *count, which must be zero on entry), and, with
 * hs non-NULL, f110qp_half_space_rows_dev(gap, x) into hs [B][2][3] (sc may be NULL when hs is). */
int f110qp_replan_start_dev(const f110qp_replan_config* rp, const f110qp_scan_config* sc, int batch,
                            const double* x, const int* have_path, const double* x_ref,
                            const f110qp_gap_record* gap, double* pose, int* kind, int* list,
                            int* count, float* hs, void* stream);

/* One tick's state machine and plant step (one launch, one thread per car): f110qp_advance_scan_dev
 * plus the rules above. Reads kind [B] (a PLAN tick with plan_status != 0 is rewritten
 * F110QP_TICK_PLAN_FAILED), plan_status [B] on PLAN ticks, status [B] and u_plan [B][N][2] on MPC
 * ticks, the path ends of x_ref; updates u_held [B][N][2], held_len, held_idx, have_path [B]; sets
 * status to F110QP_NO_SOLVE on ticks that are not MPC ticks; writes x_next, u_lin_next, u_applied (may
 * be NULL) with f110qp_advance_scan_dev's bits for the same applied input, pose_next [B][4], and,
 * unless kind_next is NULL, the next tick's kind and its PLAN cars appended to next_list [B] /
 * *next_count (zero on entry). hs_next [B][2][3] non-NULL: the rows at x_next from gap (sc required).
 * horizon >= 2; the argument rules of f110qp_advance_dev apply, u_held 8-byte aligned. */
int f110qp_advance_replan_dev(const f110qp_rollout_config* rc, const f110qp_replan_config* rp,
                              const f110qp_scan_config* sc, int batch, int horizon, const double* x,
                              int* kind, const float* u_plan, int* status, const int* plan_status,
                              const double* x_ref, const f110qp_gap_record* gap, float* u_held,
                              int* held_len, int* held_idx, int* have_path, double* x_next,
                              double* u_lin_next, float* u_applied, double* pose_next, int* kind_next,
                              int* next_list, int* next_count, float* hs_next, void* stream);

/* T ticks of that loop (device pointers, asynchronous on `stream`). f110qp_rollout_scan_dev's
 * arguments, except:
 *   table      [T_c][P][3] doubles (f110qp_traj_table), waypoints [num_waypoints][2] doubles
 *   x_ref      [B][P][3] doubles, in/out: the paths the cars hold (read only where have_path is 1)
 *   have_path  [B], in/out: with x_ref it lets a call continue the previous one. The held plan does
 *              not carry over: it starts empty on every call, like a fresh node.
 *   kind_traj, plan_status_traj, best_traj_traj, best_global_traj [T][B], pose_traj [T+1][B][4]: each
 *              may be NULL (workspaces of the context then).
 * The context's x_ref_points must equal rp->plan.traj_discrete, its horizon be >= 2.
 * Stream order: one memset of the per-tick plan counters, the gap search (when rows are computed, as
 * f110qp_rollout_scan_dev), f110qp_replan_start_dev; then per tick the listed plan on that tick's
 * list and scan row, the launches of f110qp_solve_batch_dev_dbl, and f110qp_advance_replan_dev. No
 * host synchronisation, read-back or allocation inside the loop; every argument is checked before
 * the first launch. */
int f110qp_rollout_replan_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc,
                              const f110qp_scan_config* sc, const f110qp_replan_config* rp, int batch,
                              const double* table, const double* waypoints, double* x_ref,
                              int* have_path, const float* ranges, double* x_traj, double* u_lin_traj,
                              float* u_applied, int* status_traj, int* iters_traj, double* cost_traj,
                              float* u_plan, float* x_plan, float* hs_traj, int* kind_traj,
                              int* plan_status_traj, int* best_traj_traj, int* best_global_traj,
                              double* pose_traj, void* stream);

/* Same on host pointers (synchronous): staged through device buffers of the context, one stream
 * synchronisation at the end, as f110qp_rollout_scan. */
int f110qp_rollout_replan(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                          const f110qp_replan_config* rp, int batch, const double* table,
                          const double* waypoints, double* x_ref, int* have_path, const float* ranges,
                          double* x_traj, double* u_lin_traj, float* u_applied, int* status_traj,
                          int* iters_traj, double* cost_traj, float* u_plan, float* x_plan,
                          float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                          int* best_global_traj, double* pose_traj);

/* ---- closed loop with a simulated LiDAR: scans ray-cast at every tick's pose ---------------------
 * f110qp_rollout_replan[_dev] reads scans made before the call: one per car held while the car
 * drives on (scan_rows = 1), or T rows taken at poses the loop has not produced yet. The reference
 * runs inside the f1tenth simulator, which publishes a fresh scan at every pose: ScanCallback fills
 * the occupancy grid from each of them (src/project.cpp:56), MPC keeps the first for its gap rows
 * (src/project.cpp:45-49). The calls below put that simulator's part on the device for a static world
 * of circles (cx, cy, r): walls and obstacles. Additive: F110QP_API_VERSION stays 6. */
typedef struct {
  int    num_circles;   /* C >= 0 circles per world                                                  */
  int    world_rows;    /* 1: one world for all cars; B: circles [B][C][3], car b reads row b        */
  double lidar_offset;  /* 0.275: LiDAR ahead of the pose along the heading (occupancy_grid.cpp:63-64) */
  double max_range;     /* 10.0; positive, finite                                                    */
} f110qp_world_config;

/* Zeroes *wc, then world_rows 1, lidar_offset 0.275, max_range 10.0 (the circles are the caller's). */
void f110qp_default_world_config(f110qp_world_config* wc);

/* Circles per LDS tile of the ray-cast kernel. No limit on num_circles: a larger world is processed
 * tile after tile. */
#define F110QP_CAST_CIRCLE_TILE 256

/* The scans of B cars in a world of circles (device pointers, asynchronous on `stream`, one launch):
 *   x [B][3] double, circles [world_rows][C][3] double = (cx, cy, r) -> ranges [B][num_ranges] float32
 * (sc: num_ranges, angle_min, angle_increment; sc->scan_rows is not read).
 * list / count both NULL: all B cars. Both given: the cars list[0 .. min(*count, B)), in any order,
 * count read on the device as in f110qp_plan_listed_dev; the rows of unlisted cars are not touched,
 * count 0 changes nothing. One of the two alone is F110QP_ERR_INVALID.
 * Arithmetic, all fp64, every product and sum rounded (no fused multiply-add):
 *   LiDAR origin o = (x + lidar_offset cos(ori), y + lidar_offset sin(ori));
 *   beam i along ori + ((double)angle_min + (double)angle_increment i), d = (cos, sin) of it;
 *   per circle p = c - o, t = p.d, d2 = p.p - t t; the beam hits when d2 <= r^2 && t > 0, at
 *   th = t - sqrt(max(r^2 - d2, 0)), which counts only when th > 0;
 *   range = (float)min(min over the circles of th, max_range).
 * Consequences: a LiDAR inside a circle sees through it (th <= 0 on every beam); only r^2 enters, so
 * a negative radius acts as its absolute value; a circle with a NaN or infinite field hits nothing
 * (every compare is false) and does not disturb its neighbours; C = 0 gives max_range everywhere.
 * The result is a minimum of per-pair values that do not depend on the other circles: it is
 * bit-identical for every order of the circle list. */
int f110qp_cast_scans_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc, int batch,
                          const int* list, const int* count, const double* x, const double* circles,
                          float* ranges, void* stream);

/* f110qp_rollout_replan_dev with tick t's scan cast at tick t's pose. The per-car specification is
 * that call's, word for word; only the source of the planner's scan row changes. Arguments as
 * f110qp_rollout_replan_dev, except:
 *   wc, circles  replace ranges (f110qp_cast_scans_dev's world); sc->scan_rows is not read
 *   ranges_traj  [T][B][num_ranges] float32, may be NULL: row t holds every car's scan at x_traj row t.
 * Planner scan: tick t's planning stage reads the scan cast at x_traj row t. With ranges_traj NULL
 * the cast runs on tick t's plan list only (the list and counter the listed plan reads next, in
 * stream order) into one buffer of the context of B rows; with ranges_traj it runs for all B cars
 * into row t. Trajectories, kinds and statuses are bit-identical either way.
 * Gap rows are the reference's: MPC sees the first scan only. When rows are computed (gap_mode
 * ACTIVE, or hs_traj given) one all-cars cast at x_traj row 0 and one f110qp_gap_search_dev on it run
 * in front of the loop; the records are held and the rows follow the car inside
 * f110qp_advance_replan_dev exactly as in f110qp_rollout_replan_dev at scan_rows = 1. A fresh gap
 * search per tick is not part of this call.
 * Stream order: the memset of the plan counters, then (rows computed) the cast at row 0 and the gap
 * search, f110qp_replan_start_dev; per tick the cast, the listed plan, the launches of
 * f110qp_solve_batch_dev_dbl, f110qp_advance_replan_dev. No host synchronisation, read-back or
 * allocation inside the loop; every argument is checked before the first launch (the checks of
 * f110qp_rollout_replan_dev and of f110qp_cast_scans_dev's world). */
int f110qp_rollout_world_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc,
                             const f110qp_scan_config* sc, const f110qp_replan_config* rp,
                             const f110qp_world_config* wc, int batch, const double* table,
                             const double* waypoints, double* x_ref, int* have_path, const double* circles,
                             double* x_traj, double* u_lin_traj, float* u_applied, int* status_traj,
                             int* iters_traj, double* cost_traj, float* u_plan, float* x_plan,
                             float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                             int* best_global_traj, double* pose_traj, float* ranges_traj, void* stream);

/* Same on host pointers (synchronous): staged through device buffers of the context, one stream
 * synchronisation at the end, as f110qp_rollout_replan. */
int f110qp_rollout_world(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                         const f110qp_replan_config* rp, const f110qp_world_config* wc, int batch,
                         const double* table, const double* waypoints, double* x_ref, int* have_path,
                         const double* circles, double* x_traj, double* u_lin_traj, float* u_applied,
                         int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                         float* x_plan, float* hs_traj, int* kind_traj, int* plan_status_traj,
                         int* best_traj_traj, int* best_global_traj, double* pose_traj,
                         float* ranges_traj);

/* ---- head-to-head races: the cars of a race see each other in the simulated LiDAR -----------------
 * In the world calls above every car drives alone. The reference is a racing controller: its gap rows
 * and its occupancy-grid planner exist to get past an opponent, and the simulator it runs in
 * publishes a scan that contains the other car. Model:
 *   - the B cars form B / G races of G consecutive cars: race g is cars gG .. gG + G - 1. Cars of
 *     different races never see each other;
 *   - at the tick whose poses are x [B][3], car b's LiDAR sees the static circles exactly as before
 *     (world_rows 1 or B stays orthogonal) and, for every other car m of its race, one more circle
 *       (x_m + center_offset cos(ori_m), y_m + center_offset sin(ori_m), car_radius),
 *     in fp64, each product and sum rounded, sincos(double): the expressions of the LiDAR origin;
 *   - a car never sees itself.
 * Opponent circles enter the same per-pair test and the same minimum as the static circles, so every
 * consequence stated at f110qp_cast_scans_dev carries over: a LiDAR inside an opponent's circle sees
 * through it; an opponent with a non-finite pose hits nothing and disturbs nobody; the result is
 * bit-identical for every order of the race's cars and of the static circles.
 * car_radius 0.3 covers a 0.58 x 0.31 m car and center_offset 0.1651 is half the 0.3302 wheelbase of
 * Model::Linearize (the circle sits over the middle of the car, the pose at its rear axle): both are
 * modelling choices of this library, not values of the reference. Additive: F110QP_API_VERSION stays 6. */
typedef struct {
  int    group_size;     /* G >= 1; batch % G == 0                                          */
  double car_radius;     /* finite, > 0                                                     */
  double center_offset;  /* finite: circle centre ahead of the pose along the heading       */
} f110qp_race_config;

/* Zeroes *race, then group_size 1, car_radius 0.3, center_offset 0.1651. */
void f110qp_default_race_config(f110qp_race_config* race);

/* f110qp_cast_scans_dev with the race-mates in every scan (one launch). Arguments and list / count
 * rules as there; x is read both as the casting poses and as the opponents' poses, so a listed car
 * reads the poses of its unlisted race-mates from x. num_circles == 0 with circles == NULL is valid:
 * the world is then the opponents only. group_size 1 gives f110qp_cast_scans_dev's bits.
 * F110QP_ERR_INVALID before any HIP call: a NULL race, group_size < 1, batch not a multiple of
 * group_size, a non-finite or non-positive car_radius, a non-finite center_offset, and every rule of
 * f110qp_cast_scans_dev. */
int f110qp_cast_scans_race_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                               const f110qp_race_config* race, int batch, const int* list,
                               const int* count, const double* x, const double* circles, float* ranges,
                               void* stream);

/* f110qp_rollout_world_dev, word for word, with every cast passing the race: the all-cars cast at row
 * 0 in front of the loop and the per-tick listed or all-cars cast read x_traj row t as the casting
 * poses and as the opponents' poses (row t is complete for every car when tick t's cast runs). The
 * gap records come from the first scan, so they hold the opponents where they stood at tick 0: the
 * reference keeps its first scan too (src/project.cpp:45-49), so this is its behaviour and not a
 * shortcut. Launches per tick, stream order and the absence of host synchronisation, read-back and
 * allocation inside the loop are f110qp_rollout_world_dev's; every argument is checked before the
 * first launch (that call's checks and f110qp_cast_scans_race_dev's race rules). */
int f110qp_rollout_race_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc,
                            const f110qp_scan_config* sc, const f110qp_replan_config* rp,
                            const f110qp_world_config* wc, const f110qp_race_config* race, int batch,
                            const double* table, const double* waypoints, double* x_ref, int* have_path,
                            const double* circles, double* x_traj, double* u_lin_traj, float* u_applied,
                            int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                            float* x_plan, float* hs_traj, int* kind_traj, int* plan_status_traj,
                            int* best_traj_traj, int* best_global_traj, double* pose_traj,
                            float* ranges_traj, void* stream);

/* Same on host pointers (synchronous), staged as f110qp_rollout_world. */
int f110qp_rollout_race(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                        const f110qp_replan_config* rp, const f110qp_world_config* wc,
                        const f110qp_race_config* race, int batch, const double* table,
                        const double* waypoints, double* x_ref, int* have_path, const double* circles,
                        double* x_traj, double* u_lin_traj, float* u_applied, int* status_traj,
                        int* iters_traj, double* cost_traj, float* u_plan, float* x_plan, float* hs_traj,
                        int* kind_traj, int* plan_status_traj, int* best_traj_traj, int* best_global_traj,
                        double* pose_traj, float* ranges_traj);

/* ---- contact: car-to-wall and car-to-car clearance, crashed cars park -------------------------------
 * In the calls above nothing can touch anything: a car that meets a wall drives through it, and in a race it
 * stays a moving circle in its race-mates' scans while it does. The f1tenth simulator the reference runs in
 * stops a car on collision; the calls below give this library's stand-in the same. Model: the body of a car
 * is the race model's circle, centre (x + center_offset cos(ori), y + center_offset sin(ori)), radius
 * car_radius (f110qp_race_config); a car touches the static circles of its world and the other cars of its
 * race, never a car of another race. A circle body and both numbers are modelling choices of this library, not
 * the reference's. There is no swept test between ticks: contact is judged at the poses of the rows only. At
 * 4.5 m/s and the default plant_dt a car moves 0.045 m per tick, against a body radius of 0.3 m plus the
 * walls' 0.12 m, so a car cannot step over a wall circle or a race-mate between two rows; a world of circles
 * thinner than a tick's travel, or a much larger plant_dt, is outside what this model detects.
 * Additive: F110QP_API_VERSION stays 6, and no call above changes its results. */

/* The clearance of rows x B poses (device pointers, asynchronous on `stream`, one launch):
 *   x [rows][B][3] double, circles [world_rows][C][3] double = (cx, cy, r)
 *   -> clearance [rows][B] double, nearest [rows][B] int (may be NULL).
 * The B cars of every row are B / G races as in f110qp_cast_scans_race_dev (G = race->group_size), the world
 * is f110qp_cast_scans_dev's (wc->lidar_offset and wc->max_range are checked as there and not read).
 * Arithmetic, all fp64, every product and sum rounded (no fused multiply-add), with off = race->center_offset
 * and R = race->car_radius:
 *   body centre q = (x + off cos(ori), y + off sin(ori)), one sincos(double): the LiDAR origin's and the race
 *   circle's expressions;
 *   static circle j = (cx, cy, r) of car b's world: dx = cx - qx, dy = cy - qy, d = sqrt(dx dx + dy dy) (the
 *   correctly rounded square root), v_j = (d - |r|) - R;
 *   race-mate m, every other car of b's race at the same row of x, with q_m built as q is: dx = q_m.x - q.x,
 *   dy = q_m.y - q.y, v = (d - R) - R;
 *   clearance[row][b] = the minimum of these values, nearest[row][b] = the index of the minimum: j for a static
 *   circle, C + i for the race-mate whose index inside the race is i; the lowest index wins on equal values.
 *   A candidate replaces the running minimum only when v < best, or when v == best with a lower index; the
 *   start value is +inf and -1, which is also the answer for C = 0, G = 1.
 * Consequences: a circle or mate with a NaN field gives a NaN v, which passes no compare: it is never chosen
 * and does not disturb the others (the same holds for an infinite centre coordinate: v = +inf never replaces
 * the start value; an infinite radius is, by the arithmetic, contact with everything: v = -inf). A car whose
 * own pose is non-finite keeps +inf and -1. A negative radius acts as its absolute value. Because the squares
 * are the same bits either way, car a's value against b is bit-identical to b's against a. The result is a
 * minimum of per-pair values that do not depend on the other obstacles: bit-identical for every order of the
 * circle list and of the race's cars, apart from nearest mapping through the permutation. Negative on
 * overlap, zero at touch.
 * F110QP_ERR_INVALID before any HIP call: every world rule of f110qp_cast_scans_dev, every race rule of
 * f110qp_cast_scans_race_dev, rows < 1, a NULL x or clearance. num_circles == 0 with circles == NULL is valid.
 * Workgroups stride over the cars, one car each, at most min(batch, 1024) of them (what the device holds at
 * once). */
int f110qp_clearance_dev(const f110qp_world_config* wc, const f110qp_race_config* race, int batch, int rows,
                         const double* x, const double* circles, double* clearance, int* nearest, void* stream);

typedef struct {
  int    stop_on_contact;  /* 0: record only; 1: a crashed car parks                       */
  double margin;           /* contact when clearance <= margin; default 0.0; finite        */
} f110qp_contact_config;

/* Zeroes *cc: stop_on_contact 0, margin 0.0. */
void f110qp_default_contact_config(f110qp_contact_config* cc);

/* f110qp_rollout_race_dev with every row's clearance recorded and, optionally, crashed cars parked.
 * Arguments as f110qp_rollout_race_dev, plus cc and
 *   clear_traj    [T+1][B] double: row t is f110qp_clearance_dev at x_traj row t
 *   nearest_traj  [T+1][B] int, may be NULL
 *   crash_tick    [B] int: the first row whose clearance is <= cc->margin, or -1 if there is none.
 * Stream order: f110qp_rollout_race_dev's, with one clearance launch on x_traj row 0 behind
 * f110qp_replan_start_dev (it also initialises crash_tick) and one on row t + 1 behind tick t's plant step:
 * one launch more per tick, no memset of its own inside the loop, no host synchronisation, read-back or
 * allocation inside the loop; every argument is checked before the first launch (that call's checks, a NULL
 * cc, a stop_on_contact other than 0 or 1, a non-finite margin, a NULL clear_traj or crash_tick).
 * stop_on_contact = 0: every array f110qp_rollout_race_dev writes is bit-identical to that call's.
 * stop_on_contact = 1: a car with crash_tick[b] = k parks from tick k on. At every tick t >= k: x_traj,
 * u_lin_traj and pose_traj row t + 1 repeat row t's bits; u_applied[t] = (0, 0); kind_traj[t] =
 * F110QP_TICK_CRASHED, written over the kind the previous tick announced, the way PLAN_FAILED is written over
 * PLAN; status_traj[t] = F110QP_NO_SOLVE (the car's rows of iters_traj, cost_traj, u_plan and x_plan are
 * unspecified, as on any tick without a solve); the car is not appended to the next plan list; its path flag
 * and held plan stay as they are; its half-space rows follow the unchanged pose; it stays where it stands as
 * a circle in its race-mates' scans and clearances. The car may have been listed for planning at tick k
 * itself, because that list was built before the crash was known: that plan is wasted and harmless (it may
 * rewrite the car's row of x_ref and of the plan records of tick k; nothing reads them again). Cars of a race
 * in which nobody has crashed yet are bit-identical to the stop_on_contact = 0 run. */
int f110qp_rollout_contact_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc,
                               const f110qp_scan_config* sc, const f110qp_replan_config* rp,
                               const f110qp_world_config* wc, const f110qp_race_config* race,
                               const f110qp_contact_config* cc, int batch, const double* table,
                               const double* waypoints, double* x_ref, int* have_path, const double* circles,
                               double* x_traj, double* u_lin_traj, float* u_applied, int* status_traj,
                               int* iters_traj, double* cost_traj, float* u_plan, float* x_plan,
                               float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                               int* best_global_traj, double* pose_traj, float* ranges_traj,
                               double* clear_traj, int* nearest_traj, int* crash_tick, void* stream);

/* Same on host pointers (synchronous), staged as f110qp_rollout_race; the three records are copied back. */
int f110qp_rollout_contact(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                           const f110qp_replan_config* rp, const f110qp_world_config* wc,
                           const f110qp_race_config* race, const f110qp_contact_config* cc, int batch,
                           const double* table, const double* waypoints, double* x_ref, int* have_path,
                           const double* circles, double* x_traj, double* u_lin_traj, float* u_applied,
                           int* status_traj, int* iters_traj, double* cost_traj, float* u_plan, float* x_plan,
                           float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                           int* best_global_traj, double* pose_traj, float* ranges_traj, double* clear_traj,
                           int* nearest_traj, int* crash_tick);

/* ---- rectangular car bodies: clearance, opponents in the LiDAR, rollout ---------------------------------
 * The race and contact calls above model a car as a circle of radius 0.3 m: twice as wide as the 0.58 x 0.31 m
 * car. The calls below take the car as an oriented rectangle, as the f1tenth simulator the reference runs in
 * does; they sit next to the circle calls, which keep their bits. Additive: F110QP_API_VERSION stays 6.
 *
 * The rectangle of the car at pose (x, y, ori): centre q = (x + off cos(ori), y + off sin(ori)) with off =
 * race->center_offset (the LiDAR origin's and the race circle's expressions, one sincos(double)), axes
 * f = (cos, sin) and l = (-sin, cos), half extents hl = half_length along f and hw = half_width along l.
 * race->car_radius is checked as before and not read.
 * Arithmetic: all fp64, every product and sum rounded (no fused multiply-add), the correctly rounded square
 * root, in the expression order written here. min and max of a NaN and a number give the number (fmin, fmax).
 *
 * 1. Point against rectangle, sd(p; q, f, hl, hw): d = p - q, u = d.x f.x + d.y f.y, w = d.y f.x - d.x f.y,
 *    au = |u| - hl, aw = |w| - hw. If au <= 0 and aw <= 0: sd = max(au, aw) (negative inside). Otherwise
 *    ex = (au < 0 ? 0 : au), ey = (aw < 0 ? 0 : aw), sd = sqrt(ex ex + ey ey): a NaN au or aw stays a NaN.
 * 2. Body against a static circle (cx, cy, r): v = sd(c; body) - |r|.
 * 3. Body b against race-mate m at the same row, with d = q_m - q_b, cc = |f_b.x f_m.x + f_b.y f_m.y| and
 *    cr = |f_m.x f_b.y - f_m.y f_b.x|, el = hl cc + hw cr and ew = hl cr + hw cc (the other car's extent on an
 *    f axis and on an l axis): the separating-axis gaps
 *      g_fb = (|d.f_b| - hl) - el, g_lb = (|d.l_b| - hw) - ew, g_fm = (|d.f_m| - hl) - el,
 *      g_lm = (|d.l_m| - hw) - ew     (d.f and d.l as u and w above),
 *    g = max(max(g_fb, g_fm), max(g_lb, g_lm)). If g <= 0 the rectangles touch or overlap and v = g (-g is
 *    the penetration depth). Otherwise v = min(cm(m, b), cm(b, m)), cm(A, B) = the least sd against B of the
 *    four corners of A, ((q.x + hl f.x) - hw f.y, (q.y + hl f.y) + hw f.x), ((q.x + hl f.x) + hw f.y,
 *    (q.y + hl f.y) - hw f.x), ((q.x - hl f.x) - hw f.y, (q.y - hl f.y) + hw f.x), ((q.x - hl f.x) + hw f.y,
 *    (q.y - hl f.y) - hw f.x), folded min(min(v0, v1), min(v2, v3)): the distance of two disjoint convex
 *    polygons is attained at a vertex of one of them, so this is the exact distance.
 *    Swapping b and m negates d and the cross term exactly and leaves cc's products as they are; the eight
 *    corner terms are the same function with the roles swapped: v is bit-identical in both directions.
 * 4. Clearance and nearest follow f110qp_clearance_dev rule for rule: index j for a circle, C + i for the mate
 *    with index i inside the race; a candidate replaces the running minimum only on v < best, or v == best with
 *    a lower index, from (+inf, -1); a NaN v is never chosen; a car with a non-finite pose keeps (+inf, -1); a
 *    negative radius acts as |r|; bit-identical for every order of the circles and of the race's cars.
 * 5. LiDAR, a beam along (dx, dy) from the origin o against the rectangle of mate m (a slab test in the
 *    mate's frame): p = q_m - o, o' = (-(p.f_m), -(p.l_m)), d' = (d.f_m, d.l_m). Per axis a with half extent h:
 *    when d'_a != 0, t1 = (-h - o'_a) / d'_a, t2 = (h - o'_a) / d'_a and the axis contributes
 *    [min(t1, t2), max(t1, t2)]; when d'_a == 0 it contributes (-inf, +inf) if |o'_a| <= h and a miss
 *    otherwise. th = the larger of the two lower ends; a hit when th <= the smaller of the two upper ends and
 *    th > 0, so a LiDAR inside an opponent's rectangle sees through it, as with a circle. An opponent with a
 *    non-finite pose hits nothing. range = (float)min(min over the static circles of th (the test of
 *    f110qp_cast_scans_dev, unchanged), min over the mates of th, max_range): per (beam, obstacle) pair the
 *    value depends on nothing else, so the result is bit-identical for every order of circles and cars. */
typedef struct {
  double half_length;  /* 0.29  (0.58 m car), finite, > 0 */
  double half_width;   /* 0.155 (0.31 m car), finite, > 0 */
} f110qp_body_config;

/* Zeroes *body, then half_length 0.29, half_width 0.155. */
void f110qp_default_body_config(f110qp_body_config* body);

/* f110qp_clearance_dev for rectangular bodies (rules 1 to 4; one launch): arguments and rules of that call.
 * F110QP_ERR_INVALID before any HIP call: every rule of f110qp_clearance_dev, a NULL body, a non-finite or
 * non-positive half_length or half_width. Workgroups stride over the cars, at most min(batch, 512) of them. */
int f110qp_clearance_body_dev(const f110qp_world_config* wc, const f110qp_race_config* race,
                              const f110qp_body_config* body, int batch, int rows, const double* x,
                              const double* circles, double* clearance, int* nearest, void* stream);

/* f110qp_cast_scans_race_dev with every race-mate the rectangle of rule 5 in place of the race circle (one
 * launch): arguments, list / count rules and errors of that call, plus the body rules above. The static circles
 * keep f110qp_cast_scans_dev's test; group_size 1 gives that call's bits. At most min(batch, 512) workgroups. */
int f110qp_cast_scans_body_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                               const f110qp_race_config* race, const f110qp_body_config* body, int batch,
                               const int* list, const int* count, const double* x, const double* circles,
                               float* ranges, void* stream);

/* f110qp_rollout_contact_dev with every cast f110qp_cast_scans_body_dev's and every clearance launch
 * f110qp_clearance_body_dev's: clear_traj row t is f110qp_clearance_body_dev at x_traj row t. Everything else
 * is that call's: arguments (body follows cc), launch count, stream order, no host synchronisation, read-back
 * or allocation inside the loop, parking at stop_on_contact = 1, and every argument checked before the first
 * launch (that call's checks and the body rules). With group_size 1 every array but clear_traj, nearest_traj
 * and crash_tick is bit-identical to f110qp_rollout_contact_dev's at stop_on_contact = 0. */
int f110qp_rollout_body_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                            const f110qp_replan_config* rp, const f110qp_world_config* wc,
                            const f110qp_race_config* race, const f110qp_contact_config* cc,
                            const f110qp_body_config* body, int batch, const double* table,
                            const double* waypoints, double* x_ref, int* have_path, const double* circles,
                            double* x_traj, double* u_lin_traj, float* u_applied, int* status_traj,
                            int* iters_traj, double* cost_traj, float* u_plan, float* x_plan, float* hs_traj,
                            int* kind_traj, int* plan_status_traj, int* best_traj_traj, int* best_global_traj,
                            double* pose_traj, float* ranges_traj, double* clear_traj, int* nearest_traj,
                            int* crash_tick, void* stream);

/* Same on host pointers (synchronous), staged as f110qp_rollout_contact. */
int f110qp_rollout_body(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                        const f110qp_replan_config* rp, const f110qp_world_config* wc,
                        const f110qp_race_config* race, const f110qp_contact_config* cc,
                        const f110qp_body_config* body, int batch, const double* table, const double* waypoints,
                        double* x_ref, int* have_path, const double* circles, double* x_traj,
                        double* u_lin_traj, float* u_applied, int* status_traj, int* iters_traj,
                        double* cost_traj, float* u_plan, float* x_plan, float* hs_traj, int* kind_traj,
                        int* plan_status_traj, int* best_traj_traj, int* best_global_traj, double* pose_traj,
                        float* ranges_traj, double* clear_traj, int* nearest_traj, int* crash_tick);

/* ---- straight walls: segments in the LiDAR, the clearance and the rollout -------------------------------
 * The worlds above are made of circles only, so a track wall is a chain of discs and every scan carries their
 * ripple. The calls below take a world that holds straight wall segments next to its circles, as the map of the
 * f1tenth simulator the reference runs in does; the body is the rectangle of the section above. They sit next
 * to the body calls, which keep their bits. Additive: F110QP_API_VERSION stays 6. The disc-body families get no
 * walls.
 *
 * segments is [wall_rows][S][4] double, each row (ax, ay, bx, by): the wall from a to b. A wall has no thickness
 * and is seen from both sides. wall_rows is independent of wc->world_rows. Arithmetic as everywhere in this
 * family: all fp64, every product and sum rounded (no fused multiply-add), sincos(double), the correctly rounded
 * square root and division; min and max of a NaN and a number give the number (fmin, fmax).
 *
 * W1. A beam against a segment. With the LiDAR origin o and the beam direction d = (cos, sin), both exactly as
 *     f110qp_cast_scans_dev builds them, A = a - o and B = b - o:
 *       ca = d.x A.y - d.y A.x,  cb = d.x B.y - d.y B.x,  ta = A.x d.x + A.y d.y,  tb = B.x d.x + B.y d.y,
 *       den = ca - cb.
 *     The beam meets the segment when the ends straddle it, (ca <= 0 && cb >= 0) || (ca >= 0 && cb <= 0), and
 *     den != 0, and th = ta + (tb - ta) * (ca / den) is > 0.
 *     range = (float)min(circles' th, mates' th (rule 5), segments' th, max_range).
 *     Consequences. A polyline whose consecutive segments share a vertex's bits cannot leak: ca of a shared
 *     vertex is the same number in both neighbours, so if the outer ends lie on opposite sides of the beam's
 *     line, one of the two straddles. (The usual form, which solves for the segment's own parameter and accepts
 *     it in [0, 1], computes that parameter separately for the two neighbours, and a beam through the joint can
 *     miss both; a leaked beam reads max_range, which the gap finder takes for a gap in the wall.) A segment seen
 *     exactly edge-on hits nothing (den == 0), and so does a zero-length segment. A LiDAR on a wall does not see
 *     that wall (th is not > 0). A segment with a NaN field fails every compare and disturbs nobody; one with an
 *     infinite field gives a NaN th by the arithmetic and hits nothing either. The value of a (beam, segment)
 *     pair depends on nothing else: the scan is bit-identical for every order of the segment list. Bits under
 *     swapping a and b are not promised.
 * W2. The rectangle against a segment. The body's frame is that of rules 1 to 3. Both ends into it: with
 *     d = a - q, a' = (ua, wa) = (d.x f.x + d.y f.y, d.y f.x - d.x f.y) (rule 1's u and w), b' = (ub, wb)
 *     likewise; e = b' - a', ee = e.x e.x + e.y e.y. When ee is NaN or +inf (a NaN or infinite field or pose)
 *     v = +inf, which no compare takes. Otherwise, with sd'(u, w) rule 1's value from au on (the point in the
 *     body's own frame: au = |u| - hl, aw = |w| - hw, ...), m = min(sd'(a'), sd'(b')).
 *     The crossing test is the slab test of rule 5 with o' = a', d' = e and the window [0, 1] in place of
 *     th > 0: the segment crosses or touches the rectangle when
 *       max(max(lower end on f, lower end on l), 0) <= min(min(upper end on f, upper end on l), 1).
 *     Crossing: v = min(m, 0): negative when an end lies inside, zero for a wall that passes through.
 *     Not crossing: v = min(m, k), k the least distance from the four corners to the segment. For a corner c
 *     of (hl, hw), (hl, -hw), (-hl, hw), (-hl, -hw) (rule 3's order): g = c - a', s = (g.x e.x + g.y e.y) / ee
 *     clamped by s < 0 ? 0 : (s > 1 ? 1 : s), s = 0 when ee == 0; r = g - s e (each product rounded), distance
 *     sqrt(r.x r.x + r.y r.y); folded min(min(k0, k1), min(k2, k3)). The distance of two disjoint convex sets is
 *     attained at a vertex of one of them, so this is the exact distance.
 *     In clearance and nearest, segment k has index C + G + k; circles keep j and mates C + i. The update rule,
 *     the start value (+inf, -1), the NaN rule and the order independence are rule 4's.
 *     Contact stays clearance <= margin: against a wall the value is <= 0 on contact (zero for a wall that
 *     touches or passes through with both ends outside), not strictly negative on overlap.
 * There is no swept test, as before: a tick moves a car 0.045 m against a half width of 0.155 m, so a car cannot
 * step over a wall between two rows. */
typedef struct {
  int num_segments;  /* S >= 0 segments per world                                        */
  int wall_rows;     /* 1: one set for all cars; B: segments [B][S][4], car b reads row b */
} f110qp_walls_config;

/* Zeroes *walls, then wall_rows 1. */
void f110qp_default_walls_config(f110qp_walls_config* walls);

/* f110qp_cast_scans_body_dev, word for word, with the segments in every scan (rule W1; one launch): walls
 * follows body, segments follows circles. F110QP_ERR_INVALID before any HIP call, on top of that call's rules:
 * a NULL walls, num_segments < 0, wall_rows other than 1 or batch, segments == NULL with num_segments > 0 (and
 * num_circles + group_size + num_segments above INT_MAX). num_segments == 0 with segments == NULL is valid and
 * gives f110qp_cast_scans_body_dev's bits; num_circles == 0 is valid. No cap on S. At most min(batch, 512)
 * workgroups. */
int f110qp_cast_scans_walls_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                                const f110qp_race_config* race, const f110qp_body_config* body,
                                const f110qp_walls_config* walls, int batch, const int* list, const int* count,
                                const double* x, const double* circles, const double* segments, float* ranges,
                                void* stream);

/* f110qp_clearance_body_dev, word for word, with the segments as a third stretch of the obstacle list (rule W2;
 * one launch). Errors as f110qp_cast_scans_walls_dev's wall rules on top of that call's; num_segments == 0 gives
 * f110qp_clearance_body_dev's bits. At most min(batch, 512) workgroups. */
int f110qp_clearance_walls_dev(const f110qp_world_config* wc, const f110qp_race_config* race,
                               const f110qp_body_config* body, const f110qp_walls_config* walls, int batch,
                               int rows, const double* x, const double* circles, const double* segments,
                               double* clearance, int* nearest, void* stream);

/* f110qp_rollout_body_dev, word for word, with every cast f110qp_cast_scans_walls_dev's and every clearance
 * launch f110qp_clearance_walls_dev's (walls follows body, segments follows circles): that call's launch count,
 * stream order, parking, and absence of host synchronisation, read-back and allocation inside the loop; every
 * argument is checked before the first launch (that call's checks and the wall rules). num_segments == 0 gives
 * f110qp_rollout_body_dev's bits in every array. */
int f110qp_rollout_walls_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                             const f110qp_replan_config* rp, const f110qp_world_config* wc,
                             const f110qp_race_config* race, const f110qp_contact_config* cc,
                             const f110qp_body_config* body, const f110qp_walls_config* walls, int batch,
                             const double* table, const double* waypoints, double* x_ref, int* have_path,
                             const double* circles, const double* segments, double* x_traj, double* u_lin_traj,
                             float* u_applied, int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                             float* x_plan, float* hs_traj, int* kind_traj, int* plan_status_traj,
                             int* best_traj_traj, int* best_global_traj, double* pose_traj, float* ranges_traj,
                             double* clear_traj, int* nearest_traj, int* crash_tick, void* stream);

/* Same on host pointers (synchronous), staged as f110qp_rollout_body; the segments are staged in. */
int f110qp_rollout_walls(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                         const f110qp_replan_config* rp, const f110qp_world_config* wc,
                         const f110qp_race_config* race, const f110qp_contact_config* cc,
                         const f110qp_body_config* body, const f110qp_walls_config* walls, int batch,
                         const double* table, const double* waypoints, double* x_ref, int* have_path,
                         const double* circles, const double* segments, double* x_traj, double* u_lin_traj,
                         float* u_applied, int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                         float* x_plan, float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                         int* best_global_traj, double* pose_traj, float* ranges_traj, double* clear_traj,
                         int* nearest_traj, int* crash_tick);

/* ---- closed loop with a refreshed MPC scan: the gap rows follow the world --------------------------------
 * In every world family above the gap records come from one all-cars cast at row 0 and are held for the whole
 * call, as the reference holds its first scan (src/project.cpp:45-49): only the end-point geometry follows the
 * car, and the rows of tick 40 describe where the walls and the opponents stood at tick 0. The family below is
 * f110qp_rollout_walls[_dev] with a refresh period for the scan MPC holds. The refresh period is a modelling
 * choice of this library, not the reference's; every = 0 is the reference. Additive: F110QP_API_VERSION stays 6,
 * and no call above changes its results. The disc-body families get no refresh. */
typedef struct {
  int every;   /* K >= 0. 0: never (the reference: MPC keeps its first scan). K >= 1: MPC's scan is replaced */
               /* at every tick t with 1 <= t <= T - 1 and t % K == 0 by the scan cast at x_traj row t       */
} f110qp_refresh_config;

/* Zeroes *rf: every = 0. */
void f110qp_default_refresh_config(f110qp_refresh_config* rf);

/* The gap search of `batch` scans and the end-point geometry at the given poses in ONE launch (device pointers,
 * asynchronous, one wavefront per car): ranges [B][num_ranges] float32, states [B][3] double -> gap_out [B] and
 * hs_out [B][2][3] float32. gap_out is bit-identical to f110qp_gap_search_dev on the same scans, and hs_out to
 * f110qp_half_space_rows_dev on those records and states (and so to f110qp_find_half_spaces_dev_dbl). A scan
 * without a gap gives the record with NaN r_lo / r_hi and NaN rows, as those calls do. sc->scan_rows is not read.
 * F110QP_ERR_INVALID before any HIP call: a NULL sc, ranges, states, gap_out or hs_out, batch < 1, and every sc
 * rule that f110qp_gap_search_dev checks. */
int f110qp_gap_refresh_dev(const f110qp_scan_config* sc, int batch, const float* ranges, const double* states,
                           f110qp_gap_record* gap_out, float* hs_out, void* stream);

/* f110qp_rollout_walls_dev, word for word, with rf following walls.
 *   Argument check. F110QP_ERR_INVALID before the first launch for a NULL rf or every < 0, on top of every check
 *     of the walls call.
 *   every == 0. The call makes the launches of f110qp_rollout_walls_dev, and every array is bit-identical to
 *     that call's. So is a call whose every exceeds T - 1.
 *   No rows computed (gap_mode INACTIVE and hs_traj NULL): rf is checked and otherwise not read; no extra launch.
 *   Refresh tick. At a tick t with 1 <= t <= T - 1 and t % every == 0, tick t's cast runs for all B cars (parked
 *     cars included) at x_traj row t: with ranges_traj into row t, where it already goes; without it into the
 *     context's buffer of B rows, in place of the listed cast. The listed plan reads the rows it would have read
 *     (a car's scan does not depend on the list).
 *   Refresh launch. One f110qp_gap_refresh_dev launch follows on that scan row and x_traj row t. It replaces all
 *     B held records and overwrites the rows that tick t's solve reads (those that tick t - 1's plant step had
 *     computed from the old record). It runs before the listed plan and the solve of tick t.
 *   Later ticks. From tick t on the fused plant step builds the next rows from the new records, as it does from
 *     the first ones.
 *   Non-refresh tick. Exactly the walls call's launches.
 *   Added work. A refresh tick adds one launch (and, with ranges_traj NULL, casts all cars instead of the listed
 *     ones). No memset, host synchronisation, read-back or allocation is added inside the loop.
 *   Inherited. Parking, clearances, crash_tick, NaN rows (a refreshed scan without a gap), fail_u and every
 *     stream-order statement are the walls call's. */
int f110qp_rollout_refresh_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                               const f110qp_replan_config* rp, const f110qp_world_config* wc,
                               const f110qp_race_config* race, const f110qp_contact_config* cc,
                               const f110qp_body_config* body, const f110qp_walls_config* walls,
                               const f110qp_refresh_config* rf, int batch, const double* table,
                               const double* waypoints, double* x_ref, int* have_path, const double* circles,
                               const double* segments, double* x_traj, double* u_lin_traj, float* u_applied,
                               int* status_traj, int* iters_traj, double* cost_traj, float* u_plan, float* x_plan,
                               float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                               int* best_global_traj, double* pose_traj, float* ranges_traj, double* clear_traj,
                               int* nearest_traj, int* crash_tick, void* stream);

/* Same on host pointers (synchronous), staged as f110qp_rollout_walls: the call adds no array. */
int f110qp_rollout_refresh(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                           const f110qp_replan_config* rp, const f110qp_world_config* wc,
                           const f110qp_race_config* race, const f110qp_contact_config* cc,
                           const f110qp_body_config* body, const f110qp_walls_config* walls,
                           const f110qp_refresh_config* rf, int batch, const double* table,
                           const double* waypoints, double* x_ref, int* have_path, const double* circles,
                           const double* segments, double* x_traj, double* u_lin_traj, float* u_applied,
                           int* status_traj, int* iters_traj, double* cost_traj, float* u_plan, float* x_plan,
                           float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                           int* best_global_traj, double* pose_traj, float* ranges_traj, double* clear_traj,
                           int* nearest_traj, int* crash_tick);

/* ---- a noisy LiDAR: seeded range noise and dropout, for Monte Carlo closed loops --------------------------
 * Every scan above is the exact geometric range, so two cars with the same start in the same world drive the
 * same bits. The family below is f110qp_rollout_refresh[_dev] with range noise and dropout on every scan it
 * casts: one batch gives M independent hypotheses of one situation, and a run repeats exactly. The noise is
 * built from integers only (a counter-based hash and a sum of four 16-bit fields as the bell curve; no log, cos
 * or library generator), so any host computes the same bits. A modelling choice of this library, not the
 * reference's; the all-zero config is the refresh family. Additive: F110QP_API_VERSION stays 6, and no call above
 * changes its results. The disc-body families get no noise.
 *
 * Z1. Draws. All arithmetic is unsigned 64-bit and wraps. K = 0x9E3779B97F4A7C15, and mix(z) is
 *       z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 *     For car b, tick t and beam i (the beam's index in the whole scan):
 *       kc = mix(seed + K * (uint64)(car_base + b + 1))
 *       kt = mix(kc + K * (uint64)(t + 1))
 *       h  = mix(kt + K * (uint64)(i + 1))
 *       h2 = mix(h + K)
 *       g  = (h & 0xffff) + ((h >> 16) & 0xffff) + ((h >> 32) & 0xffff) + (h >> 48) - 131070,
 *            a signed integer in [-131070, 131070];
 *       d  = h2 >> 40, 24 bits.
 *     Known answers for seed 1234, car_base + b = 0, t = 0, beams 0 to 3:
 *       h = 0x52b6d2127195ace2, 0x47208de8f3630884, 0x4c2edc5013e0a4f2, 0x8f2930e8f7aeddb0
 *       g = 17217, -12047, -7854, 38257
 *       d = 5026570, 3948636, 15546533, 623436
 * Z2. A beam. r is the float32 range f110qp_cast_scans_walls_dev writes for that beam, q = (double)r,
 *     mr = (float)max_range and drop24 = (unsigned)floor(dropout * 16777216.0) (taken on the host, once per
 *     call; dropout = 1 drops every beam). In this order:
 *       1. r == mr (no return): the output is r, untouched;
 *       2. d < drop24: the output is mr;
 *       3. otherwise sigma = sigma_abs + sigma_rel * q, e = (sigma * (double)g) * U and the output is
 *          (float)fmin(fmax(q + e, 0.0), max_range).
 *     Every product and sum is rounded (no fused multiply-add), as everywhere in this family.
 *     U = 0x1.bb67ae86627e8p-16, the double nearest to sqrt(3 / (2^32 - 1)): the reciprocal of the standard
 *     deviation of the sum of four uniform 16-bit fields.
 *     Consequences. g * U has mean 0 and standard deviation 1 and lies within +-3.4642: the noise is bounded.
 *     The value of a beam depends only on (r, seed, car_base + b, t, i) and the config: not on the list, the
 *     grid, the tile, the other cars or the batch size. With sigma_abs = sigma_rel = dropout = 0 the output is
 *     r exactly. The noise is applied to the float32-rounded range on purpose: the noisy scan is a pure function
 *     of the noise-free scan.
 * Z3. Ticks. In a rollout the all-cars cast at row 0 uses t = 0, and tick t's cast (listed or all-cars, refresh
 *     or not) uses t: tick 0's listed cast at the same pose equals row 0's scan, as in the families above. */
typedef struct {
  unsigned long long seed;   /* the run                                                      */
  long long car_base;        /* >= 0: car b draws from stream car_base + b (what a sharded   */
                             /* caller sets to the shard's first global car)                 */
  double sigma_abs;          /* >= 0, metres                                                 */
  double sigma_rel;          /* >= 0, per metre of range: sigma = sigma_abs + sigma_rel * q  */
  double dropout;            /* in [0, 1]: share of beams that return nothing                */
} f110qp_noise_config;

/* Zeroes *noise: no noise. */
void f110qp_default_noise_config(f110qp_noise_config* noise);

/* f110qp_cast_scans_walls_dev, word for word, with rules Z1 and Z2 on every beam it writes (one launch, the noise
 * in the kernel's own store loop): noise follows walls, and tick (rule Z3's t) follows batch. F110QP_ERR_INVALID
 * before any HIP call, on top of that call's rules: a NULL noise, a negative or non-finite sigma_abs or
 * sigma_rel, dropout outside [0, 1] or NaN, car_base < 0 or car_base + batch above LLONG_MAX, tick < 0. The
 * all-zero config gives f110qp_cast_scans_walls_dev's bits (through the same kernel as any other config).
 * Listed cars get the bits of the all-cars cast; unlisted rows are not touched. At most min(batch, 512)
 * workgroups. */
int f110qp_cast_scans_noisy_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                                const f110qp_race_config* race, const f110qp_body_config* body,
                                const f110qp_walls_config* walls, const f110qp_noise_config* noise, int batch,
                                int tick, const int* list, const int* count, const double* x,
                                const double* circles, const double* segments, float* ranges, void* stream);

/* f110qp_rollout_refresh_dev, word for word, with noise following rf: every cast is f110qp_cast_scans_noisy_dev's
 * with rule Z3's tick, so the planner, the gap records at row 0 and every refreshed record read noisy scans, and
 * ranges_traj holds them. The clearances never read the noise. That call's launch count, stream order, parking
 * and absence of host synchronisation, read-back and allocation inside the loop; every argument is checked before
 * the first launch (that call's checks, then rf, the noise rules above coming behind the walls'). The all-zero
 * config gives f110qp_rollout_refresh_dev's bits in every array. */
int f110qp_rollout_noisy_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                             const f110qp_replan_config* rp, const f110qp_world_config* wc,
                             const f110qp_race_config* race, const f110qp_contact_config* cc,
                             const f110qp_body_config* body, const f110qp_walls_config* walls,
                             const f110qp_refresh_config* rf, const f110qp_noise_config* noise, int batch,
                             const double* table, const double* waypoints, double* x_ref, int* have_path,
                             const double* circles, const double* segments, double* x_traj, double* u_lin_traj,
                             float* u_applied, int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                             float* x_plan, float* hs_traj, int* kind_traj, int* plan_status_traj,
                             int* best_traj_traj, int* best_global_traj, double* pose_traj, float* ranges_traj,
                             double* clear_traj, int* nearest_traj, int* crash_tick, void* stream);

/* Same on host pointers (synchronous), staged as f110qp_rollout_refresh: the call adds no array. */
int f110qp_rollout_noisy(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                         const f110qp_replan_config* rp, const f110qp_world_config* wc,
                         const f110qp_race_config* race, const f110qp_contact_config* cc,
                         const f110qp_body_config* body, const f110qp_walls_config* walls,
                         const f110qp_refresh_config* rf, const f110qp_noise_config* noise, int batch,
                         const double* table, const double* waypoints, double* x_ref, int* have_path,
                         const double* circles, const double* segments, double* x_traj, double* u_lin_traj,
                         float* u_applied, int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                         float* x_plan, float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                         int* best_global_traj, double* pose_traj, float* ranges_traj, double* clear_traj,
                         int* nearest_traj, int* crash_tick);

/* ---- occupancy-grid maps: raster walls in the LiDAR, the clearance and the rollout --------------------------
 * Every world above is hand-built geometry: circles and straight segments. The reference drives in the f1tenth
 * simulator on a map_server map, a raster image with a resolution and an origin, and a building map has tens of
 * thousands of boundary edges where the walls cast is linear in the segment count. The family below is
 * f110qp_rollout_noisy[_dev] with such a map under every cast and every clearance: a beam walks the grid cell by
 * cell, which costs the beam's length in cells whatever the map holds. Additive: F110QP_API_VERSION stays 6, and
 * no call above changes its results. The disc-body families get no map.
 *
 * grid is [H][W] unsigned char, row j at y, column i at x: cell (i, j) is the square whose lower-left corner is
 * (origin_x + i resolution, origin_y + j resolution). Nonzero means occupied. There is one map for all cars (no
 * per-car rows), and outside the map is free space. Arithmetic is this family's: all fp64, every product, sum and
 * quotient rounded (no fused multiply-add), sincos(double), floor, fmin / fmax.
 *
 * G1. A beam against the grid. With the LiDAR origin o and the beam direction d = (cos, sin), both exactly as
 *     f110qp_cast_scans_dev builds them:
 *       px = (o.x - origin_x) / resolution,  py likewise;  gx = d.x / resolution,  gy = d.y / resolution;
 *       ix = (int)floor(px),  iy = (int)floor(py).
 *     The start cell outside [0, W) x [0, H), or px or py not finite: the grid gives no hit. The start cell
 *     occupied: th = 0. Otherwise the beam walks. The next boundary in x is kx = ix + 1 when d.x > 0 and kx = ix
 *     when d.x < 0, its parameter tx = ((double)kx - px) / gx, and tx = +inf when d.x == 0; ty likewise. Both are
 *     computed afresh from the integer boundary at every step, never accumulated: a cell's entry parameter depends
 *     on that boundary alone, and it is monotone along the walk. Each step, in this order:
 *       1. tx <= ty: t = tx and ix moves by the sign of d.x; otherwise t = ty and iy moves by the sign of d.y;
 *       2. t > max_range, or t is NaN: no hit;
 *       3. the new cell is outside the map: no hit;
 *       4. the new cell is occupied: th = t + 0.0 (t, with the -0 that the quotient 0 / g gives for a negative g
 *          made +0: a LiDAR exactly on a cell boundary that looks down the axis into an occupied neighbour).
 *     On the tie tx == ty the beam steps in x first: a beam through a lattice corner visits the x-side cell. The
 *     walk takes at most W + H + 2 steps.
 *     range = (float)min(circles' th, mates' th, segments' th, grid th, max_range); rule Z2's noise then runs on
 *     that float as before.
 *     Consequences. A 4-connected wall cannot leak. Nor can one that is only 8-connected: the walk moves along one
 *     axis a step, so between two cells that touch at a corner it visits one of the two cells beside that corner,
 *     and on the exact tie the x-side one. A LiDAR inside an occupied cell reads 0. th is never -0, so rule Z2's
 *     fmax never meets zeros of two signs. The value of a (beam, map) pair does not depend on the batch, the list,
 *     the tile, or where the kernel keeps the map.
 * G2. The rectangle against the grid. The body's frame is that of rules 1 to 3, q its centre. With
 *     R = sqrt(hl hl + hw hw) + reach, the window is the cells (i, j) with
 *       floor((q.x - R - origin_x) / resolution) <= i <= floor((q.x + R - origin_x) / resolution)
 *     and the same in y, clipped to the map. A non-finite pose visits no cell. For each occupied cell of the window
 *     the corners are x0 = origin_x + (double)i resolution, x1 = origin_x + (double)(i + 1) resolution, y0 and y1
 *     likewise; v is the minimum (fmin) of rule W2's value over the four edges in the order (x0,y0)-(x1,y0),
 *     (x1,y0)-(x1,y1), (x1,y1)-(x0,y1), (x0,y1)-(x0,y0); and when x0 <= q.x < x1 && y0 <= q.y < y1 the body's
 *     centre is in the cell and v = min(v, 0).
 *     In clearance and nearest the cell has index C + G + S + j W + i, which must fit an int. The update rule, the
 *     start value (+inf, -1), the NaN rule and the order independence are rule 4's.
 *     Consequence. The grid's share of the clearance is exact wherever it is <= reach; a larger value, or +inf,
 *     says only "more than reach". Contact (<= margin, margin far below reach) is therefore exact. */
typedef struct {
  int width, height;          /* W, H >= 0 cells; W * H == 0: no map                        */
  double origin_x, origin_y;  /* world position of the lower-left corner of cell (0, 0)     */
  double resolution;          /* > 0 and finite, metres per cell                            */
  double reach;               /* >= 0, metres: how far beyond the body the clearance looks  */
} f110qp_grid_config;

/* Zeroes *grid_cfg, then resolution 0.05 and reach 1.0. */
void f110qp_default_grid_config(f110qp_grid_config* grid_cfg);

/* f110qp_cast_scans_noisy_dev, word for word (tick included), with rule G1 under every beam: grid_cfg follows
 * noise, grid follows segments. No launch is added: the walk runs inside the cast's own launch, between the last
 * obstacle tile and the store loop that applies rule Z2. The workgroup keeps the cells within max_range of its
 * LiDAR in LDS, one bit a cell, when that square fits (about 10 m at 0.05 m a cell); otherwise it reads the map
 * from global memory: the same walk, the same bits. F110QP_ERR_INVALID before any HIP call, on top of that call's
 * rules: a NULL grid_cfg, a negative width or height, width * height > 0 with grid == NULL, resolution not finite
 * or <= 0, reach negative or not finite, a non-finite origin, num_circles + group_size + num_segments +
 * width * height above INT_MAX. width * height == 0 with grid == NULL is valid and gives
 * f110qp_cast_scans_noisy_dev's bits. At most min(batch, 512) workgroups. */
int f110qp_cast_scans_grid_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                               const f110qp_race_config* race, const f110qp_body_config* body,
                               const f110qp_walls_config* walls, const f110qp_noise_config* noise,
                               const f110qp_grid_config* grid_cfg, int batch, int tick, const int* list,
                               const int* count, const double* x, const double* circles, const double* segments,
                               const unsigned char* grid, float* ranges, void* stream);

/* f110qp_clearance_walls_dev, word for word, with the occupied cells of the map as a fourth stretch of the obstacle
 * list (rule G2; one launch, that call's grid-stride launch): grid_cfg follows walls, grid follows segments. Errors
 * as f110qp_cast_scans_grid_dev's grid rules on top of that call's; an empty map gives f110qp_clearance_walls_dev's
 * bits. At most min(batch, 512) workgroups. */
int f110qp_clearance_grid_dev(const f110qp_world_config* wc, const f110qp_race_config* race,
                              const f110qp_body_config* body, const f110qp_walls_config* walls,
                              const f110qp_grid_config* grid_cfg, int batch, int rows, const double* x,
                              const double* circles, const double* segments, const unsigned char* grid,
                              double* clearance, int* nearest, void* stream);

/* f110qp_rollout_noisy_dev, word for word, with every cast f110qp_cast_scans_grid_dev's and every clearance launch
 * f110qp_clearance_grid_dev's (grid_cfg follows noise, grid follows segments): that call's launch count, stream
 * order, parking, refresh and noise ticks, and absence of host synchronisation, read-back and allocation inside
 * the loop; every argument is checked before the first launch (that call's checks with the grid rules behind the
 * noise's). An empty map gives f110qp_rollout_noisy_dev's bits in every array. */
int f110qp_rollout_grid_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                            const f110qp_replan_config* rp, const f110qp_world_config* wc,
                            const f110qp_race_config* race, const f110qp_contact_config* cc,
                            const f110qp_body_config* body, const f110qp_walls_config* walls,
                            const f110qp_refresh_config* rf, const f110qp_noise_config* noise,
                            const f110qp_grid_config* grid_cfg, int batch, const double* table,
                            const double* waypoints, double* x_ref, int* have_path, const double* circles,
                            const double* segments, const unsigned char* grid, double* x_traj, double* u_lin_traj,
                            float* u_applied, int* status_traj, int* iters_traj, double* cost_traj, float* u_plan,
                            float* x_plan, float* hs_traj, int* kind_traj, int* plan_status_traj,
                            int* best_traj_traj, int* best_global_traj, double* pose_traj, float* ranges_traj,
                            double* clear_traj, int* nearest_traj, int* crash_tick, void* stream);

/* Same on host pointers (synchronous), staged as f110qp_rollout_noisy; the map is staged in once. */
int f110qp_rollout_grid(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                        const f110qp_replan_config* rp, const f110qp_world_config* wc,
                        const f110qp_race_config* race, const f110qp_contact_config* cc,
                        const f110qp_body_config* body, const f110qp_walls_config* walls,
                        const f110qp_refresh_config* rf, const f110qp_noise_config* noise,
                        const f110qp_grid_config* grid_cfg, int batch, const double* table, const double* waypoints,
                        double* x_ref, int* have_path, const double* circles, const double* segments,
                        const unsigned char* grid, double* x_traj, double* u_lin_traj, float* u_applied,
                        int* status_traj, int* iters_traj, double* cost_traj, float* u_plan, float* x_plan,
                        float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                        int* best_global_traj, double* pose_traj, float* ranges_traj, double* clear_traj,
                        int* nearest_traj, int* crash_tick);

/* ---- distance field of the raster map: exact transform, inflation, pose lookups -----------------------------
 * The map of the family above is static: one map serves all cars and all ticks, and rule G2 answers "how far is
 * the wall" only up to reach. The calls below compute the map's exact Euclidean distance transform once, on the
 * device, and read two things off it: the map inflated by a radius, and the wall distance at any [rows][B][3]
 * pose array (x_traj among them). They run after the fact and take no context. Additive: F110QP_API_VERSION
 * stays 6, and no call above changes its results.
 *
 * The map is the grid family's: grid [H][W] unsigned char, nonzero occupied, cell (i, j) at linear index j W + i,
 * and its f110qp_grid_config as it is. Every call below checks that family's rules on the config first (a NULL
 * config, a negative width or height, resolution not finite or <= 0, reach negative or not finite, a non-finite
 * origin), although no call below reads reach in its arithmetic. On top of them width and height are at most
 * F110QP_FIELD_MAX_SIDE = 32,768: then every squared cell distance is at most 2 x 32,767^2 = 2,147,352,578 <
 * 2^31 - 1, the sums below fit an int, and INT_MAX is free as a mark.
 *
 * D1. Squared distance. d2[j][i] (int) is the minimum over the occupied cells (p, q) of (i - p)^2 + (j - q)^2; it
 *     is 0 on an occupied cell, and INT_MAX everywhere on a map with no occupied cell. Integer arithmetic alone.
 * D2. Nearest cell. nearest[j][i] (int) is q W + p of a minimiser of D1, among several the least linear index;
 *     -1 where d2 is INT_MAX.
 *     Consequence. The rule is separable. Along a row the nearer of a cell's two occupied row-neighbours wins, and
 *     the smaller p wins a tie; down a column the least q wins among the rows that reach the minimum, and that
 *     row's p is its row's. (A minimiser in row q is a nearest occupied cell of row q to column i, and of two
 *     such cells the one with the smaller p has the smaller index.) So the result depends on nothing but the map:
 *     not on the order of a search, a tile, or the number of threads.
 * D3. Metres. dist(d2) = resolution * sqrt((double)d2): fp64, the correctly rounded root, one rounded product, no
 *     fused multiply-add. dist(INT_MAX) = +inf. It is the distance between the centre of the cell and the centre
 *     of the nearest occupied cell.
 *     Consequences. A point in a cell and a point in an occupied cell are each within resolution sqrt(2) / 2 of
 *     their cell's centre, so for a point q in a free cell the distance from q to the occupied area is at least
 *     dist - resolution sqrt(2). For the rectangle of rules 1 to 3 centred in that cell, every point of which is
 *     within sqrt(hl hl + hw hw) of its centre, the grid's share of rule G2's clearance is at least
 *     dist - resolution sqrt(2) - sqrt(hl hl + hw hw).
 * D4. Lookup of a point. With px = (x - origin_x) / resolution and py likewise (rule G1's expressions), a point
 *     is outside the map when it fails 0 <= px < W && 0 <= py < H; a non-finite point fails that test. A point
 *     outside the map gives dist = NaN (0x7ff8000000000000) and cell = -1: the field says nothing there, and
 *     f110qp_mc_fan_dev counts a NaN as a missing sample. Otherwise ix = (int)floor(px), iy likewise,
 *     dist = dist(d2[iy][ix]) and cell = nearest[iy][ix]. The point is the pose's (x, y) as stored: the heading is
 *     not read, and a caller who wants the body centre passes body centres. That keeps sincos out of the rule, so
 *     the lookup is exact to the bit.
 * Inflation. out[j][i] = (dist(d2[j][i]) <= radius) ? 1 : 0, radius >= 0 and finite. Radius 0 gives the map back
 *     as 0 / 1.
 *     Consequence, from D3. Take radius >= sqrt(hl hl + hw hw) + resolution sqrt(2). Then a body centred anywhere
 *     in a cell that the inflated map leaves free has a positive rule-G2 clearance to the original map (as far
 *     as reach lets rule G2 see: beyond it the rule says "more than reach", which is positive too). */
#define F110QP_FIELD_MAX_SIDE 32768

/* Rules D1 and D2 on the device, asynchronous on `stream`: grid [H][W] -> d2 [H][W] int and, unless NULL, nearest
 * [H][W] int. work is [H][W] int of the caller's scratch; its contents after the call are unspecified. Two
 * launches (the rows, the columns), no allocation, no synchronisation, no read-back. F110QP_ERR_INVALID before
 * any HIP call: the grid family's rules, a side above F110QP_FIELD_MAX_SIDE, and, with width * height > 0, a NULL
 * grid, d2 or work. width * height == 0 returns F110QP_OK and launches nothing. */
int f110qp_grid_distance_dev(const f110qp_grid_config* grid_cfg, const unsigned char* grid, int* d2, int* nearest,
                             int* work, void* stream);

/* The inflation of d2 [H][W] (f110qp_grid_distance_dev's) at `radius` metres -> out [H][W] unsigned char of 0 / 1,
 * a map that every call of the grid family accepts under the same grid_cfg. One launch. F110QP_ERR_INVALID before
 * any HIP call: the rules above, radius negative or not finite, and, with width * height > 0, a NULL d2 or out. */
int f110qp_grid_inflate_dev(const f110qp_grid_config* grid_cfg, const int* d2, double radius, unsigned char* out,
                            void* stream);

/* Rule D4 at the poses x [rows][batch][3] double (the heading is not read) -> dist [rows][batch] double and, unless
 * NULL, cell [rows][batch] int; nearest is NULL exactly when cell is. batch and rows as f110qp_progress_dev
 * (>= 1, rows x batch <= 2^30). One launch of at most 2,048 workgroups striding over the poses.
 * F110QP_ERR_INVALID before any HIP call: the rules above, batch or rows < 1 or too large, a NULL x or dist, nearest
 * given without cell or cell without nearest, and, with width * height > 0, a NULL d2. With width * height == 0
 * every pose is outside the map. */
int f110qp_grid_lookup_dev(const f110qp_grid_config* grid_cfg, const int* d2, const int* nearest, int batch, int rows,
                           const double* x, double* dist, int* cell, void* stream);

/* f110qp_grid_distance_dev and, where `inflated` is not NULL, f110qp_grid_inflate_dev at `radius`, on host pointers
 * (synchronous): grid [H][W] -> d2 [H][W], nearest [H][W] unless NULL, inflated [H][W] unless NULL (radius is read
 * only with it). Staged through device buffers that the call owns and frees on every way out, one synchronisation;
 * the same bits as the device calls. */
int f110qp_grid_field(const f110qp_grid_config* grid_cfg, const unsigned char* grid, double radius, int* d2,
                      int* nearest, unsigned char* inflated);

/* f110qp_grid_distance_dev, then f110qp_grid_lookup_dev, on host pointers (synchronous): the map and x
 * [rows][batch][3] -> dist [rows][batch] and, unless NULL, cell [rows][batch]. Staged as f110qp_grid_field; the same
 * bits as the device calls. */
int f110qp_wall_distance(const f110qp_grid_config* grid_cfg, const unsigned char* grid, int batch, int rows,
                         const double* x, double* dist, int* cell);

/* ---- raster LiDAR through the distance field: beams skip free space ----------------------------------------
 * Rule G1 visits every cell of a beam, with one division a visit. d2[j][i] of rule D1 says how far the nearest
 * occupied cell is, so a beam standing in cell (i, j) can cross that many cells without looking at any of them.
 * The calls below are the grid family's cast and rollout with rule F1 in place of rule G1: the same arguments with
 * one more array, the same bits. They are not a family of their own. Additive: F110QP_API_VERSION stays 6, and no
 * call above changes its results.
 *
 * F1. A beam against the grid through its field. d2 is [H][W] int as f110qp_grid_distance_dev writes it for `grid`;
 *     it is the caller's to keep the two consistent, nothing checks it. A cell is occupied exactly when d2 <= 0.
 *     The start, px, py, gx, gy, tx, ty, the tie rule and the step budget W + H + 2 are rule G1's, word for word.
 *     At the start cell: the start cell outside the map, or px or py not finite: the grid gives no hit and
 *     visits = 0. Otherwise D = d2[iy][ix] and visits = 1; D <= 0: th = 0. Otherwise repeat, while budget is left:
 *       1. m = max(1, isqrt(D - 1)), capped by the remaining budget (isqrt(D - 1) is the largest m with m m < D;
 *          INT_MAX gives 46,340). Rule G1's step 1, the move alone, is applied m times without reading the map;
 *          t is the parameter of the last of them. The budget drops by m;
 *       2. t > limit, or t is NaN: no hit;
 *       3. the cell reached is outside the map: no hit;
 *       4. D = d2 of the cell reached, visits grows by 1; D <= 0: th = t + 0.0.
 *     limit is what the beam's minimum already holds from circles, mates and segments, at most max_range.
 *     Consequences. Within m steps the walk stays within m cells of where it stood, which is less than sqrt(D):
 *     no cell it passes is occupied. The parameter only grows and the map is convex, so a t past the limit or a
 *     cell outside the map at a skipped step leaves both at the landing too. Rule G1 computes every boundary's
 *     parameter from the integer boundary, so the walk's state after m steps is a function of the start, the
 *     direction and m alone, and a jump that lands in that state returns the walk's own bits. Hence th, and with
 *     it range and rule Z2's output, equal rule G1's bit for bit on every (beam, map) pair with a consistent d2.
 *     With an inconsistent d2 the result is unspecified; every read is still inside [0, W) x [0, H).
 *     How the m moves are made is the implementation's choice. With X(k) and Y(l) the k-th and l-th boundary
 *     parameters ahead in rule G1's expressions (both never decrease), the walk has taken a x-moves and b = m - a
 *     y-moves exactly when (a == 0 or X(a - 1) <= Y(b)) and (b == 0 or Y(b - 1) < X(a)); then
 *     t = max(X(a - 1), Y(b - 1)). */

/* f110qp_cast_scans_grid_dev, parameter for parameter, with rule F1 in place of rule G1: d2 follows grid, visits
 * follows ranges. visits is [batch][num_ranges] int, the cells of d2 each beam read, or NULL; a car that is not
 * listed keeps its row of visits as it keeps its ranges. grid is not read by this call; it keeps its place so that
 * one argument list serves both casts. The map's cells are read from global memory (L2): the workgroup keeps no
 * copy. F110QP_ERR_INVALID before any HIP call: that call's rules, then a side above F110QP_FIELD_MAX_SIDE, then
 * width * height > 0 with d2 == NULL. width * height == 0 gives f110qp_cast_scans_noisy_dev's bits and visits 0.
 * One launch, at most min(batch, 512) workgroups. */
int f110qp_grid_cast_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc, const f110qp_race_config* race,
                         const f110qp_body_config* body, const f110qp_walls_config* walls,
                         const f110qp_noise_config* noise, const f110qp_grid_config* grid_cfg, int batch, int tick,
                         const int* list, const int* count, const double* x, const double* circles,
                         const double* segments, const unsigned char* grid, const int* d2, float* ranges, int* visits,
                         void* stream);

/* f110qp_rollout_grid_dev, word for word, with every cast f110qp_grid_cast_dev's (d2 follows grid); every clearance
 * stays f110qp_clearance_grid_dev's, which reads grid. The same launch count and stream order, no synchronisation
 * and no allocation inside the loop; that call's checks with f110qp_grid_cast_dev's two behind the grid's. Every
 * array equals f110qp_rollout_grid_dev's bit for bit when d2 is grid's field. */
int f110qp_rollout_field_dev(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                             const f110qp_replan_config* rp, const f110qp_world_config* wc,
                             const f110qp_race_config* race, const f110qp_contact_config* cc,
                             const f110qp_body_config* body, const f110qp_walls_config* walls,
                             const f110qp_refresh_config* rf, const f110qp_noise_config* noise,
                             const f110qp_grid_config* grid_cfg, int batch, const double* table,
                             const double* waypoints, double* x_ref, int* have_path, const double* circles,
                             const double* segments, const unsigned char* grid, const int* d2, double* x_traj,
                             double* u_lin_traj, float* u_applied, int* status_traj, int* iters_traj,
                             double* cost_traj, float* u_plan, float* x_plan, float* hs_traj, int* kind_traj,
                             int* plan_status_traj, int* best_traj_traj, int* best_global_traj, double* pose_traj,
                             float* ranges_traj, double* clear_traj, int* nearest_traj, int* crash_tick,
                             void* stream);

/* Same on host pointers (synchronous), with f110qp_rollout_grid's parameter list unchanged: the map is staged in
 * once, f110qp_grid_distance_dev's two launches run on the context's stream into the staging buffer before the
 * first tick, and the device loop reads that field. On top of f110qp_rollout_grid's rules a side above
 * F110QP_FIELD_MAX_SIDE is invalid. */
int f110qp_rollout_field(f110qp_ctx* ctx, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                         const f110qp_replan_config* rp, const f110qp_world_config* wc,
                         const f110qp_race_config* race, const f110qp_contact_config* cc,
                         const f110qp_body_config* body, const f110qp_walls_config* walls,
                         const f110qp_refresh_config* rf, const f110qp_noise_config* noise,
                         const f110qp_grid_config* grid_cfg, int batch, const double* table, const double* waypoints,
                         double* x_ref, int* have_path, const double* circles, const double* segments,
                         const unsigned char* grid, double* x_traj, double* u_lin_traj, float* u_applied,
                         int* status_traj, int* iters_traj, double* cost_traj, float* u_plan, float* x_plan,
                         float* hs_traj, int* kind_traj, int* plan_status_traj, int* best_traj_traj,
                         int* best_global_traj, double* pose_traj, float* ranges_traj, double* clear_traj,
                         int* nearest_traj, int* crash_tick);

/* ---- race standings: progress along the track, laps and positions ---------------------------------------
 * The calls above return poses; the calls below say who is ahead. They run after the fact on x_traj, or on any
 * [rows][B][3] pose array: nothing inside a closed loop reads a standing, so there is no rollout family of
 * their own. Additive: F110QP_API_VERSION stays 6, and no call above changes its results.
 *
 * The path is waypoints [W][2] double, W >= 2, closed: segment j runs from a = wp[j] to b = wp[(j + 1) % W].
 * Its cumulative length is cum [W + 1] double: cum[0] = 0, cum[j + 1] = cum[j] + sqrt(ex ex + ey ey) with
 * e = b - a, summed in index order (the correctly rounded square root, every product and sum rounded);
 * L = cum[W] is the path's length. The device call takes cum as an argument: the lengths are the caller's bits.
 *
 * Projection. The projected point is the pose's (x, y) itself, which is what Trajectory::get_best_global_idx
 * measures from; ori is not read. All fp64, every product and sum rounded (no fused multiply-add). Per
 * segment j, with p = (x, y):
 *   e = b - a, w = p - a, ee = ex ex + ey ey
 *   t = (wx ex + wy ey) / ee, clamped by t < 0 ? 0 : (t > 1 ? 1 : t); t = 0 when ee == 0
 *   c = a + t e, d = p - c, d2 = dx dx + dy dy
 * The winner is the minimum d2, the lowest j on equal values: a candidate replaces the running (best, index)
 * only when d2 < best, or d2 == best with a lower j, from the start (+inf, -1). Per pose:
 *   seg     = the winner's j
 *   s       = cum[j] + t (cum[j + 1] - cum[j])
 *   lateral = sqrt(d2), negated unless ex wy - ey wx >= 0: positive to the left of the direction of travel.
 * Consequences: a NaN passes no compare, so a segment with a non-finite end point has a NaN d2 and is never
 * chosen, and the segments next to it are undisturbed; a pose with a non-finite x or y has a NaN or +inf d2 on
 * every segment, keeps the start value and gives seg = -1, s = NaN, lateral = NaN. A pose exactly on a vertex
 * is at d2 = 0 on the segment that starts there (t = 0, c = a) and, where a + (b - a) is b exactly, on the one
 * that ends there too (t = 1): the lower index wins, and at vertex 0 that is segment 0 over segment W - 1, so
 * s = 0 there and never L. The minimum is over
 * per-segment values that do not depend on the other segments: the result is the exact minimum (no cull).
 * Limit: the nearest point is global. A track whose distinct sections come closer to each other than the cars
 * stray from the path is outside this model: a car between two such sections is projected onto whichever is
 * nearer, and its s jumps. The shipped ellipse and a world of walls 1.6 m to either side of it are inside it. */

/* Host, plain C++ (no HIP call, no environment): cum [num_waypoints + 1] of waypoints [num_waypoints][2] as
 * above. F110QP_ERR_INVALID: a NULL pointer, num_waypoints < 2. */
int f110qp_path_lengths(const double* waypoints, int num_waypoints, double* cum);

/* The projection of rows x B poses (device pointers, asynchronous on `stream`, one launch, no allocation,
 * synchronisation or read-back):
 *   x [rows][B][3] double, waypoints [W][2] double, cum [W + 1] double
 *   -> seg [rows][B] int (may be NULL), s [rows][B] double, lateral [rows][B] double (may be NULL).
 * F110QP_ERR_INVALID before any HIP call: a NULL x, waypoints, cum or s; batch < 1, rows < 1,
 * num_waypoints < 2; rows x batch above 2^30. No cap on num_waypoints. Workgroups stride over the cars, one car
 * each, at most min(batch, 1024) of them (what the device holds at once). */
int f110qp_progress_dev(int batch, int rows, const double* x, const double* waypoints, const double* cum,
                        int num_waypoints, int* seg, double* s, double* lateral, void* stream);

/* Standings. The B cars of every row are B / G races as in f110qp_cast_scans_race_dev (only race->group_size
 * is read; car_radius and center_offset are checked as there). With L = path_length and
 *   wrap(v) = v > L/2 ? v - L : (v <= -L/2 ? v + L : v):
 *   row 0, relative to the race's first car g0 = G (b / G):  dist[0][b] = s[0][g0] + wrap(s[0][b] - s[0][g0])
 *   row r >= 1:  dist[r][b] = dist[r-1][b] + wrap(s[r][b] - s[r-1][b]), accumulated in row order
 *   lap[r][b]  = (int)floor((dist[r][b] - dist[0][b]) / L), INT_MIN where dist is NaN
 *   rank[r][b] = the number of race-mates m with dist[r][m] > dist[r][b], or equal with m < b. A car with a
 *                NaN dist is behind every car with a number, and among NaN cars the lower index is ahead.
 * dist is the distance driven along the path, unwrapped: it grows past L on the second lap and falls when a
 * car reverses. 0 is the leader, and the ranks of a race are a permutation of 0 .. G-1 at every row. A NaN s
 * makes that row and every later row of the car NaN (by the sums; a NaN s of the race's first car at row 0
 * does the same to the whole race). A parked car's pose repeats, so its dist stands still: no special case.
 * The model holds while a car moves less than L/2 along the path between two rows, and while a race's cars
 * stand within L/2 of its first car at row 0.
 *   s [rows][B] double -> dist [rows][B] double, lap [rows][B] int (may be NULL), rank [rows][B] int.
 * Device pointers, asynchronous on `stream`: two launches (the sums in row order, then the ranks) with nothing
 * but the stream's order between them; no allocation, synchronisation or read-back. No cap on G.
 * F110QP_ERR_INVALID before any HIP call: every race rule of f110qp_cast_scans_race_dev; batch < 1, rows < 1;
 * rows x batch above 2^30; a path_length that is not positive and finite; a NULL s, dist or rank. */
int f110qp_standings_dev(const f110qp_race_config* race, int batch, int rows, const double* s, double path_length,
                         double* dist, int* lap, int* rank, void* stream);

/* Both on host pointers (synchronous): cum by f110qp_path_lengths, L = cum[W]; x, waypoints and cum staged
 * through device buffers that the call owns and frees on every exit path (there is no context), the two device
 * calls, every output that was given copied back, one synchronisation. seg, lateral and lap may be NULL.
 * Bit-identical to the two device calls. F110QP_ERR_INVALID as theirs, before any HIP call (a path whose
 * length is not positive and finite included). */
int f110qp_race_standings(const f110qp_race_config* race, int batch, int rows, const double* x,
                          const double* waypoints, int num_waypoints, int* seg, double* s, double* lateral,
                          double* dist, int* lap, int* rank);

/* ---- Monte Carlo outcomes: per-situation quantile fans, survival, car records ------------------------------
 * With the noisy family one batch is M reproducible hypotheses of one situation. The calls below say what became
 * of them, on the device: the order statistics of every situation at every row, how many hypotheses are still
 * running, and every car's own record. Like the standings they run after the fact, on clear_traj, crash_tick,
 * status_traj and kind_traj of a rollout, or on any [rows][B] double array (lateral, s and dist of the standings
 * calls). Every result is a selection or a count: no arithmetic touches a value and there is no tolerance.
 * Additive: F110QP_API_VERSION stays 6, and no call above changes its results.
 *
 * Layout. A batch is S situations x M hypotheses x G cars of one hypothesis (G the race size, 1 without races):
 * B = S M G and car b = (s M + m) G + g. A sample set is k = s G + g, K = S G = B / M of them; the M members of
 * set k are the cars (s M + m) G + g for m = 0 .. M-1 with s = k / G and g = k % G: M values at stride G. With the
 * noisy family every car draws its own stream (car_base + b), so M copies of one start are M hypotheses with
 * nothing else to set.
 *
 * M1. Key. With u the 64 bits of a sample, its key is ~u when the sign bit is set and u | 1 << 63 otherwise,
 *     compared as unsigned: a total order with -inf < ... < -0 < +0 < ... < +inf.
 * M2. NaN. A NaN of any payload and either sign is not a sample. n is the number of the set's values at that row
 *     that are not NaN, and count[r][k] = n.
 * M3. The fan. fan[r][k][q] is the sample at position (int)floor(prob[q] * (double)(n - 1)) of the ascending
 *     order of keys, the product being one rounded fp64 product. The output has that sample's own bits, so a -0
 *     stays -0. For n = 0 the output is the NaN 0x7ff8000000000000. Equal keys are equal bits, so the result does
 *     not depend on the sort's stability, on the thread mapping or on the batch size.
 * M4. Survival. alive[r][k], r = 0 .. T, is the number of members with crash_tick < 0 or crash_tick > r: a car
 *     that crashed at row r is not alive at row r. crashed[k] is the number of members with
 *     0 <= crash_tick <= T.
 * M5. Car records. (min_clear, min_row)[b] is the minimum of clear_traj over rows 0 .. T under the clearance
 *     kernel's replace rule from (+inf, -1): a row replaces the running pair only when its value is smaller, or
 *     equal with a lower row, so the lowest row wins on equal values, a NaN passes no compare, and a column of
 *     NaN or of +inf keeps (+inf, -1). A tick is unsolved when kind_traj is NULL or the tick's kind is
 *     F110QP_TICK_MPC, and its status is neither F110QP_SOLVED nor F110QP_SOLVED_INACCURATE. unsolved[b] counts
 *     the unsolved ticks, first_unsolved[b] is the first one or -1, plan_failed[b] counts the ticks of kind
 *     F110QP_TICK_PLAN_FAILED. */
#define F110QP_MC_MAX_HYPOTHESES 4096
#define F110QP_MC_MAX_PROBS 8
typedef struct {
  int hypotheses;   /* M, 1 .. F110QP_MC_MAX_HYPOTHESES */
  int group_size;   /* G >= 1 */
  int num_probs;    /* Q, 1 .. F110QP_MC_MAX_PROBS */
  double prob[F110QP_MC_MAX_PROBS];  /* each in [0, 1]; any order, repeats allowed */
} f110qp_mc_config;

/* M 1, G 1, Q 3, prob {0, 0.5, 1} (the rest of prob zero). */
void f110qp_default_mc_config(f110qp_mc_config* mc);

/* The three device calls take device pointers and are asynchronous on `stream`: one launch each, no allocation,
 * synchronisation or read-back. F110QP_ERR_INVALID before any HIP call, with a last_error text that names the
 * field. The config rules, which every call that takes mc applies in full: a NULL mc; hypotheses outside
 * 1 .. 4096; group_size < 1; batch < 1 or not a multiple of hypotheses x group_size; num_probs outside 1 .. 8; a
 * prob[q], q < num_probs, that is NaN or outside [0, 1]. The shape rules: rows < 1 or ticks < 1; rows x batch
 * above 2^30, rows being ticks + 1 where a call takes ticks.
 *
 * Rules M1 to M3 on v [rows][B] double -> fan [rows][K][Q] double, count [rows][K] int (may be NULL; fan does not
 * depend on it). Also invalid: a NULL v or fan. Two kernels by M: sets of at most 64 values (M padded to a power
 * of two) are sorted by a bitonic network over lane shuffles, 64 / padded M sets per wave; larger ones in LDS by
 * one 256-thread workgroup per (row, set). Workgroups stride over the (row, set) items, at most 2,048 of them on
 * the first path and 1,024 on the second (what the device holds at once). For G = 1 a set's loads are
 * contiguous, for G > 1 they are G doubles apart. */
int f110qp_mc_fan_dev(const f110qp_mc_config* mc, int batch, int rows, const double* v, double* fan, int* count,
                      void* stream);

/* Rule M4 on crash_tick [B] int -> alive [ticks + 1][K] int, crashed [K] int (may be NULL). Also invalid: a NULL
 * crash_tick or alive. */
int f110qp_mc_survival_dev(const f110qp_mc_config* mc, int batch, int ticks, const int* crash_tick, int* alive,
                           int* crashed, void* stream);

/* Rule M5 on clear_traj [ticks + 1][B] double, status_traj [ticks][B] int or NULL, kind_traj [ticks][B] int or
 * NULL -> min_clear [B] double, min_row, unsolved, first_unsolved, plan_failed [B] int (each of the four may be
 * NULL). No config: a car's record does not depend on the layout. Also invalid: a NULL clear_traj or min_clear;
 * unsolved or first_unsolved given without status_traj; plan_failed given without kind_traj. */
int f110qp_mc_outcomes_dev(int batch, int ticks, const double* clear_traj, const int* status_traj,
                           const int* kind_traj, double* min_clear, int* min_row, int* unsolved,
                           int* first_unsolved, int* plan_failed, void* stream);

/* The three on host pointers (synchronous), the fan taken on clear_traj (rows = ticks + 1): the four inputs
 * staged through device buffers that the call owns and frees on every exit path (there is no context), the three
 * device calls, every output that was given copied back, one synchronisation. status_traj and kind_traj may be
 * NULL as above; count, crashed, min_row, unsolved, first_unsolved and plan_failed may be NULL. Bit-identical to
 * the device calls. F110QP_ERR_INVALID as theirs, before any HIP call; also a NULL crash_tick, fan or alive. */
int f110qp_mc_summary(const f110qp_mc_config* mc, int batch, int ticks, const double* clear_traj,
                      const int* crash_tick, const int* status_traj, const int* kind_traj, double* fan, int* count,
                      int* alive, int* crashed, double* min_clear, int* min_row, int* unsolved, int* first_unsolved,
                      int* plan_failed);

#ifdef __cplusplus
}
#endif
#endif /* F110QP_H */
