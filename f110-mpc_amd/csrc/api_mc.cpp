// api_mc.cpp — the C ABI's Monte Carlo outcomes (include/f110qp.h): f110qp_mc_fan_dev, f110qp_mc_survival_dev and
// f110qp_mc_outcomes_dev on the device, f110qp_mc_summary on host pointers. Host-side responsibilities only: the
// argument rules (every one answers before the first HIP call), the launches, and the synchronous call's own
// staging. No C++ exception crosses this boundary.
#include "api_common.h"

namespace {

// A check returns the message of the rule that failed, or null.
const char* check_mc(const f110qp_mc_config* mc, int batch) {
  if (!mc) return "mc config is NULL";
  if (mc->hypotheses < 1 || mc->hypotheses > F110QP_MC_MAX_HYPOTHESES) return "hypotheses must be in 1..4096";
  if (mc->group_size < 1) return "group_size < 1";
  if (batch < 1) return "batch must be >= 1";
  if ((long long)batch % ((long long)mc->hypotheses * mc->group_size) != 0)
    return "batch must be a multiple of hypotheses x group_size";
  if (mc->num_probs < 1 || mc->num_probs > F110QP_MC_MAX_PROBS) return "num_probs must be in 1..8";
  for (int q = 0; q < mc->num_probs; q++)
    if (!(mc->prob[q] >= 0.0 && mc->prob[q] <= 1.0)) return "every prob must be in [0, 1]";
  return nullptr;
}

const char* check_rows(int batch, int rows) {
  if (batch < 1) return "batch must be >= 1";
  if (rows < 1) return "rows must be >= 1";
  if ((long long)rows * batch > (1ll << 30)) return "rows x batch too large";
  return nullptr;
}

// ticks + 1 rows of batch cars.
const char* check_ticks(int batch, int ticks) {
  if (batch < 1) return "batch must be >= 1";
  if (ticks < 1) return "ticks must be >= 1";
  if (((long long)ticks + 1) * batch > (1ll << 30)) return "rows x batch too large (rows = ticks + 1)";
  return nullptr;
}

const char* check_outcomes(int batch, int ticks, const double* clear_traj, const int* status_traj,
                           const int* kind_traj, const double* min_clear, const int* unsolved,
                           const int* first_unsolved, const int* plan_failed) {
  if (const char* m = check_ticks(batch, ticks)) return m;
  if (!clear_traj || !min_clear) return "clear_traj/min_clear must be non-NULL";
  if ((unsolved || first_unsolved) && !status_traj) return "unsolved/first_unsolved need status_traj";
  if (plan_failed && !kind_traj) return "plan_failed needs kind_traj";
  return nullptr;
}

}  // namespace

extern "C" {

void f110qp_default_mc_config(f110qp_mc_config* mc) {
  if (!mc) return;
  *mc = f110qp_mc_config{};
  mc->hypotheses = 1;
  mc->group_size = 1;
  mc->num_probs = 3;
  mc->prob[0] = 0.0;
  mc->prob[1] = 0.5;
  mc->prob[2] = 1.0;
}

int f110qp_mc_fan_dev(const f110qp_mc_config* mc, int batch, int rows, const double* v, double* fan, int* count,
                      void* stream) {
  if (const char* m = check_mc(mc, batch)) return fail(F110QP_ERR_INVALID, m);
  if (const char* m = check_rows(batch, rows)) return fail(F110QP_ERR_INVALID, m);
  if (!v || !fan) return fail(F110QP_ERR_INVALID, "v/fan must be non-NULL");
  const hipError_t e = f110qp::launch_mc_fan(mc->hypotheses, mc->group_size, mc->num_probs, mc->prob, batch, rows, v,
                                             fan, count, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "mc fan launch");
  return F110QP_OK;
}

int f110qp_mc_survival_dev(const f110qp_mc_config* mc, int batch, int ticks, const int* crash_tick, int* alive,
                           int* crashed, void* stream) {
  if (const char* m = check_mc(mc, batch)) return fail(F110QP_ERR_INVALID, m);
  if (const char* m = check_ticks(batch, ticks)) return fail(F110QP_ERR_INVALID, m);
  if (!crash_tick || !alive) return fail(F110QP_ERR_INVALID, "crash_tick/alive must be non-NULL");
  const hipError_t e = f110qp::launch_mc_survival(mc->hypotheses, mc->group_size, batch, ticks, crash_tick, alive,
                                                  crashed, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "mc survival launch");
  return F110QP_OK;
}

int f110qp_mc_outcomes_dev(int batch, int ticks, const double* clear_traj, const int* status_traj,
                           const int* kind_traj, double* min_clear, int* min_row, int* unsolved,
                           int* first_unsolved, int* plan_failed, void* stream) {
  if (const char* m = check_outcomes(batch, ticks, clear_traj, status_traj, kind_traj, min_clear, unsolved,
                                     first_unsolved, plan_failed))
    return fail(F110QP_ERR_INVALID, m);
  const hipError_t e = f110qp::launch_mc_outcomes(batch, ticks, clear_traj, status_traj, kind_traj, min_clear,
                                                  min_row, unsolved, first_unsolved, plan_failed, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "mc outcomes launch");
  return F110QP_OK;
}

int f110qp_mc_summary(const f110qp_mc_config* mc, int batch, int ticks, const double* clear_traj,
                      const int* crash_tick, const int* status_traj, const int* kind_traj, double* fan, int* count,
                      int* alive, int* crashed, double* min_clear, int* min_row, int* unsolved, int* first_unsolved,
                      int* plan_failed) {
  if (const char* m = check_mc(mc, batch)) return fail(F110QP_ERR_INVALID, m);
  if (const char* m = check_outcomes(batch, ticks, clear_traj, status_traj, kind_traj, min_clear, unsolved,
                                     first_unsolved, plan_failed))
    return fail(F110QP_ERR_INVALID, m);
  if (!crash_tick || !fan || !alive) return fail(F110QP_ERR_INVALID, "crash_tick/fan/alive must be non-NULL");
  const size_t B = (size_t)batch, T = (size_t)ticks, K = B / (size_t)mc->hypotheses, Q = (size_t)mc->num_probs;
  const size_t nr = (T + 1) * B, nt = T * B, nk = (T + 1) * K;

  // one device buffer, freed with `dev` on every way out: the doubles, then the ints
  const size_t nd = nr + nk * Q + B, ni = B + 2 * nt + 2 * nk + K + 4 * B;
  DevBuf dev;
  hipError_t e = dev.ensure(nd * sizeof(double) + ni * sizeof(int));
  if (e != hipSuccess) return hip_fail(e, "mc staging allocation");
  double* dclear = (double*)dev.p;
  double *dfan = dclear + nr, *dmin = dfan + nk * Q;
  int* dcrash = (int*)(dmin + B);
  int *dstat = dcrash + B, *dkind = dstat + nt, *dcount = dkind + nt, *dalive = dcount + nk, *dhit = dalive + nk;
  int *drow = dhit + K, *duns = drow + B, *dfirst = duns + B, *dpf = dfirst + B;
  const hipStream_t st = nullptr;
  auto up = [&](void* d, const void* host, size_t bytes) {
    if (host && e == hipSuccess) e = hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st);
  };
  up(dclear, clear_traj, nr * sizeof(double));
  up(dcrash, crash_tick, B * sizeof(int));
  up(dstat, status_traj, nt * sizeof(int));
  up(dkind, kind_traj, nt * sizeof(int));
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return hip_fail(e, "mc H2D");
  }
  int rv = f110qp_mc_fan_dev(mc, batch, ticks + 1, dclear, dfan, count ? dcount : nullptr, st);
  if (!rv) rv = f110qp_mc_survival_dev(mc, batch, ticks, dcrash, dalive, crashed ? dhit : nullptr, st);
  if (!rv)
    rv = f110qp_mc_outcomes_dev(batch, ticks, dclear, status_traj ? dstat : nullptr, kind_traj ? dkind : nullptr, dmin,
                                min_row ? drow : nullptr, unsolved ? duns : nullptr,
                                first_unsolved ? dfirst : nullptr, plan_failed ? dpf : nullptr, st);
  if (rv) {
    (void)hipStreamSynchronize(st);
    return rv;
  }
  auto back = [&](void* host, const void* d, size_t bytes) {
    if (host && e == hipSuccess) e = hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, st);
  };
  back(fan, dfan, nk * Q * sizeof(double));
  back(count, dcount, nk * sizeof(int));
  back(alive, dalive, nk * sizeof(int));
  back(crashed, dhit, K * sizeof(int));
  back(min_clear, dmin, B * sizeof(double));
  back(min_row, drow, B * sizeof(int));
  back(unsolved, duns, B * sizeof(int));
  back(first_unsolved, dfirst, B * sizeof(int));
  back(plan_failed, dpf, B * sizeof(int));
  const hipError_t es = hipStreamSynchronize(st);  // the one synchronisation, also before `dev` is freed
  if (e != hipSuccess) return hip_fail(e, "mc D2H");
  if (es != hipSuccess) return hip_fail(es, "mc synchronise");
  return F110QP_OK;
}

}  // extern "C"
