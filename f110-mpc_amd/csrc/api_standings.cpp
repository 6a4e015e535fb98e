// api_standings.cpp — the C ABI's race standings (include/f110qp.h): f110qp_path_lengths on the host,
// f110qp_progress_dev and f110qp_standings_dev on the device, f110qp_race_standings on host pointers.
// Host-side responsibilities only: the argument rules (standings_host.h, which the CPU test builds under
// sanitizers), the launches, and the synchronous call's own staging. No C++ exception crosses this boundary.
#include <new>
#include <vector>

#include "api_common.h"
#include "standings_host.h"

extern "C" {

int f110qp_path_lengths(const double* waypoints, int num_waypoints, double* cum) {
  if (const char* m = standings::check_path_lengths(waypoints, num_waypoints, cum)) return fail(F110QP_ERR_INVALID, m);
  standings::path_lengths(waypoints, num_waypoints, cum);
  return F110QP_OK;
}

int f110qp_progress_dev(int batch, int rows, const double* x, const double* waypoints, const double* cum,
                        int num_waypoints, int* seg, double* s, double* lateral, void* stream) {
  if (const char* m = standings::check_progress(batch, rows, x, waypoints, cum, num_waypoints, s))
    return fail(F110QP_ERR_INVALID, m);
  const hipError_t e = f110qp::launch_progress(batch, rows, x, waypoints, cum, num_waypoints, seg, s, lateral,
                                               (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "progress launch");
  return F110QP_OK;
}

int f110qp_standings_dev(const f110qp_race_config* race, int batch, int rows, const double* s, double path_length,
                         double* dist, int* lap, int* rank, void* stream) {
  if (const char* m = standings::check_standings(race, batch, rows, s, path_length, dist, rank))
    return fail(F110QP_ERR_INVALID, m);
  const hipError_t e =
      f110qp::launch_standings(race->group_size, batch, rows, s, path_length, dist, lap, rank, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "standings launch");
  return F110QP_OK;
}

int f110qp_race_standings(const f110qp_race_config* race, int batch, int rows, const double* x,
                          const double* waypoints, int num_waypoints, int* seg, double* s, double* lateral,
                          double* dist, int* lap, int* rank) {
  if (const char* m = standings::check_race_standings(race, batch, rows, x, waypoints, num_waypoints, s, dist, rank))
    return fail(F110QP_ERR_INVALID, m);
  const size_t W = (size_t)num_waypoints, n = (size_t)rows * (size_t)batch;
  std::vector<double> cum;
  try {
    cum.resize(W + 1);
  } catch (const std::bad_alloc&) {
    return fail(F110QP_ERR_ALLOC, "out of host memory for the path's lengths");
  }
  standings::path_lengths(waypoints, num_waypoints, cum.data());
  const double L = cum[W];
  if (const char* m = standings::check_path_length(L)) return fail(F110QP_ERR_INVALID, m);

  // one device buffer, freed with `dev` on every way out: the doubles, then the ints
  const size_t nd = n * 3 + W * 2 + (W + 1) + n * 3, ni = (n * 3 + 1) & ~(size_t)1;
  DevBuf dev;
  hipError_t e = dev.ensure(nd * sizeof(double) + ni * sizeof(int));
  if (e != hipSuccess) return hip_fail(e, "standings staging allocation");
  double* dx = (double*)dev.p;
  double *dwp = dx + n * 3, *dcum = dwp + W * 2, *ds = dcum + (W + 1), *dlat = ds + n, *ddist = dlat + n;
  int* dseg = (int*)(ddist + n);
  int *dlap = dseg + n, *drank = dlap + n;
  const hipStream_t st = nullptr;
  if ((e = hipMemcpyAsync(dx, x, n * 3 * sizeof(double), hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(dwp, waypoints, W * 2 * sizeof(double), hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(dcum, cum.data(), (W + 1) * sizeof(double), hipMemcpyHostToDevice, st)) != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return hip_fail(e, "standings H2D");
  }
  int rv = f110qp_progress_dev(batch, rows, dx, dwp, dcum, num_waypoints, seg ? dseg : nullptr, ds,
                               lateral ? dlat : nullptr, st);
  if (!rv) rv = f110qp_standings_dev(race, batch, rows, ds, L, ddist, lap ? dlap : nullptr, drank, st);
  if (rv) {
    (void)hipStreamSynchronize(st);
    return rv;
  }
  auto back = [&](void* host, const void* d, size_t bytes) {
    if (host && e == hipSuccess) e = hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, st);
  };
  back(seg, dseg, n * sizeof(int));
  back(s, ds, n * sizeof(double));
  back(lateral, dlat, n * sizeof(double));
  back(dist, ddist, n * sizeof(double));
  back(lap, dlap, n * sizeof(int));
  back(rank, drank, n * sizeof(int));
  const hipError_t es = hipStreamSynchronize(st);  // the one synchronisation, also before `dev` is freed
  if (e != hipSuccess) return hip_fail(e, "standings D2H");
  if (es != hipSuccess) return hip_fail(es, "standings synchronise");
  return F110QP_OK;
}

}  // extern "C"
