// standings_host.h — the host half of the standings calls (include/f110qp.h) that needs no device: the path's
// cumulative lengths and the argument rules of f110qp_progress_dev, f110qp_standings_dev and
// f110qp_race_standings. Plain C++ without a HIP header, so host/tests/standings_host.cpp runs it on the CPU
// under AddressSanitizer and UBSan. A check returns the message of the rule that failed, or null.
#pragma once
#include <cmath>

#include "f110qp.h"

namespace standings {

// cum [W + 1] of the closed path wp [W][2]: the sums in index order, every operation rounded.
inline void path_lengths(const double* wp, int W, double* cum) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  cum[0] = 0.0;
  for (int j = 0; j < W; j++) {
    const int jn = j + 1 == W ? 0 : j + 1;
    const double ex = wp[2 * jn + 0] - wp[2 * j + 0], ey = wp[2 * jn + 1] - wp[2 * j + 1];
    cum[j + 1] = cum[j] + std::sqrt(ex * ex + ey * ey);
  }
}

inline const char* check_path_lengths(const double* wp, int W, const double* cum) {
  if (!wp || !cum) return "waypoints/cum must be non-NULL";
  if (W < 2) return "num_waypoints must be >= 2";
  return nullptr;
}

inline const char* check_shape(int batch, int rows) {
  if (batch < 1) return "batch must be >= 1";
  if (rows < 1) return "rows must be >= 1";
  if ((long long)rows * batch > (1ll << 30)) return "rows x batch too large";
  return nullptr;
}

// The race rules of f110qp_cast_scans_race_dev (api_rollout.cpp's race_params) without a world.
inline const char* check_race(const f110qp_race_config* race, int batch) {
  if (!race) return "race config is NULL";
  if (race->group_size < 1) return "group_size < 1";
  if (batch % race->group_size != 0) return "batch must be a multiple of group_size";
  if (!(race->car_radius > 0.0) || !std::isfinite(race->car_radius)) return "car_radius must be positive and finite";
  if (!std::isfinite(race->center_offset)) return "center_offset must be finite";
  return nullptr;
}

inline const char* check_progress(int batch, int rows, const double* x, const double* wp, const double* cum, int W,
                                  const double* s) {
  if (const char* m = check_shape(batch, rows)) return m;
  if (W < 2) return "num_waypoints must be >= 2";
  if (!x || !wp || !cum || !s) return "x/waypoints/cum/s must be non-NULL";
  return nullptr;
}

inline const char* check_path_length(double L) {
  if (!(L > 0.0) || !std::isfinite(L)) return "path_length must be positive and finite";
  return nullptr;
}

inline const char* check_standings(const f110qp_race_config* race, int batch, int rows, const double* s, double L,
                                   const double* dist, const int* rank) {
  if (const char* m = check_shape(batch, rows)) return m;
  if (const char* m = check_race(race, batch)) return m;
  if (const char* m = check_path_length(L)) return m;
  if (!s || !dist || !rank) return "s/dist/rank must be non-NULL";
  return nullptr;
}

// f110qp_race_standings before it computes the path's length (which it checks next).
inline const char* check_race_standings(const f110qp_race_config* race, int batch, int rows, const double* x,
                                        const double* wp, int W, const double* s, const double* dist,
                                        const int* rank) {
  if (const char* m = check_shape(batch, rows)) return m;
  if (const char* m = check_race(race, batch)) return m;
  if (W < 2) return "num_waypoints must be >= 2";
  if (!x || !wp || !s || !dist || !rank) return "x/waypoints/s/dist/rank must be non-NULL";
  return nullptr;
}

}  // namespace standings
