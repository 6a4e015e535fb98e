// standings_host.cpp — the host half of the standings calls (csrc/standings_host.h) on the CPU: the path's
// cumulative lengths into exactly sized heap arrays (W = 2, a duplicated waypoint, a non-finite waypoint, the
// closing segment back to waypoint 0) and every argument rule of f110qp_progress_dev, f110qp_standings_dev and
// f110qp_race_standings. Built with -fsanitize=address,undefined (tests/test_standings_host.py): a read past
// the waypoints or a write past cum is an error of the sanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "standings_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      g_fail++;                                                     \
    }                                                               \
  } while (0)

static bool says(const char* m, const char* word) { return m && std::strstr(m, word); }

// cum of W waypoints in heap arrays of exactly 2 W and W + 1 doubles
static double* lengths(const double* src, int W) {
  double* wp = (double*)std::malloc(sizeof(double) * 2 * W);
  std::memcpy(wp, src, sizeof(double) * 2 * W);
  double* cum = (double*)std::malloc(sizeof(double) * (W + 1));
  CHECK(standings::check_path_lengths(wp, W, cum) == nullptr);
  standings::path_lengths(wp, W, cum);
  std::free(wp);
  return cum;
}

static void test_path_lengths() {
  const double two[] = {0, 0, 3, 4};  // there and back
  double* c = lengths(two, 2);
  CHECK(c[0] == 0.0 && c[1] == 5.0 && c[2] == 10.0);
  std::free(c);
  const double sq[] = {0, 0, 2, 0, 2, 0, 2, 2, 0, 2};  // waypoint 1 twice: segment 1 has no length
  c = lengths(sq, 5);
  CHECK(c[1] == 2.0 && c[2] == 2.0 && c[3] == 4.0 && c[4] == 6.0 && c[5] == 8.0);
  std::free(c);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double bad[] = {0, 0, 1, 0, nan, 1, 0, 1};
  c = lengths(bad, 4);
  CHECK(c[1] == 1.0 && std::isnan(c[2]) && std::isnan(c[4]));
  std::free(c);
  // in index order, every sum rounded: 1 + 2^-53 + 2^-53 stays 1 from the left
  const double t = std::ldexp(1.0, -53);
  const double row[] = {0, 0, 1, 0, 1, t, 1, 2 * t};
  c = lengths(row, 4);
  CHECK(c[1] == 1.0 && c[2] == 1.0 && c[3] == 1.0);
  std::free(c);
  CHECK(says(standings::check_path_lengths(nullptr, 4, (double*)row), "non-NULL"));
  CHECK(says(standings::check_path_lengths(row, 4, nullptr), "non-NULL"));
  CHECK(says(standings::check_path_lengths(row, 1, (double*)row), "num_waypoints"));
  CHECK(says(standings::check_path_lengths(row, -1, (double*)row), "num_waypoints"));
}

static void test_rules() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double d[1] = {0};
  int i[1] = {0};
  f110qp_race_config race;
  std::memset(&race, 0, sizeof(race));
  race.group_size = 2;
  race.car_radius = 0.3;
  race.center_offset = 0.1651;

  CHECK(standings::check_progress(4, 3, d, d, d, 2, d) == nullptr);
  CHECK(says(standings::check_progress(0, 3, d, d, d, 2, d), "batch"));
  CHECK(says(standings::check_progress(-1, 3, d, d, d, 2, d), "batch"));
  CHECK(says(standings::check_progress(4, 0, d, d, d, 2, d), "rows"));
  CHECK(says(standings::check_progress(1 << 16, 1 << 15, d, d, d, 2, d), "too large"));
  CHECK(standings::check_progress(1 << 15, 1 << 15, d, d, d, 2, d) == nullptr);  // 2^30 itself
  CHECK(says(standings::check_progress(2147483647, 2147483647, d, d, d, 2, d), "too large"));  // no int overflow
  CHECK(says(standings::check_progress(4, 3, d, d, d, 1, d), "num_waypoints"));
  CHECK(says(standings::check_progress(4, 3, nullptr, d, d, 2, d), "non-NULL"));
  CHECK(says(standings::check_progress(4, 3, d, nullptr, d, 2, d), "non-NULL"));
  CHECK(says(standings::check_progress(4, 3, d, d, nullptr, 2, d), "non-NULL"));
  CHECK(says(standings::check_progress(4, 3, d, d, d, 2, nullptr), "non-NULL"));

  CHECK(standings::check_standings(&race, 4, 3, d, 70.0, d, i) == nullptr);
  CHECK(says(standings::check_standings(nullptr, 4, 3, d, 70.0, d, i), "race config"));
  CHECK(says(standings::check_standings(&race, 0, 3, d, 70.0, d, i), "batch"));
  CHECK(says(standings::check_standings(&race, 4, -2, d, 70.0, d, i), "rows"));
  CHECK(says(standings::check_standings(&race, 5, 3, d, 70.0, d, i), "multiple of group_size"));
  for (const double L : {0.0, -1.0, nan, inf, -inf}) CHECK(says(standings::check_standings(&race, 4, 3, d, L, d, i), "path_length"));
  CHECK(says(standings::check_standings(&race, 4, 3, nullptr, 70.0, d, i), "non-NULL"));
  CHECK(says(standings::check_standings(&race, 4, 3, d, 70.0, nullptr, i), "non-NULL"));
  CHECK(says(standings::check_standings(&race, 4, 3, d, 70.0, d, nullptr), "non-NULL"));
  f110qp_race_config r = race;
  r.group_size = 0;
  CHECK(says(standings::check_standings(&r, 4, 3, d, 70.0, d, i), "group_size"));
  r = race;
  for (const double v : {0.0, -0.3, nan, inf}) {
    r.car_radius = v;
    CHECK(says(standings::check_standings(&r, 4, 3, d, 70.0, d, i), "car_radius"));
  }
  r = race;
  for (const double v : {nan, inf, -inf}) {
    r.center_offset = v;
    CHECK(says(standings::check_standings(&r, 4, 3, d, 70.0, d, i), "center_offset"));
  }

  CHECK(standings::check_race_standings(&race, 4, 3, d, d, 2, d, d, i) == nullptr);
  CHECK(says(standings::check_race_standings(nullptr, 4, 3, d, d, 2, d, d, i), "race config"));
  CHECK(says(standings::check_race_standings(&race, 4, 3, d, d, 1, d, d, i), "num_waypoints"));
  CHECK(says(standings::check_race_standings(&race, 4, 3, nullptr, d, 2, d, d, i), "non-NULL"));
  CHECK(says(standings::check_race_standings(&race, 4, 3, d, nullptr, 2, d, d, i), "non-NULL"));
  CHECK(says(standings::check_race_standings(&race, 4, 3, d, d, 2, nullptr, d, i), "non-NULL"));
  CHECK(says(standings::check_race_standings(&race, 4, 3, d, d, 2, d, nullptr, i), "non-NULL"));
  CHECK(says(standings::check_race_standings(&race, 4, 3, d, d, 2, d, d, nullptr), "non-NULL"));
}

int main() {
  test_path_lengths();
  test_rules();
  if (g_fail) return 1;
  std::printf("standings host ok\n");
  return 0;
}
