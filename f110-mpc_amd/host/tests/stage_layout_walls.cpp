// stage_layout_walls.cpp — the staging table of f110qp_rollout_walls (csrc/api_stage.h) on the CPU: the walls
// family's field set (the contact records and every optional array on, which is the table's largest) with the
// segments present, absent and alone (no circles). B = 3, T = 3, N = 5 as host/tests/stage_layout.cpp.
// Built with -fsanitize=address,undefined (tests/test_stage_layout_walls.py): the copies of a call are replayed
// with memcpy between exactly sized heap arrays, so a wrong size or offset is an error of the sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_stage.h"

static int g_fail = 0;
static char g_case[64];
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAIL %s:%d (%s): %s\n", __FILE__, __LINE__, g_case, #cond); \
      g_fail++;                                                             \
    }                                                                       \
  } while (0)

constexpr size_t B = 3, T = 3, N = 5, P = 7, TC = 4, W = 2, NR = 5;

template <class E>
static E* host_array(std::vector<void*>& pool, bool on, size_t bytes) {
  if (!on || !bytes) return nullptr;
  void* p = std::malloc(bytes);
  std::memset(p, 0x11, bytes);
  pool.push_back(p);
  return (E*)p;
}

static const stage::Field* find(const stage::Layout& L, const void* host) {
  for (int i = 0; i < L.n; i++)
    if (L.f[i].host == host && L.f[i].bytes) return &L.f[i];
  return nullptr;
}

// The copies of a call replayed against a buffer of exactly L.total bytes.
static void replay(const stage::Layout& L, int present) {
  size_t end = 0;
  int on = 0;
  for (int i = 0; i < L.n; i++) {
    const stage::Field& f = L.f[i];
    CHECK(f.offset % 8 == 0);
    if (!f.bytes) {
      CHECK(f.h2d_bytes() == 0 && f.d2h_bytes() == 0);
      continue;
    }
    on++;
    CHECK(f.offset >= end && f.offset < end + 8);
    end = f.offset + f.bytes;
  }
  CHECK(on == present);
  CHECK(L.total == end);
  char* dev = (char*)std::malloc(L.total);
  std::memset(dev, 0x22, L.total);
  std::vector<void*> slots(L.n);
  stage::Layout M = L;
  for (int i = 0; i < M.n; i++) M.f[i].slot = &slots[i];
  M.bind(dev);
  for (int i = 0; i < L.n; i++) {
    const stage::Field& f = L.f[i];
    CHECK(slots[i] == (f.bytes ? dev + f.offset : nullptr));
    if (f.h2d_bytes()) std::memcpy(dev + f.offset, f.host, f.h2d_bytes());
  }
  for (int i = 0; i < L.n; i++) {
    const stage::Field& f = L.f[i];
    if (f.d2h_bytes()) std::memcpy((char*)f.host + f.d2h_begin(), dev + f.offset + f.d2h_begin(), f.d2h_bytes());
  }
  std::free(dev);
}

// circles and segments: per world; rows: 1 or B sets of segments
static void walls_case(bool optional, size_t circles, size_t segments, size_t rows) {
  std::snprintf(g_case, sizeof g_case, "walls opt %d C %zu S %zu rows %zu", (int)optional, circles, segments, rows);
  std::vector<void*> pool;
  RolloutIO h{};
  h.B = (int)B, h.N = (int)N, h.T = (int)T;
  h.x_ref = host_array<double>(pool, true, B * P * 3 * 8);
  h.x_traj = host_array<double>(pool, true, (T + 1) * B * 3 * 8);
  h.u_lin_traj = host_array<double>(pool, true, (T + 1) * B * 2 * 8);
  h.u_applied = host_array<float>(pool, true, T * B * 2 * 4);
  h.status_traj = host_array<int>(pool, true, T * B * 4);
  h.iters_traj = host_array<int>(pool, optional, T * B * 4);
  h.cost_traj = host_array<double>(pool, optional, T * B * 8);
  h.u_plan = host_array<float>(pool, optional, T * B * N * 2 * 4);
  h.x_plan = host_array<float>(pool, optional, T * B * (N + 1) * 3 * 4);
  f110qp_scan_config sc{};
  sc.num_ranges = (int)NR;
  sc.scan_rows = 1;
  ReplanIO r{};
  r.table = host_array<double>(pool, true, TC * P * 3 * 8);
  r.waypoints = host_array<double>(pool, true, W * 2 * 8);
  r.have_path = host_array<int>(pool, true, B * 4);
  r.tr.hs = host_array<float>(pool, optional, T * B * 6 * 4);
  r.tr.kind = host_array<int>(pool, optional, T * B * 4);
  r.tr.plan_status = host_array<int>(pool, optional, T * B * 4);
  r.tr.best_traj = host_array<int>(pool, optional, T * B * 4);
  r.tr.best_global = host_array<int>(pool, optional, T * B * 4);
  r.tr.pose = host_array<double>(pool, optional, (T + 1) * B * 4 * 8);
  const size_t sbytes = rows * segments * 4 * 8;
  const WorldIO w{host_array<double>(pool, circles > 0, circles * 3 * 8), circles * 3 * 8,
                  host_array<float>(pool, optional, T * B * NR * 4), host_array<double>(pool, true, sbytes), sbytes};
  const ContactIO k{host_array<double>(pool, true, (T + 1) * B * 8), host_array<int>(pool, optional, (T + 1) * B * 4),
                    host_array<int>(pool, true, B * 4)};
  stage::Layout L;
  RolloutIO d;
  ReplanIO dr;
  WorldIO dw;
  ContactIO dk;
  stage::replan_fields(L, h, &d, r, &dr, sc, TC, P, W, &w, &dw, &k, &dk);
  CHECK(L.n == 25 && L.n <= stage::Layout::kMaxFields);  // every field of the family is declared, present or not
  // the nine's five, table, waypoints, have_path, clear_traj, crash_tick; 12 optional arrays
  replay(L, 10 + (optional ? 12 : 0) + (circles > 0) + (sbytes > 0));
  const stage::Field* sf = find(L, w.segments);
  if (sbytes) {
    CHECK(sf && sf->bytes == sbytes && sf->dir == stage::kIn && sf->h2d_bytes() == sbytes && sf->d2h_bytes() == 0);
    CHECK(dw.segments != nullptr);
    if (circles) CHECK(sf->offset > find(L, w.circles)->offset);  // behind the circles
  } else {
    CHECK(!sf);
  }
  const stage::Field* cf = find(L, k.clear_traj);
  CHECK(cf && cf->dir == stage::kOut && cf->d2h_bytes() == (T + 1) * B * 8);
  for (void* p : pool) std::free(p);
}

int main() {
  for (int opt = 0; opt < 2; opt++) {
    walls_case(opt, 2, 5, 1);      // one world, one set of segments
    walls_case(opt, 2, 5, B);      // a set per car
    walls_case(opt, B * 2, 5, 1);  // a world per car
    walls_case(opt, 2, 0, 1);      // no segments
    walls_case(opt, 0, 5, 1);      // segments alone
    walls_case(opt, 0, 0, 1);      // neither
  }
  if (g_fail) return 1;
  std::printf("stage layout walls ok\n");
  return 0;
}
