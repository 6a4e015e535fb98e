// stage_layout.cpp — the staging table of the host-pointer rollouts (csrc/api_stage.h) on the CPU: the
// field sets of f110qp_rollout / _scan and of f110qp_rollout_replan / _world, as the library declares
// them, for every optional array on, off and alone. B = 3, T = 3, N = 5: T*B*4 = 36 is no multiple of 8.
// Built with -fsanitize=address,undefined (tests/test_stage_layout.py): the copies of a call are replayed
// with memcpy between exactly sized heap arrays, so a wrong size or offset is an error of the sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_stage.h"

static int g_fail = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAIL %s:%d (%s): %s\n", __FILE__, __LINE__, g_case, #cond); \
      g_fail++;                                                             \
    }                                                                       \
  } while (0)
static char g_case[64];

constexpr size_t B = 3, T = 3, N = 5, P = 7, TC = 4, W = 2, NR = 5, C = 2;

// an exactly sized heap array (or null when `on` is false), filled with a host pattern
template <class E>
static E* host_array(std::vector<void*>& pool, bool on, size_t bytes) {
  if (!on) return nullptr;
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

// The properties of every layout, then the copies of a call replayed against a buffer of L.total bytes.
static void check_layout(const stage::Layout& L, int present) {
  size_t end = 0;
  int on = 0;
  for (int i = 0; i < L.n; i++) {
    const stage::Field& f = L.f[i];
    CHECK(f.offset % 8 == 0);
    if (!f.bytes) {  // absent: no space, no copy
      CHECK(f.h2d_bytes() == 0 && f.d2h_bytes() == 0);
      continue;
    }
    on++;
    CHECK(f.offset >= end);  // declared in order: no overlap with any field before it
    CHECK(f.offset < end + 8);
    end = f.offset + f.bytes;
    CHECK(f.row0 < f.bytes && f.h2d_bytes() <= f.bytes && f.d2h_begin() + f.d2h_bytes() <= f.bytes);
  }
  CHECK(on == present);
  CHECK(L.total == end);  // the end of the last field
  char* dev = (char*)std::malloc(L.total);
  std::memset(dev, 0x22, L.total);
  std::vector<void*> slots(L.n);
  stage::Layout M = L;  // bind into slots of our own: the device copies of the records are the caller's
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
    if (!f.bytes) continue;
    const unsigned char* h = (const unsigned char*)f.host;
    // row 0 and the inputs keep the host's bytes; what came back that was not uploaded is the device's
    if (f.row0) CHECK(h[0] == 0x11 && h[f.row0 - 1] == 0x11 && h[f.row0] == 0x22 && h[f.bytes - 1] == 0x22);
    else CHECK(h[0] == (f.dir == stage::kOut ? 0x22 : 0x11) && h[f.bytes - 1] == h[0]);
  }
  std::free(dev);
}

enum { IT = 1, CO = 2, UP = 4, XP = 8, HS = 16, KIND = 32, PS = 64, BT = 128, BG = 256, POSE = 512, SCANS = 1024 };

static RolloutIO host_io(std::vector<void*>& pool, int opt, size_t xr_points) {
  RolloutIO h{};
  h.B = (int)B, h.N = (int)N, h.T = (int)T;
  h.x_ref = host_array<double>(pool, true, B * xr_points * 3 * 8);
  h.x_traj = host_array<double>(pool, true, (T + 1) * B * 3 * 8);
  h.u_lin_traj = host_array<double>(pool, true, (T + 1) * B * 2 * 8);
  h.u_applied = host_array<float>(pool, true, T * B * 2 * 4);
  h.status_traj = host_array<int>(pool, true, T * B * 4);
  h.iters_traj = host_array<int>(pool, opt & IT, T * B * 4);
  h.cost_traj = host_array<double>(pool, opt & CO, T * B * 8);
  h.u_plan = host_array<float>(pool, opt & UP, T * B * N * 2 * 4);
  h.x_plan = host_array<float>(pool, opt & XP, T * B * (N + 1) * 3 * 4);
  return h;
}

static int bits(int v) { return __builtin_popcount((unsigned)v); }

static void check_rows0(const stage::Layout& L, const RolloutIO& h) {
  const stage::Field* xt = find(L, h.x_traj);
  const stage::Field* ul = find(L, h.u_lin_traj);
  CHECK(xt && xt->row0 == B * 3 * 8 && xt->h2d_bytes() == B * 3 * 8 && xt->d2h_bytes() == T * B * 3 * 8);
  CHECK(ul && ul->row0 == B * 2 * 8 && ul->h2d_bytes() == B * 2 * 8 && ul->d2h_bytes() == T * B * 2 * 8);
}

// f110qp_rollout (scan_rows 0: no scans; opt & HS: the held rows) and f110qp_rollout_scan (opt & HS: hs_traj)
static void rollout_case(int opt, int scan_rows) {
  std::snprintf(g_case, sizeof g_case, "rollout opt %d scan_rows %d", opt, scan_rows);
  std::vector<void*> pool;
  const RolloutIO h = host_io(pool, opt, P);
  f110qp_scan_config sc{};
  sc.num_ranges = (int)NR;
  sc.scan_rows = scan_rows;
  const ScanLoop sl{&sc, host_array<float>(pool, scan_rows > 0, (size_t)scan_rows * B * NR * 4),
                    host_array<float>(pool, scan_rows > 0 && (opt & HS), T * B * 6 * 4)};
  const float* hs = host_array<float>(pool, !scan_rows && (opt & HS), B * 6 * 4);
  stage::Layout L;
  RolloutIO d;
  ScanLoop dsl;
  const float* d_hs;
  stage::rollout_fields(L, h, &d, P, hs, &d_hs, scan_rows ? &sl : nullptr, &dsl);
  CHECK(d.B == h.B && d.N == h.N && d.T == h.T);
  check_layout(L, 5 + bits(opt) + (scan_rows > 0));
  check_rows0(L, h);
  CHECK(find(L, h.x_ref)->dir == stage::kIn);
  for (void* p : pool) std::free(p);
}

// f110qp_rollout_replan (world false) and f110qp_rollout_world / _race (world; opt & SCANS: ranges_traj)
static void replan_case(int opt, bool world, int scan_rows, size_t waypoints, size_t circles) {
  std::snprintf(g_case, sizeof g_case, "replan opt %d world %d scan_rows %d", opt, (int)world, scan_rows);
  std::vector<void*> pool;
  const RolloutIO h = host_io(pool, opt, P);
  f110qp_scan_config sc{};
  sc.num_ranges = (int)NR;
  sc.scan_rows = scan_rows;
  ReplanIO r{};
  r.table = host_array<double>(pool, true, TC * P * 3 * 8);
  r.waypoints = host_array<double>(pool, waypoints > 0, waypoints * 2 * 8);
  r.have_path = host_array<int>(pool, true, B * 4);
  r.ranges = host_array<float>(pool, !world, (size_t)scan_rows * B * NR * 4);
  r.tr.hs = host_array<float>(pool, opt & HS, T * B * 6 * 4);
  r.tr.kind = host_array<int>(pool, opt & KIND, T * B * 4);
  r.tr.plan_status = host_array<int>(pool, opt & PS, T * B * 4);
  r.tr.best_traj = host_array<int>(pool, opt & BT, T * B * 4);
  r.tr.best_global = host_array<int>(pool, opt & BG, T * B * 4);
  r.tr.pose = host_array<double>(pool, opt & POSE, (T + 1) * B * 4 * 8);
  const WorldIO w{host_array<double>(pool, world && circles, circles * 3 * 8), circles * 3 * 8,
                  host_array<float>(pool, world && (opt & SCANS), T * B * NR * 4)};
  stage::Layout L;
  RolloutIO d;
  ReplanIO dr;
  WorldIO dw;
  stage::replan_fields(L, h, &d, r, &dr, sc, TC, P, waypoints, world ? &w : nullptr, &dw);
  const int fixed = 5 + 2 + (waypoints > 0) + (world ? (circles > 0) : 1);  // the nine's five, table, have_path
  check_layout(L, fixed + bits(world ? opt : opt & ~SCANS));
  check_rows0(L, h);
  CHECK(find(L, h.x_ref)->dir == stage::kInOut && find(L, r.have_path)->dir == stage::kInOut);
  // pose_traj [T+1][B][4]: rows of B*4*8 bytes; every row is the device's (the start kernel writes row 0),
  // so all of it is copied back and none uploaded
  if (const stage::Field* po = find(L, r.tr.pose))
    CHECK(po->bytes == (T + 1) * (B * 4 * 8) && po->row0 == 0 && po->h2d_bytes() == 0 && po->d2h_bytes() == po->bytes);
  for (void* p : pool) std::free(p);
}

int main() {
  const int ropt[] = {0, IT | CO | UP | XP | HS, IT, CO, UP, XP, HS};
  for (int opt : ropt) {
    rollout_case(opt, 0);
    rollout_case(opt, 1);
    rollout_case(opt, (int)T);
  }
  const int all = IT | CO | UP | XP | HS | KIND | PS | BT | BG | POSE | SCANS;
  std::vector<int> popt{0, all};
  for (int b = 1; b <= SCANS; b <<= 1) popt.push_back(b);
  for (int opt : popt) {
    replan_case(opt, false, 1, W, 0);
    replan_case(opt, false, (int)T, 0, 0);
    replan_case(opt, true, 1, W, C);      // one world
    replan_case(opt, true, 1, 0, B * C);  // a world per car
    replan_case(opt, true, 1, W, 0);      // a race without circles
  }
  if (g_fail) return 1;
  std::printf("stage layout ok\n");
  return 0;
}
