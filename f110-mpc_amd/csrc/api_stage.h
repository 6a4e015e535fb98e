// api_stage.h — the argument records of the closed-loop families and the staging table of their
// host-pointer calls: which arrays of a call are copied to the device, which come back, and where each
// stands in the context's staging buffer (f110qp_ctx::rdev). Layout arithmetic only, no HIP call and no
// HIP header, so host/tests/stage_layout.cpp runs it on the CPU; api_rollout.cpp issues the copies.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "f110qp.h"

#pragma GCC visibility push(hidden)

// The nine arrays every closed-loop family shares, device or host pointers, and tick t's rows of them.
struct RolloutIO {
  int B, N, T;         // cars, horizon, ticks (N and T set by the argument check)
  double* x_ref;       // [B][x_ref_points][3]; written by the re-planning families only
  double* x_traj;      // [T+1][B][3], row 0 the caller's
  double* u_lin_traj;  // [T+1][B][2], row 0 the caller's
  float* u_applied;    // [T][B][2]
  int* status_traj;    // [T][B]
  int* iters_traj;     // [T][B] or null
  double* cost_traj;   // [T][B] or null
  float* u_plan;       // [T][B][N][2] or null
  float* x_plan;       // [T][B][N+1][3] or null
  size_t n_up() const { return (size_t)B * N * 2; }
  size_t n_xp() const { return (size_t)B * (N + 1) * 3; }
  double* x(size_t t) const { return x_traj + t * B * 3; }
  double* ul(size_t t) const { return u_lin_traj + t * B * 2; }
  float* ua(size_t t) const { return u_applied + t * B * 2; }
  int* st(size_t t) const { return status_traj + t * B; }
  int* it(size_t t) const { return iters_traj ? iters_traj + t * B : nullptr; }
  double* cost(size_t t) const { return cost_traj ? cost_traj + t * B : nullptr; }
  // tick t's plans: the caller's row, or the one-tick workspace when the caller keeps none
  float* up(size_t t, float* work) const { return u_plan ? u_plan + t * n_up() : work; }
  float* xp(size_t t, float* work) const { return x_plan ? x_plan + t * n_xp() : work; }
};

// f110qp_rollout_scan[_dev]: the half-spaces follow the car.
struct ScanLoop {
  const f110qp_scan_config* sc;
  const float* ranges;  // [scan_rows][B][num_ranges]
  float* hs_traj;       // [T][B][6] or null: one row set in the context
};

// The optional per-tick arrays of a re-planning rollout; a null one lives in the context (ReplanWork).
struct ReplanTraj {
  float* hs;         // [T][B][6]
  int* kind;         // [T][B]
  int* plan_status;  // [T][B]
  int* best_traj;    // [T][B]
  int* best_global;  // [T][B]
  double* pose;      // [T+1][B][4], row 0 written by the start kernel
};

// What the re-planning families (replan, world, race) take on top of RolloutIO.
struct ReplanIO {
  const double* table;      // [steer_discrete + 1][traj_discrete][3]
  const double* waypoints;  // [num_waypoints][2] or null
  int* have_path;           // [B], in / out
  const float* ranges;      // [scan_rows][B][num_ranges]; the world and race rollouts cast theirs instead
  ReplanTraj tr;
};

// The world and race rollouts' host arrays (the checked CastParams stay in api_rollout.cpp's WorldLoop).
struct WorldIO {
  const double* circles;  // [world_rows][C][3] or null
  size_t circle_bytes;    // 0: no circles
  float* ranges_traj;     // [T][B][num_ranges] or null
  // the walls family's, trailing so that three initialisers still make a WorldIO
  const double* segments;  // [wall_rows][S][4] or null
  size_t segment_bytes;    // 0: no segments
  // the grid family's, trailing likewise
  const unsigned char* grid;  // [H][W] or null
  size_t grid_bytes;          // 0: no map (the field is then not declared)
  // f110qp_rollout_field's, trailing likewise: the map's distance field and its scratch, device only
  int* field;          // [2][H][W]; the host side is null
  size_t field_bytes;  // 0: not declared
};

// What the contact rollout records on top of the race rollout's arrays.
struct ContactIO {
  double* clear_traj;  // [T+1][B]
  int* nearest_traj;   // [T+1][B] or null
  int* crash_tick;     // [B]
};

namespace stage {

enum Dir { kWork = 0, kIn = 1, kOut = 2, kInOut = 3 };  // kWork: device only, no copy either way

// One array of a host-pointer call. row0 > 0 (the [T+1] trajectories): the leading row0 bytes are the
// caller's row 0, which is uploaded and not copied back; the rest is copied back and not uploaded.
struct Field {
  void* host;     // the caller's array (only read unless dir has kOut)
  void* slot;     // the pointer variable that receives the device address (Layout::bind)
  size_t bytes;   // 0: absent, takes no space
  size_t row0;
  size_t offset;  // in the staging buffer, a multiple of 8
  int dir;
  size_t h2d_bytes() const { return !(dir & kIn) ? 0 : row0 ? row0 : bytes; }
  size_t d2h_begin() const { return row0; }
  size_t d2h_bytes() const { return dir & kOut ? bytes - row0 : 0; }
};

struct Layout {
  static constexpr int kMaxFields = 32;  // the walls family declares 25
  Field f[kMaxFields];
  int n = 0;
  size_t total = 0;  // bytes of the staging buffer: the end of the last field

  // Declares one array: every field starts at an 8-byte multiple, so the doubles and the float2 rows
  // (u_applied, u_plan) are aligned wherever they stand. *dev receives the device address at bind().
  template <class H, class D>
  void add(H* host, D** dev, size_t bytes, bool present, Dir dir, size_t row0 = 0) {
    if (n == kMaxFields) std::abort();
    const bool on = present && bytes > 0;
    const size_t offset = (total + 7) & ~(size_t)7;
    f[n++] = Field{const_cast<void*>(static_cast<const void*>(host)), dev, on ? bytes : 0, on ? row0 : 0, offset,
                   on ? dir : 0};
    if (on) total = offset + bytes;
  }

  // The device addresses, once the buffer exists: base + offset, or null for an absent field.
  void bind(void* base) const {
    for (int i = 0; i < n; i++) {
      void* p = f[i].bytes ? (char*)base + f[i].offset : nullptr;
      std::memcpy(f[i].slot, &p, sizeof(p));
    }
  }
};

// The nine shared arrays, h the host's and *d the device's. xr_dir: kIn, or kInOut where the loop
// re-plans. A new optional per-tick array is one line here (or below) and one member of its record.
inline void io_fields(Layout& L, const RolloutIO& h, RolloutIO* d, size_t xr_points, Dir xr_dir) {
  const size_t B = (size_t)h.B, T = (size_t)h.T, TB = T * B;
  *d = h;
  L.add(h.x_ref, &d->x_ref, B * xr_points * 3 * 8, true, xr_dir);
  L.add(h.x_traj, &d->x_traj, (T + 1) * B * 3 * 8, true, kInOut, B * 3 * 8);
  L.add(h.u_lin_traj, &d->u_lin_traj, (T + 1) * B * 2 * 8, true, kInOut, B * 2 * 8);
  L.add(h.u_applied, &d->u_applied, TB * 2 * 4, true, kOut);
  L.add(h.status_traj, &d->status_traj, TB * 4, true, kOut);
  L.add(h.iters_traj, &d->iters_traj, TB * 4, h.iters_traj, kOut);
  L.add(h.cost_traj, &d->cost_traj, TB * 8, h.cost_traj, kOut);
  L.add(h.u_plan, &d->u_plan, T * h.n_up() * 4, h.u_plan, kOut);
  L.add(h.x_plan, &d->x_plan, T * h.n_xp() * 4, h.x_plan, kOut);
}

// f110qp_rollout (hs [B][6] held, when gap rows are active; sl null) and f110qp_rollout_scan (sl).
inline void rollout_fields(Layout& L, const RolloutIO& h, RolloutIO* d, size_t xr_points, const float* hs,
                           const float** d_hs, const ScanLoop* sl, ScanLoop* d_sl) {
  const size_t B = (size_t)h.B, T = (size_t)h.T;
  io_fields(L, h, d, xr_points, kIn);
  L.add(hs, d_hs, B * 6 * 4, hs, kIn);
  if (!sl) return;
  *d_sl = *sl;
  L.add(sl->ranges, &d_sl->ranges, (size_t)sl->sc->scan_rows * B * (size_t)sl->sc->num_ranges * 4, true, kIn);
  L.add(sl->hs_traj, &d_sl->hs_traj, T * B * 6 * 4, sl->hs_traj, kOut);
}

// f110qp_rollout_replan (w null: r.ranges read) and f110qp_rollout_world / _race (w: its circles staged
// in, its ranges_traj, when given, copied back) and f110qp_rollout_contact (w and k: its three records,
// every row of them the device's); the walls family's segments (w->segment_bytes > 0) are staged in behind the
// circles, the grid family's map (w->grid_bytes > 0) behind ranges_traj. table_rows = steer_discrete + 1.
inline void replan_fields(Layout& L, const RolloutIO& h, RolloutIO* d, const ReplanIO& r, ReplanIO* dr,
                          const f110qp_scan_config& sc, size_t table_rows, size_t xr_points, size_t num_waypoints,
                          const WorldIO* w, WorldIO* dw, const ContactIO* k = nullptr, ContactIO* dk = nullptr) {
  const size_t B = (size_t)h.B, T = (size_t)h.T, TB = T * B, nr = (size_t)sc.num_ranges;
  io_fields(L, h, d, xr_points, kInOut);
  *dr = r;
  L.add(r.table, &dr->table, table_rows * xr_points * 3 * 8, true, kIn);
  L.add(r.waypoints, &dr->waypoints, num_waypoints * 2 * 8, true, kIn);
  L.add(r.have_path, &dr->have_path, B * 4, true, kInOut);
  L.add(r.ranges, &dr->ranges, (size_t)sc.scan_rows * B * nr * 4, !w, kIn);
  L.add(r.tr.hs, &dr->tr.hs, TB * 6 * 4, r.tr.hs, kOut);
  L.add(r.tr.kind, &dr->tr.kind, TB * 4, r.tr.kind, kOut);
  L.add(r.tr.plan_status, &dr->tr.plan_status, TB * 4, r.tr.plan_status, kOut);
  L.add(r.tr.best_traj, &dr->tr.best_traj, TB * 4, r.tr.best_traj, kOut);
  L.add(r.tr.best_global, &dr->tr.best_global, TB * 4, r.tr.best_global, kOut);
  L.add(r.tr.pose, &dr->tr.pose, (T + 1) * B * 4 * 8, r.tr.pose, kOut);
  if (!w) return;
  *dw = *w;
  L.add(w->circles, &dw->circles, w->circle_bytes, true, kIn);
  L.add(w->segments, &dw->segments, w->segment_bytes, true, kIn);
  L.add(w->ranges_traj, &dw->ranges_traj, TB * nr * 4, w->ranges_traj, kOut);
  if (w->grid_bytes) L.add(w->grid, &dw->grid, w->grid_bytes, true, kIn);  // only the grid family declares it
  if (w->field_bytes) L.add(w->field, &dw->field, w->field_bytes, true, kWork);  // only f110qp_rollout_field
  if (!k) return;
  *dk = *k;
  L.add(k->clear_traj, &dk->clear_traj, (T + 1) * B * 8, true, kOut);
  L.add(k->nearest_traj, &dk->nearest_traj, (T + 1) * B * 4, k->nearest_traj, kOut);
  L.add(k->crash_tick, &dk->crash_tick, B * 4, true, kOut);
}

}  // namespace stage

#pragma GCC visibility pop
