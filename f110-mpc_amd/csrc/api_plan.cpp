// api_plan.cpp — the C ABI's half-space and planning-stage entry points (include/f110qp.h):
// Constraints::FindHalfSpaces for one scan on the host (reference src/constraints.cpp:116-265) and for a
// batch on the device, the trajectory table, the waypoint parser and f110qp_plan_batch[_dev].
// No C++ exception crosses this boundary.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.h"

int validate_plan(const f110qp_plan_config* c, int* G) {
  if (!c) return fail(F110QP_ERR_INVALID, "plan config is NULL");
  if (!(c->discrete > 0.f) || c->size <= 0 || !(c->dilation >= 0.f))
    return fail(F110QP_ERR_INVALID, "occupancy grid size/discrete/dilation");
  const int g = (int)((float)c->size / c->discrete);  // occupancy_grid.cpp:9
  if (g < 1 || g > 200) return fail(F110QP_ERR_INVALID, "grid_blocks must be in [1, 200]");
  if (c->steer_discrete < 1 || c->steer_discrete > 255 || c->traj_discrete < 2 || c->traj_discrete > 1024)
    return fail(F110QP_ERR_INVALID, "steer_discrete in [1, 255], traj_discrete in [2, 1024]");
  *G = g;
  return F110QP_OK;
}

// f110qp_find_half_spaces_dev[_dbl]: IN the element type of the states.
template <typename IN>
static int half_spaces_dev(int batch, const IN* states, const float* ranges, int nr, float angle_min,
                           float angle_inc, float angle_max, float ftg_thresh, float divider, float buffer,
                           float* hs, int* gap_lo, int* gap_hi, void* stream) {
  if (batch < 0 || nr <= 0 || nr > 65535) return fail(F110QP_ERR_INVALID, "bad batch / num_ranges (1..65535)");
  if (batch == 0) return F110QP_OK;
  if (!states || !ranges || !hs) return fail(F110QP_ERR_INVALID, "NULL pointer argument");
  if (!(angle_inc > 0.f)) return fail(F110QP_ERR_INVALID, "angle_increment must be > 0");
  hipError_t e = f110qp::launch_half_spaces(batch, states, ranges, nr, angle_min, angle_inc,
                                            angle_max, ftg_thresh, divider, buffer, hs, gap_lo,
                                            gap_hi, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "half-space kernel launch");
  return F110QP_OK;
}

namespace {
// device staging of f110qp_plan_batch, one set per host thread
struct PlanBufs {
  DevBuf pose, ranges, table, wp, grid, valid, bg, bt, xr, x0, st;
  hipStream_t stream = nullptr;
  ~PlanBufs() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};
thread_local PlanBufs g_plan;
}  // namespace

extern "C" {

// Constraints::FindHalfSpaces (src/constraints.cpp:116-265) for one scan, host code with the
// reference's float32 member types; the ROS marker publish (:191-229) is not reproduced.
int f110qp_find_half_spaces(const double state[3], const float* ranges, int nr, float angle_min,
                            float angle_inc, float angle_max, float ftg_thresh, float divider,
                            float buffer, double l1[3], double l2[3]) {
  if (!state || !ranges || !l1 || !l2 || nr <= 0)
    return fail(F110QP_ERR_INVALID, "NULL pointer or empty scan");
  int num_scans = (int)((angle_max - angle_min) / angle_inc + 1);
  if (num_scans > nr) num_scans = nr;
  int max_gap = -1, best_lo = 0, best_hi = 0, lo = -1, hi = -1;
  bool in_gap = false;
  const float lim = 1.571f / divider;
  for (int ii = 0; ii < num_scans; ii++) {
    const float angle = angle_min + ii * angle_inc;
    if (angle > -lim && angle < lim) {
      if (ranges[ii] > ftg_thresh) {
        if (in_gap) hi = ii;
        else { lo = ii; in_gap = true; }
      } else {
        in_gap = false;
      }
      if (hi - lo > max_gap) { max_gap = hi - lo; best_hi = hi; best_lo = lo; }
    }
  }
  if (best_hi - best_lo > 2 * buffer) {
    best_hi = (int)(best_hi - buffer);
    best_lo = (int)(best_lo + buffer);
  }
  if (best_lo < 0 || best_hi < 0 || best_lo >= nr || best_hi >= nr)
    return fail(F110QP_ERR_INVALID, "scan holds no gap (reference reads ranges[-1] here)");
  const double poseX = state[0], poseY = state[1];
  const float cur = (float)state[2];
  const float ang1 = angle_min + best_lo * angle_inc + cur;
  const float ang2 = angle_min + best_hi * angle_inc + cur;
  const float p1x = (float)(ranges[best_lo] * std::cos((double)ang1) + poseX);
  const float p1y = (float)(ranges[best_lo] * std::sin((double)ang1) + poseY);
  const float p2x = (float)(ranges[best_hi] * std::cos((double)ang2) + poseX);
  const float p2y = (float)(ranges[best_hi] * std::sin((double)ang2) + poseY);
  const float px = (float)poseX, py = (float)poseY;
  float a1 = py - p1y, b1 = p1x - px, c1 = px * p1y - py * p1x;
  if (a1 * p2x + b1 * p2y + c1 < 0) { a1 = -a1; b1 = -b1; c1 = -c1; }
  float a2 = py - p2y, b2 = p2x - px, c2 = px * p2y - py * p2x;
  if (a2 * p1x + b2 * p1y + c2 < 0) { a2 = -a2; b2 = -b2; c2 = -c2; }
  l1[0] = a1; l1[1] = b1; l1[2] = (double)c1 + 0.5;
  l2[0] = a2; l2[1] = b2; l2[2] = (double)c2 + 0.5;
  return F110QP_OK;
}

int f110qp_find_half_spaces_dev(int batch, const float* states, const float* ranges, int nr,
                                float angle_min, float angle_inc, float angle_max,
                                float ftg_thresh, float divider, float buffer, float* hs,
                                int* gap_lo, int* gap_hi, void* stream) {
  return half_spaces_dev(batch, states, ranges, nr, angle_min, angle_inc, angle_max, ftg_thresh, divider, buffer,
                         hs, gap_lo, gap_hi, stream);
}

int f110qp_find_half_spaces_dev_dbl(int batch, const double* states, const float* ranges, int nr,
                                    float angle_min, float angle_inc, float angle_max,
                                    float ftg_thresh, float divider, float buffer, float* hs,
                                    int* gap_lo, int* gap_hi, void* stream) {
  return half_spaces_dev(batch, states, ranges, nr, angle_min, angle_inc, angle_max, ftg_thresh, divider, buffer,
                         hs, gap_lo, gap_hi, stream);
}

// ---- planning stage -----------------------------------------------------------------------

void f110qp_default_plan_config(f110qp_plan_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->size = 10;            // params.yaml:16
  c->discrete = 0.1f;      // params.yaml:17
  c->dilation = 0.15f;     // params.yaml:18
  c->lookahead = 2.5f;     // params.yaml:63
  c->speed_max = 4.5;      // params.yaml:46 (umax)
  c->steer_max = 0.4;      // params.yaml:60
  c->steer_discrete = 30;  // params.yaml:59
  c->traj_discrete = 50;   // params.yaml:61
  c->dt = 0.01;            // params.yaml:13
}

// Traj_Plan::generate_traj_table (trajectory_planner.cpp:26-72) with Model::simulate_dynamics
// (model.cpp:61-75, CAR_LENGTH = 0.35), doubles as the reference's State/Input.
int f110qp_traj_table(const f110qp_plan_config* c, double* table) {
  int G;
  int rc = validate_plan(c, &G);
  if (rc) return rc;
  if (!table) return fail(F110QP_ERR_INVALID, "table is NULL");
  const double ds = 2 * +c->steer_max / c->steer_discrete;  // :31
  const int T = c->steer_discrete + 1, P = c->traj_discrete;
  const double CAR_LENGTH = 0.35;
  for (int i = 0; i < T; i++) {
    const double steer = -c->steer_max + i * ds;  // :43
    const double v = c->speed_max;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    double* row = table + (size_t)i * P * 3;
    row[0] = s0; row[1] = s1; row[2] = s2;  // k == 0 (:54)
    for (int k = 1; k < P; k++) {
      const volatile double d0 = v * std::cos(s2), d1 = v * std::sin(s2);
      const volatile double d2 = std::tan(steer) * v / CAR_LENGTH;
      const volatile double e0 = d0 * c->dt, e1 = d1 * c->dt, e2 = d2 * c->dt;  // dynamics*dt
      s0 = s0 + e0; s1 = s1 + e1; s2 = s2 + e2;
      row[3 * k] = s0; row[3 * k + 1] = s1; row[3 * k + 2] = s2;
    }
  }
  return T;
}

// Trajectory::ReadCSV (trajectory.cpp:18-55): getline(',') then getline() and stof of each.
int f110qp_parse_waypoints(const char* text, double* wp, int max_n, int* n_out) {
  if (!text || !wp || !n_out || max_n < 0) return fail(F110QP_ERR_INVALID, "NULL argument");
  std::string buf;
  int n = 0;
  const char* s = text;
  std::string xs, ys;
  // temp.push_back(pair<float,float>(stof(coordX), stof(coordY)))
  std::vector<float> tx, ty;
  while (*s) {
    const char* comma = std::strchr(s, ',');
    if (!comma) break;
    xs.assign(s, comma - s);
    const char* eol = std::strchr(comma + 1, '\n');
    ys.assign(comma + 1, eol ? (size_t)(eol - comma - 1) : std::strlen(comma + 1));
    char* e1;
    char* e2;
    const float x = std::strtof(xs.c_str(), &e1);
    const float y = std::strtof(ys.c_str(), &e2);
    if (e1 == xs.c_str() || e2 == ys.c_str()) return fail(F110QP_ERR_INVALID, "stof: no conversion");
    tx.push_back(x);
    ty.push_back(y);
    s = eol ? eol + 1 : comma + 1 + std::strlen(comma + 1);
  }
  const unsigned int cnt = (unsigned int)tx.size();
  for (unsigned int i = 0; i < cnt && (int)i < max_n; i++) {
    const unsigned int prev = (i - 1) % cnt;  // :42-43 (unsigned wrap for i = 0)
    const float x = tx[i], y = ty[i];
    wp[3 * i] = x;
    wp[3 * i + 1] = y;
    wp[3 * i + 2] = (float)std::atan2((double)(y - ty[prev]), (double)(x - tx[prev]));  // :46
    n++;
  }
  *n_out = n;
  return F110QP_OK;
}

int f110qp_plan_batch_dev(const f110qp_plan_config* c, int batch, const double* pose,
                          const float* ranges, int nr, float angle_min, float angle_inc,
                          float angle_max, const double* table, const double* wp, int W,
                          unsigned char* grid, unsigned char* valid, int* best_global,
                          int* best_traj, float* x_ref, float* x0, int* status, void* stream) {
  int G;
  int rc = validate_plan(c, &G);
  if (rc) return rc;
  if (batch < 0 || nr <= 0 || W < 0) return fail(F110QP_ERR_INVALID, "bad batch / num_ranges / num_waypoints");
  if (batch == 0) return F110QP_OK;
  if (!pose || !ranges || !table || (W > 0 && !wp) || !best_global || !best_traj || !x_ref || !x0 || !status)
    return fail(F110QP_ERR_INVALID, "NULL pointer argument");
  if (!(angle_inc > 0.f)) return fail(F110QP_ERR_INVALID, "angle_increment must be > 0");
  f110qp::PlanKParams K;
  K.G = G;
  K.T = c->steer_discrete + 1;
  K.P = c->traj_discrete;
  K.discrete = c->discrete;
  K.dilation = c->dilation;
  K.lookahead = c->lookahead;
  hipError_t e = f110qp::launch_plan(K, batch, pose, ranges, nr, angle_min, angle_inc, angle_max,
                                     table, wp, W, grid, valid, best_global, best_traj, x_ref, x0,
                                     status, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "plan kernel launch");
  return F110QP_OK;
}

int f110qp_plan_batch(const f110qp_plan_config* c, int batch, const double* pose,
                      const float* ranges, int nr, float angle_min, float angle_inc,
                      float angle_max, const double* table, const double* wp, int W,
                      unsigned char* grid, unsigned char* valid, int* best_global,
                      int* best_traj, float* x_ref, float* x0, int* status) {
  int G;
  int rc = validate_plan(c, &G);
  if (rc) return rc;
  if (batch < 0 || nr <= 0 || W < 0) return fail(F110QP_ERR_INVALID, "bad batch / num_ranges / num_waypoints");
  if (batch == 0) return F110QP_OK;
  if (!pose || !ranges || !table || (W > 0 && !wp) || !best_global || !best_traj || !x_ref || !x0 || !status)
    return fail(F110QP_ERR_INVALID, "NULL pointer argument");
  PlanBufs& pb = g_plan;
  hipError_t e;
  if (!pb.stream && (e = hipStreamCreateWithFlags(&pb.stream, hipStreamNonBlocking)))
    return hip_fail(e, "hipStreamCreate");
  const size_t B = (size_t)batch, T = (size_t)c->steer_discrete + 1, P = (size_t)c->traj_discrete;
  const size_t s_pose = B * 4 * 8, s_r = B * nr * 4, s_tab = T * P * 3 * 8, s_wp = (size_t)W * 2 * 8;
  const size_t s_grid = B * G * G, s_valid = B * T, s_i = B * 4, s_xr = B * P * 3 * 4, s_x0 = B * 3 * 4;
  if ((e = pb.pose.ensure(s_pose)) || (e = pb.ranges.ensure(s_r)) || (e = pb.table.ensure(s_tab)) ||
      (e = pb.wp.ensure(s_wp ? s_wp : 8)) || (grid && (e = pb.grid.ensure(s_grid))) ||
      (valid && (e = pb.valid.ensure(s_valid))) || (e = pb.bg.ensure(s_i)) || (e = pb.bt.ensure(s_i)) ||
      (e = pb.xr.ensure(s_xr)) || (e = pb.x0.ensure(s_x0)) || (e = pb.st.ensure(s_i)))
    return hip_fail(e, "hipMalloc plan workspace");
  hipStream_t s = pb.stream;
  if ((e = hipMemcpyAsync(pb.pose.p, pose, s_pose, hipMemcpyHostToDevice, s)) ||
      (e = hipMemcpyAsync(pb.ranges.p, ranges, s_r, hipMemcpyHostToDevice, s)) ||
      (e = hipMemcpyAsync(pb.table.p, table, s_tab, hipMemcpyHostToDevice, s)) ||
      (W > 0 && (e = hipMemcpyAsync(pb.wp.p, wp, s_wp, hipMemcpyHostToDevice, s))))
    return hip_fail(e, "hipMemcpyAsync H2D");
  rc = f110qp_plan_batch_dev(c, batch, (const double*)pb.pose.p, (const float*)pb.ranges.p, nr, angle_min,
                             angle_inc, angle_max, (const double*)pb.table.p, (const double*)pb.wp.p, W,
                             grid ? (unsigned char*)pb.grid.p : nullptr,
                             valid ? (unsigned char*)pb.valid.p : nullptr, (int*)pb.bg.p, (int*)pb.bt.p,
                             (float*)pb.xr.p, (float*)pb.x0.p, (int*)pb.st.p, s);
  if (rc) return rc;
  if ((e = hipMemcpyAsync(best_global, pb.bg.p, s_i, hipMemcpyDeviceToHost, s)) ||
      (e = hipMemcpyAsync(best_traj, pb.bt.p, s_i, hipMemcpyDeviceToHost, s)) ||
      (e = hipMemcpyAsync(x_ref, pb.xr.p, s_xr, hipMemcpyDeviceToHost, s)) ||
      (e = hipMemcpyAsync(x0, pb.x0.p, s_x0, hipMemcpyDeviceToHost, s)) ||
      (e = hipMemcpyAsync(status, pb.st.p, s_i, hipMemcpyDeviceToHost, s)) ||
      (grid && (e = hipMemcpyAsync(grid, pb.grid.p, s_grid, hipMemcpyDeviceToHost, s))) ||
      (valid && (e = hipMemcpyAsync(valid, pb.valid.p, s_valid, hipMemcpyDeviceToHost, s))))
    return hip_fail(e, "hipMemcpyAsync D2H");
  if ((e = hipStreamSynchronize(s))) return hip_fail(e, "hipStreamSynchronize");
  return F110QP_OK;
}

}  // extern "C"
