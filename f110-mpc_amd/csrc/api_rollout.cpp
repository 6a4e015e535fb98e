// api_rollout.cpp — the C ABI's closed loops on the device (include/f110qp.h): the plant step and the
// rollout (f110qp_advance_dev, f110qp_rollout[_dev]), the rollout with gap rows from the scans
// (f110qp_rollout_scan[_dev]), with re-planning (f110qp_rollout_replan[_dev]), in a world of circles
// (f110qp_rollout_world[_dev]), with race-mates (f110qp_rollout_race[_dev]) and with contact
// (f110qp_clearance_dev, f110qp_rollout_contact[_dev]) and with rectangular bodies (f110qp_clearance_body_dev,
// f110qp_cast_scans_body_dev, f110qp_rollout_body[_dev]) and with straight walls (f110qp_cast_scans_walls_dev,
// f110qp_clearance_walls_dev, f110qp_rollout_walls[_dev]) and with a refreshed MPC scan (f110qp_gap_refresh_dev,
// f110qp_rollout_refresh[_dev]) and with a noisy LiDAR (f110qp_cast_scans_noisy_dev, f110qp_rollout_noisy[_dev]),
// and with a raster map (f110qp_cast_scans_grid_dev, f110qp_clearance_grid_dev, f110qp_rollout_grid[_dev]) and with
// that map's casts through its distance field (f110qp_grid_cast_dev, f110qp_rollout_field[_dev]), and the parts of
// each.
// Host-side responsibilities only: argument validation, workspaces, H2D/D2H of the host-pointer calls
// (the staging table of api_stage.h). No C++ exception crosses this boundary.
#include <cmath>
#include <cstring>

#include "api_common.h"
#include "api_stage.h"
#include "halfspace_geom.h"

static_assert(sizeof(f110qp_gap_record) == sizeof(f110qp::GapRecord) && sizeof(f110qp_gap_record) == 16,
              "the ABI's gap record is the kernels' GapRecord");

// ---- configs ---------------------------------------------------------------------------------------

static int rollout_params(const f110qp_rollout_config* rc, bool ticks, f110qp::AdvanceParams* ap) {
  if (!rc) return fail(F110QP_ERR_INVALID, "rollout config is NULL");
  if (ticks && rc->ticks < 1) return fail(F110QP_ERR_INVALID, "ticks must be >= 1");
  if (!(rc->plant_dt > 0.0) || !std::isfinite(rc->plant_dt))
    return fail(F110QP_ERR_INVALID, "plant_dt must be positive and finite");
  if (!(rc->car_length > 0.0) || !std::isfinite(rc->car_length))
    return fail(F110QP_ERR_INVALID, "car_length must be positive and finite");
  if (!std::isfinite(rc->v_lin) || !std::isfinite(rc->fail_u[0]) || !std::isfinite(rc->fail_u[1]))
    return fail(F110QP_ERR_INVALID, "v_lin and fail_u must be finite");
  ap->plant_dt = rc->plant_dt;
  ap->car_length = rc->car_length;
  ap->v_lin = rc->v_lin;
  ap->fail_u[0] = rc->fail_u[0];
  ap->fail_u[1] = rc->fail_u[1];
  return F110QP_OK;
}

static int replan_params(const f110qp_replan_config* rp, f110qp::PlanKParams* K) {
  if (!rp) return fail(F110QP_ERR_INVALID, "replan config is NULL");
  if (!(rp->replan_dist > 0.0) || !std::isfinite(rp->replan_dist))
    return fail(F110QP_ERR_INVALID, "replan_dist must be positive and finite");
  int G;
  const int rv = validate_plan(&rp->plan, &G);
  if (rv) return rv;
  if (rp->num_waypoints < 0) return fail(F110QP_ERR_INVALID, "num_waypoints < 0");
  K->G = G;
  K->T = rp->plan.steer_discrete + 1;
  K->P = rp->plan.traj_discrete;
  K->discrete = rp->plan.discrete;
  K->dilation = rp->plan.dilation;
  K->lookahead = rp->plan.lookahead;
  return F110QP_OK;
}

// The world of f110qp_cast_scans_dev, f110qp_clearance_dev and the world rollouts, checked; with sc's
// geometry (sc null: none) into *P.
static int world_params(const f110qp_scan_config* sc, const f110qp_world_config* wc, int batch,
                        const void* circles, f110qp::CastParams* P) {
  if (!wc) return fail(F110QP_ERR_INVALID, "world config is NULL");
  if (wc->num_circles < 0) return fail(F110QP_ERR_INVALID, "num_circles < 0");
  if (!std::isfinite(wc->lidar_offset)) return fail(F110QP_ERR_INVALID, "lidar_offset must be finite");
  if (!(wc->max_range > 0.0) || !std::isfinite(wc->max_range))
    return fail(F110QP_ERR_INVALID, "max_range must be positive and finite");
  if (wc->world_rows != 1 && wc->world_rows != batch)
    return fail(F110QP_ERR_INVALID, "world_rows must be 1 or batch");
  if (wc->num_circles > 0 && !circles) return fail(F110QP_ERR_INVALID, "num_circles > 0 needs the circles");
  if (sc) {
    P->nr = sc->num_ranges;
    P->angle_min = sc->angle_min;
    P->angle_inc = sc->angle_increment;
  }
  P->C = wc->num_circles;
  P->world_rows = wc->world_rows;
  P->lidar_offset = wc->lidar_offset;
  P->max_range = wc->max_range;
  return F110QP_OK;
}

// The races of f110qp_cast_scans_race_dev and the race rollouts, checked, into *Q.
static int race_params(const f110qp_race_config* race, int batch, int num_circles, f110qp::RaceParams* Q) {
  if (!race) return fail(F110QP_ERR_INVALID, "race config is NULL");
  if (race->group_size < 1) return fail(F110QP_ERR_INVALID, "group_size < 1");
  if (batch % race->group_size != 0) return fail(F110QP_ERR_INVALID, "batch must be a multiple of group_size");
  if (!(race->car_radius > 0.0) || !std::isfinite(race->car_radius))
    return fail(F110QP_ERR_INVALID, "car_radius must be positive and finite");
  if (!std::isfinite(race->center_offset)) return fail(F110QP_ERR_INVALID, "center_offset must be finite");
  if ((long long)num_circles + race->group_size - 1 > 0x7fffffffll)
    return fail(F110QP_ERR_INVALID, "num_circles + group_size - 1 does not fit an int");
  Q->G = race->group_size;
  Q->car_radius = race->car_radius;
  Q->center_offset = race->center_offset;
  return F110QP_OK;
}

// The contact config of f110qp_rollout_contact[_dev], checked.
static int contact_params(const f110qp_contact_config* cc) {
  if (!cc) return fail(F110QP_ERR_INVALID, "contact config is NULL");
  if (cc->stop_on_contact != 0 && cc->stop_on_contact != 1)
    return fail(F110QP_ERR_INVALID, "stop_on_contact must be 0 or 1");
  if (!std::isfinite(cc->margin)) return fail(F110QP_ERR_INVALID, "margin must be finite");
  return F110QP_OK;
}

// The rectangular body of f110qp_clearance_body_dev, f110qp_cast_scans_body_dev and f110qp_rollout_body[_dev],
// checked, into *H.
static int body_params(const f110qp_body_config* body, f110qp::BodyParams* H) {
  if (!body) return fail(F110QP_ERR_INVALID, "body config is NULL");
  if (!(body->half_length > 0.0) || !std::isfinite(body->half_length))
    return fail(F110QP_ERR_INVALID, "half_length must be positive and finite");
  if (!(body->half_width > 0.0) || !std::isfinite(body->half_width))
    return fail(F110QP_ERR_INVALID, "half_width must be positive and finite");
  H->hl = body->half_length;
  H->hw = body->half_width;
  return F110QP_OK;
}

// The straight walls of f110qp_cast_scans_walls_dev, f110qp_clearance_walls_dev and f110qp_rollout_walls[_dev],
// checked, into *Wl. obstacles: num_circles + group_size - 1, which race_params has checked to fit an int.
static int wall_params(const f110qp_walls_config* walls, int batch, long long obstacles, const void* segments,
                       f110qp::WallParams* Wl) {
  if (!walls) return fail(F110QP_ERR_INVALID, "walls config is NULL");
  if (walls->num_segments < 0) return fail(F110QP_ERR_INVALID, "num_segments < 0");
  if (walls->wall_rows != 1 && walls->wall_rows != batch)
    return fail(F110QP_ERR_INVALID, "wall_rows must be 1 or batch");
  if (walls->num_segments > 0 && !segments) return fail(F110QP_ERR_INVALID, "num_segments > 0 needs the segments");
  if (obstacles + 1 + walls->num_segments > 0x7fffffffll)
    return fail(F110QP_ERR_INVALID, "num_circles + group_size + num_segments does not fit an int");
  Wl->S = walls->num_segments;
  Wl->wall_rows = walls->wall_rows;
  return F110QP_OK;
}

// The refresh config of f110qp_rollout_refresh[_dev], checked, its period into *every.
static int refresh_params(const f110qp_refresh_config* rf, int* every) {
  if (!rf) return fail(F110QP_ERR_INVALID, "refresh config is NULL");
  if (rf->every < 0) return fail(F110QP_ERR_INVALID, "every must be >= 0");
  *every = rf->every;
  return F110QP_OK;
}

// The noise config of f110qp_cast_scans_noisy_dev and f110qp_rollout_noisy[_dev], checked, into *Z (rule Z2's
// drop24 taken here, once per call; Z->tick is the caller's).
static int noise_params(const f110qp_noise_config* noise, int batch, f110qp::NoiseParams* Z) {
  if (!noise) return fail(F110QP_ERR_INVALID, "noise config is NULL");
  if (!(noise->sigma_abs >= 0.0) || !std::isfinite(noise->sigma_abs) || !(noise->sigma_rel >= 0.0) ||
      !std::isfinite(noise->sigma_rel))
    return fail(F110QP_ERR_INVALID, "sigma_abs and sigma_rel must be >= 0 and finite");
  if (!(noise->dropout >= 0.0 && noise->dropout <= 1.0)) return fail(F110QP_ERR_INVALID, "dropout must be in [0, 1]");
  if (noise->car_base < 0) return fail(F110QP_ERR_INVALID, "car_base < 0");
  if (batch > 0 && noise->car_base > 0x7fffffffffffffffll - batch)
    return fail(F110QP_ERR_INVALID, "car_base + batch does not fit a long long");
  Z->seed = noise->seed;
  Z->car_base = (unsigned long long)noise->car_base;
  Z->sigma_abs = noise->sigma_abs;
  Z->sigma_rel = noise->sigma_rel;
  Z->drop24 = (unsigned)std::floor(noise->dropout * 16777216.0);
  Z->tick = 0;
  return F110QP_OK;
}

// The scan geometry of the re-planning kernels' argument records (ReplanStart, ReplanStep).
template <typename S>
static void scan_geometry(S* s, const f110qp_scan_config& sc) {
  s->nr = sc.num_ranges;
  s->angle_min = sc.angle_min;
  s->angle_inc = sc.angle_increment;
}

// ---- one rollout call: its configs, its checks, where it runs ----------------------------------------

// The family of a rollout call, in the order each was built on the one before: from kScan a scan
// config is read, from kReplan the loop re-plans, in kWorld the scans are cast (so neither `ranges`
// nor sc->scan_rows is read): every world family, told apart by its WorldRow below.
enum Family { kPlain, kScan, kReplan, kWorld };

// The world families, one row each, in the order each was built on the one before: the world its casts and
// clearances see, whether its rollout reads cc (every row's clearance is recorded) and rf (the scan MPC holds is
// refreshed), and what a failed launch of the cast and of the clearance entry point of its name says (null: the
// family has no such entry point). world: the circles; race: the race-mates in every cast; contact: race with cc;
// body: rectangular bodies in every cast and clearance; walls: straight segments next to the circles; refresh:
// walls with rf; noisy: rules Z1 to Z3 on every scan; grid: a raster map under every cast and clearance; field: the
// grid row with rule F1 on the map's distance field in every cast (its clearance is the grid's).
struct WorldRow {
  f110qp::WorldFamily world;
  bool cc, rf;
  const char* cast_launch;
  const char* clearance_launch;
  bool field = false;
};
namespace row {
constexpr WorldRow world{f110qp::WORLD_CIRCLES, false, false, "scan cast launch", nullptr};
constexpr WorldRow race{f110qp::WORLD_RACE, false, false, "race scan cast launch", "clearance launch"};
constexpr WorldRow contact{f110qp::WORLD_RACE, true, false, nullptr, nullptr};
constexpr WorldRow body{f110qp::WORLD_BODY, true, false, "body scan cast launch", "body clearance launch"};
constexpr WorldRow walls{f110qp::WORLD_WALLS, true, false, "walls scan cast launch", "walls clearance launch"};
constexpr WorldRow refresh{f110qp::WORLD_WALLS, true, true, nullptr, nullptr};
constexpr WorldRow noisy{f110qp::WORLD_NOISY, true, true, "noisy scan cast launch", nullptr};
constexpr WorldRow grid{f110qp::WORLD_GRID, true, true, "grid scan cast launch", "grid clearance launch"};
constexpr WorldRow field{f110qp::WORLD_GRID, true, true, "field scan cast launch", nullptr, true};
}  // namespace row

// The configs of a rollout call as the caller gave them and, once check_args has passed, the
// kernels' parameters.
struct LoopCfg {
  Family fam;
  const f110qp_rollout_config* rc;
  const f110qp_scan_config* sc;
  const f110qp_replan_config* rp;
  f110qp::AdvanceParams ap;
  f110qp::PlanKParams K;
};

// A host-pointer call (staged through the context's stream, synchronous) or a device-pointer call
// enqueued on the caller's stream.
struct Where {
  bool host;
  hipStream_t stream;
};
static Where on_host() { return Where{true, nullptr}; }
static Where on_stream(void* stream) { return Where{false, (hipStream_t)stream}; }

// Argument checks of every f110qp_rollout*[_dev], all before any device call; sets io->N and io->T.
// hs: f110qp_rollout's held rows; ranges: the scans of the scan and re-planning rollouts; r: the
// re-planning families' arrays (null below kReplan).
static int check_args(f110qp_ctx* c, LoopCfg* cfg, RolloutIO* io, const float* hs, const float* ranges,
                      const ReplanIO* r) {
  if (!c) return fail(F110QP_ERR_INVALID, "ctx is NULL");
  int rv = rollout_params(cfg->rc, true, &cfg->ap);
  if (rv) return rv;
  const bool scans = cfg->fam == kScan || cfg->fam == kReplan;  // the call reads `ranges`
  if (cfg->fam != kPlain && (rv = check_scan_config(cfg->sc, scans, cfg->rc->ticks))) return rv;
  if (r) {
    if ((rv = replan_params(cfg->rp, &cfg->K))) return rv;
    if (c->cfg.horizon < 2) return fail(F110QP_ERR_INVALID, "the re-planning rollout needs horizon >= 2");
    if (c->kp.xr_stride != cfg->rp->plan.traj_discrete)
      return fail(F110QP_ERR_INVALID, "the context's x_ref_points must equal traj_discrete");
  }
  io->N = c->cfg.horizon;
  io->T = cfg->rc->ticks;
  if (io->B < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (io->B == 0) return F110QP_OK;
  if (!io->x_ref || !io->x_traj || !io->u_lin_traj || !io->u_applied || !io->status_traj)
    return fail(F110QP_ERR_INVALID, "x_ref/x_traj/u_lin_traj/u_applied/status_traj must be non-NULL");
  if (cfg->fam == kPlain && c->cfg.gap_mode == F110QP_GAP_ACTIVE && !hs)
    return fail(F110QP_ERR_INVALID, "gap_mode ACTIVE needs the halfspace array");
  if (r && (!r->have_path || !r->table || (cfg->rp->num_waypoints > 0 && !r->waypoints)))
    return fail(F110QP_ERR_INVALID, "have_path/table/waypoints must be non-NULL");
  if (scans && !ranges) return fail(F110QP_ERR_INVALID, "ranges must be non-NULL");
  if (io->B > (1 << 30) / 64 || (scans && (long long)cfg->sc->scan_rows * io->B > (1ll << 30)))
    return fail(F110QP_ERR_INVALID, "batch too large");
  return F110QP_OK;
}

// ---- the tick loops ----------------------------------------------------------------------------------

// What both tick loops size in front of the loop, so that the loop itself only launches.
struct LoopWork {
  float* wup = nullptr;  // one tick's u_plan | x_plan when the caller keeps neither (c->rplan)
  float* wxp = nullptr;
  f110qp::GapRecord* rec = nullptr;  // with rows: one gap record per scan (c->rgap)
  float* rows = nullptr;             // tick t's rows: rows + t * rstep (hs_traj, or one row set in c->rhs)
  size_t rstep = 0;
  int backend;
  f110qp::LaneWork lw;
  f110qp::LanePlan plan;  // of every tick's solve: the same batch and knobs
};

// rows: the loop computes gap rows from scan_rows x B scans, into hs_traj when the caller gave one.
static int loop_prologue(f110qp_ctx* c, const RolloutIO& io, bool rows, int scan_rows, float* hs_traj,
                         hipStream_t s, LoopWork* w) {
  const size_t B = (size_t)io.B;
  if (!aligned8(io.u_applied) || !aligned8(io.u_plan))
    return fail(F110QP_ERR_INVALID, "u_applied / u_plan must be 8-byte aligned");
  hipError_t e;
  if (!io.u_plan || !io.x_plan) {
    if ((e = c->rplan.ensure((io.n_up() + io.n_xp()) * sizeof(float))) != hipSuccess)
      return hip_fail(e, "hipMalloc rollout plan workspace");
    w->wup = (float*)c->rplan.p;
    w->wxp = w->wup + io.n_up();
  }
  if (rows) {
    if ((e = c->rgap.ensure((size_t)scan_rows * B * sizeof(f110qp::GapRecord))) != hipSuccess)
      return hip_fail(e, "hipMalloc gap records");
    w->rec = (f110qp::GapRecord*)c->rgap.p;
    w->rows = hs_traj;
    w->rstep = B * 6;
    if (!w->rows) {
      if ((e = c->rhs.ensure(B * 6 * sizeof(float))) != hipSuccess) return hip_fail(e, "hipMalloc half-space rows");
      w->rows = (float*)c->rhs.p;
      w->rstep = 0;
    }
  }
  return lane_work(c, io.B, s, &w->backend, &w->lw, &w->plan);
}

// The T ticks of a checked rollout on device pointers (per tick the launches of one _dbl solve call,
// then the plant step). hs: the held rows of f110qp_rollout.
// sl (f110qp_rollout_scan[_dev]): the half-spaces follow the car. One gap search and the rows of tick
// 0 in front of the loop; tick t's plant step is the fused one, which writes the rows of tick t + 1
// (the last tick's is the plain one: there is no row T).
static int rollout_ticks(f110qp_ctx* c, const LoopCfg& cfg, const RolloutIO& io, const float* hs, hipStream_t s,
                         const ScanLoop* sl) {
  const size_t B = (size_t)io.B, T = (size_t)io.T;
  LoopWork w;
  const int rc = loop_prologue(c, io, sl != nullptr, sl ? sl->sc->scan_rows : 0, sl ? sl->hs_traj : nullptr, s, &w);
  if (rc) return rc;
  const bool gap = c->cfg.gap_mode == F110QP_GAP_ACTIVE;
  const float* h = gap ? hs : nullptr;
  if (sl) {
    const f110qp_scan_config& k = *sl->sc;
    hipError_t e = f110qp::launch_gap_search(k.scan_rows * io.B, sl->ranges, k.num_ranges, k.angle_min,
                                             k.angle_increment, k.angle_max, k.ftg_thresh, k.divider, k.buffer,
                                             w.rec, s);
    if (e != hipSuccess) return hip_fail(e, "gap search launch");
    e = f110qp::launch_half_space_rows(io.B, k.num_ranges, k.angle_min, k.angle_increment, w.rec, io.x(0), w.rows, s);
    if (e != hipSuccess) return hip_fail(e, "half-space rows launch");
  }
  // the scan rollout's NaN rows mean a scan without a gap: non-finite data, F110QP_NUMERICAL
  f110qp::KParams kp = c->kp;
  if (sl) kp.hs_nan_numerical = 1;
  for (size_t t = 0; t < T; t++) {
    if (sl && gap) h = w.rows + t * w.rstep;
    float* u_t = io.up(t, w.wup);
    f110qp::ObjOut oo;
    oo.cost = io.cost(t);
    const f110qp::SolveIO<double> sio{io.B, io.x(t), io.ul(t), io.x_ref, h, u_t, io.xp(t, w.wxp), io.st(t), io.it(t)};
    hipError_t e = f110qp::launch_solve(kp, sio, f110qp::WarmState(), w.backend, w.lw, w.plan, oo, s);
    if (e != hipSuccess) return hip_fail(e, "rollout solve launch");
    if (sl && t + 1 < T)
      e = f110qp::launch_advance_scan(cfg.ap, io.B, io.N, io.x(t), u_t, io.st(t), sl->sc->num_ranges,
                                      sl->sc->angle_min, sl->sc->angle_increment,
                                      w.rec + (sl->sc->scan_rows == 1 ? 0 : (t + 1) * B), io.x(t + 1), io.ul(t + 1),
                                      io.ua(t), w.rows + (t + 1) * w.rstep, s);
    else
      e = f110qp::launch_advance(cfg.ap, io.B, io.N, io.x(t), u_t, io.st(t), io.x(t + 1), io.ul(t + 1), io.ua(t), s);
    if (e != hipSuccess) return hip_fail(e, "plant step launch");
  }
  return F110QP_OK;
}

// f110qp_rollout_world[_dev] and the families on top of it: tick t's scans are cast at tick t's pose in the
// world w instead of read from `ranges`; from WORLD_RACE every cast also sees the race-mates at the poses it
// casts from, and the clearances are those of the same world.
struct WorldLoop {
  f110qp::World w;     // checked (world_of); its circles and segments device pointers in the tick loop; the
                       // loop gives every cast its tick (rule Z3, read by WORLD_NOISY alone)
  float* ranges_traj;  // [T][B][num_ranges] or null: one row set in the context, listed cars only
  int every;  // f110qp_rollout_refresh[_dev]: the refresh period of MPC's scan, 0 (every other family): never
};

// f110qp_rollout_contact[_dev]: the race rollout with one clearance launch per row of x_traj, which also
// keeps crash_tick; stop: the plant step is the parking one. The arrays are device pointers here.
struct ContactLoop {
  bool stop;
  double margin;
  ContactIO io;
};

// The T ticks of a checked re-planning rollout on device pointers. Every workspace is sized in front
// of the loop; the loop only launches: the listed plan, the launches of one _dbl solve call, the
// state machine with the plant step.
// wl (the world rollout; r.ranges is not read): per tick the cast in front of the listed plan, on that
// plan's list or, with ranges_traj, for all cars into row t. The gap records are those of one all-cars
// cast at row 0 in front of the loop, held as at scan_rows = 1. With wl->every = K >= 1 and rows computed, a
// tick t >= 1 with t % K == 0 casts for all cars and one refresh launch behind the cast replaces the held
// records and tick t's rows by those of row t's scans at row t's poses.
// cl (the contact rollout, with wl): one clearance launch on row 0 behind the start kernel and one on row
// t + 1 behind tick t's plant step, each marking crash_tick; with cl->stop the plant step parks.
static int replan_ticks(f110qp_ctx* c, const LoopCfg& cfg, const RolloutIO& io, const ReplanIO& r, hipStream_t s,
                        const WorldLoop* wl, const ContactLoop* cl = nullptr) {
  const f110qp_scan_config& sc = *cfg.sc;
  const f110qp_replan_config& rp = *cfg.rp;
  const ReplanTraj& tr = r.tr;
  const size_t B = (size_t)io.B, T = (size_t)io.T, nr = (size_t)sc.num_ranges;
  const int scan_rows = wl ? 1 : sc.scan_rows;
  const bool gap = c->cfg.gap_mode == F110QP_GAP_ACTIVE;
  const bool rows_on = gap || tr.hs;  // as f110qp_rollout_scan_dev: nothing reads them otherwise
  LoopWork w;
  const int rc = loop_prologue(c, io, rows_on, scan_rows, tr.hs, s, &w);
  if (rc) return rc;
  hipError_t e;
  float* wscan = nullptr;  // the world rollout's one row set
  if (wl && !wl->ranges_traj) {
    if ((e = c->rscan.ensure(B * nr * sizeof(float))) != hipSuccess) return hip_fail(e, "hipMalloc scan rows");
    wscan = (float*)c->rscan.p;
  }
  auto scan_row = [&](size_t t) { return wscan ? wscan : wl->ranges_traj + t * B * nr; };
  // tick t's cast at row t's poses, for all cars (list and count null) or the listed ones
  auto cast_row = [&](size_t t, const int* cars, const int* n) {
    f110qp::World ww = wl->w;
    ww.Z.tick = (int)t;
    return f110qp::launch_cast_scans(ww, io.B, cars, n, io.x(t), scan_row(t), s);
  };
  // ReplanWork, the state of the loop in c->rstate: [pose B x 4 doubles unless pose_traj] [u_held B x N
  // float2] then ints: [held_len B | held_idx B | plan_count T + 1] (zeroed by the one memset), [list B],
  // [kind 2 B unless kind_traj], [plan_status B], [best_traj B], [best_global B] unless given
  const size_t o_held = tr.pose ? 0 : B * 4 * 8, o_int = o_held + io.n_up() * 4;
  const size_t n_zero = 2 * B + T + 1;
  size_t n_int = n_zero + B;
  const size_t i_kind = n_int;
  n_int += tr.kind ? 0 : 2 * B;
  const size_t i_ps = n_int;
  n_int += tr.plan_status ? 0 : B;
  const size_t i_bt = n_int;
  n_int += tr.best_traj ? 0 : B;
  const size_t i_bg = n_int;
  n_int += tr.best_global ? 0 : B;
  if ((e = c->rstate.ensure(o_int + n_int * 4)) != hipSuccess) return hip_fail(e, "hipMalloc re-planning state");
  char* ws = (char*)c->rstate.p;
  double* wpose = (double*)ws;
  float* held = (float*)(ws + o_held);
  int* wi = (int*)(ws + o_int);
  int* held_len = wi;
  int* held_idx = wi + B;
  int* count = wi + 2 * B;
  int* list = wi + n_zero;
  if ((e = hipMemsetAsync(wi, 0, n_zero * sizeof(int), s)) != hipSuccess) return hip_fail(e, "hipMemsetAsync plan counters");
  const float* ranges = r.ranges;
  if (rows_on) {
    if (wl) {  // MPC's scan is the first one (src/project.cpp:45-49): every car's, at row 0
      ranges = scan_row(0);
      if ((e = cast_row(0, nullptr, nullptr)) != hipSuccess) return hip_fail(e, "scan cast launch");
    }
    e = f110qp::launch_gap_search(scan_rows * io.B, ranges, sc.num_ranges, sc.angle_min, sc.angle_increment,
                                  sc.angle_max, sc.ftg_thresh, sc.divider, sc.buffer, w.rec, s);
    if (e != hipSuccess) return hip_fail(e, "gap search launch");
  }
  auto kind_row = [&](size_t t) { return tr.kind ? tr.kind + t * B : wi + i_kind + (t & 1) * B; };
  auto pose_row = [&](size_t t) { return tr.pose ? tr.pose + t * B * 4 : wpose; };
  {
    f110qp::ReplanStart st{};
    st.x = io.x(0);
    st.have_path = r.have_path;
    st.x_ref = io.x_ref;
    st.P = cfg.K.P;
    st.replan_dist = rp.replan_dist;
    st.pose = pose_row(0);
    st.kind = kind_row(0);
    st.list = list;
    st.count = count;
    st.gap = w.rec;
    st.hs = w.rows;
    scan_geometry(&st, sc);
    if ((e = f110qp::launch_replan_start(io.B, st, s)) != hipSuccess) return hip_fail(e, "re-planning start launch");
  }
  // row t's clearances into clear_traj / nearest_traj, crash_tick started (row 0) or kept up
  auto clearance_row = [&](size_t t) {
    const f110qp::ContactMark mk{cl->io.crash_tick, (int)t, t == 0, cl->margin};
    return f110qp::launch_clearance(wl->w, io.B, 1, io.x(t), cl->io.clear_traj + t * B,
                                    cl->io.nearest_traj ? cl->io.nearest_traj + t * B : nullptr, mk, s);
  };
  if (cl && (e = clearance_row(0)) != hipSuccess) return hip_fail(e, "clearance launch");
  for (size_t t = 0; t < T; t++) {
    int* ps_t = tr.plan_status ? tr.plan_status + t * B : wi + i_ps;
    const float* scan_t = wl ? scan_row(t) : ranges + (scan_rows == 1 ? 0 : t * B * nr);
    if (wl) {
      const bool refresh = rows_on && wl->every > 0 && t > 0 && t % (size_t)wl->every == 0;
      const bool all = wl->ranges_traj != nullptr || refresh;
      e = cast_row(t, all ? nullptr : list, all ? nullptr : count + t);
      if (e != hipSuccess) return hip_fail(e, "scan cast launch");
      if (refresh) {  // MPC's scan becomes tick t's: new records, and the rows this tick's solve reads
        e = f110qp::launch_gap_refresh(io.B, scan_row(t), sc.num_ranges, sc.angle_min, sc.angle_increment,
                                       sc.angle_max, sc.ftg_thresh, sc.divider, sc.buffer, io.x(t), w.rec,
                                       w.rows + t * w.rstep, s);
        if (e != hipSuccess) return hip_fail(e, "gap refresh launch");
      }
    }
    e = f110qp::launch_plan_listed(cfg.K, io.B, list, count + t, pose_row(t), scan_t, sc.num_ranges, sc.angle_min,
                                   sc.angle_increment, sc.angle_max, r.table, r.waypoints, rp.num_waypoints,
                                   tr.best_global ? tr.best_global + t * B : wi + i_bg,
                                   tr.best_traj ? tr.best_traj + t * B : wi + i_bt, io.x_ref, ps_t, s);
    if (e != hipSuccess) return hip_fail(e, "listed plan launch");
    const float* h = gap ? w.rows + t * w.rstep : nullptr;
    float* u_t = io.up(t, w.wup);
    f110qp::ObjOut oo;
    oo.cost = io.cost(t);
    const f110qp::SolveIO<double> sio{io.B, io.x(t), io.ul(t), io.x_ref, h, u_t, io.xp(t, w.wxp), io.st(t), io.it(t)};
    e = f110qp::launch_solve(c->kp, sio, f110qp::WarmState(), w.backend, w.lw, w.plan, oo, s);
    if (e != hipSuccess) return hip_fail(e, "rollout solve launch");
    const bool last = t + 1 == T;  // no tick T: neither its kind and list nor its rows
    f110qp::ReplanStep S{};
    S.x = io.x(t);
    S.kind = kind_row(t);
    S.u_plan = u_t;
    S.status = io.st(t);
    S.plan_status = ps_t;
    S.x_ref = io.x_ref;
    S.P = cfg.K.P;
    S.replan_dist = rp.replan_dist;
    S.u_held = held;
    S.held_len = held_len;
    S.held_idx = held_idx;
    S.have_path = r.have_path;
    S.x_next = io.x(t + 1);
    S.u_lin_next = io.ul(t + 1);
    S.u_applied = io.ua(t);
    S.pose_next = pose_row(t + 1);
    S.kind_next = last ? nullptr : kind_row(t + 1);
    S.next_list = last ? nullptr : list;
    S.next_count = last ? nullptr : count + t + 1;
    S.gap = rows_on && !last ? w.rec + (scan_rows == 1 ? 0 : (t + 1) * B) : nullptr;
    S.hs_next = rows_on && !last ? w.rows + (t + 1) * w.rstep : nullptr;
    scan_geometry(&S, sc);
    if (cl && cl->stop) {
      S.crash_tick = cl->io.crash_tick;
      S.u_lin = io.ul(t);
      S.pose = pose_row(t);
      e = f110qp::launch_advance_replan_park(cfg.ap, io.B, io.N, S, s);
    } else {
      e = f110qp::launch_advance_replan(cfg.ap, io.B, io.N, S, s);
    }
    if (e != hipSuccess) return hip_fail(e, "plant step launch");
    if (cl && (e = clearance_row(t + 1)) != hipSuccess) return hip_fail(e, "clearance launch");
  }
  return F110QP_OK;
}

// ---- the host-pointer calls: the staging table through c->rdev ----------------------------------------

static int host_stream(f110qp_ctx* c, hipStream_t* s) {
  hipError_t e = hipSetDevice(c->cfg.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  if (!c->stream && (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
    return hip_fail(e, "hipStreamCreate");
  *s = c->stream;
  return F110QP_OK;
}

// Lays the declared fields out in c->rdev, binds their device addresses and uploads the inputs.
static int stage_in(f110qp_ctx* c, const stage::Layout& L, hipStream_t s) {
  hipError_t e = c->rdev.ensure(L.total);
  if (e != hipSuccess) return hip_fail(e, "hipMalloc rollout staging");
  L.bind(c->rdev.p);
  for (int i = 0; i < L.n; i++) {
    const stage::Field& f = L.f[i];
    if (f.h2d_bytes() &&
        (e = hipMemcpyAsync((char*)c->rdev.p + f.offset, f.host, f.h2d_bytes(), hipMemcpyHostToDevice, s)))
      return hip_fail(e, "hipMemcpyAsync H2D");
  }
  return F110QP_OK;
}

// After the loop: every output back to the caller's arrays (rows 1..T of the trajectories: row 0 is
// the caller's), then the call's one synchronisation.
static int stage_out(f110qp_ctx* c, const stage::Layout& L, hipStream_t s) {
  hipError_t e;
  for (int i = 0; i < L.n; i++) {
    const stage::Field& f = L.f[i];
    if (f.d2h_bytes() && (e = hipMemcpyAsync((char*)f.host + f.d2h_begin(), (char*)c->rdev.p + f.offset + f.d2h_begin(),
                                             f.d2h_bytes(), hipMemcpyDeviceToHost, s)))
      return hip_fail(e, "hipMemcpyAsync D2H");
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
  return F110QP_OK;
}

// f110qp_rollout (sl null: hs [B][6] held) and f110qp_rollout_scan (sl) on checked host pointers.
static int rollout_host(f110qp_ctx* c, const LoopCfg& cfg, const RolloutIO& io, const float* hs, const ScanLoop* sl) {
  hipStream_t s;
  int rv = host_stream(c, &s);
  if (rv) return rv;
  const bool held = c->cfg.gap_mode == F110QP_GAP_ACTIVE && !sl;
  stage::Layout L;
  RolloutIO d;
  ScanLoop dsl;
  const float* d_hs;
  stage::rollout_fields(L, io, &d, (size_t)c->kp.xr_stride, held ? hs : nullptr, &d_hs, sl, &dsl);
  if ((rv = stage_in(c, L, s))) return rv;
  if ((rv = rollout_ticks(c, cfg, d, d_hs, s, sl ? &dsl : nullptr))) return rv;
  return stage_out(c, L, s);
}

// f110qp_rollout_replan (wl null), f110qp_rollout_world / _race (wl, its circles and ranges_traj the
// host's) and f110qp_rollout_contact (wl and cl, its three records the host's) on checked host pointers.
static int replan_host(f110qp_ctx* c, const LoopCfg& cfg, const RolloutIO& io, const ReplanIO& r, const WorldLoop* wl,
                       const ContactLoop* cl = nullptr) {
  hipStream_t s;
  int rv = host_stream(c, &s);
  if (rv) return rv;
  stage::Layout L;
  RolloutIO d;
  ReplanIO dr;
  WorldIO hw{}, dw{};
  ContactLoop dcl{};
  if (wl)
    hw = WorldIO{wl->w.circles, (size_t)wl->w.P.world_rows * (size_t)wl->w.P.C * 3 * 8, wl->ranges_traj, wl->w.segments,
                 wl->w.family >= f110qp::WORLD_WALLS ? (size_t)wl->w.Wl.wall_rows * (size_t)wl->w.Wl.S * 4 * 8 : 0,
                 wl->w.grid, wl->w.family == f110qp::WORLD_GRID ? (size_t)wl->w.Gr.W * (size_t)wl->w.Gr.H : 0};
  // f110qp_rollout_field: d2 and the transform's scratch, [H][W] int each, device only
  if (wl && wl->w.field) hw.field_bytes = 2 * hw.grid_bytes * sizeof(int);
  if (cl) dcl = *cl;
  stage::replan_fields(L, io, &d, r, &dr, *cfg.sc, (size_t)cfg.K.T, (size_t)cfg.K.P, (size_t)cfg.rp->num_waypoints,
                       wl ? &hw : nullptr, &dw, cl ? &cl->io : nullptr, &dcl.io);
  if ((rv = stage_in(c, L, s))) return rv;
  WorldLoop dwl{};
  if (wl) {
    dwl = *wl;
    dwl.w.circles = dw.circles;
    dwl.ranges_traj = dw.ranges_traj;
    dwl.w.segments = dw.segments;
    dwl.w.grid = dw.grid;
    if (dw.field) {  // the map's field, once, in front of the first tick
      dwl.w.d2 = dw.field;
      const hipError_t e = f110qp::launch_grid_distance(dwl.w.Gr.W, dwl.w.Gr.H, dw.grid, dw.field, nullptr,
                                                        dw.field + hw.grid_bytes, s);
      if (e != hipSuccess) return hip_fail(e, "grid distance launch");
    }
  }
  if ((rv = replan_ticks(c, cfg, d, dr, s, wl ? &dwl : nullptr, cl ? &dcl : nullptr))) return rv;
  return stage_out(c, L, s);
}

// ---- the entry points' shared bodies -------------------------------------------------------------------

// f110qp_rollout[_dev] (kPlain, hs) and f110qp_rollout_scan[_dev] (cfg.sc, ranges, hst).
static int rollout_call(f110qp_ctx* c, LoopCfg cfg, RolloutIO io, const float* hs, const float* ranges, float* hst,
                        Where w) {
  const int rv = check_args(c, &cfg, &io, hs, ranges, nullptr);
  if (rv || io.B == 0) return rv;
  // gap rows inactive and no rows asked for: nothing reads them, f110qp_rollout_dev's launches
  const ScanLoop sl{cfg.sc, ranges, hst};
  const bool rows = cfg.fam == kScan && (c->cfg.gap_mode == F110QP_GAP_ACTIVE || hst);
  return w.host ? rollout_host(c, cfg, io, hs, rows ? &sl : nullptr)
                : rollout_ticks(c, cfg, io, hs, w.stream, rows ? &sl : nullptr);
}

static int replan_call(f110qp_ctx* c, LoopCfg cfg, RolloutIO io, const ReplanIO& r, Where w) {
  const int rv = check_args(c, &cfg, &io, nullptr, r.ranges, &r);
  if (rv || io.B == 0) return rv;
  return w.host ? replan_host(c, cfg, io, r, nullptr) : replan_ticks(c, cfg, io, r, w.stream, nullptr);
}

// The configs of a world-family call as the caller gave them, each set by its name; a call reads those its family
// takes (wc: all, race: from row::race, cc and rf: the rollouts of the rows that say so, body: from row::body, walls:
// from row::walls, noise: the casts and rollouts from row::noisy, grid: row::grid) and leaves the others null.
struct WorldCfgs {
  const f110qp_world_config* wc = nullptr;
  const f110qp_race_config* race = nullptr;
  const f110qp_contact_config* cc = nullptr;
  const f110qp_body_config* body = nullptr;
  const f110qp_walls_config* walls = nullptr;
  const f110qp_refresh_config* rf = nullptr;
  const f110qp_noise_config* noise = nullptr;
  const f110qp_grid_config* grid = nullptr;
  WorldCfgs& Race(const f110qp_race_config* v) { return race = v, *this; }
  WorldCfgs& Contact(const f110qp_contact_config* v) { return cc = v, *this; }
  WorldCfgs& Body(const f110qp_body_config* v) { return body = v, *this; }
  WorldCfgs& Walls(const f110qp_walls_config* v) { return walls = v, *this; }
  WorldCfgs& Refresh(const f110qp_refresh_config* v) { return rf = v, *this; }
  WorldCfgs& Noise(const f110qp_noise_config* v) { return noise = v, *this; }
  WorldCfgs& Grid(const f110qp_grid_config* v) { return grid = v, *this; }
};

// The world of a cast, a clearance or a world rollout, checked in the one order all of them share, into *w;
// contact: the call also reads k.cc, whose turn is behind the race's. sc null: no scan geometry (clearances).
// The clearances (sc null) never read the noise: theirs is not checked. field: the casts read d2 by rule F1, whose
// two rules come behind the grid's; own_d2: the call computes d2 itself (f110qp_rollout_field) and takes none.
static int world_of(f110qp::WorldFamily fam, const f110qp_scan_config* sc, const WorldCfgs& k, bool contact, int batch,
                    const double* circles, const double* segments, f110qp::World* w,
                    const unsigned char* grid = nullptr, bool field = false, const int* d2 = nullptr,
                    bool own_d2 = false) {
  int rv = world_params(sc, k.wc, batch, circles, &w->P);
  if (rv) return rv;
  if (fam >= f110qp::WORLD_RACE && (rv = race_params(k.race, batch, k.wc->num_circles, &w->Q))) return rv;
  if (contact && (rv = contact_params(k.cc))) return rv;
  if (fam >= f110qp::WORLD_BODY && (rv = body_params(k.body, &w->H))) return rv;
  const bool walls = fam >= f110qp::WORLD_WALLS;
  if (walls && (rv = wall_params(k.walls, batch, (long long)k.wc->num_circles + k.race->group_size - 1, segments,
                                 &w->Wl)))
    return rv;
  if (fam >= f110qp::WORLD_NOISY && sc && (rv = noise_params(k.noise, batch, &w->Z))) return rv;
  if (fam == f110qp::WORLD_GRID &&
      (rv = grid_params(k.grid, (long long)k.wc->num_circles + k.race->group_size + k.walls->num_segments, grid,
                        &w->Gr)))
    return rv;
  if (field) {
    if (k.grid->width > F110QP_FIELD_MAX_SIDE || k.grid->height > F110QP_FIELD_MAX_SIDE)
      return fail(F110QP_ERR_INVALID, "grid width and height must be <= 32768 for the distance field");
    if (!own_d2 && (long long)k.grid->width * k.grid->height > 0 && !d2)
      return fail(F110QP_ERR_INVALID, "width * height > 0 needs d2");
  }
  w->field = field;
  w->d2 = field ? d2 : nullptr;
  w->visits = nullptr;
  w->grid = fam == f110qp::WORLD_GRID ? grid : nullptr;
  w->family = fam;
  w->circles = circles;
  w->segments = walls ? segments : nullptr;
  return F110QP_OK;
}

// The arrays of a world-family rollout call (a.k: the rows with cc).
struct WorldArrays {
  RolloutIO io;
  ReplanIO r;
  ContactIO k;
};
static WorldArrays world_arrays(int batch, const double* table, const double* wp, double* xr, int* have, double* xt,
                                double* ult, float* ua, int* stt, int* itt, double* cot, float* up, float* xp,
                                float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset, double* clt = nullptr,
                                int* nrt = nullptr, int* crash = nullptr) {
  return WorldArrays{RolloutIO{batch, 0, 0, xr, xt, ult, ua, stt, itt, cot, up, xp},
                     ReplanIO{table, wp, have, nullptr, {hst, kt, pst, btt, bgt, poset}}, ContactIO{clt, nrt, crash}};
}

// f110qp_rollout_<family>[_dev] of the eight world families: the family's row f and the configs k it reads.
static int world_call(f110qp_ctx* c, const WorldRow& f, LoopCfg cfg, const WorldCfgs& k, WorldArrays a,
                      const double* circles, const double* segments, float* rgt, Where w,
                      const unsigned char* grid = nullptr, const int* d2 = nullptr) {
  WorldLoop wl{};
  int rv = check_args(c, &cfg, &a.io, nullptr, nullptr, &a.r);
  if (rv) return rv;
  const bool contact = f.cc;
  if ((rv = world_of(f.world, cfg.sc, k, contact, a.io.B, circles, segments, &wl.w, grid, f.field, d2, w.host)))
    return rv;
  if (f.rf && (rv = refresh_params(k.rf, &wl.every))) return rv;
  if (a.io.B == 0) return F110QP_OK;
  if (contact && (!a.k.clear_traj || !a.k.crash_tick))
    return fail(F110QP_ERR_INVALID, "clear_traj/crash_tick must be non-NULL");
  wl.ranges_traj = rgt;
  ContactLoop cl{};
  if (contact) cl = ContactLoop{k.cc->stop_on_contact == 1, k.cc->margin, a.k};
  const ContactLoop* clp = contact ? &cl : nullptr;
  return w.host ? replan_host(c, cfg, a.io, a.r, &wl, clp) : replan_ticks(c, cfg, a.io, a.r, w.stream, &wl, clp);
}

// f110qp_cast_scans[_race|_body|_walls|_noisy|_grid]_dev and f110qp_grid_cast_dev (row::field: d2 and visits) on the
// configs k their family reads; tick: rule Z3's t of the noisy and grid casts (0 elsewhere).
static int cast_call(const WorldRow& f, const f110qp_scan_config* sc, const WorldCfgs& k, int batch,
                     const int* list, const int* count, const double* x, const double* circles,
                     const double* segments, float* ranges, void* stream, int tick = 0,
                     const unsigned char* grid = nullptr, const int* d2 = nullptr, int* visits = nullptr) {
  int rv = check_scan_config(sc, false, 0);
  if (rv) return rv;
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  f110qp::World w{};
  if ((rv = world_of(f.world, sc, k, false, batch, circles, segments, &w, grid, f.field, d2))) return rv;
  w.visits = visits;
  if (tick < 0) return fail(F110QP_ERR_INVALID, "tick < 0");
  w.Z.tick = tick;
  if ((list != nullptr) != (count != nullptr))
    return fail(F110QP_ERR_INVALID, "list and count must be given together");
  if (batch == 0) return F110QP_OK;
  if (!x || !ranges) return fail(F110QP_ERR_INVALID, "x/ranges must be non-NULL");
  const hipError_t e = f110qp::launch_cast_scans(w, batch, list, count, x, ranges, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, f.cast_launch);
  return F110QP_OK;
}

// f110qp_clearance[_body|_walls|_grid]_dev on the configs k their family reads (a row with a clearance).
static int clearance_call(const WorldRow& f, const WorldCfgs& k, int batch, int rows, const double* x,
                          const double* circles, const double* segments, double* clearance, int* nearest,
                          void* stream, const unsigned char* grid = nullptr) {
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  f110qp::World w{};
  const int rv = world_of(f.world, nullptr, k, false, batch, circles, segments, &w, grid);
  if (rv) return rv;
  if (rows < 1) return fail(F110QP_ERR_INVALID, "rows must be >= 1");
  if (batch == 0) return F110QP_OK;
  if (!x || !clearance) return fail(F110QP_ERR_INVALID, "x/clearance must be non-NULL");
  if ((long long)rows * batch > (1ll << 30)) return fail(F110QP_ERR_INVALID, "rows x batch too large");
  const hipError_t e = f110qp::launch_clearance(w, batch, rows, x, clearance, nearest,
                                                f110qp::ContactMark{nullptr, 0, 0, 0.0}, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, f.clearance_launch);
  return F110QP_OK;
}

extern "C" {

// ---- closed loop on the device (f110qp_advance_dev, f110qp_rollout[_dev]) ------------------------

void f110qp_default_rollout_config(f110qp_rollout_config* rc) {
  if (!rc) return;
  std::memset(rc, 0, sizeof(*rc));
  rc->ticks = 1;
  rc->plant_dt = 0.01;    // params.yaml:13
  rc->car_length = 0.35;  // CAR_LENGTH, src/model.cpp:2
  rc->v_lin = 4.5;        // src/project.cpp:170
  rc->fail_u[0] = 0.5;    // Input(0.5, 0.0), src/project.cpp:215
  rc->fail_u[1] = 0.0;
}

int f110qp_advance_dev(const f110qp_rollout_config* rc, int batch, int horizon, const double* x,
                       const float* u_plan, const int* status, double* x_next, double* u_lin_next,
                       float* u_applied, void* stream) {
  f110qp::AdvanceParams ap;
  const int rv = rollout_params(rc, false, &ap);
  if (rv) return rv;
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (horizon < 1 || horizon > F110QP_MAX_HORIZON) return fail(F110QP_ERR_INVALID, "horizon must be in [1, 48]");
  if (batch == 0) return F110QP_OK;
  if (!x || !u_plan || !status || !x_next || !u_lin_next)
    return fail(F110QP_ERR_INVALID, "x/u_plan/status/x_next/u_lin_next must be non-NULL");
  if (x_next == x) return fail(F110QP_ERR_INVALID, "x_next must not alias x");
  if (!aligned8(u_plan) || !aligned8(u_applied))
    return fail(F110QP_ERR_INVALID, "u_plan / u_applied must be 8-byte aligned");
  const hipError_t e = f110qp::launch_advance(ap, batch, horizon, x, u_plan, status, x_next, u_lin_next,
                                              u_applied, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "plant step launch");
  return F110QP_OK;
}

int f110qp_rollout_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, int batch, const double* xr,
                       const float* hs, double* xt, double* ult, float* ua, int* stt, int* itt,
                       double* cot, float* up, float* xp, void* stream) {
  const RolloutIO io{batch, 0, 0, const_cast<double*>(xr), xt, ult, ua, stt, itt, cot, up, xp};
  return rollout_call(c, LoopCfg{kPlain, rc}, io, hs, nullptr, nullptr, on_stream(stream));
}

int f110qp_rollout(f110qp_ctx* c, const f110qp_rollout_config* rc, int batch, const double* xr,
                   const float* hs, double* xt, double* ult, float* ua, int* stt, int* itt,
                   double* cot, float* up, float* xp) {
  const RolloutIO io{batch, 0, 0, const_cast<double*>(xr), xt, ult, ua, stt, itt, cot, up, xp};
  return rollout_call(c, LoopCfg{kPlain, rc}, io, hs, nullptr, nullptr, on_host());
}

// ---- closed loop with gap rows from the scans (f110qp_rollout_scan[_dev] and its parts) --------------

void f110qp_default_scan_config(f110qp_scan_config* sc) {
  if (!sc) return;
  std::memset(sc, 0, sizeof(*sc));
  sc->ftg_thresh = 3.0f;  // the defaults of the half-space calls' bindings (params.yaml)
  sc->divider = 1.5f;
  sc->buffer = 3.0f;
  sc->scan_rows = 1;
}

int f110qp_gap_search_dev(const f110qp_scan_config* sc, int count, const float* ranges,
                          f110qp_gap_record* gap, void* stream) {
  const int rv = check_scan_config(sc, false, 0);
  if (rv) return rv;
  if (count < 0) return fail(F110QP_ERR_INVALID, "count < 0");
  if (count == 0) return F110QP_OK;
  if (!ranges || !gap) return fail(F110QP_ERR_INVALID, "ranges/gap_out must be non-NULL");
  const hipError_t e = f110qp::launch_gap_search(count, ranges, sc->num_ranges, sc->angle_min,
                                                 sc->angle_increment, sc->angle_max, sc->ftg_thresh, sc->divider,
                                                 sc->buffer, (f110qp::GapRecord*)gap, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "gap search launch");
  return F110QP_OK;
}

int f110qp_half_space_rows_dev(const f110qp_scan_config* sc, int batch, const f110qp_gap_record* gap,
                               const double* states, float* hs, void* stream) {
  const int rv = check_scan_config(sc, false, 0);
  if (rv) return rv;
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (batch == 0) return F110QP_OK;
  if (!gap || !states || !hs) return fail(F110QP_ERR_INVALID, "gap/states/hs_out must be non-NULL");
  const hipError_t e = f110qp::launch_half_space_rows(batch, sc->num_ranges, sc->angle_min, sc->angle_increment,
                                                      (const f110qp::GapRecord*)gap, states, hs,
                                                      (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "half-space rows launch");
  return F110QP_OK;
}

int f110qp_advance_scan_dev(const f110qp_rollout_config* rc, const f110qp_scan_config* sc, int batch,
                            int horizon, const double* x, const float* u_plan, const int* status,
                            const f110qp_gap_record* gap, double* x_next, double* u_lin_next,
                            float* u_applied, float* hs_next, void* stream) {
  f110qp::AdvanceParams ap;
  int rv = rollout_params(rc, false, &ap);
  if (rv) return rv;
  if ((rv = check_scan_config(sc, false, 0))) return rv;
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (horizon < 1 || horizon > F110QP_MAX_HORIZON) return fail(F110QP_ERR_INVALID, "horizon must be in [1, 48]");
  if (batch == 0) return F110QP_OK;
  if (!x || !u_plan || !status || !x_next || !u_lin_next)
    return fail(F110QP_ERR_INVALID, "x/u_plan/status/x_next/u_lin_next must be non-NULL");
  if (!gap || !hs_next) return fail(F110QP_ERR_INVALID, "gap/hs_next must be non-NULL");
  if (x_next == x) return fail(F110QP_ERR_INVALID, "x_next must not alias x");
  if (!aligned8(u_plan) || !aligned8(u_applied))
    return fail(F110QP_ERR_INVALID, "u_plan / u_applied must be 8-byte aligned");
  const hipError_t e = f110qp::launch_advance_scan(ap, batch, horizon, x, u_plan, status, sc->num_ranges,
                                                   sc->angle_min, sc->angle_increment,
                                                   (const f110qp::GapRecord*)gap, x_next, u_lin_next, u_applied,
                                                   hs_next, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "plant step launch");
  return F110QP_OK;
}

int f110qp_rollout_scan_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                            int batch, const double* xr, const float* ranges, double* xt, double* ult,
                            float* ua, int* stt, int* itt, double* cot, float* up, float* xp, float* hst,
                            void* stream) {
  const RolloutIO io{batch, 0, 0, const_cast<double*>(xr), xt, ult, ua, stt, itt, cot, up, xp};
  return rollout_call(c, LoopCfg{kScan, rc, sc}, io, nullptr, ranges, hst, on_stream(stream));
}

int f110qp_rollout_scan(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                        int batch, const double* xr, const float* ranges, double* xt, double* ult, float* ua,
                        int* stt, int* itt, double* cot, float* up, float* xp, float* hst) {
  const RolloutIO io{batch, 0, 0, const_cast<double*>(xr), xt, ult, ua, stt, itt, cot, up, xp};
  return rollout_call(c, LoopCfg{kScan, rc, sc}, io, nullptr, ranges, hst, on_host());
}

// ---- closed loop with re-planning (f110qp_rollout_replan[_dev] and its parts) ----------------------

void f110qp_default_replan_config(f110qp_replan_config* rp) {
  if (!rp) return;
  std::memset(rp, 0, sizeof(*rp));
  rp->replan_dist = 1.98;  // src/project.cpp:182
  f110qp_default_plan_config(&rp->plan);
}

int f110qp_plan_listed_dev(const f110qp_replan_config* rp, const f110qp_scan_config* sc, int batch,
                           const int* list, const int* count, const double* pose, const float* ranges,
                           const double* table, const double* wp, double* x_ref, int* plan_status,
                           int* best_traj, int* best_global, void* stream) {
  f110qp::PlanKParams K;
  int rv = replan_params(rp, &K);
  if (rv) return rv;
  if ((rv = check_scan_config(sc, false, 0))) return rv;
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (batch == 0) return F110QP_OK;
  if (!list || !count || !pose || !ranges || !table || (rp->num_waypoints > 0 && !wp) || !x_ref ||
      !plan_status || !best_traj || !best_global)
    return fail(F110QP_ERR_INVALID, "NULL pointer argument");
  const hipError_t e = f110qp::launch_plan_listed(K, batch, list, count, pose, ranges, sc->num_ranges,
                                                  sc->angle_min, sc->angle_increment, sc->angle_max, table, wp,
                                                  rp->num_waypoints, best_global, best_traj, x_ref, plan_status,
                                                  (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "listed plan launch");
  return F110QP_OK;
}

int f110qp_replan_start_dev(const f110qp_replan_config* rp, const f110qp_scan_config* sc, int batch,
                            const double* x, const int* have_path, const double* x_ref,
                            const f110qp_gap_record* gap, double* pose, int* kind, int* list, int* count,
                            float* hs, void* stream) {
  f110qp::PlanKParams K;
  int rv = replan_params(rp, &K);
  if (rv) return rv;
  if (hs && (rv = check_scan_config(sc, false, 0))) return rv;
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (batch == 0) return F110QP_OK;
  if (!x || !have_path || !x_ref || !pose || !kind || !list || !count)
    return fail(F110QP_ERR_INVALID, "x/have_path/x_ref/pose/kind/list/count must be non-NULL");
  if (hs && !gap) return fail(F110QP_ERR_INVALID, "hs needs the gap records");
  f110qp::ReplanStart st{};
  st.x = x;
  st.have_path = have_path;
  st.x_ref = x_ref;
  st.P = K.P;
  st.replan_dist = rp->replan_dist;
  st.pose = pose;
  st.kind = kind;
  st.list = list;
  st.count = count;
  st.gap = (const f110qp::GapRecord*)gap;
  st.hs = hs;
  if (hs) scan_geometry(&st, *sc);
  const hipError_t e = f110qp::launch_replan_start(batch, st, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "re-planning start launch");
  return F110QP_OK;
}

int f110qp_advance_replan_dev(const f110qp_rollout_config* rc, const f110qp_replan_config* rp,
                              const f110qp_scan_config* sc, int batch, int horizon, const double* x, int* kind,
                              const float* u_plan, int* status, const int* plan_status, const double* x_ref,
                              const f110qp_gap_record* gap, float* u_held, int* held_len, int* held_idx,
                              int* have_path, double* x_next, double* u_lin_next, float* u_applied,
                              double* pose_next, int* kind_next, int* next_list, int* next_count,
                              float* hs_next, void* stream) {
  f110qp::AdvanceParams ap;
  f110qp::PlanKParams K;
  int rv = rollout_params(rc, false, &ap);
  if (rv) return rv;
  if ((rv = replan_params(rp, &K))) return rv;
  if (hs_next && (rv = check_scan_config(sc, false, 0))) return rv;
  if (batch < 0) return fail(F110QP_ERR_INVALID, "batch < 0");
  if (horizon < 2 || horizon > F110QP_MAX_HORIZON) return fail(F110QP_ERR_INVALID, "horizon must be in [2, 48]");
  if (batch == 0) return F110QP_OK;
  if (!x || !kind || !u_plan || !status || !plan_status || !x_ref || !x_next || !u_lin_next)
    return fail(F110QP_ERR_INVALID, "x/kind/u_plan/status/plan_status/x_ref/x_next/u_lin_next must be non-NULL");
  if (!u_held || !held_len || !held_idx || !have_path || !pose_next)
    return fail(F110QP_ERR_INVALID, "u_held/held_len/held_idx/have_path/pose_next must be non-NULL");
  if (kind_next && (!next_list || !next_count))
    return fail(F110QP_ERR_INVALID, "kind_next needs next_list and next_count");
  if (hs_next && !gap) return fail(F110QP_ERR_INVALID, "hs_next needs the gap records");
  if (x_next == x) return fail(F110QP_ERR_INVALID, "x_next must not alias x");
  if (!aligned8(u_plan) || !aligned8(u_applied) || !aligned8(u_held))
    return fail(F110QP_ERR_INVALID, "u_plan / u_applied / u_held must be 8-byte aligned");
  f110qp::ReplanStep S{};
  S.x = x;
  S.kind = kind;
  S.u_plan = u_plan;
  S.status = status;
  S.plan_status = plan_status;
  S.x_ref = x_ref;
  S.P = K.P;
  S.replan_dist = rp->replan_dist;
  S.u_held = u_held;
  S.held_len = held_len;
  S.held_idx = held_idx;
  S.have_path = have_path;
  S.x_next = x_next;
  S.u_lin_next = u_lin_next;
  S.u_applied = u_applied;
  S.pose_next = pose_next;
  S.kind_next = kind_next;
  S.next_list = next_list;
  S.next_count = next_count;
  S.gap = (const f110qp::GapRecord*)gap;
  S.hs_next = hs_next;
  if (hs_next) scan_geometry(&S, *sc);
  const hipError_t e = f110qp::launch_advance_replan(ap, batch, horizon, S, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "plant step launch");
  return F110QP_OK;
}

int f110qp_rollout_replan_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                              const f110qp_replan_config* rp, int batch, const double* table, const double* wp,
                              double* xr, int* have, const float* ranges, double* xt, double* ult, float* ua,
                              int* stt, int* itt, double* cot, float* up, float* xp, float* hst, int* kt,
                              int* pst, int* btt, int* bgt, double* poset, void* stream) {
  const RolloutIO io{batch, 0, 0, xr, xt, ult, ua, stt, itt, cot, up, xp};
  const ReplanIO r{table, wp, have, ranges, {hst, kt, pst, btt, bgt, poset}};
  return replan_call(c, LoopCfg{kReplan, rc, sc, rp}, io, r, on_stream(stream));
}

int f110qp_rollout_replan(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                          const f110qp_replan_config* rp, int batch, const double* table, const double* wp,
                          double* xr, int* have, const float* ranges, double* xt, double* ult, float* ua,
                          int* stt, int* itt, double* cot, float* up, float* xp, float* hst, int* kt, int* pst,
                          int* btt, int* bgt, double* poset) {
  const RolloutIO io{batch, 0, 0, xr, xt, ult, ua, stt, itt, cot, up, xp};
  const ReplanIO r{table, wp, have, ranges, {hst, kt, pst, btt, bgt, poset}};
  return replan_call(c, LoopCfg{kReplan, rc, sc, rp}, io, r, on_host());
}

// ---- closed loop in a world of circles, with race-mates (f110qp_rollout_world / _race[_dev]) ----------

void f110qp_default_world_config(f110qp_world_config* wc) {
  if (!wc) return;
  std::memset(wc, 0, sizeof(*wc));
  wc->world_rows = 1;
  wc->lidar_offset = 0.275;  // occupancy_grid.cpp:63-64
  wc->max_range = 10.0;
}

int f110qp_cast_scans_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc, int batch, const int* list,
                          const int* count, const double* x, const double* circles, float* ranges,
                          void* stream) {
  return cast_call(row::world, sc, WorldCfgs{wc}, batch, list, count, x, circles, nullptr, ranges, stream);
}

int f110qp_rollout_world_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                             const f110qp_replan_config* rp, const f110qp_world_config* wc, int batch,
                             const double* table, const double* wp, double* xr, int* have, const double* circles,
                             double* xt, double* ult, float* ua, int* stt, int* itt, double* cot, float* up,
                             float* xp, float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset,
                             float* rgt, void* stream) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset);
  const WorldCfgs k = WorldCfgs{wc};
  return world_call(c, row::world, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, nullptr, rgt, on_stream(stream));
}

int f110qp_rollout_world(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                         const f110qp_replan_config* rp, const f110qp_world_config* wc, int batch,
                         const double* table, const double* wp, double* xr, int* have, const double* circles,
                         double* xt, double* ult, float* ua, int* stt, int* itt, double* cot, float* up,
                         float* xp, float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset,
                         float* rgt) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset);
  return world_call(c, row::world, LoopCfg{kWorld, rc, sc, rp}, WorldCfgs{wc}, a, circles, nullptr, rgt, on_host());
}

void f110qp_default_race_config(f110qp_race_config* race) {
  if (!race) return;
  std::memset(race, 0, sizeof(*race));
  race->group_size = 1;
  race->car_radius = 0.3;        // covers a 0.58 x 0.31 m car
  race->center_offset = 0.1651;  // half the 0.3302 wheelbase of Model::Linearize
}

int f110qp_cast_scans_race_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                               const f110qp_race_config* race, int batch, const int* list, const int* count,
                               const double* x, const double* circles, float* ranges, void* stream) {
  return cast_call(row::race, sc, WorldCfgs{wc}.Race(race), batch, list, count, x, circles, nullptr, ranges, stream);
}

int f110qp_rollout_race_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                            const f110qp_replan_config* rp, const f110qp_world_config* wc,
                            const f110qp_race_config* race, int batch, const double* table, const double* wp,
                            double* xr, int* have, const double* circles, double* xt, double* ult, float* ua,
                            int* stt, int* itt, double* cot, float* up, float* xp, float* hst, int* kt, int* pst,
                            int* btt, int* bgt, double* poset, float* rgt, void* stream) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset);
  const WorldCfgs k = WorldCfgs{wc}.Race(race);
  return world_call(c, row::race, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, nullptr, rgt, on_stream(stream));
}

int f110qp_rollout_race(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                        const f110qp_replan_config* rp, const f110qp_world_config* wc,
                        const f110qp_race_config* race, int batch, const double* table, const double* wp,
                        double* xr, int* have, const double* circles, double* xt, double* ult, float* ua, int* stt,
                        int* itt, double* cot, float* up, float* xp, float* hst, int* kt, int* pst, int* btt,
                        int* bgt, double* poset, float* rgt) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset);
  const WorldCfgs k = WorldCfgs{wc}.Race(race);
  return world_call(c, row::race, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, nullptr, rgt, on_host());
}

// ---- contact: clearance to walls and race-mates, crashed cars park (f110qp_clearance_dev, ----------------
// ---- f110qp_rollout_contact[_dev]) ---------------------------------------------------------------------

void f110qp_default_contact_config(f110qp_contact_config* cc) {
  if (!cc) return;
  std::memset(cc, 0, sizeof(*cc));
  cc->stop_on_contact = 0;
  cc->margin = 0.0;
}

int f110qp_clearance_dev(const f110qp_world_config* wc, const f110qp_race_config* race, int batch, int rows,
                         const double* x, const double* circles, double* clearance, int* nearest, void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race);
  return clearance_call(row::race, k, batch, rows, x, circles, nullptr, clearance, nearest, stream);
}

int f110qp_rollout_contact_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                               const f110qp_replan_config* rp, const f110qp_world_config* wc,
                               const f110qp_race_config* race, const f110qp_contact_config* cc, int batch,
                               const double* table, const double* wp, double* xr, int* have, const double* circles,
                               double* xt, double* ult, float* ua, int* stt, int* itt, double* cot, float* up,
                               float* xp, float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset,
                               float* rgt, double* clt, int* nrt, int* crash, void* stream) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc);
  return world_call(c, row::contact, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, nullptr, rgt, on_stream(stream));
}

int f110qp_rollout_contact(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                           const f110qp_replan_config* rp, const f110qp_world_config* wc,
                           const f110qp_race_config* race, const f110qp_contact_config* cc, int batch,
                           const double* table, const double* wp, double* xr, int* have, const double* circles,
                           double* xt, double* ult, float* ua, int* stt, int* itt, double* cot, float* up, float* xp,
                           float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset, float* rgt, double* clt,
                           int* nrt, int* crash) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc);
  return world_call(c, row::contact, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, nullptr, rgt, on_host());
}

// ---- rectangular car bodies (f110qp_clearance_body_dev, f110qp_cast_scans_body_dev, -----------------------
// ---- f110qp_rollout_body[_dev]) ------------------------------------------------------------------------

void f110qp_default_body_config(f110qp_body_config* body) {
  if (!body) return;
  std::memset(body, 0, sizeof(*body));
  body->half_length = 0.29;  // a 0.58 x 0.31 m car
  body->half_width = 0.155;
}

int f110qp_clearance_body_dev(const f110qp_world_config* wc, const f110qp_race_config* race,
                              const f110qp_body_config* body, int batch, int rows, const double* x,
                              const double* circles, double* clearance, int* nearest, void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Body(body);
  return clearance_call(row::body, k, batch, rows, x, circles, nullptr, clearance, nearest, stream);
}

int f110qp_cast_scans_body_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                               const f110qp_race_config* race, const f110qp_body_config* body, int batch,
                               const int* list, const int* count, const double* x, const double* circles,
                               float* ranges, void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Body(body);
  return cast_call(row::body, sc, k, batch, list, count, x, circles, nullptr, ranges, stream);
}

int f110qp_rollout_body_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                            const f110qp_replan_config* rp, const f110qp_world_config* wc,
                            const f110qp_race_config* race, const f110qp_contact_config* cc,
                            const f110qp_body_config* body, int batch, const double* table, const double* wp,
                            double* xr, int* have, const double* circles, double* xt, double* ult, float* ua,
                            int* stt, int* itt, double* cot, float* up, float* xp, float* hst, int* kt, int* pst,
                            int* btt, int* bgt, double* poset, float* rgt, double* clt, int* nrt, int* crash,
                            void* stream) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body);
  return world_call(c, row::body, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, nullptr, rgt, on_stream(stream));
}

int f110qp_rollout_body(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                        const f110qp_replan_config* rp, const f110qp_world_config* wc,
                        const f110qp_race_config* race, const f110qp_contact_config* cc,
                        const f110qp_body_config* body, int batch, const double* table, const double* wp, double* xr,
                        int* have, const double* circles, double* xt, double* ult, float* ua, int* stt, int* itt,
                        double* cot, float* up, float* xp, float* hst, int* kt, int* pst, int* btt, int* bgt,
                        double* poset, float* rgt, double* clt, int* nrt, int* crash) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body);
  return world_call(c, row::body, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, nullptr, rgt, on_host());
}

// ---- straight walls (f110qp_cast_scans_walls_dev, f110qp_clearance_walls_dev, f110qp_rollout_walls[_dev]) ------

void f110qp_default_walls_config(f110qp_walls_config* walls) {
  if (!walls) return;
  std::memset(walls, 0, sizeof(*walls));
  walls->wall_rows = 1;
}

int f110qp_cast_scans_walls_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                                const f110qp_race_config* race, const f110qp_body_config* body,
                                const f110qp_walls_config* walls, int batch, const int* list, const int* count,
                                const double* x, const double* circles, const double* segments, float* ranges,
                                void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Body(body).Walls(walls);
  return cast_call(row::walls, sc, k, batch, list, count, x, circles, segments, ranges, stream);
}

int f110qp_clearance_walls_dev(const f110qp_world_config* wc, const f110qp_race_config* race,
                               const f110qp_body_config* body, const f110qp_walls_config* walls, int batch, int rows,
                               const double* x, const double* circles, const double* segments, double* clearance,
                               int* nearest, void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Body(body).Walls(walls);
  return clearance_call(row::walls, k, batch, rows, x, circles, segments, clearance, nearest, stream);
}

int f110qp_rollout_walls_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                             const f110qp_replan_config* rp, const f110qp_world_config* wc,
                             const f110qp_race_config* race, const f110qp_contact_config* cc,
                             const f110qp_body_config* body, const f110qp_walls_config* walls, int batch,
                             const double* table, const double* wp, double* xr, int* have, const double* circles,
                             const double* segments, double* xt, double* ult, float* ua, int* stt, int* itt,
                             double* cot, float* up, float* xp, float* hst, int* kt, int* pst, int* btt, int* bgt,
                             double* poset, float* rgt, double* clt, int* nrt, int* crash, void* stream) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls);
  return world_call(c, row::walls, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_stream(stream));
}

int f110qp_rollout_walls(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                         const f110qp_replan_config* rp, const f110qp_world_config* wc,
                         const f110qp_race_config* race, const f110qp_contact_config* cc,
                         const f110qp_body_config* body, const f110qp_walls_config* walls, int batch,
                         const double* table, const double* wp, double* xr, int* have, const double* circles,
                         const double* segments, double* xt, double* ult, float* ua, int* stt, int* itt, double* cot,
                         float* up, float* xp, float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset,
                         float* rgt, double* clt, int* nrt, int* crash) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls);
  return world_call(c, row::walls, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_host());
}

// ---- a refreshed MPC scan (f110qp_gap_refresh_dev, f110qp_rollout_refresh[_dev]) -------------------------------

void f110qp_default_refresh_config(f110qp_refresh_config* rf) {
  if (!rf) return;
  std::memset(rf, 0, sizeof(*rf));
}

int f110qp_gap_refresh_dev(const f110qp_scan_config* sc, int batch, const float* ranges, const double* states,
                           f110qp_gap_record* gap, float* hs, void* stream) {
  const int rv = check_scan_config(sc, false, 0);
  if (rv) return rv;
  if (batch < 1) return fail(F110QP_ERR_INVALID, "batch < 1");
  if (!ranges || !states || !gap || !hs)
    return fail(F110QP_ERR_INVALID, "ranges/states/gap_out/hs_out must be non-NULL");
  const hipError_t e = f110qp::launch_gap_refresh(batch, ranges, sc->num_ranges, sc->angle_min, sc->angle_increment,
                                                  sc->angle_max, sc->ftg_thresh, sc->divider, sc->buffer, states,
                                                  (f110qp::GapRecord*)gap, hs, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "gap refresh launch");
  return F110QP_OK;
}

int f110qp_rollout_refresh_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                               const f110qp_replan_config* rp, const f110qp_world_config* wc,
                               const f110qp_race_config* race, const f110qp_contact_config* cc,
                               const f110qp_body_config* body, const f110qp_walls_config* walls,
                               const f110qp_refresh_config* rf, int batch, const double* table, const double* wp,
                               double* xr, int* have, const double* circles, const double* segments, double* xt,
                               double* ult, float* ua, int* stt, int* itt, double* cot, float* up, float* xp,
                               float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset, float* rgt,
                               double* clt, int* nrt, int* crash, void* stream) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls).Refresh(rf);
  return world_call(c, row::refresh, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_stream(stream));
}

int f110qp_rollout_refresh(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                           const f110qp_replan_config* rp, const f110qp_world_config* wc,
                           const f110qp_race_config* race, const f110qp_contact_config* cc,
                           const f110qp_body_config* body, const f110qp_walls_config* walls,
                           const f110qp_refresh_config* rf, int batch, const double* table, const double* wp,
                           double* xr, int* have, const double* circles, const double* segments, double* xt,
                           double* ult, float* ua, int* stt, int* itt, double* cot, float* up, float* xp, float* hst,
                           int* kt, int* pst, int* btt, int* bgt, double* poset, float* rgt, double* clt, int* nrt,
                           int* crash) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls).Refresh(rf);
  return world_call(c, row::refresh, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_host());
}

// ---- a noisy LiDAR (f110qp_cast_scans_noisy_dev, f110qp_rollout_noisy[_dev]) ------------------------------------

void f110qp_default_noise_config(f110qp_noise_config* noise) {
  if (!noise) return;
  std::memset(noise, 0, sizeof(*noise));
}

int f110qp_cast_scans_noisy_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                                const f110qp_race_config* race, const f110qp_body_config* body,
                                const f110qp_walls_config* walls, const f110qp_noise_config* noise, int batch,
                                int tick, const int* list, const int* count, const double* x, const double* circles,
                                const double* segments, float* ranges, void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Body(body).Walls(walls).Noise(noise);
  return cast_call(row::noisy, sc, k, batch, list, count, x, circles, segments, ranges, stream, tick);
}

int f110qp_rollout_noisy_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                             const f110qp_replan_config* rp, const f110qp_world_config* wc,
                             const f110qp_race_config* race, const f110qp_contact_config* cc,
                             const f110qp_body_config* body, const f110qp_walls_config* walls,
                             const f110qp_refresh_config* rf, const f110qp_noise_config* noise, int batch,
                             const double* table, const double* wp, double* xr, int* have, const double* circles,
                             const double* segments, double* xt, double* ult, float* ua, int* stt, int* itt,
                             double* cot, float* up, float* xp, float* hst, int* kt, int* pst, int* btt, int* bgt,
                             double* poset, float* rgt, double* clt, int* nrt, int* crash, void* stream) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls).Refresh(rf).Noise(noise);
  return world_call(c, row::noisy, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_stream(stream));
}

int f110qp_rollout_noisy(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                         const f110qp_replan_config* rp, const f110qp_world_config* wc,
                         const f110qp_race_config* race, const f110qp_contact_config* cc,
                         const f110qp_body_config* body, const f110qp_walls_config* walls,
                         const f110qp_refresh_config* rf, const f110qp_noise_config* noise, int batch,
                         const double* table, const double* wp, double* xr, int* have, const double* circles,
                         const double* segments, double* xt, double* ult, float* ua, int* stt, int* itt, double* cot,
                         float* up, float* xp, float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset,
                         float* rgt, double* clt, int* nrt, int* crash) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls).Refresh(rf).Noise(noise);
  return world_call(c, row::noisy, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_host());
}

// ---- a raster map (f110qp_cast_scans_grid_dev, f110qp_clearance_grid_dev, f110qp_rollout_grid[_dev]) -----------

void f110qp_default_grid_config(f110qp_grid_config* gc) {
  if (!gc) return;
  std::memset(gc, 0, sizeof(*gc));
  gc->resolution = 0.05;  // map_server's usual cell
  gc->reach = 1.0;
}

int f110qp_cast_scans_grid_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc,
                               const f110qp_race_config* race, const f110qp_body_config* body,
                               const f110qp_walls_config* walls, const f110qp_noise_config* noise,
                               const f110qp_grid_config* gc, int batch, int tick, const int* list, const int* count,
                               const double* x, const double* circles, const double* segments,
                               const unsigned char* grid, float* ranges, void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Body(body).Walls(walls).Noise(noise).Grid(gc);
  return cast_call(row::grid, sc, k, batch, list, count, x, circles, segments, ranges, stream, tick, grid);
}

int f110qp_clearance_grid_dev(const f110qp_world_config* wc, const f110qp_race_config* race,
                              const f110qp_body_config* body, const f110qp_walls_config* walls,
                              const f110qp_grid_config* gc, int batch, int rows, const double* x,
                              const double* circles, const double* segments, const unsigned char* grid,
                              double* clearance, int* nearest, void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Body(body).Walls(walls).Grid(gc);
  return clearance_call(row::grid, k, batch, rows, x, circles, segments, clearance, nearest, stream, grid);
}

int f110qp_rollout_grid_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                            const f110qp_replan_config* rp, const f110qp_world_config* wc,
                            const f110qp_race_config* race, const f110qp_contact_config* cc,
                            const f110qp_body_config* body, const f110qp_walls_config* walls,
                            const f110qp_refresh_config* rf, const f110qp_noise_config* noise,
                            const f110qp_grid_config* gc, int batch, const double* table, const double* wp, double* xr,
                            int* have, const double* circles, const double* segments, const unsigned char* grid,
                            double* xt, double* ult, float* ua, int* stt, int* itt, double* cot, float* up, float* xp,
                            float* hst, int* kt, int* pst, int* btt, int* bgt, double* poset, float* rgt, double* clt,
                            int* nrt, int* crash, void* stream) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls).Refresh(rf).Noise(noise).Grid(gc);
  return world_call(c, row::grid, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_stream(stream), grid);
}

int f110qp_rollout_grid(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                        const f110qp_replan_config* rp, const f110qp_world_config* wc,
                        const f110qp_race_config* race, const f110qp_contact_config* cc,
                        const f110qp_body_config* body, const f110qp_walls_config* walls,
                        const f110qp_refresh_config* rf, const f110qp_noise_config* noise,
                        const f110qp_grid_config* gc, int batch, const double* table, const double* wp, double* xr,
                        int* have, const double* circles, const double* segments, const unsigned char* grid, double* xt,
                        double* ult, float* ua, int* stt, int* itt, double* cot, float* up, float* xp, float* hst,
                        int* kt, int* pst, int* btt, int* bgt, double* poset, float* rgt, double* clt, int* nrt,
                        int* crash) {
  const WorldArrays a = world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt,
                                     bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls).Refresh(rf).Noise(noise).Grid(gc);
  return world_call(c, row::grid, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_host(), grid);
}

// ---- the raster map's casts through its distance field (f110qp_grid_cast_dev, f110qp_rollout_field[_dev]) ------

int f110qp_grid_cast_dev(const f110qp_scan_config* sc, const f110qp_world_config* wc, const f110qp_race_config* race,
                         const f110qp_body_config* body, const f110qp_walls_config* walls,
                         const f110qp_noise_config* noise, const f110qp_grid_config* gc, int batch, int tick,
                         const int* list, const int* count, const double* x, const double* circles,
                         const double* segments, const unsigned char* grid, const int* d2, float* ranges, int* visits,
                         void* stream) {
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Body(body).Walls(walls).Noise(noise).Grid(gc);
  return cast_call(row::field, sc, k, batch, list, count, x, circles, segments, ranges, stream, tick, grid, d2, visits);
}

int f110qp_rollout_field_dev(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                             const f110qp_replan_config* rp, const f110qp_world_config* wc,
                             const f110qp_race_config* race, const f110qp_contact_config* cc,
                             const f110qp_body_config* body, const f110qp_walls_config* walls,
                             const f110qp_refresh_config* rf, const f110qp_noise_config* noise,
                             const f110qp_grid_config* gc, int batch, const double* table, const double* wp,
                             double* xr, int* have, const double* circles, const double* segments,
                             const unsigned char* grid, const int* d2, double* xt, double* ult, float* ua, int* stt,
                             int* itt, double* cot, float* up, float* xp, float* hst, int* kt, int* pst, int* btt,
                             int* bgt, double* poset, float* rgt, double* clt, int* nrt, int* crash, void* stream) {
  const WorldArrays a =
      world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt, bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls).Refresh(rf).Noise(noise).Grid(gc);
  return world_call(c, row::field, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_stream(stream), grid,
                    d2);
}

int f110qp_rollout_field(f110qp_ctx* c, const f110qp_rollout_config* rc, const f110qp_scan_config* sc,
                         const f110qp_replan_config* rp, const f110qp_world_config* wc,
                         const f110qp_race_config* race, const f110qp_contact_config* cc,
                         const f110qp_body_config* body, const f110qp_walls_config* walls,
                         const f110qp_refresh_config* rf, const f110qp_noise_config* noise,
                         const f110qp_grid_config* gc, int batch, const double* table, const double* wp, double* xr,
                         int* have, const double* circles, const double* segments, const unsigned char* grid, double* xt,
                         double* ult, float* ua, int* stt, int* itt, double* cot, float* up, float* xp, float* hst,
                         int* kt, int* pst, int* btt, int* bgt, double* poset, float* rgt, double* clt, int* nrt,
                         int* crash) {
  const WorldArrays a =
      world_arrays(batch, table, wp, xr, have, xt, ult, ua, stt, itt, cot, up, xp, hst, kt, pst, btt, bgt, poset, clt, nrt, crash);
  const WorldCfgs k = WorldCfgs{wc}.Race(race).Contact(cc).Body(body).Walls(walls).Refresh(rf).Noise(noise).Grid(gc);
  return world_call(c, row::field, LoopCfg{kWorld, rc, sc, rp}, k, a, circles, segments, rgt, on_host(), grid);
}

}  // extern "C"
