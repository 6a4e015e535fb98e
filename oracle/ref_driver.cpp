// ref_driver: runs the reference's own compiled State / Input / Cost / Model / Constraints / MPC
// classes on recorded inputs and writes what they compute (TEST INFRASTRUCTURE ONLY).
//
// It is linked from the reference's unmodified .cpp files, which are named only on the compiler's
// command line (oracle/Makefile, target `ref`), and the stand-in headers of oracle/refshim/.
// Everything in this file is this project's own text, including the few lines of glue in
// run_loop() that stand for the MPC branch of the reference's odometry callback: how the index
// of the next input advances between two callbacks is this project's modelling choice
// (include/f110qp.h, f110qp_advance_dev), not something the reference's tick fixes.
//
//   ref_driver MODE IN OUT PARAMS_YAML [key=value ...]
//
// IN and OUT are flat arrays of native float64 (numpy tofile / fromfile); float32 quantities are
// carried exactly. PARAMS_YAML is a flat `key: value` file; key=value arguments override it.
//   model      IN  n, then n x (x, y, ori, v, steer, dt)
//              OUT n x (A[9] row-major, B[6] row-major, C[3], simulate_dynamics[3])
//   halfspace  IN  n, then n x (x, y, ori, scan)        scan = angle_min, inc, max, nr, ranges[nr]
//              OUT n x (l1[3], l2[3])
//              The gap indices best_lo / best_hi are locals of FindHalfSpaces: not available.
//   tick       IN  S, calls, then calls x (x0[3], u_lin[2], x_ref[S][3], scan)   one MPC object
//              OUT calls x QP                           (see dump_qp)
//   loop       IN  cars, T, S, then cars x (x0[3], u_lin0[2], x_ref[S][3], scan)
//              OUT cars x (T x (x[3], u_lin[2], status, QP, z[n], count, plan[count][2],
//                               u_applied[2]), x_T[3], u_lin_T[2])
//              solve() is answered by f110o_solve of liboracle on the same inputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "f110-mpc/mpc.h"
#include "f110_oracle.h"

// visualizer.cpp is not compiled; MPC::Visualize (never called here) needs this symbol
visualization_msgs::Marker Visualizer::GenerateList(std::vector<geometry_msgs::Point>&, std::vector<std_msgs::ColorRGBA>&,
                                                    int, double, double, double) {
  return visualization_msgs::Marker();
}

namespace {

struct Reader {
  std::vector<double> d;
  size_t pos = 0;
  double next() {
    if (pos >= d.size()) { std::fprintf(stderr, "ref_driver: input too short\n"); std::exit(2); }
    return d[pos++];
  }
  int next_int() { return (int)next(); }
};

std::vector<double> out;

void load_params(const char* yaml, int argc, char** argv, int first) {
  auto& p = ros::refshim_params();
  std::ifstream f(yaml);
  if (!f) { std::fprintf(stderr, "ref_driver: cannot read %s\n", yaml); std::exit(2); }
  std::string line;
  auto trim = [](std::string s) {
    size_t a = s.find_first_not_of(" \t\r\"'"), b = s.find_last_not_of(" \t\r\"'");
    return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
  };
  while (std::getline(f, line)) {
    size_t h = line.find('#');
    if (h != std::string::npos) line.erase(h);
    size_t c = line.find(':');
    if (c == std::string::npos) continue;
    std::string k = trim(line.substr(0, c)), v = trim(line.substr(c + 1));
    if (!k.empty() && !v.empty()) p[k] = v;
  }
  for (int i = first; i < argc; i++) {
    const char* eq = std::strchr(argv[i], '=');
    if (!eq) { std::fprintf(stderr, "ref_driver: expected key=value, got %s\n", argv[i]); std::exit(2); }
    p[std::string(argv[i], eq - argv[i])] = std::string(eq + 1);
  }
}

sensor_msgs::LaserScan read_scan(Reader& in) {
  sensor_msgs::LaserScan s;
  s.angle_min = (float)in.next();
  s.angle_increment = (float)in.next();
  s.angle_max = (float)in.next();
  int nr = in.next_int();
  s.ranges.resize((size_t)nr);
  for (int i = 0; i < nr; i++) s.ranges[(size_t)i] = (float)in.next();
  return s;
}

void put(const Eigen::MatrixXd& m, bool row_major) {
  if (row_major) {
    for (int i = 0; i < m.rows(); i++)
      for (int j = 0; j < m.cols(); j++) out.push_back(m(i, j));
  } else {
    for (int k = 0; k < m.size(); k++) out.push_back(m(k));
  }
}

void put_csc(const Eigen::SparseMatrix<double>& a) {
  std::vector<int> cp, ri;
  std::vector<double> v;
  a.toCSC(cp, ri, v);
  out.push_back((double)ri.size());
  for (int x : cp) out.push_back(x);
  for (int x : ri) out.push_back(x);
  for (double x : v) out.push_back(x);
}

// QP = update_path, set_calls, update_calls, n, m, P (nnz, colptr[n+1], rowind, val), q[n],
//      A (nnz, colptr[n+1], rowind, val), l[m], u[m]
void dump_qp(const OsqpEigen::Capture& c, bool update_path) {
  out.push_back(update_path ? 1.0 : 0.0);
  out.push_back(c.set_calls);
  out.push_back(c.update_calls);
  out.push_back(c.num_variables);
  out.push_back(c.num_constraints);
  put_csc(c.hessian);
  put(c.gradient, false);
  put_csc(c.linear);
  put(c.lower, false);
  put(c.upper, false);
}

std::vector<State> read_path(Reader& in, int S) {
  std::vector<State> p;
  for (int i = 0; i < S; i++) {
    double x = in.next(), y = in.next(), o = in.next();
    p.push_back(State(x, y, o));
  }
  return p;
}

void run_model(Reader& in) {
  int n = in.next_int();
  Model model;
  for (int i = 0; i < n; i++) {
    double x = in.next(), y = in.next(), o = in.next(), v = in.next(), d = in.next(), dt = in.next();
    State s(x, y, o), s2;
    Input u(v, d);
    model.Linearize(s, u, dt);
    put(model.A(), true);
    put(model.B(), true);
    put(model.C(), true);
    model.simulate_dynamics(s, u, dt, s2);
    out.push_back(s2.x());
    out.push_back(s2.y());
    out.push_back(s2.ori());
  }
}

void run_halfspace(Reader& in) {
  int n = in.next_int();
  ros::NodeHandle nh;
  Constraints con(nh);
  for (int i = 0; i < n; i++) {
    double x = in.next(), y = in.next(), o = in.next();
    State s(x, y, o);
    sensor_msgs::LaserScan scan = read_scan(in);
    con.FindHalfSpaces(s, scan);
    put(con.l1(), false);
    put(con.l2(), false);
  }
}

void run_tick(Reader& in) {
  int S = in.next_int(), calls = in.next_int();
  ros::NodeHandle nh;
  MPC mpc(nh);
  OsqpEigen::Solver* solver = OsqpEigen::Solver::last();
  OsqpEigen::Solver::solve_fn() = nullptr;  // solve() returns zeros
  for (int c = 0; c < calls; c++) {
    double x = in.next(), y = in.next(), o = in.next(), v = in.next(), d = in.next();
    std::vector<State> path = read_path(in, S);
    sensor_msgs::LaserScan::ConstPtr scan(new sensor_msgs::LaserScan(read_scan(in)));
    const int updates_before = solver->capture().update_calls;
    mpc.UpdateScan(scan);
    mpc.Update(State(x, y, o), Input(v, d), path);
    dump_qp(solver->capture(), solver->capture().update_calls > updates_before);
  }
}

// what the installed solve() answers with in loop mode
struct LoopTick {
  f110o_params prm;
  double x0[3], u_lin[2];
  std::vector<double> x_ref, z;
  int status;
} tick;

bool oracle_solve(const OsqpEigen::Capture& qp, Eigen::VectorXd& sol) {
  const int N = tick.prm.horizon;
  std::vector<double> u((size_t)2 * N), x((size_t)3 * (N + 1));
  tick.z.assign((size_t)qp.num_variables, 0.0);
  double obj = 0;
  tick.status = f110o_solve(&tick.prm, tick.x0, tick.u_lin, tick.x_ref.data(), nullptr, 0, u.data(), x.data(),
                            tick.z.data(), nullptr, &obj, nullptr);
  if (tick.status != F110O_SOLVED) return false;
  for (int i = 0; i < qp.num_variables; i++) sol(i) = tick.z[(size_t)i];  // already (states, inputs)
  return true;
}

void run_loop(Reader& in) {
  int cars = in.next_int(), T = in.next_int(), S = in.next_int();
  ros::NodeHandle nh;
  // the oracle's view of the same parameters
  f110o_default_params(&tick.prm, 0);
  nh.getParam("horizon", tick.prm.horizon);
  nh.getParam("dt", tick.prm.dt);
  nh.getParam("q0", tick.prm.q[0]); nh.getParam("q1", tick.prm.q[1]); nh.getParam("q2", tick.prm.q[2]);
  nh.getParam("r0", tick.prm.r[0]); nh.getParam("r1", tick.prm.r[1]);
  nh.getParam("des_vel", tick.prm.u_des[0]); nh.getParam("des_steer", tick.prm.u_des[1]);
  nh.getParam("umin", tick.prm.u_min[0]); nh.getParam("umax", tick.prm.u_max[0]);
  double plant_dt = 0.01;
  nh.getParam("plant_dt", plant_dt);
  OsqpEigen::Solver::solve_fn() = oracle_solve;
  for (int c = 0; c < cars; c++) {
    MPC mpc(nh);
    Model plant;
    OsqpEigen::Solver* solver = OsqpEigen::Solver::last();
    double x = in.next(), y = in.next(), o = in.next();
    State state(x, y, o);
    double v0 = in.next(), d0 = in.next();
    Input next_input(v0, d0);
    std::vector<State> path = read_path(in, S);
    tick.x_ref.clear();
    for (State& s : path) { tick.x_ref.push_back(s.x()); tick.x_ref.push_back(s.y()); tick.x_ref.push_back(s.ori()); }
    sensor_msgs::LaserScan::ConstPtr scan(new sensor_msgs::LaserScan(read_scan(in)));
    mpc.UpdateScan(scan);
    for (int t = 0; t < T; t++) {
      // ---- glue standing for the callback: this project's own lines -------------------------
      Input input_to_pass = next_input;
      input_to_pass.set_v(4.5);
      tick.x0[0] = state.x(); tick.x0[1] = state.y(); tick.x0[2] = state.ori();
      tick.u_lin[0] = input_to_pass.v(); tick.u_lin[1] = input_to_pass.steer_ang();
      tick.status = 0;
      const int updates_before = solver->capture().update_calls;
      mpc.Update(state, input_to_pass, path);
      if (tick.status != F110O_SOLVED) {  // box rows only: cannot happen; the failure path is not recorded
        std::fprintf(stderr, "ref_driver: car %d tick %d: oracle status %d\n", c, t, tick.status);
        std::exit(3);
      }
      std::vector<Input> plan = mpc.solved_trajectory();
      // the drive thread publishes plan[0] (a float32 message) and advances the index once
      // before the next callback: the car is driven by plan[0], the next tick linearises at
      // plan[1] (plan[0] when the plan has one entry)
      Input applied((double)(float)plan[0].v(), (double)(float)plan[0].steer_ang());
      next_input = plan[plan.size() > 1 ? 1 : 0];
      // ---------------------------------------------------------------------------------------
      out.push_back(tick.x0[0]); out.push_back(tick.x0[1]); out.push_back(tick.x0[2]);
      out.push_back(tick.u_lin[0]); out.push_back(tick.u_lin[1]);
      out.push_back(tick.status);
      dump_qp(solver->capture(), solver->capture().update_calls > updates_before);
      for (double zz : tick.z) out.push_back(zz);
      out.push_back((double)plan.size());
      for (Input& u : plan) { out.push_back(u.v()); out.push_back(u.steer_ang()); }
      out.push_back(applied.v()); out.push_back(applied.steer_ang());
      State moved;
      plant.simulate_dynamics(state, applied, plant_dt, moved);
      state = moved;
    }
    Input last = next_input;
    last.set_v(4.5);
    out.push_back(state.x()); out.push_back(state.y()); out.push_back(state.ori());
    out.push_back(last.v()); out.push_back(last.steer_ang());
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: ref_driver model|halfspace|tick|loop IN OUT PARAMS_YAML [key=value ...]\n");
    return 2;
  }
  load_params(argv[4], argc, argv, 5);
  Reader in;
  {
    std::ifstream f(argv[2], std::ios::binary);
    if (!f) { std::fprintf(stderr, "ref_driver: cannot read %s\n", argv[2]); return 2; }
    f.seekg(0, std::ios::end);
    size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    in.d.resize(bytes / sizeof(double));
    f.read(reinterpret_cast<char*>(in.d.data()), (std::streamsize)(in.d.size() * sizeof(double)));
  }
  const std::string mode = argv[1];
  if (mode == "model") run_model(in);
  else if (mode == "halfspace") run_halfspace(in);
  else if (mode == "tick") run_tick(in);
  else if (mode == "loop") run_loop(in);
  else { std::fprintf(stderr, "ref_driver: unknown mode %s\n", argv[1]); return 2; }
  if (in.pos != in.d.size()) { std::fprintf(stderr, "ref_driver: %zu unread input values\n", in.d.size() - in.pos); return 2; }
  std::ofstream o(argv[3], std::ios::binary);
  o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
  return o ? 0 : 2;
}
