// Stand-in for <OsqpEigen/OsqpEigen.h> (TEST INFRASTRUCTURE ONLY; see ../Eigen/Dense).
// No solver: Solver records what MPC::Update hands to data()->set* (first call) or to update*
// (later calls), counts which of the two paths ran, and answers solve() through a function
// pointer that the driver installs. settings() accepts everything and ignores it.
#ifndef F110_REFSHIM_OSQPEIGEN_H
#define F110_REFSHIM_OSQPEIGEN_H

#include "../Eigen/Dense"
#include "../Eigen/Sparse"

namespace OsqpEigen {

const double INFTY = 1e30;  // OSQP_INFTY

struct Capture {
  int num_variables = 0, num_constraints = 0;
  Eigen::SparseMatrix<double> hessian, linear;
  Eigen::VectorXd gradient, lower, upper;
  int set_calls = 0;     // setHessianMatrix + setGradient + ... of the first Update
  int update_calls = 0;  // updateGradient + updateLinearConstraintsMatrix + updateBounds
  int init_calls = 0, solve_calls = 0;
};

class Settings {
 public:
  template <typename T> void setWarmStart(T) {}
  template <typename T> void setVerbosity(T) {}
};

class Data {
 public:
  explicit Data(Capture* c) : c_(c) {}
  void setNumberOfVariables(int n) { c_->num_variables = n; }
  void setNumberOfConstraints(int m) { c_->num_constraints = m; }
  bool setHessianMatrix(const Eigen::SparseMatrix<double>& h) { c_->hessian = h; c_->set_calls++; return true; }
  bool setGradient(Eigen::VectorXd& g) { c_->gradient = g; c_->set_calls++; return true; }
  bool setLinearConstraintsMatrix(const Eigen::SparseMatrix<double>& a) { c_->linear = a; c_->set_calls++; return true; }
  bool setLowerBound(Eigen::VectorXd& l) { c_->lower = l; c_->set_calls++; return true; }
  bool setUpperBound(Eigen::VectorXd& u) { c_->upper = u; c_->set_calls++; return true; }

 private:
  Capture* c_;
};

class Solver {
 public:
  // the driver's answer to solve(): fills `solution` (num_variables long) and returns success
  typedef bool (*SolveFn)(const Capture& qp, Eigen::VectorXd& solution);
  static SolveFn& solve_fn() {
    static SolveFn f = nullptr;
    return f;
  }
  // the solver constructed last: how the driver reaches the one MPC keeps private
  static Solver*& last() {
    static Solver* s = nullptr;
    return s;
  }

  Solver() : data_(&cap_) { last() = this; }
  Solver(const Solver&) = delete;
  Solver& operator=(const Solver&) = delete;

  Settings* settings() { return &settings_; }
  Data* data() { return &data_; }
  bool initSolver() { cap_.init_calls++; return true; }
  bool updateGradient(Eigen::VectorXd& g) { cap_.gradient = g; cap_.update_calls++; return true; }
  bool updateLinearConstraintsMatrix(const Eigen::SparseMatrix<double>& a) { cap_.linear = a; cap_.update_calls++; return true; }
  bool updateBounds(Eigen::VectorXd& l, Eigen::VectorXd& u) { cap_.lower = l; cap_.upper = u; cap_.update_calls++; return true; }
  bool solve() {
    cap_.solve_calls++;
    solution_ = Eigen::VectorXd::Zero(cap_.num_variables);
    return solve_fn() ? solve_fn()(cap_, solution_) : true;
  }
  Eigen::VectorXd getSolution() { return solution_; }
  const Capture& capture() const { return cap_; }

 private:
  Capture cap_;
  Settings settings_;
  Data data_;
  Eigen::VectorXd solution_;
};

}  // namespace OsqpEigen

#endif
