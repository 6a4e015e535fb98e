// Stand-alone self-test of the stand-in Eigen headers (TEST INFRASTRUCTURE ONLY). It builds a
// handful of matrices with the operations the reference's files use and prints them, one
// `name rows cols v...` line each (row-major, %.17g); tests/test_refshim.py rebuilds the same
// matrices in numpy and compares. Needs nothing but this directory.
#include <cstdio>
#include <vector>

#include "Eigen/Dense"
#include "Eigen/Sparse"

using Eigen::MatrixXd;
using Eigen::VectorXd;

static void show(const char* name, const MatrixXd& m) {
  std::printf("%s %d %d", name, m.rows(), m.cols());
  for (int i = 0; i < m.rows(); i++)
    for (int j = 0; j < m.cols(); j++) std::printf(" %.17g", m(i, j));
  std::printf("\n");
}

static MatrixXd ramp(int r, int c, double start) {  // m(i,j) = start + 10 i + j
  MatrixXd m(r, c);
  for (int i = 0; i < r; i++)
    for (int j = 0; j < c; j++) m(i, j) = start + 10 * i + j;
  return m;
}

int main() {
  // comma initialiser: scalars into a vector and into a 2x3 matrix (row by row)
  VectorXd v3;
  v3.resize(3);
  v3 << 1.5, -2.5, 3.25;
  show("comma_vec", v3);
  MatrixXd s23(2, 3);
  s23 << 1, 2, 3, 4, 5, 6;
  show("comma_scalars", s23);
  // a << M1, -M2 : two 3x3 blocks side by side
  MatrixXd M1 = ramp(3, 3, 1.0), M2 = MatrixXd::Identity(3, 3);
  MatrixXd side(3, 6);
  side << M1, -M2;
  show("comma_side", side);
  // two bands: (2x2, 2x1) over (1x3)
  MatrixXd bands(3, 3);
  bands << ramp(2, 2, 1.0), ramp(2, 1, 50.0), ramp(1, 3, 70.0);
  show("comma_bands", bands);
  // vertical stack into a vector: Zero, replicate, replicate
  VectorXd pair2(2);
  pair2(0) = -7.0;
  pair2(1) = 9.0;
  VectorXd stack(3 + 2 * 3 + 2 * 2);
  stack << VectorXd::Zero(3), pair2.replicate(3, 1), 4.0, 5.0, pair2.replicate(1, 1);
  show("comma_stack", stack);
  // v.head(n) << -a, -c.replicate(h,1) ; the tail stays
  VectorXd h = VectorXd::Ones(11);
  VectorXd a3(3), c3(3);
  a3 << 1, 2, 3;
  c3 << 0.5, 0.25, 0.125;
  h.head(9) << -a3, -c3.replicate(2, 1);
  show("head_comma", h);
  // replicate in both directions, rectangular identity, ones, unary minus
  show("replicate", ramp(2, 3, 1.0).replicate(2, 2));
  show("identity_3x2", MatrixXd::Identity(3, 2));
  show("ones_2x3", MatrixXd::Ones(2, 3));
  // block assignment
  MatrixXd big = MatrixXd::Zero(5, 4);
  big.block(1, 2, 3, 2) = ramp(3, 2, 1.0);
  big.block(4, 0, 1, 1) = MatrixXd::Ones(1, 1);
  show("block", big);
  // products and sums: int * diagonal * vector, matrix * matrix, vector + vector * scalar
  Eigen::DiagonalMatrix<double, 3> q;
  q.diagonal() << 10.0, 0.1, 0.0;
  MatrixXd Q = q;
  show("diag_dense", Q);
  VectorXd x(3);
  x << 0.1, 0.7, -3.0;
  MatrixXd g = -1 * Q * x;
  show("neg_diag_times_vec", g);
  show("matmul", ramp(2, 3, 1.0) * ramp(3, 2, 0.5));
  VectorXd sum = x + a3 * 0.01;
  show("axpy", sum);
  // linear index on a matrix is column-major; size / rows / cols
  MatrixXd lin = ramp(2, 3, 1.0);
  VectorXd order(6);
  for (int k = 0; k < lin.size(); k++) order(k) = lin(k);
  show("linear_index", order);
  // resize keeps values when the size is unchanged (as Eigen does for a vector), (i,0) access
  VectorXd rs(3);
  rs << 4, 5, 6;
  rs.resize(3, 1);
  rs(1, 0) = -5;
  show("resize_keep", rs);

  // sparse: insert / coeffRef, explicit zeros kept, compressed column order
  Eigen::SparseMatrix<double> sp;
  sp.resize(4, 3);
  sp.setZero();
  sp.insert(3, 0) = 3.0;
  sp.insert(0, 0) = 0.0;   // an explicit zero
  sp.insert(2, 2) = -1;    // int assigned through the reference
  sp.insert(1, 2) = 7.0;
  sp.coeffRef(3, 0) = 30.0;  // overwrite
  sp.coeffRef(0, 2) = 0.0;   // created as a stored zero
  std::vector<int> cp, ri;
  std::vector<double> val;
  sp.toCSC(cp, ri, val);
  MatrixXd m_cp((int)cp.size(), 1), m_ri((int)ri.size(), 1), m_val((int)val.size(), 1);
  for (size_t k = 0; k < cp.size(); k++) m_cp((int)k) = cp[k];
  for (size_t k = 0; k < ri.size(); k++) m_ri((int)k) = ri[k];
  for (size_t k = 0; k < val.size(); k++) m_val((int)k) = val[k];
  show("csc_colptr", m_cp);
  show("csc_rowind", m_ri);
  show("csc_val", m_val);
  sp.setZero();
  MatrixXd nz(1, 1);
  nz(0) = sp.nonZeros();
  show("setzero_nnz", nz);
  return 0;
}
