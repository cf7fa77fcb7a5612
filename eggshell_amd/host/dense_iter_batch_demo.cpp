// dense_iter_batch_demo -- sparse::{Jacobi,GaussSeidel,SOR}IterationBatch against a loop of the single calls on the
// same systems, for tests/test_gpu_adapter_dense_iter_batch.py.  Eight systems (1, 6, 12, 20, 33, 48, 64 and 96 rows;
// symmetric positive definite and strictly diagonally dominant, so all three splittings converge) are solved by each
// method in the 2-argument form (every row an equality) and in the 5-argument form (mixed rows with a box), once as a
// batch and once as eight calls.  Every number is printed with 17 significant digits, one line per vector:
// "<method>_<eq|mixed>_<batch|single><k> values...".
#include <cstdio>
#include <vector>

#include "eggshell_api.h"

namespace {

const int kSizes[8] = {1, 6, 12, 20, 33, 48, 64, 96};

void print(const char *method, const char *form, const char *how, int k, const VectorXd &v) {
  std::printf("%s_%s_%s%d", method, form, how, k);
  for (int i = 0; i < v.size(); ++i) std::printf(" %.17g", v(i));
  std::printf("\n");
}

void make(int k, MatrixXd *A, VectorXd *b, ArrayXb *C, VectorXd *lo, VectorXd *hi) {
  const int m = kSizes[k];
  A->resize(m, m); b->resize(m); C->resize(m); lo->resize(m); hi->resize(m);
  for (int i = 0; i < m; ++i) {
    double off = 0.0;
    for (int j = 0; j < m; ++j) {
      if (j == i) continue;
      const int a = i < j ? i : j, c = i < j ? j : i;
      (*A)(i, j) = ((a * 31 + c * 17 + (a * c) % 11 + 7 * k) % 23 - 11) / 11.0;
      off += (*A)(i, j) < 0 ? -(*A)(i, j) : (*A)(i, j);
    }
    (*A)(i, i) = 1.5 * off + 1.0 + 0.125 * (i % 5);
    (*b)(i) = ((i * 13 + k) % 11 - 5) * 0.3;
    (*C)(i) = (i + k) % 3 != 0;
    (*lo)(i) = -0.02 * (1 + i % 3);
    (*hi)(i) = 0.03 * (1 + i % 4);
  }
}

typedef std::vector<VectorXd> (*BatchEq)(const std::vector<MatrixXd> &, const std::vector<VectorXd> &);
typedef std::vector<VectorXd> (*BatchMixed)(const std::vector<MatrixXd> &, const std::vector<VectorXd> &, const std::vector<ArrayXb> &,
                                            const std::vector<VectorXd> &, const std::vector<VectorXd> &);
typedef VectorXd (*SingleEq)(const MatrixXd &, const VectorXd &);
typedef VectorXd (*SingleMixed)(const MatrixXd &, const VectorXd &, const ArrayXb &, const VectorXd &, const VectorXd &);

void run(const char *method, BatchEq batch_eq, BatchMixed batch_mixed, SingleEq single_eq, SingleMixed single_mixed) {
  std::vector<MatrixXd> A(8);
  std::vector<VectorXd> b(8), lo(8), hi(8);
  std::vector<ArrayXb> C(8);
  for (int k = 0; k < 8; ++k) make(k, &A[k], &b[k], &C[k], &lo[k], &hi[k]);
  const std::vector<VectorXd> xe = batch_eq(A, b), xm = batch_mixed(A, b, C, lo, hi);
  for (int k = 0; k < 8; ++k) {
    print(method, "eq", "batch", k, xe[k]);
    print(method, "eq", "single", k, single_eq(A[k], b[k]));
    print(method, "mixed", "batch", k, xm[k]);
    print(method, "mixed", "single", k, single_mixed(A[k], b[k], C[k], lo[k], hi[k]));
  }
}

}  // namespace

int main() {
  try {
    run("jacobi", sparse::JacobiIterationBatch, sparse::JacobiIterationBatch, sparse::JacobiIteration, sparse::JacobiIteration);
    run("gs", sparse::GaussSeidelIterationBatch, sparse::GaussSeidelIterationBatch, sparse::GaussSeidelIteration, sparse::GaussSeidelIteration);
    run("sor", sparse::SORIterationBatch, sparse::SORIterationBatch, sparse::SORIteration, sparse::SORIteration);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "dense_iter_batch_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
