// mixed_batch_demo -- Lcp::MixedConstraintsSolverBatch against a loop of Lcp::MixedConstraintsSolver on the same
// problems, for tests/test_gpu_adapter_mixed_batch.py.  Eight problems (1, 6, 12, 20, 33, 48, 64 and 96 rows; symmetric
// positive definite and strictly diagonally dominant, mixed equality / inequality rows) are solved once as a batch and
// once as eight calls.  Every number is printed with 17 significant digits, one line per vector:
// "<x|w|ok>_<batch|single><k> values...".
#include <cstdio>
#include <limits>
#include <vector>

#include "eggshell_api.h"

namespace {

const int kSizes[8] = {1, 6, 12, 20, 33, 48, 64, 96};

void print(const char *what, const char *how, int k, const VectorXd &v) {
  std::printf("%s_%s%d", what, how, k);
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
    (*lo)(i) = 0.0;
    (*hi)(i) = std::numeric_limits<double>::infinity();
  }
}

}  // namespace

int main() {
  try {
    std::vector<MatrixXd> A(8);
    std::vector<VectorXd> b(8), lo(8), hi(8), x, w;
    std::vector<ArrayXb> C(8);
    for (int k = 0; k < 8; ++k) make(k, &A[k], &b[k], &C[k], &lo[k], &hi[k]);
    const std::vector<bool> ok = Lcp::MixedConstraintsSolverBatch(A, b, C, lo, hi, &x, &w);
    for (int k = 0; k < 8; ++k) {
      VectorXd xs, ws;
      const bool oks = Lcp::MixedConstraintsSolver(A[k], b[k], C[k], lo[k], hi[k], xs, ws);
      print("x", "batch", k, x[k]);
      print("w", "batch", k, w[k]);
      std::printf("ok_batch%d %d\n", k, ok[k] ? 1 : 0);
      print("x", "single", k, xs);
      print("w", "single", k, ws);
      std::printf("ok_single%d %d\n", k, oks ? 1 : 0);
    }
    // a mismatched argument is refused
    int refused = 0;
    std::vector<VectorXd> b7(b.begin(), b.begin() + 7);
    try { (void)Lcp::MixedConstraintsSolverBatch(A, b7, C, lo, hi, &x, &w); } catch (const egs::Error &e) { refused = e.status; }
    std::printf("refused %d\n", refused);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "mixed_batch_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
