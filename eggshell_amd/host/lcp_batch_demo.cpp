// lcp_batch_demo -- lcp::SolveLCPBatch against a loop of lcp::SolveLCP on the same problems, for
// tests/test_gpu_adapter_lcp_batch.py.  Eight mixed box problems (lower triangles with a sentinel above them, some
// rows unbounded) are solved both ways under three Settings: the default (SolveLCP_BoxSchur), schur_complement =
// false with MURTY, and schur_complement = false with COTTLE_DANTZIG.  Every number is printed with 17 significant
// digits, one line per array: "<settings>_<batch|single><k>_<x|w|A|ok> values...".
#include <cstdio>
#include <vector>

#include "eggshell_api.h"

namespace {

const int kSizes[8] = {1, 6, 12, 20, 33, 48, 64, 96};

void print(const char *tag, const char *how, int k, const char *what, const double *v, size_t count) {
  std::printf("%s_%s%d_%s", tag, how, k, what);
  for (size_t i = 0; i < count; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

// k-th problem; all_bounded = every row keeps finite bounds (what schur_complement = false is about)
void make(int k, bool all_bounded, MatrixXd *A, VectorXd *b, VectorXd *lo, VectorXd *hi) {
  const int m = kSizes[k];
  MatrixXd M(m, m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) M(i, j) = ((i * 31 + j * 17 + (i * j) % 11 + 7 * k) % 23 - 11) / 11.0;
  A->resize(m, m); b->resize(m); lo->resize(m); hi->resize(m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      if (j > i) { (*A)(i, j) = 555.0; continue; }      // must be neither read nor written
      double s = 0.0;
      for (int r = 0; r < m; ++r) s += M(r, i) * M(r, j);
      (*A)(i, j) = s + (i == j ? 0.25 : 0.0);
    }
  for (int i = 0; i < m; ++i) {
    (*b)(i) = ((i * 13 + k) % 11 - 5) * 0.3;
    // problem 2 has no unbounded row, problem 5 no bounded one
    const bool bounded = all_bounded || k == 2 || (k != 5 && ((i + k) % 2 == 1 || i % 7 == 0));
    (*lo)(i) = bounded ? -0.05 * (1 + i % 3) : -__DBL_MAX__;
    (*hi)(i) = bounded ? 0.04 * (1 + i % 4) : __DBL_MAX__;
  }
}

void run(const char *tag, const lcp::Settings &settings, bool all_bounded) {
  std::vector<MatrixXd> A(8);
  std::vector<VectorXd> b(8), lo(8), hi(8), x, w;
  for (int k = 0; k < 8; ++k) make(k, all_bounded, &A[k], &b[k], &lo[k], &hi[k]);
  std::vector<MatrixXd> A1 = A;
  const std::vector<bool> ok = lcp::SolveLCPBatch(settings, &A, b, lo, hi, &x, &w);
  for (int k = 0; k < 8; ++k) {
    const int m = kSizes[k];
    const double okd = ok[k] ? 1.0 : 0.0;
    print(tag, "batch", k, "ok", &okd, 1);
    print(tag, "batch", k, "x", x[k].data(), m);
    print(tag, "batch", k, "w", w[k].data(), m);
    print(tag, "batch", k, "A", A[k].data(), (size_t)m * m);
    VectorXd xs, ws;
    const double ok1 = lcp::SolveLCP(settings, A1[k], b[k], lo[k], hi[k], &xs, &ws) ? 1.0 : 0.0;
    print(tag, "single", k, "ok", &ok1, 1);
    print(tag, "single", k, "x", xs.data(), m);
    print(tag, "single", k, "w", ws.data(), m);
    print(tag, "single", k, "A", A1[k].data(), (size_t)m * m);
  }
}

}  // namespace

int main() {
  try {
    lcp::Settings def;
    run("default", def, false);
    lcp::Settings murty;
    murty.schur_complement = false;
    run("noschur", murty, true);
    lcp::Settings dantzig;
    dantzig.schur_complement = false;
    dantzig.algorithm = lcp::COTTLE_DANTZIG;
    run("dantzig", dantzig, true);
    // the two refusals of toolkit/lcp.cc:762-784 hold for the batch as for the single call
    int refused[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
      lcp::Settings bad;
      bad.box_lcp = false;
      bad.schur_complement = pass == 0;
      bad.algorithm = lcp::COTTLE_DANTZIG;
      std::vector<MatrixXd> A(1);
      std::vector<VectorXd> b(1), lo(1), hi(1), x, w;
      make(1, true, &A[0], &b[0], &lo[0], &hi[0]);
      try { (void)lcp::SolveLCPBatch(bad, &A, b, lo, hi, &x, &w); } catch (const egs::Error &e) { refused[pass] = e.status; }
    }
    std::printf("refused %d %d\n", refused[0], refused[1]);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "lcp_batch_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
