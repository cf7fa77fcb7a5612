// dense_iter.hip -- the reference's projected iterations on an EXPLICIT dense matrix:
//   sparse::{Jacobi,GaussSeidel,SOR}Iteration(const MatrixXd& A, const VectorXd& b[, C, x_lo, x_hi])
//       sparse_iterations.h:13-24, sparse_iterations.cc:72-144 (BaseIteration), :35-49 (GetResidualError)
//   sparse::MatrixSolveDiagonal / MatrixSolveLowerTriangle / MatrixSolveUpperTriangle (the dense twins)
//       sparse_iterations_utils.cc:25-40, 110-128, 245-262; ApplyProjection :12-21
// These are the solvers the reference's own unit tests run on random 3..50-row matrices (sparse_iterations.cc:355-513);
// the ensemble path uses the matrix-free twins (step_solve.hip and friends).  One workgroup does the whole solve --
// x0 = b, then sweep / residual / stopping test until err <= tol or max_iters sweeps, as the reference's loop -- with
// every vector in LDS and one read-back for the caller.  A sweep is a chain of n dependent scalar updates; rows work in
// parallel wherever the reference's summation order allows it:
//   * N x + b: a thread per row, the row's products in increasing column order;
//   * forward solve (Gauss-Seidel): column by column -- thread j finishes x_j, every thread i > j adds L(i,j) x_j to its
//     running sum, which is the reference's `substitutions += L(i, j) * x(j)` order, j increasing;
//   * backward solve (SOR): the reference sums U(i, j) x(j) for j = i + 1 .. n - 1 in INCREASING j, i.e. starting with the
//     value that was finished last, so row i's sum cannot start before x_{i+1} is known: thread i runs it when its turn
//     comes (n^2 / 2 dependent multiply-adds per sweep; fine at the reference's sizes);
//   * residual: w = A x - b a thread per row; the four partial sums of squares in index order by one thread, so that the
//     stopping test sees the bits the sequential code sees (oracle/dense_iter.c) and stops at the same sweep.
// The batch form (dense_iterate_batch) runs many such systems in one pipeline, a workgroup per problem and nothing shared
// between workgroups.  A problem of up to 96 rows (kDantzigMaxRows, the fused limit of the LCP batch entries) is one
// wavefront with the matrix in LDS (dense_iterate_small_kernel below); a larger one is the single call's workgroup,
// unchanged (dense_iterate_body, shared by both kernels).  The summation orders above bind every one of them.
// Not restated: the spectral-radius gate of :113-121 (EigenSolver; the reference Panics when rho(M^-1 N) >= 1): a
// splitting that does not converge runs to max_iters and reports its residual.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "dense_lcp.h"
#include "packed_block.h"
#include "runtime.h"

namespace egs {

namespace {

constexpr int kDenseIterMax = 1024;

__device__ __forceinline__ double dproj(double x, bool is_eq, double lo, double hi) {   // sparse_iterations_utils.cc:12-21
  if (is_eq) return x;
  if (x < lo) return lo;
  if (x > hi) return hi;
  return x;
}

struct DenseIterOut { double residual; int32_t iterations, pad; };

// The whole solve of one system by one 1024-thread workgroup, the matrix in device memory.  hist (may be NULL):
// [max_iters + 1], entry s = the error after sweep s, entry 0 that of x0 = b; entries the loop does not reach are NaN.
__device__ __forceinline__ void dense_iterate_body(int n, const double *A, const double *b, const uint8_t *C, const double *lo,
                                                   const double *hi, int method, double ksor, int max_iters, double tol,
                                                   double *x_out, DenseIterOut *out, double *hist) {
  __shared__ double x[kDenseIterMax], xn[kDenseIterMax], rhs[kDenseIterMax], w[kDenseIterMax];
  __shared__ double s_err;
  const int tid = threadIdx.x;
  auto residual = [&]() {           // sparse_iterations.cc:35-49
    for (int i = tid; i < n; i += 1024) {
      double t = 0.0;
      const double *row = A + (size_t)i * n;
      for (int j = 0; j < n; ++j) t = t + row[j] * x[j];
      w[i] = t - b[i];
    }
    __syncthreads();
    if (tid == 0) {
      double s_eq = 0.0, s_lo = 0.0, s_hi = 0.0, s_in = 0.0;
      for (int i = 0; i < n; ++i) {
        const double wi = w[i], xi = x[i];
        if (C[i]) s_eq += wi * wi;
        else {
          if (xi == lo[i] && wi < 0) s_lo += wi * wi;
          if (xi == hi[i] && wi > 0) s_hi += wi * wi;
          if (xi > lo[i] && xi < hi[i]) s_in += wi * wi;
        }
      }
      s_err = sqrt(s_eq) + (sqrt(s_lo) + sqrt(s_hi) + sqrt(s_in));
    }
    __syncthreads();
    return s_err;
  };
  for (int i = tid; i < n; i += 1024) x[i] = b[i];          // x0 = b (:124)
  __syncthreads();
  double err = residual();
  int it = 0;
  if (hist && tid == 0) hist[0] = err;
  while (err > tol && it < max_iters) {
    for (int i = tid; i < n; i += 1024) {                     // rhs = N x + b (:130)
      const double *row = A + (size_t)i * n;
      double t = 0.0;
      if (method == 0) { for (int j = 0; j < n; ++j) if (j != i) t = t + (-row[j]) * x[j]; }
      else if (method == 1) { for (int j = i + 1; j < n; ++j) t = t + (-row[j]) * x[j]; }
      else {
        for (int j = 0; j < i; ++j) t = t + (-row[j]) * x[j];
        t = t + ((ksor - 1.0) * row[i]) * x[i];
      }
      rhs[i] = t + b[i];
      w[i] = 0.0;                                             // running substitution sums of the forward solve
    }
    __syncthreads();
    if (method == 0) {                                        // MatrixSolveDiagonal (utils :25-40)
      for (int i = tid; i < n; i += 1024) xn[i] = dproj(1.0 / A[(size_t)i * n + i] * rhs[i], C[i] != 0, lo[i], hi[i]);
      __syncthreads();
    } else if (method == 1) {                                 // MatrixSolveLowerTriangle (utils :110-128), column by column
      for (int j = 0; j < n; ++j) {
        if (tid == 0) xn[j] = dproj((rhs[j] - w[j]) / A[(size_t)j * n + j], C[j] != 0, lo[j], hi[j]);
        __syncthreads();
        const double xj = xn[j];
        for (int i = j + 1 + tid; i < n; i += 1024) w[i] += A[(size_t)i * n + j] * xj;
        __syncthreads();
      }
    } else {                                                  // MatrixSolveUpperTriangle (utils :245-262)
      for (int i = n - 1; i >= 0; --i) {
        if (tid == 0) {
          double sub = 0.0;
          const double *row = A + (size_t)i * n;
          for (int j = i + 1; j < n; ++j) sub += row[j] * xn[j];
          xn[i] = dproj((rhs[i] - sub) / (ksor * row[i]), C[i] != 0, lo[i], hi[i]);
        }
        __syncthreads();
      }
    }
    for (int i = tid; i < n; i += 1024) x[i] = xn[i];
    __syncthreads();
    err = residual();
    ++it;
    if (hist && tid == 0) hist[it] = err;
  }
  for (int i = tid; i < n; i += 1024) x_out[i] = x[i];
  if (hist) for (int s = it + 1 + tid; s <= max_iters; s += 1024) hist[s] = __builtin_nan("");
  if (tid == 0) { out->residual = err; out->iterations = it; out->pad = 0; }
}

__global__ void __launch_bounds__(1024) dense_iterate_kernel(int n, const double *A, const double *b, const uint8_t *C, const double *lo,
                                                             const double *hi, int method, double ksor, int max_iters, double tol,
                                                             double *x_out, DenseIterOut *out) {
  dense_iterate_body(n, A, b, C, lo, hi, method, ksor, max_iters, tol, x_out, out, nullptr);
}

// ---- the batch: a workgroup per problem ---------------------------------------------------------------------------

constexpr int kDenseIterSmall = kDantzigMaxRows;   // 96: up to here one wavefront with the matrix in LDS

struct DenseIterProblem { int64_t a_off, v_off; int32_t n, pad; };   // offsets in doubles into A resp. the vectors; a_off is even
struct DenseIterSet {
  const DenseIterProblem *prob;   // [count]
  const int32_t *sel;             // the launch's problems: workgroup g solves problem sel[g]
  const double *A, *b, *lo, *hi;
  const uint8_t *C;
  double *x;
  DenseIterOut *out;              // [count]
  double *hist;                   // [count][max_iters + 1] or NULL
  int method, max_iters;
  double ksor, tol;
};

__global__ void __launch_bounds__(1024) dense_iterate_medium_kernel(DenseIterSet S) {
  const int k = S.sel[blockIdx.x];
  const DenseIterProblem P = S.prob[k];
  dense_iterate_body(P.n, S.A + P.a_off, S.b + P.v_off, S.C + P.v_off, S.lo + P.v_off, S.hi + P.v_off, S.method, S.ksor, S.max_iters,
                     S.tol, S.x + P.v_off, S.out + k, S.hist ? S.hist + (size_t)k * ((size_t)S.max_iters + 1) : nullptr);
}

// the value lane `lane` (wave-uniform) holds, in every lane
__device__ __forceinline__ double lane_value(double v, int lane) {
  const int l = __builtin_amdgcn_readlane(__double2loint(v), lane), h = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(h, l);
}

// n <= 96: one wavefront.  Lane t owns rows t and t + 64 and keeps what only those rows touch (b, lo, hi, C, the diagonal,
// rhs, the running sums of the solves and its entries of x) in registers; the matrix, copied once, and x, which every
// row reads, are in LDS, and between that copy and the final store of x global memory sees one history entry per sweep.
// Rows work side by side wherever the orders at the top of this file allow it:
//   * the row sums of N x + b and of A x - b: lane = row, the columns in increasing order, x_j one broadcast read;
//   * forward solve: column by column -- the owner of row j finishes x_j, a readlane hands it to every lane, and each
//     row i > j adds L(i, j) x_j to its running sum (register to register, no LDS round trip on the dependent chain);
//   * backward solve: row i's sum starts with the value finished last, so only the products U(i, j) x_j are made side by
//     side (lane = column) and the additions run in increasing j on readlanes of them;
//   * the four sums of squares: every lane squares its w, ballots say which sum a row belongs to, and the sums run over
//     the rows in index order on readlanes; a row outside a sum adds +0.0, which leaves a sum of squares as it is.
// Row stride in LDS: n | 1 doubles, the smallest odd number >= n.  The matrix is only ever read by ds_read_b64 with
// lane = row at one column (both row sums and the forward solve's column walk have that shape) or lane = column at one
// row.  ds_read_b64 serves 32 lanes per cycle and the bank of byte address a is (a / 4) mod 64, so a double sits on
// bank pair (index mod 32): 32 consecutive rows at stride s are conflict-free exactly when i -> i s mod 32 is one to
// one, i.e. when s is odd (an even n would put rows i and i + 32 / gcd(n, 32) on one pair: 32-way at n = 96 or 64,
// 8-way at n = 24).  32 consecutive columns of one row are conflict-free at any stride.  96 rows: 96 x 97 x 8 B + x =
// 75 264 B, two workgroups per CU.
__global__ void __launch_bounds__(64) dense_iterate_small_kernel(DenseIterSet S) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int k = S.sel[blockIdx.x];
  const DenseIterProblem P = S.prob[k];
  const int n = P.n, stride = n | 1, n0 = n < 64 ? n : 64, method = S.method, max_iters = S.max_iters;
  const double ksor = S.ksor, tol = S.tol;
  double *Am = lds, *xs = lds + n * stride;
  {                                                             // the matrix, 16 bytes per lane and load
    const double *Ag = S.A + P.a_off;
    const double2 *A2 = reinterpret_cast<const double2 *>(Ag);
    const int nn = n * n;
    for (int e = tid; e < nn / 2; e += 64) {
      const double2 v = A2[e];
      const int ra = (2 * e) / n, rb = (2 * e + 1) / n;
      Am[ra * stride + (2 * e - ra * n)] = v.x;
      Am[rb * stride + (2 * e + 1 - rb * n)] = v.y;
    }
    if ((nn & 1) && tid == 0) Am[(n - 1) * stride + (n - 1)] = Ag[nn - 1];
  }
  const int r0 = tid, r1 = tid + 64;
  const bool have0 = r0 < n, have1 = r1 < n;
  const int c0 = have0 ? r0 : 0, c1 = have1 ? r1 : 0;          // a lane without a row reads row / column 0 and drops the result
  const double *row0 = Am + c0 * stride, *row1 = Am + c1 * stride;
  const double *bg = S.b + P.v_off, *log = S.lo + P.v_off, *hig = S.hi + P.v_off;
  const uint8_t *Cg = S.C + P.v_off;
  const double b0 = have0 ? bg[r0] : 0.0, b1 = have1 ? bg[r1] : 0.0;
  const double lo0 = have0 ? log[r0] : 0.0, lo1 = have1 ? log[r1] : 0.0;
  const double hi0 = have0 ? hig[r0] : 0.0, hi1 = have1 ? hig[r1] : 0.0;
  const bool eq0 = have0 ? Cg[r0] != 0 : true, eq1 = have1 ? Cg[r1] != 0 : true;
  double x0 = b0, x1 = b1;                                      // x0 = b (:124)
  if (have0) xs[r0] = x0;
  if (have1) xs[r1] = x1;
  __syncthreads();
  const double d0 = have0 ? row0[r0] : 1.0, d1 = have1 ? row1[r1] : 1.0;
  auto residual = [&]() -> double {                             // sparse_iterations.cc:35-49, of the x in x0 / x1 and xs
    double t0 = 0.0, t1 = 0.0;
    for (int j = 0; j < n; ++j) {
      const double xj = xs[j];
      t0 = t0 + row0[j] * xj;
      t1 = t1 + row1[j] * xj;
    }
    const double w0 = t0 - b0, w1 = t1 - b1;
    const double q0 = w0 * w0, q1 = w1 * w1;
    const unsigned long long m_eq0 = __ballot(have0 && eq0), m_eq1 = __ballot(have1 && eq1);
    const unsigned long long m_lo0 = __ballot(have0 && !eq0 && x0 == lo0 && w0 < 0), m_lo1 = __ballot(have1 && !eq1 && x1 == lo1 && w1 < 0);
    const unsigned long long m_hi0 = __ballot(have0 && !eq0 && x0 == hi0 && w0 > 0), m_hi1 = __ballot(have1 && !eq1 && x1 == hi1 && w1 > 0);
    const unsigned long long m_in0 = __ballot(have0 && !eq0 && x0 > lo0 && x0 < hi0), m_in1 = __ballot(have1 && !eq1 && x1 > lo1 && x1 < hi1);
    double s_eq = 0.0, s_lo = 0.0, s_hi = 0.0, s_in = 0.0;
    for (int i = 0; i < n0; ++i) {
      const double q = lane_value(q0, i);
      s_eq += (m_eq0 >> i & 1) ? q : 0.0;
      s_lo += (m_lo0 >> i & 1) ? q : 0.0;
      s_hi += (m_hi0 >> i & 1) ? q : 0.0;
      s_in += (m_in0 >> i & 1) ? q : 0.0;
    }
    for (int i = 64; i < n; ++i) {
      const double q = lane_value(q1, i - 64);
      s_eq += (m_eq1 >> (i - 64) & 1) ? q : 0.0;
      s_lo += (m_lo1 >> (i - 64) & 1) ? q : 0.0;
      s_hi += (m_hi1 >> (i - 64) & 1) ? q : 0.0;
      s_in += (m_in1 >> (i - 64) & 1) ? q : 0.0;
    }
    return sqrt(s_eq) + (sqrt(s_lo) + sqrt(s_hi) + sqrt(s_in));
  };
  double *hist = S.hist ? S.hist + (size_t)k * ((size_t)max_iters + 1) : nullptr;
  double err = residual();
  int it = 0;
  if (hist && tid == 0) hist[0] = err;
  while (err > tol && it < max_iters) {
    double t0 = 0.0, t1 = 0.0;                                  // rhs = N x + b (:130)
    if (method == 0) {
      for (int j = 0; j < n; ++j) {
        const double xj = xs[j];
        if (j != r0) t0 = t0 + (-row0[j]) * xj;
        if (j != r1) t1 = t1 + (-row1[j]) * xj;
      }
    } else if (method == 1) {
      for (int j = 1; j < n; ++j) {
        const double xj = xs[j];
        if (j > r0) t0 = t0 + (-row0[j]) * xj;
        if (j > r1) t1 = t1 + (-row1[j]) * xj;
      }
    } else {
      for (int j = 0; j < n - 1; ++j) {
        const double xj = xs[j];
        if (j < r0) t0 = t0 + (-row0[j]) * xj;
        if (j < r1) t1 = t1 + (-row1[j]) * xj;
      }
      t0 = t0 + ((ksor - 1.0) * d0) * x0;
      t1 = t1 + ((ksor - 1.0) * d1) * x1;
    }
    const double rhs0 = t0 + b0, rhs1 = t1 + b1;
    double xn0 = 0.0, xn1 = 0.0;
    if (method == 0) {                                          // MatrixSolveDiagonal (utils :25-40)
      xn0 = dproj(1.0 / d0 * rhs0, eq0, lo0, hi0);
      xn1 = dproj(1.0 / d1 * rhs1, eq1, lo1, hi1);
    } else if (method == 1) {                                   // MatrixSolveLowerTriangle (utils :110-128), column by column
      double w0 = 0.0, w1 = 0.0;
      for (int j = 0; j < n0; ++j) {
        const double xj = lane_value(dproj((rhs0 - w0) / d0, eq0, lo0, hi0), j);
        if (tid == j) xn0 = xj;
        if (r0 > j) w0 += row0[j] * xj;
        w1 += row1[j] * xj;
      }
      for (int j = 64; j < n; ++j) {
        const double xj = lane_value(dproj((rhs1 - w1) / d1, eq1, lo1, hi1), j - 64);
        if (tid == j - 64) xn1 = xj;
        if (r1 > j) w1 += row1[j] * xj;
      }
    } else {                                                    // MatrixSolveUpperTriangle (utils :245-262)
      for (int i = n - 1; i >= 0; --i) {
        const double *rowi = Am + i * stride;
        const double p0 = rowi[c0] * xn0, p1 = rowi[c1] * xn1;  // lane = column; only columns > i are summed
        double sub = 0.0;
        for (int j = i + 1; j < n0; ++j) sub += lane_value(p0, j);
        for (int j = i + 1 > 64 ? i + 1 : 64; j < n; ++j) sub += lane_value(p1, j - 64);
        if (i >= 64) {
          if (tid == i - 64) xn1 = dproj((rhs1 - sub) / (ksor * d1), eq1, lo1, hi1);
        } else {
          if (tid == i) xn0 = dproj((rhs0 - sub) / (ksor * d0), eq0, lo0, hi0);
        }
      }
    }
    x0 = xn0; x1 = xn1;
    __syncthreads();                                            // every read of the old x is done
    if (have0) xs[r0] = x0;
    if (have1) xs[r1] = x1;
    __syncthreads();
    err = residual();
    ++it;
    if (hist && tid == 0) hist[it] = err;
  }
  double *xg = S.x + P.v_off;
  if (have0) xg[r0] = x0;
  if (have1) xg[r1] = x1;
  if (hist) for (int s = it + 1 + tid; s <= max_iters; s += 64) hist[s] = __builtin_nan("");
  if (tid == 0) { S.out[k].residual = err; S.out[k].iterations = it; S.out[k].pad = 0; }
}

size_t small_lds_bytes(int n) { return ((size_t)n * (n | 1) + n) * sizeof(double); }

}  // namespace

void dense_iterate(hipStream_t s, int n, const double *A, const double *b, const uint8_t *C, const double *lo, const double *hi,
                   int method, double omega, int max_iters, double tol, double *x, int *iterations, double *residual) {
  if (n < 0 || n > kDenseIterMax) throw std::invalid_argument("dense iteration: 0 <= n <= 1024");
  if (method < 0 || method > 2) throw std::invalid_argument("dense iteration: method 0 (Jacobi), 1 (Gauss-Seidel) or 2 (SOR)");
  if (!(omega > 0.0 && omega < 2.0)) throw std::invalid_argument("dense iteration: 0 < omega < 2");
  if (iterations) *iterations = 0;
  if (residual) *residual = 0.0;
  if (n == 0) return;                      // sparse_iterations.cc:79-81
  for (int i = 0; i < n; ++i)
    if (A[(size_t)i * n + i] == 0.0) throw std::invalid_argument("dense iteration: zero on the diagonal (the reference CHECKs det != 0)");
  ScopedDevBuf<double> dA((size_t)n * n), dv(4 * (size_t)n);
  ScopedDevBuf<uint8_t> dC(n);
  ScopedDevBuf<DenseIterOut> dout(1);
  double *db = dv.p, *dlo = dv.p + n, *dhi = dv.p + 2 * n, *dx = dv.p + 3 * n;
  HIPCHK(hipMemcpyAsync(dA.p, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(db, b, n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dlo, lo, n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dhi, hi, n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dC.p, C, (size_t)n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(dense_iterate_kernel, dim3(1), dim3(1024), 0, s, n, dA.p, db, dC.p, dlo, dhi, method, 1.0 / omega, max_iters, tol, dx, dout.p);
  HIPCHK(hipGetLastError());
  DenseIterOut o{};
  HIPCHK(hipMemcpyAsync(x, dx, n * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&o, dout.p, sizeof o, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (iterations) *iterations = o.iterations;
  if (residual) *residual = o.residual;
}

void dense_iterate_batch(hipStream_t s, const LaunchHooks &hooks, int count, const int32_t *n, const double *A, const double *b,
                         const uint8_t *C, const double *lo, const double *hi, int method, double omega, int max_iters, double tol,
                         double *x, int32_t *iterations, double *residual, double *history) {
  // everything is checked before anything is launched or written
  if (count < 0) throw std::invalid_argument("dense iteration batch: count < 0");
  if (method < 0 || method > 2) throw std::invalid_argument("dense iteration: method 0 (Jacobi), 1 (Gauss-Seidel) or 2 (SOR)");
  if (!(omega > 0.0 && omega < 2.0)) throw std::invalid_argument("dense iteration: 0 < omega < 2");
  if (max_iters < 0) throw std::invalid_argument("dense iteration: max_iters < 0");
  size_t at = 0, vt = 0, dat = 0;      // doubles of A as the caller packs them, rows, doubles of A with every matrix at an even offset
  int n_small_max = 0;
  std::vector<int32_t> small, medium;
  for (int k = 0; k < count; ++k) {
    const int nk = n[k];
    if (nk < 0 || nk > kDenseIterMax) throw std::invalid_argument("dense iteration batch: 0 <= n <= 1024, problem " + std::to_string(k));
    for (int i = 0; i < nk; ++i)
      if (A[at + (size_t)i * nk + i] == 0.0)
        throw std::invalid_argument("dense iteration batch: zero on the diagonal of problem " + std::to_string(k) + " (the reference CHECKs det != 0)");
    if (nk > kDenseIterSmall) medium.push_back(k);
    else if (nk > 0) { small.push_back(k); n_small_max = std::max(n_small_max, nk); }
    at += (size_t)nk * nk; vt += nk; dat += ((size_t)nk * nk + 1) & ~size_t(1);
  }
  if (count == 0) return;
  const size_t hlen = (size_t)max_iters + 1, nsel = small.size() + medium.size();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (nsel == 0) {                      // sparse_iterations.cc:79-81, every problem
    for (int k = 0; k < count; ++k) {
      if (iterations) iterations[k] = 0;
      if (residual) residual[k] = 0.0;
      if (history) { std::fill(history + k * hlen, history + (k + 1) * hlen, nan); history[k * hlen] = 0.0; }
    }
    return;
  }
  // one packed block, the same layout on both sides (packed_block.h).  read back: x out [hist]; uploaded: A b lo hi
  // prob sel C.  Every problem of the call is in it, in the caller's order, so only A (padded below) is copied piecewise.
  const size_t nc = (size_t)count;
  PackedBlock blk;
  const auto s_x = blk.add<double>(Zone::Download, vt);
  const auto s_out = blk.add<DenseIterOut>(Zone::Download, nc);
  const auto s_hist = blk.add<double>(Zone::Download, history ? nc * hlen : 0);
  const auto s_A = blk.add<double>(Zone::Upload, dat, 16), s_b = blk.add<double>(Zone::Upload, vt), s_lo = blk.add<double>(Zone::Upload, vt),
             s_hi = blk.add<double>(Zone::Upload, vt);
  const auto s_prob = blk.add<DenseIterProblem>(Zone::Upload, nc);
  const auto s_sel = blk.add<int32_t>(Zone::Upload, nsel);
  const auto s_C = blk.add<uint8_t>(Zone::Upload, vt);
  char *h = static_cast<char *>(hooks.take(hooks.self, blk.host_bytes()));
  ScopedDevBuf<char> d(blk.total_bytes());
  blk.bind(h, d.p);
  double *hA = blk.host(s_A), *hb = blk.host(s_b), *hlo = blk.host(s_lo), *hhi = blk.host(s_hi);
  DenseIterProblem *hprob = blk.host(s_prob);
  int32_t *hsel = blk.host(s_sel);
  uint8_t *hC = blk.host(s_C);
  size_t ap = 0, vp = 0, dp = 0;
  for (int k = 0; k < count; ++k) {
    const size_t nk = (size_t)n[k];
    if (nk) std::memcpy(hA + dp, A + ap, nk * nk * sizeof(double));
    if ((nk * nk) & 1) hA[dp + nk * nk] = 0.0;
    hprob[k] = DenseIterProblem{(int64_t)dp, (int64_t)vp, (int32_t)nk, 0};
    ap += nk * nk; vp += nk; dp += (nk * nk + 1) & ~size_t(1);
  }
  if (vt) {
    std::memcpy(hb, b, vt * sizeof(double));
    if (C) { std::memcpy(hlo, lo, vt * sizeof(double)); std::memcpy(hhi, hi, vt * sizeof(double)); std::memcpy(hC, C, vt); }
    else { std::memset(hlo, 0, vt * sizeof(double)); std::memset(hhi, 0, vt * sizeof(double)); std::memset(hC, 1, vt); }   // sparse_iterations.cc:229-233
  }
  std::copy(small.begin(), small.end(), hsel);
  std::copy(medium.begin(), medium.end(), hsel + small.size());
  HIPCHK(hipMemcpyAsync(d.p + blk.upload_begin(), h + blk.upload_begin(), blk.upload_end() - blk.upload_begin(), hipMemcpyHostToDevice, s));
  DenseIterSet S{};
  S.prob = blk.device(s_prob);
  S.A = blk.device(s_A); S.b = blk.device(s_b); S.lo = blk.device(s_lo); S.hi = blk.device(s_hi);
  S.C = blk.device(s_C);
  S.x = blk.device(s_x); S.out = blk.device(s_out);
  S.hist = history ? blk.device(s_hist) : nullptr;
  S.method = method; S.max_iters = max_iters; S.ksor = 1.0 / omega; S.tol = tol;
  if (hooks.mark) hooks.mark(hooks.self, true);
  if (!small.empty()) {
    const size_t lds = small_lds_bytes(n_small_max);
    if (lds > 48 * 1024)
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(dense_iterate_small_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    S.sel = blk.device(s_sel);
    hipLaunchKernelGGL(dense_iterate_small_kernel, dim3((unsigned)small.size()), dim3(64), lds, s, S);
    HIPCHK(hipGetLastError());
  }
  if (!medium.empty()) {
    S.sel = blk.device(s_sel) + small.size();
    hipLaunchKernelGGL(dense_iterate_medium_kernel, dim3((unsigned)medium.size()), dim3(1024), 0, s, S);
    HIPCHK(hipGetLastError());
  }
  if (hooks.mark) hooks.mark(hooks.self, false);
  HIPCHK(hipMemcpyAsync(h, d.p, blk.download_bytes(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (vt) std::memcpy(x, blk.host(s_x), vt * sizeof(double));
  const DenseIterOut *hout = blk.host(s_out);
  const double *hh = blk.host(s_hist);
  for (int k = 0; k < count; ++k) {
    const bool ran = n[k] > 0;          // a problem without rows was not launched (sparse_iterations.cc:79-81)
    if (iterations) iterations[k] = ran ? hout[k].iterations : 0;
    if (residual) residual[k] = ran ? hout[k].residual : 0.0;
    if (!history) continue;
    if (ran) std::memcpy(history + k * hlen, hh + k * hlen, hlen * sizeof(double));
    else { std::fill(history + k * hlen, history + (k + 1) * hlen, nan); history[k * hlen] = 0.0; }
  }
}

}  // namespace egs
