// dense_lcp.h -- dense direct LCP on the GPU (entry 3 of the C ABI):
// Lcp::MixedConstraintsSolver + Lcp::MurtyPrincipalPivot, eggshell/lcp.cc:141-336.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace egs {

// The scratch, pinned records and side stream of the entries below that need any, and the stream they enqueue on
// (runtime.h): a context owns one.  The pure-Dantzig entries and dense_iterate need none and take the stream itself.
struct DenseWorkspace;

// A [N][N] row-major symmetric, b, C, lo, hi [N] on the host; x, w [N] out.
// use_bounds = false reproduces the reference (Murty on [0, inf), quirk Q3).
// block_pivoting = true replaces the reference's single-index rule by block
// principal pivoting (same solution, far fewer factorisations, no 1000-pivot cap).
// Returns the reference's bool; *pivots = number of principal pivots (solves).
// Throws std::invalid_argument for a bad argument and egs::HipError (runtime.h) for a failed HIP call, as every entry here.
// max_pivots > 0 / max_seconds > 0: give up (return false) after that many principal pivots / that
// much wall time (lcp::Settings::max_iterations, max_time; toolkit/lcp.h:161-167).
bool dense_mixed_constraints(DenseWorkspace &ws, int N, const double *A, const double *b, const uint8_t *C,
                             const double *lo, const double *hi, bool use_bounds, bool block_pivoting, double *x,
                             double *w, int *pivots, std::string *msg, int max_pivots = 0, double max_seconds = 0.0);
// The same with A (row-major, symmetric: the lower triangle is read) and b already on the device.
// x / w (host, [N]) may be NULL; dx_out (device, [N]) receives the solution if not NULL.
bool dense_mixed_constraints_device(DenseWorkspace &ws, int N, const double *dA, const double *db, const uint8_t *C,
                                    const double *lo, const double *hi, bool use_bounds, bool block_pivoting,
                                    int max_pivots, double max_seconds, double *x, double *w, double *dx_out,
                                    int *pivots, std::string *msg);
// 2-norm condition number of a symmetric positive definite device matrix, what the reference gets from a JacobiSVD
// (utils.cc:256-261): lambda_max by power iteration on A times 1 / lambda_min by inverse iteration with the blocked
// Cholesky factor (N <= 1024; 60 iterations each, accurate to a few per cent unless the extreme eigenvalues are
// clustered, and never above the true value).  *pivot_bound (may be NULL) = (max L_ii / min L_ii)^2, the cheap lower
// bound, which is also what is returned beyond 1024 rows.  *spd = false (and +inf) if the factorisation breaks down.
double dense_condition_estimate(DenseWorkspace &ws, int N, const double *dA, bool *spd, double *pivot_bound = nullptr);

// lcp::SolveLCP_BoxDantzig / SolveLCP_BoxMurty with the incremental Cholesky factor of toolkit/lcp.cc (dantzig.hip):
// one workgroup per problem.  n <= kDantzigMaxRows: one wavefront, everything in LDS; up to kIncrementalMaxRows:
// four wavefronts, the matrices in global memory.  A (host, row-major n x n; only the lower triangle is read) is
// permuted in place as the reference leaves it (lower triangle written back); perm[k] = original index of final row
// k (may be NULL).  Needs lo <= 0 <= hi (and lo < hi for Dantzig, toolkit/lcp.cc:448-450).
// algorithm 1 = SolveLCP_BoxDantzig (:444-619), 0 = SolveLCP_BoxMurty on a LinearReducer (:213-328, 380-442; with
// lo = 0, hi = +inf it is SolveLCP_Murty, :333-378).  max_steps > 0 = Settings::max_iterations, else 20 n + 1000;
// max_seconds > 0 = Settings::max_time.
constexpr int kDantzigMaxRows = 96;
constexpr int kIncrementalMaxRows = 1024;
bool box_lcp_incremental(hipStream_t stream, int algorithm, int n, double *A, const double *b, const double *lo, const double *hi,
                         double *x, double *w, int32_t *perm, int max_steps, double max_seconds, int *pivots, std::string *msg);
// `count` problems in one launch: problem k's matrix at A + sum_{j<k} n_j^2, its vectors at sum_{j<k} n_j.
// ok / pivots / reason [count] (reason: 0 solved, 1 step limit, 2 non-positive pivot, 3 time limit; may be NULL).
void box_lcp_incremental_batch(hipStream_t stream, int algorithm, int count, const int32_t *n, double *A, const double *b,
                               const double *lo, const double *hi, int max_steps, double max_seconds, double *x, double *w,
                               int32_t *perm, int32_t *ok, int32_t *pivots, int32_t *reason);
// One problem that lives on the device (dA n x n contiguous, permuted in place; dx / dw out); h_lo / h_hi = host
// copies of the bounds for the precondition check.
bool box_lcp_incremental_device(hipStream_t stream, int algorithm, int n, double *dA, const double *db, const double *dlo,
                                const double *dhi, const double *h_lo, const double *h_hi, int max_steps, double max_seconds,
                                double *dx, double *dw, int *pivots, std::string *msg);

// lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747): the two-pointer partition that brings the unbounded rows to the
// front (A's lower triangle permuted in place, perm[k] = original index of row k, *nub_out = their number), Z = L L',
// the Schur complement R = C - B Z^-1 B' and the reduced right-hand side on the blocked MFMA factorisation, the box
// LCP on R by the incremental-factor solver above (algorithm 0 / 1; beyond kIncrementalMaxRows bounded rows by block
// principal pivoting), then y = Z^-1 (c - B' z).  nub_arg >= 0 is the reference's test hook (:623-626), -1 scans the
// bounds; q6 keeps the reference's literal classification test.  A: host, row-major, only the
// lower triangle is read or written.
bool box_lcp_schur(DenseWorkspace &ws, int n, double *A, const double *b, const double *lo, const double *hi, int algorithm,
                   int nub_arg, bool q6, int max_steps, double max_seconds, double *x, double *w, int32_t *perm, int *nub_out,
                   int *pivots, std::string *msg);

// `count` SolveLCP_BoxSchur problems of n <= kDantzigMaxRows rows in ONE launch, a workgroup per problem with the
// partition, the elimination, the inner box LCP and the back-substitution all on chip (dantzig.hip).  sel[k] = the
// problem's number in the caller's packed arrays (n, nub, ok, nub_out, pivots indexed by it; its matrix at A +
// a_off[sel[k]], its vectors at v_off[sel[k]]).  One upload, one launch, one read-back through page-locked memory
// that `hooks.take` hands out (valid until the call returns); hooks.mark(begin) brackets the launch for the caller's
// kernel timer (may be NULL).  The bounds must already satisfy lo <= 0 <= hi on the bounded rows.  Problems with more
// rows are NOT fused: they go through box_lcp_schur one at a time.
//
// The three fused pipelines below (this one, mixed_constraints_fused, dense_iterate_batch) lay their block out with
// packed_block.h: the sections read back, the sections uploaded, then device-only scratch, the same offsets on both
// sides; hooks.take is asked for the block's host_bytes().  host/packed_block_check.cpp runs their section lists on the
// CPU under the sanitizers.  The caller (dense.cpp) makes the hooks from its context and empties the staging arena
// before the call.
struct LaunchHooks {
  void *(*take)(void *self, size_t bytes);
  void (*mark)(void *self, bool begin);
  void *self;
};
void box_lcp_schur_fused(hipStream_t stream, const LaunchHooks &hooks, int algorithm, int count, const int32_t *sel, const int32_t *n,
                         const int64_t *a_off, const int64_t *v_off, double *A, const double *b, const double *lo, const double *hi,
                         const int32_t *nub, bool q6, int max_steps, double max_seconds, double *x, double *w, int32_t *perm,
                         int32_t *ok, int32_t *nub_out, int32_t *pivots);

// `count` Lcp::MixedConstraintsSolver problems of at most kFusedDenseMax (112, dense_world.h) rows each in ONE pipeline
// (mixed_batch.hip): a workgroup per problem runs the partition, the Cholesky of A_ee, the Schur complement, the
// reference's Murty loop and the back-substitution of dense_world_fused_kernel on the caller's packed matrix.  sel[f] =
// the problem's number in the caller's packed arrays (n, ok, pivots indexed by it; its full row-major matrix at A +
// a_off[sel[f]], its vectors at v_off[sel[f]]); A is read only.  One page-locked block from `hooks.take`, one device
// allocation, one upload, at most one launch per size class (32 / 64 / 112 rows), one read-back, one synchronisation.
// use_bounds = false is the reference (quirk Q3); max_pivots > 0 tightens its cap min(1000, 2^n_i).  ok[k] = the
// reference's bool, x / w of a failed problem are zero.  The matrices must already have passed the symmetry check.
// fr != NULL: the pyramid form (egs_mixed_friction_solve_batch; mixed_solve_device.h).  normal_row / mu: packed like the
// vectors, already validated (a normal row is a plain inequality row of the same problem, mu >= 0 on pyramid rows);
// max_outer >= 1; beta (packed, may be NULL), outer / change (indexed like ok) receive each problem's outcome.  Solve
// k + 1 starts its Murty set from solve k's final set.
struct MixedFrictionBatch {
  const int32_t *normal_row;
  const double *mu;
  int max_outer;
  double tol;
  double *beta;
  int32_t *outer;
  double *change;
};
void mixed_constraints_fused(DenseWorkspace &ws, const LaunchHooks &hooks, int count, const int32_t *sel, const int32_t *n,
                             const int64_t *a_off, const int64_t *v_off, const double *A, const double *b, const uint8_t *C,
                             const double *lo, const double *hi, bool use_bounds, int max_pivots, double *x, double *w, int32_t *ok,
                             int32_t *pivots, const MixedFrictionBatch *fr = nullptr);

// One pyramid problem of any size by the same fixed-point iteration on the host (the route beyond kFusedDenseMax rows):
// every outer solve is dense_mixed_constraints(use_bounds) on the problem WITHOUT its pinned rows, the pyramid rows as
// inequality rows with bounds [-beta, +beta]; beta follows the read-back x.  Each solve starts its Murty set from
// scratch.  A, b, C, lo, hi, normal_row, mu: host, validated as above.  x, w [N] out (w = A x - b on the pinned rows),
// beta [N] (may be NULL), *pivots summed over the solves, *outer, *change.  Returns the inner solver's bool.
bool mixed_friction_host(DenseWorkspace &ws, int N, const double *A, const double *b, const uint8_t *C, const double *lo,
                         const double *hi, const int32_t *normal_row, const double *mu, int max_pivots, int max_outer, double tol,
                         double *x, double *w, double *beta, int *pivots, int *outer, double *change, std::string *msg);

// sparse::{Jacobi,GaussSeidel,SOR}Iteration on an explicit dense matrix (sparse_iterations.cc:72-144; dense_iter.hip):
// A row-major n x n (n <= 1024), C / lo / hi as the reference's 5-argument overloads (all-equality for the 2-argument
// ones), method 0 / 1 / 2, omega = 1.5 in the reference (:15), max_iters = 500 (:19), tol = 1e-9 (constants.h:5).
void dense_iterate(hipStream_t stream, int n, const double *A, const double *b, const uint8_t *C, const double *lo,
                   const double *hi, int method, double omega, int max_iters, double tol, double *x, int *iterations,
                   double *residual);

// `count` such systems in one pipeline (dense_iter.hip): packed as the LCP batches, problem k's matrix at A + sum_{j<k}
// n_j^2 and its vectors at sum_{j<k} n_j; C, lo and hi all NULL = every row an equality.  Problems of up to
// kDantzigMaxRows rows go to one launch (a wavefront each, the matrix in LDS), larger ones (up to 1024 rows) to a second
// (dense_iterate's workgroup each); n_k = 0 is allowed.  One upload, one read-back and one synchronisation through
// page-locked memory that `hooks.take` hands out; hooks.mark brackets the launches.  iterations / residual [count] are
// what dense_iterate reports for each problem alone; history (may be NULL) is [count][max_iters + 1]: entry s = the
// error after sweep s (entry 0: of x0 = b), NaN beyond the problem's sweep count.  Throws std::invalid_argument, before
// anything is launched or written, for a size outside 0..1024, a method or omega dense_iterate refuses, max_iters < 0,
// or a zero on a diagonal (the message names the first such problem).
void dense_iterate_batch(hipStream_t stream, const LaunchHooks &hooks, int count, const int32_t *n, const double *A, const double *b,
                         const uint8_t *C, const double *lo, const double *hi, int method, double omega, int max_iters, double tol,
                         double *x, int32_t *iterations, double *residual, double *history);

}  // namespace egs
