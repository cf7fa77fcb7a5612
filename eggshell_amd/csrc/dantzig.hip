// dantzig.hip -- the incremental-factor box LCP of the reference's toolkit:
//   lcp::SolveLCP_BoxDantzig             toolkit/lcp.cc:444-619   (Cottle-Dantzig principal pivoting)
//   AddCholeskyRow / SwapCholeskyRows    toolkit/lcp.cc:91-157    (the factor grows / shrinks by one row,
//                                                                  O(n^2) per pivot instead of a fresh O(n^3))
//   RankUpdate                           toolkit/lcp.cc:76-83     (Eigen's llt_rank_update_lower: method C1 of
//                                                                  Gill, Golub, Murray, Saunders 1974)
//   MatrixPermutation::SwapRowsAndColumns toolkit/lcp.cc:171-195  (A permuted IN PLACE, lower triangle only)
// The algorithm is one long dependent chain of pivots, each a handful of O(n^2) sweeps, on the few dozen
// to ~100 rows the reference's ensembles hand it -- there is nothing in ONE problem to spread over a GPU, so
// one workgroup runs a whole solve and the GPU-natural unit is a BATCH: one workgroup per problem, thousands of
// problems per launch (egs_box_lcp_batch; what a batch of ensembles hands the solver).  Two instantiations:
//   n <= 96   one wavefront, A, L and every vector in LDS (two n x n fp64 matrices in 160 KB);
//   n <= 1024 four wavefronts, A permuted in place in global memory, L in a global work area, vectors in LDS.
// Row-parallel loops take a lane per row; every scalar chain (dot products, the ratio test's argmin) runs in the
// reference's element order on all lanes at once, so the pivot sequence -- and with it the permutation left in
// A -- is the sequential algorithm's.  Every loop has an exit: a step cap (the caller's, else 20 n + 1000) and
// an optional wall-clock limit (lcp::Settings::max_iterations / max_time, toolkit/lcp.h:161-167).
// The solver bodies are __device__ functions (dantzig_solve, murty_solve) shared by these kernels and by
// box_schur_kernel below: lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747) fused into one launch for a batch of
// problems of n <= 96 rows (egs_box_lcp_schur_batch).
#include "dense_lcp.h"
#include "packed_block.h"
#include "runtime.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace egs {

namespace {

struct LcpResult {
  int32_t ok, pivots, reason, pad;      // reason: 0 solved, 1 step limit, 2 non-positive pivot, 3 time limit
};

// `count` problems, one workgroup each.  Offsets are in doubles; A is permuted in place (lower triangle).
struct LcpSet {
  const int32_t *ids;                   // block -> problem number (NULL: the block number itself)
  const int32_t *n;
  const int64_t *a_off, *v_off;
  double *A;
  const double *b, *lo, *hi;
  double *x, *w;
  int32_t *perm;
  LcpResult *res;
  double *L;                            // global instantiation: work area for the factor, laid out as A
  int max_steps;                        // <= 0: 20 n + 1000
  long long max_ticks;                  // wall_clock64 ticks (100 MHz), 0 = no limit
};

// the barrier: a scheduling fence plus "my LDS / global writes have landed" for the workgroup
__device__ __forceinline__ void wsync() { __syncthreads(); }

// lane 0 looks at the clock, everyone gets the same answer
__device__ bool out_of_time(long long t0, long long max_ticks, int *flag, int lane) {
  if (max_ticks <= 0) return false;
  if (lane == 0) *flag = ((long long)wall_clock64() - t0 > max_ticks) ? 1 : 0;
  wsync();
  const bool r = *flag != 0;
  wsync();
  return r;
}

#define AT(M, r, c) (M)[(r) * n + (c)]

// L y = b on the top-left m x m block, column by column (toolkit/lcp.cc:52-54)
template <int NT>
__device__ void lsolve(const double *L, int n, int m, double *x, int lane) {
  for (int j = 0; j < m; ++j) {
    const double xj = x[j] / AT(L, j, j);
    wsync();
    if (lane == 0) x[j] = xj;
    for (int k = j + 1 + lane; k < m; k += NT) x[k] = x[k] - AT(L, k, j) * xj;
    wsync();
  }
}
// L' x = y (toolkit/lcp.cc:58-62)
template <int NT>
__device__ void ltsolve(const double *L, int n, int m, double *x, int lane) {
  for (int j = m - 1; j >= 0; --j) {
    const double xj = x[j] / AT(L, j, j);
    wsync();
    if (lane == 0) x[j] = xj;
    for (int k = lane; k < j; k += NT) x[k] = x[k] - AT(L, j, k) * xj;
    wsync();
  }
}
template <int NT>
__device__ void lltsolve(const double *L, int n, int m, double *x, int lane) {
  lsolve<NT>(L, n, m, x, lane);
  ltsolve<NT>(L, n, m, x, lane);
}

// L L' += sigma vec vec' on the p x p block at (i0, i0) (toolkit/lcp.cc:76-83); temp = p doubles, vec may be temp
template <int NT>
__device__ bool rank_update(double *L, int n, int i0, int p, const double *vec, double sigma, double *temp, int lane) {
  for (int k = lane; k < p; k += NT) temp[k] = vec[k];
  wsync();
  double beta = 1.0;
  for (int j = 0; j < p; ++j) {
    const double Ljj = AT(L, i0 + j, i0 + j);
    const double dj = Ljj * Ljj;
    const double wj = temp[j];
    const double swj2 = sigma * (wj * wj);
    const double gamma = dj * beta + swj2;
    const double xx = dj + swj2 / beta;
    if (!(xx > 0.0)) return false;
    const double nLjj = sqrt(xx);
    beta = beta + swj2 / dj;
    const double f0 = wj / Ljj, f1 = nLjj / Ljj, f2 = (gamma != 0.0) ? nLjj * sigma * wj / gamma : 0.0;
    wsync();
    if (lane == 0) AT(L, i0 + j, i0 + j) = nLjj;
    for (int k = j + 1 + lane; k < p; k += NT) {
      const double lk = AT(L, i0 + k, i0 + j);
      const double tk = temp[k] - f0 * lk;
      temp[k] = tk;
      if (gamma != 0.0) AT(L, i0 + k, i0 + j) = f1 * lk + f2 * tk;
    }
    wsync();
  }
  return true;
}

// toolkit/lcp.cc:91-102
template <int NT>
__device__ bool add_cholesky_row(const double *A, int n, int m, double *L, int lane) {
  if (m == 1) {
    const double d = AT(A, 0, 0);
    if (!(d > 0.0)) return false;
    wsync();
    if (lane == 0) AT(L, 0, 0) = sqrt(d);
    wsync();
    return true;
  }
  double *ell = &AT(L, m - 1, 0);
  for (int k = lane; k < m - 1; k += NT) ell[k] = AT(A, m - 1, k);
  wsync();
  lsolve<NT>(L, n, m - 1, ell, lane);
  double s = 0.0;
  for (int k = 0; k < m - 1; ++k) s = s + ell[k] * ell[k];
  const double d = AT(A, m - 1, m - 1) - s;
  if (!(d > 0.0)) return false;
  wsync();
  if (lane == 0) AT(L, m - 1, m - 1) = sqrt(d);
  wsync();
  return true;
}

// toolkit/lcp.cc:110-157; wq, temp = n doubles each
template <int NT>
__device__ bool swap_cholesky_rows(const double *A, int n, int i, int m, double *L, double *wq, double *temp, int lane) {
  if (m <= 1 || i == m - 1) return true;
  if (i == 0) {
    const double head = (AT(A, m - 1, m - 1) - AT(A, 0, 0)) * 0.5;
    for (int k = lane; k < m - 1; k += NT) wq[k] = (k == 0) ? head + 1.0 : AT(A, m - 1, k) - AT(A, k, 0);
    wsync();
    if (!rank_update<NT>(L, n, 0, m - 1, wq, 0.5, temp, lane)) return false;
    if (lane == 0) wq[0] = head - 1.0;
    wsync();
    return rank_update<NT>(L, n, 0, m - 1, wq, -0.5, temp, lane);
  }
  double *l1 = &AT(L, i, 0);
  for (int k = lane; k < i; k += NT) l1[k] = AT(A, m - 1, k);
  wsync();
  lsolve<NT>(L, n, i, l1, lane);
  double s = 0.0;
  for (int k = 0; k < i; ++k) s = s + l1[k] * l1[k];
  const double d = AT(A, m - 1, m - 1) - s;
  if (!(d > 0.0)) return false;
  const double e = sqrt(d);
  wsync();
  if (lane == 0) AT(L, i, i) = e;
  const int p = m - 2 - i;
  if (p > 0) {
    for (int k = lane; k < p; k += NT) wq[k] = AT(L, i + 1 + k, i);
    wsync();
    if (!rank_update<NT>(L, n, i + 1, p, wq, 1.0, temp, lane)) return false;
    for (int k = lane; k < p; k += NT) {
      double t = 0.0;
      for (int c = 0; c < i; ++c) t = t + AT(L, i + 1 + k, c) * l1[c];
      const double v = (AT(A, m - 1, i + 1 + k) - t) / e;
      AT(L, i + 1 + k, i) = v;
      wq[k] = v;
    }
    wsync();
    if (!rank_update<NT>(L, n, i + 1, p, wq, -1.0, temp, lane)) return false;
  }
  wsync();
  return true;
}

// toolkit/lcp.cc:171-195
template <int NT>
__device__ void swap_rows_and_columns(double *A, int n, int i, int j, int *perm, int lane) {
  if (i == j) return;
  if (i > j) { const int t = i; i = j; j = t; }
  wsync();
  for (int c = lane; c < i; c += NT) { const double t = AT(A, i, c); AT(A, i, c) = AT(A, j, c); AT(A, j, c) = t; }
  for (int r = j + 1 + lane; r < n; r += NT) { const double t = AT(A, r, i); AT(A, r, i) = AT(A, r, j); AT(A, r, j) = t; }
  for (int k = i + 1 + lane; k < j; k += NT) { const double t = AT(A, k, i); AT(A, k, i) = AT(A, j, k); AT(A, j, k) = t; }
  if (lane == 0) {
    const double t = AT(A, i, i); AT(A, i, i) = AT(A, j, j); AT(A, j, j) = t;
    const int q = perm[i]; perm[i] = perm[j]; perm[j] = q;
  }
  wsync();
}

__device__ __forceinline__ void swap_entry(double *v, int a, int b, int lane) {
  if (lane == 0) { const double t = v[a]; v[a] = v[b]; v[b] = t; }
}

// Per-problem pointers of a workgroup: GLOBAL = false copies A into LDS (written back at the end), true works in place.
template <int NT, bool GLOBAL>
struct LcpView {
  int n, prob;
  double *A, *L, *vec;      // vec: the first of the problem's LDS vectors
  double *gA;
  long long v_off;
  __device__ LcpView(const LcpSet &S, unsigned char *smem, int lane) {
    prob = S.ids ? S.ids[blockIdx.x] : (int)blockIdx.x;
    n = S.n[prob];
    gA = S.A + S.a_off[prob];
    v_off = S.v_off[prob];
    double *base = reinterpret_cast<double *>(smem);
    if (GLOBAL) { A = gA; L = S.L + S.a_off[prob]; vec = base; }
    else { A = base; L = A + (size_t)n * n; vec = L + (size_t)n * n; }
  }
};

// The LDS vectors of one inner solve: x, w, the bounds and right-hand side, six work vectors, the permutation(s)
// and the clock flag.  The stand-alone kernels carve them from one block; the fused Schur kernel points lo / hi / b
// at the vectors it already holds.
struct LcpWork {
  double *x, *w, *lo, *hi, *b, *s0, *s1, *s2, *s3, *s4, *s5;
  int *perm, *iperm, *flag;
};
__device__ __forceinline__ LcpWork carve_work(double *vec, int n) {
  LcpWork W;
  W.x = vec; W.w = W.x + n; W.lo = W.w + n; W.hi = W.lo + n; W.b = W.hi + n; W.s0 = W.b + n; W.s1 = W.s0 + n; W.s2 = W.s1 + n;
  W.s3 = W.s2 + n; W.s4 = W.s3 + n; W.s5 = W.s4 + n;
  W.perm = reinterpret_cast<int *>(W.s5 + n); W.iperm = W.perm + n; W.flag = W.perm + 2 * n;
  return W;
}

// SolveLCP_BoxDantzig, toolkit/lcp.cc:444-619, on an n x n matrix (leading dimension n) the workgroup can write.
// On entry: L = 0, x = w = 0, lo / hi / b loaded, perm = identity, everything visible.  On return x, w, lo, hi are in
// the pivoting order perm describes (perm[k] = original index of final row k).
template <int NT>
__device__ bool dantzig_solve(double *A, double *L, int n, const LcpWork &W, int max_steps_arg, long long max_ticks, int lane,
                              int &steps, int &reason) {
  double *x = W.x, *w = W.w, *lo = W.lo, *hi = W.hi, *b = W.b, *dxS = W.s0, *dwNS = W.s1, *limit = W.s2, *v = W.s3, *wq = W.s4,
         *temp = W.s5;
  int *perm = W.perm, *flag = W.flag;
  const int max_steps = max_steps_arg > 0 ? max_steps_arg : 20 * n + 1000;
  const long long t0 = (long long)wall_clock64();
  reason = 0;

  int index = 0;
  steps = 0;
  bool ok = true;
  for (int i = 0; i < n && ok; ++i) {
    double s = 0.0;
    for (int k = 0; k < i; ++k) s = s + AT(A, i, k) * x[k];
    const double wi0 = s - b[i];
    wsync();
    if (lane == 0) { w[i] = wi0; x[i] = 0.0; }
    wsync();
    if (wi0 == 0.0) continue;
    if (lo[i] == 0.0 && wi0 >= 0.0) continue;
    if (hi[i] == 0.0 && wi0 <= 0.0) continue;
    const double dir = (wi0 <= 0.0) ? 1.0 : -1.0;
    for (int k = lane; k < index; k += NT) dxS[k] = -dir * AT(A, i, k);
    wsync();
    lltsolve<NT>(L, n, index, dxS, lane);
    const double delta_xi = dir;
    while (true) {
      if (++steps > max_steps) { ok = false; reason = 1; break; }
      if (out_of_time(t0, max_ticks, flag, lane)) { ok = false; reason = 3; break; }
      // delta_w on the rows outside the set, one lane per row, the row's products in column order
      for (int r = index + lane; r < i; r += NT) {
        double t = 0.0;
        for (int k = 0; k < index; ++k) t = t + AT(A, r, k) * dxS[k];
        dwNS[r - index] = t + AT(A, i, r) * dir;
      }
      double delta_wi = 0.0;
      for (int k = 0; k < index; ++k) delta_wi = delta_wi + AT(A, i, k) * dxS[k];
      delta_wi = delta_wi + AT(A, i, i) * dir;
      for (int j = lane; j < index; j += NT) limit[j] = (dxS[j] > 0.0) ? hi[j] : lo[j];
      wsync();
      // the ratio test, in the reference's scan order on every lane
      double best_alpha = -w[i] / delta_wi;
      int best_index = i;
      bool index_i_into_set = true;
      const double index_i_limit = (dir > 0.0) ? hi[i] : lo[i];
      {
        const double alpha = (index_i_limit - x[i]) / delta_xi;
        if (alpha > 0.0 && alpha < best_alpha) { best_alpha = alpha; best_index = i; index_i_into_set = false; }
      }
      for (int j = 0; j < index; ++j) {
        const double alpha = (limit[j] - x[j]) / dxS[j];
        if (alpha > 0.0 && alpha < best_alpha) { best_alpha = alpha; best_index = j; }
      }
      for (int j = index; j < i; ++j) {
        const double alpha = -w[j] / dwNS[j - index];
        if (alpha > 0.0 && alpha < best_alpha) { best_alpha = alpha; best_index = j; }
      }
      wsync();
      for (int k = lane; k < index; k += NT) x[k] = x[k] + best_alpha * dxS[k];
      for (int r = index + lane; r < i; r += NT) w[r] = w[r] + best_alpha * dwNS[r - index];
      if (lane == 0) { x[i] = x[i] + best_alpha * delta_xi; w[i] = w[i] + best_alpha * delta_wi; }
      wsync();
      index_i_into_set = (best_index == i && index_i_into_set);
      if (best_index < index) {
        if (lane == 0) x[best_index] = limit[best_index];
        wsync();
        if (!swap_cholesky_rows<NT>(A, n, best_index, index, L, wq, temp, lane)) { ok = false; reason = 2; break; }
        swap_rows_and_columns<NT>(A, n, index - 1, best_index, perm, lane);
        swap_entry(x, index - 1, best_index, lane); swap_entry(lo, index - 1, best_index, lane); swap_entry(hi, index - 1, best_index, lane);
        --index;
        wsync();
        for (int k = lane; k < index; k += NT) dxS[k] = -dir * AT(A, i, k);
        wsync();
        lltsolve<NT>(L, n, index, dxS, lane);
      } else if (best_index < i || index_i_into_set) {
        if (lane == 0) w[index_i_into_set ? i : best_index] = 0.0;
        wsync();
        swap_rows_and_columns<NT>(A, n, index, best_index, perm, lane);
        swap_entry(x, index, best_index, lane); swap_entry(w, index, best_index, lane);
        swap_entry(lo, index, best_index, lane); swap_entry(hi, index, best_index, lane);
        wsync();
        if (!add_cholesky_row<NT>(A, n, index + 1, L, lane)) { ok = false; reason = 2; break; }
        if (best_index != i) {
          double t = 0.0;
          for (int k = 0; k < index; ++k) t = t + AT(A, index, k) * dxS[k];
          const double value = (-dir * AT(A, i, index) - t) / (AT(L, index, index) * AT(L, index, index));
          for (int k = lane; k < index; k += NT) v[k] = AT(L, index, k);
          wsync();
          if (lane == 0) dxS[index] = value;
          ltsolve<NT>(L, n, index, v, lane);
          for (int k = lane; k < index; k += NT) dxS[k] = dxS[k] - value * v[k];
          wsync();
        }
        ++index;
      } else {
        if (lane == 0) x[i] = index_i_limit;
        wsync();
      }
      if (best_index == i) break;
    }
  }
  wsync();
  return ok;
}

template <int NT, bool GLOBAL>
__global__ void __launch_bounds__(NT) box_dantzig_kernel(const LcpSet S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  const LcpView<NT, GLOBAL> V(S, smem, lane);
  const int n = V.n;
  double *A = V.A, *L = V.L;
  const LcpWork W = carve_work(V.vec, n);
  double *x = W.x, *w = W.w, *lo = W.lo, *hi = W.hi, *b = W.b;
  int *perm = W.perm;
  const double *gb = S.b + V.v_off, *glo = S.lo + V.v_off, *ghi = S.hi + V.v_off;
  for (int k = lane; k < n * n; k += NT) { if (!GLOBAL) A[k] = V.gA[k]; L[k] = 0.0; }
  for (int k = lane; k < n; k += NT) { x[k] = 0.0; w[k] = 0.0; lo[k] = glo[k]; hi[k] = ghi[k]; b[k] = gb[k]; perm[k] = k; }
  wsync();
  int steps, reason;
  const bool ok = dantzig_solve<NT>(A, L, n, W, S.max_steps, S.max_ticks, lane, steps, reason);
  for (int k = lane; k < n; k += NT) { S.x[V.v_off + perm[k]] = x[k]; S.w[V.v_off + perm[k]] = w[k]; if (S.perm) S.perm[V.v_off + k] = perm[k]; }
  if (!GLOBAL)
    for (int k = lane; k < n * n; k += NT) {
      const int r = k / n, c = k - r * n;
      if (c <= r) V.gA[k] = A[k];      // the lower triangle only, as the reference
    }
  if (lane == 0) { LcpResult r; r.ok = ok ? 1 : 0; r.pivots = steps; r.reason = ok ? 0 : reason; r.pad = 0; S.res[V.prob] = r; }
}

// in-place Cholesky of the lower triangle, column by column, a lane per row below the pivot (toolkit/lcp.cc:46-48)
template <int NT>
__device__ bool cholesky(double *L, int n, int lane) {
  for (int j = 0; j < n; ++j) {
    double d = AT(L, j, j);
    for (int k = 0; k < j; ++k) d = d - AT(L, j, k) * AT(L, j, k);
    if (!(d > 0.0)) return false;
    d = sqrt(d);
    wsync();
    if (lane == 0) AT(L, j, j) = d;
    for (int i = j + 1 + lane; i < n; i += NT) {
      double s = AT(L, i, j);
      for (int k = 0; k < j; ++k) s = s - AT(L, i, k) * AT(L, j, k);
      AT(L, i, j) = s / d;
    }
    wsync();
  }
  return true;
}

// SolveLCP_BoxMurty on a LinearReducer (toolkit/lcp.cc:213-328, 380-442); SolveLCP_Murty (:333-378) is the same loop
// with lo = 0, hi = +inf.  On entry: L = the lower triangle of A (0 above it), x = w = 0, lo / hi / b loaded, s0 (xs) = b,
// s1 (c) = 0, perm = iperm = identity.  x and w come back in the caller's order; returns "no factor broke down",
// solved = the loop ended on a solution.
template <int NT>
__device__ bool murty_solve(double *A, double *L, int n, const LcpWork &W, int max_steps_arg, long long max_ticks, int lane,
                            int &it, int &reason, bool &solved) {
  double *x = W.x, *w = W.w, *lo = W.lo, *hi = W.hi, *b = W.b, *xs = W.s0, *c = W.s1, *c2 = W.s2, *t = W.s3, *wq = W.s4, *temp = W.s5;
  int *perm = W.perm, *iperm = W.iperm, *flag = W.flag;
  const int max_iterations = max_steps_arg > 0 ? max_steps_arg : 20 * n + 1000;
  const long long t0 = (long long)wall_clock64();
  reason = 0;
  // LinearReducer::LinearReducer (:213-224): factor all of A, xs = A^-1 b
  bool ok = cholesky<NT>(L, n, lane);
  if (!ok) reason = 2;
  if (ok) lltsolve<NT>(L, n, n, xs, lane);
  int index = n;
  it = 0;
  solved = false;
  for (; ok && it < max_iterations; ++it) {
    if (out_of_time(t0, max_ticks, flag, lane)) { ok = false; reason = 3; break; }
    // SubSolve (:245-296)
    wsync();
    if (index == 0) {
      for (int i = lane; i < n; i += NT) x[i] = c[i];
    } else if (index >= n) {
      for (int i = lane; i < n; i += NT) x[perm[i]] = xs[i];
    } else {
      for (int i = lane; i < n; i += NT) c2[i] = c[perm[i]];
      wsync();
      for (int k = lane; k < index; k += NT) {
        double s = 0.0;
        for (int r = index; r < n; ++r) s = s + AT(A, r, k) * (c2[r] - xs[r]);
        t[k] = s;
      }
      wsync();
      lltsolve<NT>(L, n, index, t, lane);
      for (int i = lane; i < n; i += NT) x[perm[i]] = (i < index) ? xs[i] - t[i] : c[perm[i]];
    }
    wsync();
    // MultiplyA (:298-322) on the rows outside the set; w = A x - b there, 0 inside (:396-404).  c2 = x permuted
    for (int i = lane; i < n; i += NT) c2[i] = x[perm[i]];
    wsync();
    for (int r = lane; r < n; r += NT) {
      if (r < index) { w[perm[r]] = 0.0; continue; }
      double s = 0.0;
      for (int k = 0; k < index; ++k) s = s + AT(A, r, k) * c2[k];
      double u = 0.0;
      for (int k = index; k < n; ++k) u = u + ((k <= r) ? AT(A, r, k) : AT(A, k, r)) * c2[k];
      w[perm[r]] = (s + u) - b[perm[r]];
    }
    wsync();
    // first violated index in the caller's order (:408-431), found by every lane
    int who = -1, dirn = 0;      // dirn: -1 leaves the set clamped at lo, -2 at hi, +1 enters the set
    for (int i = 0; i < n; ++i) {
      if (iperm[i] < index) {
        if (x[i] < lo[i]) { who = i; dirn = -1; break; }
        if (x[i] > hi[i]) { who = i; dirn = -2; break; }
      } else {
        if ((c[i] == lo[i] && w[i] < 0.0) || (c[i] == hi[i] && w[i] > 0.0)) { who = i; dirn = 1; break; }
      }
    }
    if (who < 0) { solved = true; break; }
    const int p = iperm[who];
    wsync();
    if (dirn < 0) {       // RemoveIndex (:236-243)
      if (lane == 0) c[who] = (dirn == -1) ? lo[who] : hi[who];
      if (!swap_cholesky_rows<NT>(A, n, p, index, L, wq, temp, lane)) { ok = false; reason = 2; break; }
      --index;
    }
    if (index != p) {
      const int a = perm[index], bq = perm[p];
      swap_rows_and_columns<NT>(A, n, index, p, perm, lane);
      if (lane == 0) { iperm[a] = p; iperm[bq] = index; const double tt = xs[index]; xs[index] = xs[p]; xs[p] = tt; }
      wsync();
    }
    if (dirn > 0) {       // AddIndex (:226-234)
      ++index;
      if (!add_cholesky_row<NT>(A, n, index, L, lane)) { ok = false; reason = 2; break; }
      if (lane == 0) c[who] = 0.0;
    }
    wsync();
  }
  wsync();
  return ok;
}

template <int NT, bool GLOBAL>
__global__ void __launch_bounds__(NT) box_murty_kernel(const LcpSet S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  const LcpView<NT, GLOBAL> V(S, smem, lane);
  const int n = V.n;
  double *A = V.A, *L = V.L;
  const LcpWork W = carve_work(V.vec, n);
  double *x = W.x, *w = W.w, *lo = W.lo, *hi = W.hi, *b = W.b, *xs = W.s0, *c = W.s1;
  int *perm = W.perm, *iperm = W.iperm;
  const double *gb = S.b + V.v_off, *glo = S.lo + V.v_off, *ghi = S.hi + V.v_off;
  for (int k = lane; k < n * n; k += NT) {
    const int r = k / n, q = k - r * n;
    const double a = V.gA[k];
    if (!GLOBAL) A[k] = a;
    L[k] = (q <= r) ? a : 0.0;
  }
  for (int k = lane; k < n; k += NT) { x[k] = 0.0; w[k] = 0.0; lo[k] = glo[k]; hi[k] = ghi[k]; b[k] = gb[k]; xs[k] = gb[k]; c[k] = 0.0; perm[k] = k; iperm[k] = k; }
  wsync();
  int it, reason;
  bool solved;
  const bool ok = murty_solve<NT>(A, L, n, W, S.max_steps, S.max_ticks, lane, it, reason, solved);
  for (int k = lane; k < n; k += NT) { S.x[V.v_off + k] = x[k]; S.w[V.v_off + k] = w[k]; if (S.perm) S.perm[V.v_off + k] = perm[k]; }
  if (!GLOBAL)
    for (int k = lane; k < n * n; k += NT) {
      const int r = k / n, q = k - r * n;
      if (q <= r) V.gA[k] = A[k];
    }
  if (lane == 0) {
    LcpResult r;
    r.ok = (ok && solved) ? 1 : 0; r.pivots = it; r.reason = (ok && solved) ? 0 : (ok ? 1 : reason); r.pad = 0;
    S.res[V.prob] = r;
  }
}

// ---- lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747), fused: one workgroup (one wavefront) per problem of
// n <= kDantzigMaxRows rows does the partition, the elimination of the unbounded rows, the box LCP on the Schur
// complement and the back-substitution, all in LDS.  The operation order is the column-oriented one of the plain
// restatement the tests check against: one accumulation chain per entry, terms in increasing k.
struct SchurSet {
  const int32_t *n;
  const int64_t *a_off, *v_off;         // in doubles, per problem of this launch
  double *A;                            // lower triangles permuted in place
  const double *b, *lo, *hi;
  const int32_t *nub;                   // >= 0: the reference's test hook, < 0: scan the bounds
  double *x, *w;
  int32_t *perm;                        // the partition's permutation
  LcpResult *res;                       // pad = nub
  int q6, max_steps;
  long long max_ticks;
};

// LDS of a problem of n rows: 2 n^2 doubles of matrices (L_Z nub^2 + Q nub ni + R ni^2 + the inner factor ni^2 for any
// split nub + ni = n; A and its factor when nub = 0), 7 n outer and 8 n inner vectors, 4 n + 4 ints.
constexpr int kSchurVectors = 15;
__host__ __device__ constexpr size_t schur_lds_bytes(int n) {
  return (2 * (size_t)n * n + kSchurVectors * (size_t)n) * sizeof(double) + (4 * (size_t)n + 4) * sizeof(int);
}

template <int ALG>      // 0 = SolveLCP_BoxMurty inside, 1 = SolveLCP_BoxDantzig
__global__ void __launch_bounds__(64) box_schur_kernel(const SchurSet S) {
  constexpr int NT = 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x, prob = blockIdx.x;
  const int n = S.n[prob];
  double *gA = S.A + S.a_off[prob];
  const long long vo = S.v_off[prob];
  double *M = reinterpret_cast<double *>(smem);
  double *ob = M + 2 * (size_t)n * n, *olo = ob + n, *ohi = olo + n, *t = ohi + n, *rhs = t + n, *z = rhs + n, *zw = z + n;
  LcpWork W;
  W.x = zw + n; W.w = W.x + n; W.s0 = W.w + n; W.s1 = W.s0 + n; W.s2 = W.s1 + n; W.s3 = W.s2 + n; W.s4 = W.s3 + n; W.s5 = W.s4 + n;
  int *operm = reinterpret_cast<int *>(W.s5 + n);
  W.perm = operm + n; W.iperm = W.perm + n; W.flag = W.iperm + n;
  const double big = 1.7976931348623157e308, inf = __builtin_huge_val();

  for (int k = lane; k < n; k += NT) { ob[k] = S.b[vo + k]; olo[k] = S.lo[vo + k]; ohi[k] = S.hi[vo + k]; operm[k] = k; }
  wsync();
  // the partition (:652-683): every lane walks the two pointers, the swaps are shared out
  int nub = S.nub[prob];
  if (nub < 0) {
    nub = 0;
    int nb = n - 1;
    while (true) {
      for (; nub <= nb; ++nub) if (S.q6 ? (olo[nub] > -big || ohi[nub] < -big) : (olo[nub] > -big || ohi[nub] < big)) break;
      for (; nb >= nub; --nb) if (S.q6 ? (olo[nb] <= -big && ohi[nb] >= -big) : (olo[nb] <= -big && ohi[nb] >= big)) break;
      if (nub > nb) break;
      swap_rows_and_columns<NT>(gA, n, nub, nb, operm, lane);
      swap_entry(ob, nub, nb, lane); swap_entry(olo, nub, nb, lane); swap_entry(ohi, nub, nb, lane);
      wsync();
    }
  }
  const int ni = n - nub;
  // "infinity" is DBL_MAX or the real one (toolkit/lcp.h:149-150): the inner solver sees the real one
  for (int k = nub + lane; k < n; k += NT) { if (olo[k] <= -big) olo[k] = -inf; if (ohi[k] >= big) ohi[k] = inf; }
  for (int k = lane; k < n; k += NT) { S.perm[vo + k] = operm[k]; z[k] = 0.0; zw[k] = 0.0; }
  W.lo = olo + nub; W.hi = ohi + nub; W.b = (nub == 0) ? ob : rhs;
  for (int k = lane; k < ni; k += NT) { W.x[k] = 0.0; W.w[k] = 0.0; W.perm[k] = k; W.iperm[k] = k; }
  wsync();

  int steps = 0, reason = 0;
  bool ok = true;
  double *A = M, *L = M + (size_t)n * n;      // the inner solver's matrix and factor; reseated below when 0 < nub < n
  if (nub == n) {
    // x = A.llt().solve(b), w = 0 (:687-692)
    for (int k = lane; k < n * n; k += NT) { const int r = k / n, q = k - r * n; M[k] = (q <= r) ? gA[k] : 0.0; }
    for (int k = lane; k < n; k += NT) z[k] = ob[k];
    wsync();
    ok = cholesky<NT>(M, n, lane);
    if (ok) lltsolve<NT>(M, n, n, z, lane);
    else reason = 2;
  } else {
    if (nub == 0) {
      for (int k = lane; k < n * n; k += NT) A[k] = gA[k];
    } else {
      double *LZ = M, *Q = LZ + (size_t)nub * nub, *R = Q + (size_t)nub * ni;
      A = R; L = R + (size_t)ni * ni;
      for (int k = lane; k < nub * nub; k += NT) { const int r = k / nub, q = k - r * nub; LZ[k] = (q <= r) ? gA[(size_t)r * n + q] : 0.0; }
      wsync();
      ok = cholesky<NT>(LZ, nub, lane);                          // L L' = Z
      if (!ok) reason = 2;
      if (ok) {
        for (int j = lane; j < ni; j += NT) {                    // Q = L^-1 B', a lane per column of B' (row of B)
          const double *brow = gA + (size_t)(nub + j) * n;
          for (int k = 0; k < nub; ++k) Q[k * ni + j] = brow[k];
          for (int c = 0; c < nub; ++c) {
            const double xc = Q[c * ni + j] / LZ[c * nub + c];
            Q[c * ni + j] = xc;
            for (int k = c + 1; k < nub; ++k) Q[k * ni + j] = Q[k * ni + j] - LZ[k * nub + c] * xc;
          }
        }
        for (int k = lane; k < nub; k += NT) t[k] = ob[k];
        wsync();
        for (int e = lane; e < ni * ni; e += NT) {               // R = C - Q'Q, lower triangle (:717-719)
          const int i = e / ni, j = e - i * ni;
          double r = 0.0;
          if (j <= i) {
            double sum = 0.0;
            for (int k = 0; k < nub; ++k) sum = sum + Q[k * ni + i] * Q[k * ni + j];
            r = gA[(size_t)(nub + i) * n + nub + j] - sum;
          }
          R[e] = r;
        }
        lltsolve<NT>(LZ, nub, nub, t, lane);                     // t = Z^-1 c
        for (int i = lane; i < ni; i += NT) {                    // rhs = d - B t
          const double *brow = gA + (size_t)(nub + i) * n;
          double sum = 0.0;
          for (int k = 0; k < nub; ++k) sum = sum + brow[k] * t[k];
          rhs[i] = ob[nub + i] - sum;
        }
        wsync();
      }
    }
    if (ok) {
      if (ALG == 1) {
        for (int k = lane; k < ni * ni; k += NT) L[k] = 0.0;
        wsync();
        ok = dantzig_solve<NT>(A, L, ni, W, S.max_steps, S.max_ticks, lane, steps, reason);
        if (ok) for (int k = lane; k < ni; k += NT) { z[W.perm[k]] = W.x[k]; zw[W.perm[k]] = W.w[k]; }
      } else {
        for (int k = lane; k < ni * ni; k += NT) { const int r = k / ni, q = k - r * ni; L[k] = (q <= r) ? A[k] : 0.0; }
        for (int k = lane; k < ni; k += NT) { W.s0[k] = W.b[k]; W.s1[k] = 0.0; }
        wsync();
        bool solved = false;
        ok = murty_solve<NT>(A, L, ni, W, S.max_steps, S.max_ticks, lane, steps, reason, solved);
        if (ok && !solved) { ok = false; reason = 1; }
        if (ok || nub == 0) for (int k = lane; k < ni; k += NT) { z[k] = W.x[k]; zw[k] = W.w[k]; }
      }
      wsync();
      if (nub == 0) {
        // entirely an LCP (:695-700): the inner solver's pivoting order stays in the caller's lower triangle
        for (int k = lane; k < n * n; k += NT) { const int r = k / n, q = k - r * n; if (q <= r) gA[k] = A[k]; }
      } else if (ok) {
        for (int k = lane; k < nub; k += NT) {                   // y = Z^-1 (c - B' z)
          double sum = 0.0;
          for (int i = 0; i < ni; ++i) sum = sum + gA[(size_t)(nub + i) * n + k] * z[i];
          t[k] = ob[k] - sum;
        }
        wsync();
        lltsolve<NT>(M, nub, nub, t, lane);
      }
    }
  }
  wsync();
  // Unpermute (:741-744); a problem that failed after the partition reports zeros
  if (nub == n) {
    for (int k = lane; k < n; k += NT) { S.x[vo + k] = z[k]; S.w[vo + k] = 0.0; }
  } else {
    for (int k = lane; k < nub; k += NT) { S.x[vo + operm[k]] = ok ? t[k] : 0.0; S.w[vo + operm[k]] = 0.0; }
    for (int k = lane; k < ni; k += NT) { S.x[vo + operm[nub + k]] = z[k]; S.w[vo + operm[nub + k]] = zw[k]; }
  }
  if (lane == 0) { LcpResult r; r.ok = ok ? 1 : 0; r.pivots = steps; r.reason = ok ? 0 : reason; r.pad = nub; S.res[prob] = r; }
}

#undef AT

size_t lds_bytes(int n, bool global) {
  return ((global ? 0 : 2 * (size_t)n * n) + 11 * (size_t)n) * sizeof(double) + (3 * (size_t)n + 4) * sizeof(int);
}

template <int NT, bool GLOBAL>
void launch_kind(hipStream_t stream, int algorithm, const LcpSet &S, int blocks, size_t lds) {
  if (blocks <= 0) return;
  auto kd = box_dantzig_kernel<NT, GLOBAL>;
  auto km = box_murty_kernel<NT, GLOBAL>;
  const void *fn = algorithm == 1 ? reinterpret_cast<const void *>(kd) : reinterpret_cast<const void *>(km);
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (algorithm == 1) hipLaunchKernelGGL(kd, dim3(blocks), dim3(NT), lds, stream, S);
  else hipLaunchKernelGGL(km, dim3(blocks), dim3(NT), lds, stream, S);
  HIPCHK(hipGetLastError());
}

// Everything on the device already: matrices at dA + a_off[k], vectors at v_off[k].  hn / ha / hv = the host copies
// of the size and offset tables.  One launch for the problems that fit LDS, one for the larger ones.
void solve_set(hipStream_t stream, int algorithm, int count, const int32_t *hn, const int64_t *ha, const int64_t *hv, double *dA,
               const double *db, const double *dlo, const double *dhi, int max_steps, double max_seconds, double *dx, double *dw,
               int32_t *dperm, LcpResult *dres) {
  std::vector<int32_t> small, large;
  int n_small = 0, n_large = 0;
  int64_t a_total = 0;
  for (int k = 0; k < count; ++k) {
    if (hn[k] <= kDantzigMaxRows) { small.push_back(k); n_small = std::max(n_small, (int)hn[k]); }
    else { large.push_back(k); n_large = std::max(n_large, (int)hn[k]); }
    a_total = std::max(a_total, ha[k] + (int64_t)hn[k] * hn[k]);
  }
  ScopedDevBuf<int32_t> d_n(count), d_ids(count);
  ScopedDevBuf<int64_t> d_off(2 * (size_t)count);
  ScopedDevBuf<double> d_L(large.empty() ? 0 : (size_t)a_total);
  std::vector<int32_t> ids(small);
  ids.insert(ids.end(), large.begin(), large.end());
  HIPCHK(hipMemcpyAsync(d_n.p, hn, count * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_ids.p, ids.data(), count * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_off.p, ha, count * sizeof(int64_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_off.p + count, hv, count * sizeof(int64_t), hipMemcpyHostToDevice, stream));
  LcpSet S{};
  S.n = d_n.p; S.a_off = d_off.p; S.v_off = d_off.p + count;
  S.A = dA; S.b = db; S.lo = dlo; S.hi = dhi; S.x = dx; S.w = dw; S.perm = dperm; S.res = dres; S.L = d_L.p;
  S.max_steps = max_steps;
  S.max_ticks = max_seconds > 0 ? (long long)(max_seconds * 1e8) + 1 : 0;     // wall_clock64 counts at 100 MHz
  S.ids = d_ids.p;
  launch_kind<64, false>(stream, algorithm, S, (int)small.size(), lds_bytes(n_small, false));
  S.ids = d_ids.p + small.size();
  launch_kind<256, true>(stream, algorithm, S, (int)large.size(), lds_bytes(n_large, true));
  HIPCHK(hipStreamSynchronize(stream));      // the tables above are freed on return
}

void check_problem(int algorithm, int n, const double *lo, const double *hi) {
  if (n <= 0 || n > kIncrementalMaxRows) throw std::invalid_argument("incremental box LCP: 1 <= n <= 1024");
  for (int i = 0; i < n; ++i) {
    // lo <= 0 <= hi (toolkit/lcp.h:134); Dantzig also needs lo < hi (toolkit/lcp.cc:448-450)
    if (!(lo[i] <= 0.0) || !(hi[i] >= 0.0) || (algorithm == 1 && !(lo[i] < hi[i])))
      throw std::invalid_argument("incremental box LCP: needs lo <= 0 <= hi (and lo < hi for Cottle-Dantzig)");
  }
}

const char *reason_text(int reason) {
  switch (reason) {
    case 1: return "incremental box LCP: iteration limit reached";
    case 2: return "incremental box LCP: a factor update met a non-positive pivot (A not positive definite?)";
    case 3: return "incremental box LCP: time limit reached";
    default: return "";
  }
}

}  // namespace

void box_lcp_incremental_batch(hipStream_t stream, int algorithm, int count, const int32_t *n, double *A, const double *b,
                               const double *lo, const double *hi, int max_steps, double max_seconds, double *x, double *w,
                               int32_t *perm, int32_t *ok, int32_t *pivots, int32_t *reason) {
  if (algorithm != 0 && algorithm != 1) throw std::invalid_argument("incremental box LCP: algorithm 0 (Murty) or 1 (Cottle-Dantzig)");
  if (count <= 0) return;
  std::vector<int64_t> ha(count), hv(count);
  int64_t at = 0, vt = 0;
  for (int k = 0; k < count; ++k) {
    ha[k] = at; hv[k] = vt;
    check_problem(algorithm, n[k], lo + vt, hi + vt);
    at += (int64_t)n[k] * n[k]; vt += n[k];
  }
  ScopedDevBuf<double> dA((size_t)at), dv(5 * (size_t)vt);
  ScopedDevBuf<int32_t> dperm((size_t)vt);
  ScopedDevBuf<LcpResult> dres(count);
  double *db = dv.p, *dlo = dv.p + vt, *dhi = dv.p + 2 * vt, *dx = dv.p + 3 * vt, *dw = dv.p + 4 * vt;
  HIPCHK(hipMemcpyAsync(dA.p, A, (size_t)at * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(db, b, (size_t)vt * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(dlo, lo, (size_t)vt * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(dhi, hi, (size_t)vt * sizeof(double), hipMemcpyHostToDevice, stream));
  solve_set(stream, algorithm, count, n, ha.data(), hv.data(), dA.p, db, dlo, dhi, max_steps, max_seconds, dx, dw, dperm.p, dres.p);
  std::vector<LcpResult> r(count);
  std::vector<double> hA((size_t)at);
  HIPCHK(hipMemcpyAsync(hA.data(), dA.p, (size_t)at * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(x, dx, (size_t)vt * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(w, dw, (size_t)vt * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (perm) HIPCHK(hipMemcpyAsync(perm, dperm.p, (size_t)vt * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(r.data(), dres.p, count * sizeof(LcpResult), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  // only the lower triangle of the caller's A is ever written (toolkit/lcp.h:73)
  for (int k = 0; k < count; ++k) {
    const int nk = n[k];
    double *Ak = A + ha[k];
    const double *Hk = hA.data() + ha[k];
    for (int rr = 0; rr < nk; ++rr)
      for (int c = 0; c <= rr; ++c) Ak[(size_t)rr * nk + c] = Hk[(size_t)rr * nk + c];
    if (ok) ok[k] = r[k].ok;
    if (pivots) pivots[k] = r[k].pivots;
    if (reason) reason[k] = r[k].reason;
  }
}

void box_lcp_schur_fused(hipStream_t stream, const LaunchHooks &hooks, int algorithm, int count, const int32_t *sel, const int32_t *n,
                         const int64_t *a_off, const int64_t *v_off, double *A, const double *b, const double *lo, const double *hi,
                         const int32_t *nub, bool q6, int max_steps, double max_seconds, double *x, double *w, int32_t *perm,
                         int32_t *ok, int32_t *nub_out, int32_t *pivots) {
  if (algorithm != 0 && algorithm != 1) throw std::invalid_argument("SolveLCP_BoxSchur: algorithm 0 (Murty) or 1 (Cottle-Dantzig)");
  if (count <= 0) return;
  size_t at = 0, vt = 0;
  int n_max = 0;
  for (int k = 0; k < count; ++k) {
    const int nk = n[sel[k]];
    if (nk < 1 || nk > kDantzigMaxRows) throw std::invalid_argument("SolveLCP_BoxSchur, fused: 1 <= n <= 96");
    at += (size_t)nk * nk; vt += nk; n_max = std::max(n_max, nk);
  }
  // one packed block, the same layout on both sides (packed_block.h).  read back: x w perm res A; uploaded: b lo hi
  // a_off v_off n nub and, permuted in place by the device, A: the last section read back, so the upload starts there
  const size_t nc = (size_t)count;
  PackedBlock blk;
  const auto s_x = blk.add<double>(Zone::Download, vt), s_w = blk.add<double>(Zone::Download, vt);
  const auto s_perm = blk.add<int32_t>(Zone::Download, vt);
  const auto s_res = blk.add<LcpResult>(Zone::Download, nc, 8);
  const auto s_A = blk.add<double>(Zone::Download, at);
  const auto s_b = blk.add<double>(Zone::Upload, vt), s_lo = blk.add<double>(Zone::Upload, vt), s_hi = blk.add<double>(Zone::Upload, vt);
  const auto s_aoff = blk.add<int64_t>(Zone::Upload, nc), s_voff = blk.add<int64_t>(Zone::Upload, nc);
  const auto s_n = blk.add<int32_t>(Zone::Upload, nc), s_nub = blk.add<int32_t>(Zone::Upload, nc);
  char *h = static_cast<char *>(hooks.take(hooks.self, blk.host_bytes()));
  ScopedDevBuf<char> d(blk.total_bytes());
  blk.bind(h, d.p);
  int64_t *haoff = blk.host(s_aoff), *hvoff = blk.host(s_voff);
  size_t ap = 0, vp = 0;
  for (int k = 0; k < count; ++k) {
    const int j = sel[k], nk = n[j];
    haoff[k] = (int64_t)ap; hvoff[k] = (int64_t)vp; blk.host(s_n)[k] = nk; blk.host(s_nub)[k] = nub ? nub[j] : -1;
    ap += (size_t)nk * nk; vp += nk;
  }
  const auto rows = [&](int k) { return (size_t)n[sel[k]]; };
  const auto entries = [&](int k) { return (size_t)n[sel[k]] * (size_t)n[sel[k]]; };
  const auto a_at = [&](int k) { return (size_t)haoff[k]; };
  const auto v_at = [&](int k) { return (size_t)hvoff[k]; };
  gather_ragged(blk.host(s_A), A, count, sel, a_off, entries, a_at);
  gather_ragged(blk.host(s_b), b, count, sel, v_off, rows, v_at);
  gather_ragged(blk.host(s_lo), lo, count, sel, v_off, rows, v_at);
  gather_ragged(blk.host(s_hi), hi, count, sel, v_off, rows, v_at);
  HIPCHK(hipMemcpyAsync(d.p + s_A.offset, h + s_A.offset, blk.upload_end() - s_A.offset, hipMemcpyHostToDevice, stream));
  SchurSet S{};
  S.n = blk.device(s_n); S.nub = blk.device(s_nub);
  S.a_off = blk.device(s_aoff); S.v_off = blk.device(s_voff);
  S.A = blk.device(s_A); S.b = blk.device(s_b); S.lo = blk.device(s_lo); S.hi = blk.device(s_hi);
  S.x = blk.device(s_x); S.w = blk.device(s_w);
  S.perm = blk.device(s_perm); S.res = blk.device(s_res);
  S.q6 = q6 ? 1 : 0; S.max_steps = max_steps;
  S.max_ticks = max_seconds > 0 ? (long long)(max_seconds * 1e8) + 1 : 0;
  const size_t lds = schur_lds_bytes(n_max);
  auto km = box_schur_kernel<0>;
  auto kd = box_schur_kernel<1>;
  const void *fn = algorithm == 1 ? reinterpret_cast<const void *>(kd) : reinterpret_cast<const void *>(km);
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (hooks.mark) hooks.mark(hooks.self, true);
  if (algorithm == 1) hipLaunchKernelGGL(kd, dim3(count), dim3(64), lds, stream, S);
  else hipLaunchKernelGGL(km, dim3(count), dim3(64), lds, stream, S);
  HIPCHK(hipGetLastError());
  if (hooks.mark) hooks.mark(hooks.self, false);
  HIPCHK(hipMemcpyAsync(h, d.p, blk.download_bytes(), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  scatter_ragged(x, blk.host(s_x), count, sel, v_off, rows, v_at);
  scatter_ragged(w, blk.host(s_w), count, sel, v_off, rows, v_at);
  if (perm) scatter_ragged(perm, blk.host(s_perm), count, sel, v_off, rows, v_at);
  const LcpResult *hres = blk.host(s_res);
  for (int k = 0; k < count; ++k) {
    const int j = sel[k], nk = n[j];
    double *Ak = A + a_off[j];
    const double *Hk = blk.host(s_A) + haoff[k];
    for (int r = 0; r < nk; ++r) std::memcpy(Ak + (size_t)r * nk, Hk + (size_t)r * nk, (size_t)(r + 1) * sizeof(double));   // the lower triangle only
    ok[j] = hres[k].ok;
    if (nub_out) nub_out[j] = hres[k].pad;
    if (pivots) pivots[j] = hres[k].pivots;
  }
}

bool box_lcp_incremental(hipStream_t stream, int algorithm, int n, double *A, const double *b, const double *lo, const double *hi,
                         double *x, double *w, int32_t *perm, int max_steps, double max_seconds, int *pivots, std::string *msg) {
  int32_t nn = n, ok = 0, piv = 0, reason = 0;
  box_lcp_incremental_batch(stream, algorithm, 1, &nn, A, b, lo, hi, max_steps, max_seconds, x, w, perm, &ok, &piv, &reason);
  if (pivots) *pivots = piv;
  if (!ok && msg) *msg = reason_text(reason);
  return ok != 0;
}

bool box_lcp_incremental_device(hipStream_t stream, int algorithm, int n, double *dA, const double *db, const double *dlo,
                                const double *dhi, const double *h_lo, const double *h_hi, int max_steps, double max_seconds,
                                double *dx, double *dw, int *pivots, std::string *msg) {
  if (algorithm != 0 && algorithm != 1) throw std::invalid_argument("incremental box LCP: algorithm 0 (Murty) or 1 (Cottle-Dantzig)");
  check_problem(algorithm, n, h_lo, h_hi);
  ScopedDevBuf<LcpResult> dres(1);
  const int32_t hn = n;
  const int64_t zero = 0;
  solve_set(stream, algorithm, 1, &hn, &zero, &zero, dA, db, dlo, dhi, max_steps, max_seconds, dx, dw, nullptr, dres.p);
  LcpResult r{};
  HIPCHK(hipMemcpy(&r, dres.p, sizeof r, hipMemcpyDeviceToHost));
  if (pivots) *pivots = r.pivots;
  if (!r.ok && msg) *msg = reason_text(r.reason);
  return r.ok != 0;
}

}  // namespace egs
