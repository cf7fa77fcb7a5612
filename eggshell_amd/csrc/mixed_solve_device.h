// mixed_solve_device.h -- Lcp::MixedConstraintsSolver (lcp.cc:276-336) inside ONE workgroup, the device code that
// dense_world_fused_kernel (dense_world.hip, a world's ensembles) and mixed_batch_kernel (mixed_batch.hip, a caller's
// packed matrices) share: partition by C, packed right-looking Cholesky of A_ee with [A_ei | b_e] riding through the
// forward substitution, the Schur complement, the reference's Murty loop (lcp.cc:157-274, as murty_small_kernel in
// dense_murty.hip) and x_e = A_ee^-1 (b_e - A_ei x_i).  Every fused operation is an explicit fma: both kernels compute
// the same bits from the same rows.
//
// The PYRAMID form (template flag PYR; egs_mixed_friction_solve_batch) wraps the Murty loop in the
// Tresca fixed-point iteration on the bounds of the Coulomb pyramid's tangential rows: the partition and the Schur
// complement run once (neither depends on the bounds), every outer solve is the box LCP with the pyramid rows bounded
// by [-beta, +beta] (beta = 0: the row is PINNED, x = 0 and no condition on w), beta follows the normal rows' x after
// each solve, and x_e is back-substituted once after the last.  Solve k + 1 starts its Murty set from solve k's final
// set (rows at a bound move with it, a row released from the pin starts free).  The form with the flag off is the code
// it was before the flag existed.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace egs {

__device__ __forceinline__ int dtri(int r, int c) { return r * (r + 1) / 2 + c; }   // c <= r

// The workgroup's index lists and flags: one __shared__ instance per kernel.
template <int MAXN>
struct MixedSolveShared {
  int idx[MAXN], idxE[MAXN], idxI[MAXN];
  unsigned char S[MAXN];
  int first, oob, wbad, ns, state, fail, ne, ni, badb;
  double resid2, good, best;
};

// The packed triangle and the eleven vectors, carved from dynamic LDS: mixed_solve_lds_doubles(MAXN) doubles.
constexpr size_t mixed_solve_lds_doubles(int maxn) { return (size_t)maxn * (maxn + 1) / 2 + 11 * (size_t)maxn; }
struct MixedSolveLds {
  double *T;                                        // packed lower triangle: Cholesky factors of A_ee and A(S,S)
  double *x, *w, *r, *Cv, *lo, *hi, *b, *y, *bx, *bw, *y2;
  __device__ __forceinline__ MixedSolveLds(double *sm, int maxn) {
    T = sm;
    x = T + maxn * (maxn + 1) / 2;
    w = x + maxn; r = w + maxn; Cv = r + maxn; lo = Cv + maxn;
    hi = lo + maxn; b = hi + maxn; y = b + maxn; bx = y + maxn;
    bw = bx + maxn; y2 = bw + maxn;
  }
};

// right-looking Cholesky of the packed n x n triangle in T, in place; yv (may be NULL) rides along as an extra
// row, so L z = yv is solved by the same column steps.  *fail = 1 on a non-positive pivot.
template <int BLOCK>
__device__ __forceinline__ void packed_cholesky(double *T, int n, double *yv, int *fail) {
  const int tid = threadIdx.x;
  for (int j = 0; j < n; ++j) {
    const double d = T[dtri(j, j)];
    if (!(d > 0.0)) { if (tid == 0) *fail = 1; }
    const double rt = sqrt(d > 0.0 ? d : 1.0);
    for (int i = j + 1 + tid; i < n; i += BLOCK) T[dtri(i, j)] /= rt;
    if (yv && tid == BLOCK - 1) yv[j] /= rt;
    __syncthreads();
    if (tid == 0) T[dtri(j, j)] = rt;
    const int tx = tid & 15, ty = tid >> 4;
    for (int i = j + 1 + ty; i < n; i += BLOCK / 16) {
      const double lij = T[dtri(i, j)];
      for (int k = j + 1 + tx; k <= i; k += 16) T[dtri(i, k)] = __builtin_fma(-lij, T[dtri(k, j)], T[dtri(i, k)]);
    }
    if (yv) {
      const double yj = yv[j];
      for (int i = j + 1 + tid; i < n; i += BLOCK) yv[i] = __builtin_fma(-T[dtri(i, j)], yj, yv[i]);
    }
    __syncthreads();
  }
}

// L^T v = z for the factor in T, in ONE wavefront (no workgroup barrier per step)
__device__ __forceinline__ void packed_back_solve(const double *T, int n, double *yv) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    for (int j = n - 1; j >= 0; --j) {
      if (tid == (j & 63)) yv[j] = yv[j] / T[dtri(j, j)];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const double yj = yv[j];
      for (int i = tid; i < j; i += 64) yv[i] = __builtin_fma(-T[dtri(j, i)], yj, yv[i]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  __syncthreads();
}

// Rows with is_eq(i) go to sh.idxE, the others to sh.idxI, each in row order (lcp.cc:279-285).  Clears the flags of
// the solve; ends with a barrier.
template <int MAXN, typename IsEq>
__device__ __forceinline__ void mixed_partition(MixedSolveShared<MAXN> &sh, int N, IsEq is_eq) {
  if (threadIdx.x == 0) {
    int ne = 0, ni = 0;
    for (int i = 0; i < N; ++i) {
      if (is_eq(i)) sh.idxE[ne++] = i;
      else sh.idxI[ni++] = i;
    }
    sh.ne = ne; sh.ni = ni; sh.fail = 0; sh.state = 0; sh.badb = 0;
  }
  __syncthreads();
}

struct MixedSolveResult {
  int solved;     // the reference's bool
  int pivots;     // principal pivots of the Murty loop (the pyramid form: summed over its solves)
};

// What the pyramid form takes and reports beside the plain one; the plain form's is empty.
//   nrow[i] (row i of the problem) = the row whose x bounds row i (a plain inequality row), or -1: a plain row;
//   mu[i] >= 0 its coefficient; max_outer >= 1 solves at most; tol the stopping change.
//   nrow == NULL: the rows come in triples (t, t, n) as a world's constraints do, and mu[i] >= 0 on rows 3c and 3c + 1
//   makes them pyramid rows of row 3c + 2 (normal_of below; mu[i] < 0: plain rows).
//   ext: one more LDS vector of MAXN doubles, behind mixed_solve_lds_doubles(MAXN) -- the normal row of every
//   inequality row as its index among the inequality rows (MAXN ints), then the two words of the change reduction.
//   On return: outer = solves made, change = the last delta; the bound of inequality row k stands in L.hi[k].
template <bool PYR>
struct MixedPyramid {};
template <>
struct MixedPyramid<true> {
  const int32_t *nrow;
  const double *mu;
  int max_outer;
  double tol;
  double *ext;
  int outer;
  double change;
  __device__ __forceinline__ int normal_of(int row) const {
    if (nrow) return nrow[row];
    const int r = row % 3;
    return (r < 2 && mu[row] >= 0.0) ? row - r + 2 : -1;
  }
};
constexpr size_t mixed_pyramid_lds_doubles(int maxn) { return mixed_solve_lds_doubles(maxn) + (size_t)maxn; }

// The solve on the partition mixed_partition left in sh.  A: N x N row-major, symmetric; vb, vlo, vhi: the rows'
// right-hand side and bounds (the bounds are read only with use_bounds).  Z (sh.ne x (sh.ni + 1) doubles) and Lh (sh.ni^2
// doubles) are the caller's workspace, LDS or global.  max_pivots > 0 tightens the reference's cap min(1000, 2^ni).
// On return, when solved: L.x[k] and L.w[k] belong to row sh.idxI[k], L.y2[k] to row sh.idxE[k] (whose w is 0).
// PYR: the pyramid form, with pyr as described above (the partition must then list every pyramid row as an inequality
// row, and the dynamic LDS holds mixed_pyramid_lds_doubles(MAXN) doubles); without it pyr is empty and the code is the
// plain solve.
template <int MAXN, int BLOCK, bool PYR>
__device__ __forceinline__ MixedSolveResult mixed_solve_stage(MixedSolveShared<MAXN> &sh, const MixedSolveLds &L, const double *A, int N,
                                                               const double *vb, const double *vlo, const double *vhi, double *Z,
                                                               double *Lh, int use_bounds, int max_pivots, MixedPyramid<PYR> &pyr) {
  const int tid = threadIdx.x;
  const int NONE = 0x7fffffff;
  double *T = L.T, *x = L.x, *w = L.w, *r = L.r, *Cv = L.Cv, *lo = L.lo, *hi = L.hi, *b = L.b, *y = L.y, *bx = L.bx, *bw = L.bw,
         *y2 = L.y2;
  const int *idxE = sh.idxE, *idxI = sh.idxI;
  int *idx = sh.idx;
  unsigned char *S = sh.S;

  // ---- the Schur complement over the equality rows (lcp.cc:286-294)
  const int ne = sh.ne, ni = sh.ni, ni1 = ni + 1;
  if (ne > 0) {
    for (int q = tid; q < ne * ne; q += BLOCK) {
      const int rr = q / ne, cc = q - rr * ne;
      if (cc <= rr) T[dtri(rr, cc)] = A[(size_t)idxE[rr] * N + idxE[cc]];
    }
    // Z = [A_ei | b_e], ne x (ni + 1)
    for (int q = tid; q < ne * ni1; q += BLOCK) {
      const int rr = q / ni1, cc = q - rr * ni1;
      Z[q] = cc < ni ? A[(size_t)idxE[rr] * N + idxI[cc]] : vb[idxE[rr]];
    }
    __syncthreads();
    packed_cholesky<BLOCK>(T, ne, nullptr, &sh.fail);
    // Z = L^-1 Z (forward substitution on all columns at once)
    for (int j = 0; j < ne; ++j) {
      const double d = T[dtri(j, j)];
      for (int c = tid; c < ni1; c += BLOCK) Z[(size_t)j * ni1 + c] /= d;
      __syncthreads();
      for (int q = tid; q < (ne - j - 1) * ni1; q += BLOCK) {
        const int i = j + 1 + q / ni1, c = q % ni1;
        Z[(size_t)i * ni1 + c] = __builtin_fma(-T[dtri(i, j)], Z[(size_t)j * ni1 + c], Z[(size_t)i * ni1 + c]);
      }
      __syncthreads();
    }
  }
  // lhs = A_ii - A_ie A_ee^-1 A_ei, its rhs = b_i - A_ie A_ee^-1 b_e   (lcp.cc:293-294)
  for (int q = tid; q < ni * ni1; q += BLOCK) {
    const int rr = q / ni1, cc = q - rr * ni1;
    double s = 0.0;
    for (int k = 0; k < ne; ++k) s = __builtin_fma(Z[(size_t)k * ni1 + rr], Z[(size_t)k * ni1 + cc], s);
    if (cc < ni) Lh[(size_t)rr * ni + cc] = A[(size_t)idxI[rr] * N + idxI[cc]] - s;
    else b[rr] = vb[idxI[rr]] - s;
  }
  // the inequality rows' bounds: the reference calls the no-bounds overload (lcp.cc:298, quirk Q3)
  const bool box_fix = use_bounds != 0;
  int *nloc = nullptr;                      // pyramid form: the normal row of inequality row k, among the inequality rows
  unsigned long long *red = nullptr;        // and the two words of the change reduction
  if constexpr (PYR) {
    nloc = reinterpret_cast<int *>(pyr.ext);
    red = reinterpret_cast<unsigned long long *>(nloc + MAXN);
    for (int k = tid; k < ni; k += BLOCK) {
      const int f = pyr.normal_of(idxI[k]);
      int at = -1;
      if (f >= 0)
        for (int j = 0; j < ni; ++j) if (idxI[j] == f) at = j;
      nloc[k] = at;
    }
    __syncthreads();
  }
  for (int k = tid; k < ni; k += BLOCK) {
    if constexpr (PYR) {
      if (nloc[k] >= 0) { lo[k] = 0.0; hi[k] = 0.0; continue; }   // beta^0 = 0: pinned, outside the lo < hi rule
    }
    lo[k] = box_fix ? vlo[idxI[k]] : 0.0;
    hi[k] = box_fix ? vhi[idxI[k]] : INFINITY;
    if (!(lo[k] < hi[k]) || !(lo[k] <= 0) || !(box_fix ? hi[k] >= 0 : hi[k] > 0)) sh.badb = 1;   // lcp.cc:161-164
  }
  __syncthreads();
  const bool schur_failed = sh.fail != 0;
  int solved = (!schur_failed && !sh.badb) ? 1 : 0;
  int pivots = 0;

  // ---- MurtyPrincipalPivot on lhs (lcp.cc:157-274), the loop of murty_small_kernel
  if (solved && ni > 0) {
    const int n = ni;
    const double *M = Lh;
    const double p2 = pow(2.0, n);
    int max_iterations = p2 > 1000 ? 1000 : (int)p2;   // lcp.cc:168
    if (max_pivots > 0 && max_pivots < max_iterations) max_iterations = max_pivots;   // the caller's own cap
    for (int i = tid; i < n; i += BLOCK) {
      S[i] = 1; Cv[i] = lo[i];
      if constexpr (PYR) {
        if (nloc[i] >= 0) S[i] = 0;             // a pinned row is clamped to 0 and never enters the set
      }
      x[i] = 0.0; w[i] = -b[i]; r[i] = -b[i];   // lcp.cc:184-185
      bx[i] = 0.0; bw[i] = -b[i];
    }
    __syncthreads();
    auto check = [&]() {     // CheckMurtySolution (lcp.cc:20-103) + goodness (lcp.cc:107-113)
      if (tid == 0) { sh.first = NONE; sh.oob = 0; sh.wbad = 0; }
      __syncthreads();
      for (int i = tid; i < n; i += BLOCK) {
        const double xi = x[i], wi = w[i];
        if constexpr (PYR) {
          if (nloc[i] >= 0 && hi[i] == 0.0) continue;      // pinned: x = 0, its w carries no condition
        }
        bool off;
        if (S[i]) off = (xi < lo[i]) || (xi > hi[i]);
        else off = (Cv[i] == lo[i] && wi < 0) || (Cv[i] == hi[i] && wi > 0);
        if (off) atomicMin(&sh.first, i);
        if (xi < lo[i] || xi > hi[i]) sh.oob = 1;
        if ((xi == lo[i] && wi < 0) || (xi == hi[i] && wi > 0)) sh.wbad = 1;
      }
      __syncthreads();
      if (tid == 0) {
        double res2 = 0.0, good = 0.0;
        for (int i = 0; i < n; ++i) {
          const double d = r[i] - w[i];
          res2 += d * d;
          if (!(x[i] > 0)) good += x[i];
          if (!(w[i] > 0)) good += w[i];
        }
        sh.resid2 = res2; sh.good = good;
      }
      __syncthreads();
    };
    auto is_solution = [&](double tol) { return sh.first == NONE && !sh.oob && !sh.wbad && sqrt(sh.resid2) <= tol; };
    // r = M x - b: two threads per row (even / odd columns), four independent chains each
    auto residual_vector = [&]() {
      const int half = tid & 1;
      for (int i = tid >> 1; i < n; i += BLOCK / 2) {
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
        const double *row = M + (size_t)i * n;
        int c = half;
        for (; c + 6 < n; c += 8) {
          p0 = __builtin_fma(row[c], x[c], p0);
          p1 = __builtin_fma(row[c + 2], x[c + 2], p1);
          p2 = __builtin_fma(row[c + 4], x[c + 4], p2);
          p3 = __builtin_fma(row[c + 6], x[c + 6], p3);
        }
        for (; c < n; c += 2) p0 = __builtin_fma(row[c], x[c], p0);
        const double part = (p0 + p1) + (p2 + p3);
        if (half) y2[i] = part;
        else r[i] = part;
      }
      __syncthreads();
      for (int i = tid; i < n; i += BLOCK) r[i] = (r[i] + y2[i]) - b[i];
      __syncthreads();
    };

    check();
    if (tid == 0) sh.best = sh.good;
    __syncthreads();
    int outer = 1;
    bool again;
    do {   // one pass; the pyramid form: the solves of the fixed-point iteration
      again = false;
      int iter = 0;
      bool force = PYR ? (box_fix || outer > 1) : box_fix;
      while (iter < max_iterations) {
        if (!force) {
          if (is_solution(1e-9)) { if (tid == 0) sh.state = 1; __syncthreads(); break; }
          if (tid == 0 && sh.first != NONE) {             // lcp.cc:36-62: flip the first offender
            const int i = sh.first;
            if (S[i]) { S[i] = 0; Cv[i] = (x[i] < lo[i]) ? lo[i] : hi[i]; }
            else S[i] = 1;
          }
          __syncthreads();
        }
        force = false;
        if (tid == 0) {                                  // index list of S
          int ns = 0;
          for (int i = 0; i < n; ++i) if (S[i]) idx[ns++] = i;
          sh.ns = ns;
        }
        for (int i = tid; i < n; i += BLOCK) x[i] = S[i] ? 0.0 : Cv[i];   // x = x_clamped
        __syncthreads();
        const int ns = sh.ns;
        // right-hand side: b(S), minus M(S,!S) x(!S) for the true box problem (lcp.cc:199-216)
        if (box_fix) {
          residual_vector();                              // r = M x_clamped - b
          for (int k = tid; k < ns; k += BLOCK) y[k] = -r[idx[k]];
        } else {
          for (int k = tid; k < ns; k += BLOCK) y[k] = b[idx[k]];
        }
        for (int q = tid; q < ns * ns; q += BLOCK) {      // gather M(S,S), lower triangle
          const int rr = q / ns, cc = q - rr * ns;
          if (cc <= rr) T[dtri(rr, cc)] = M[(size_t)idx[rr] * n + idx[cc]];
        }
        __syncthreads();
        packed_cholesky<BLOCK>(T, ns, y, &sh.fail);
        packed_back_solve(T, ns, y);
        for (int k = tid; k < ns; k += BLOCK) x[idx[k]] = y[k];
        __syncthreads();
        residual_vector();                               // r = M x - b
        for (int i = tid; i < n; i += BLOCK) w[i] = S[i] ? 0.0 : r[i];     // lcp.cc:219-223
        __syncthreads();
        ++pivots;
        check();
        if (sh.good > sh.best) {                         // lcp.cc:125-137 (uniform: shared value)
          for (int i = tid; i < n; i += BLOCK) { bx[i] = x[i]; bw[i] = w[i]; }
          __syncthreads();
          if (tid == 0) sh.best = sh.good;
          __syncthreads();
        }
        ++iter;
        if (sh.fail) break;
      }
      solved = (sh.state == 1);
      if (!solved && !sh.fail) {
        // capped: the best-seen iterate (reference rule only), re-checked at the looser 1e-8 (lcp.cc:241-246)
        if (!box_fix) {
          for (int i = tid; i < n; i += BLOCK) { x[i] = bx[i]; w[i] = bw[i]; }
          __syncthreads();
        }
        residual_vector();
        check();
        solved = is_solution(1e-8) ? 1 : 0;
      }
      if constexpr (PYR) {
        // beta^{k+1} from x^k, and delta_k = max |beta^{k+1} - beta^k| / max(1, max beta^{k+1}): both maxima of
        // non-negative doubles, taken on their bit patterns
        pyr.outer = outer;
        if (!solved) break;
        if (tid == 0) { red[0] = 0ull; red[1] = 0ull; }
        __syncthreads();
        for (int i = tid; i < n; i += BLOCK) {
          const int f = nloc[i];
          if (f < 0) continue;
          const double xf = x[f];
          const double bn = xf > 0.0 ? pyr.mu[idxI[i]] * xf : 0.0;     // one rounding, as project_pyramid's
          atomicMax(&red[0], (unsigned long long)__double_as_longlong(fabs(bn - hi[i])));
          atomicMax(&red[1], (unsigned long long)__double_as_longlong(bn));
        }
        __syncthreads();
        const double dmax = __longlong_as_double((long long)red[0]), bmax = __longlong_as_double((long long)red[1]);
        pyr.change = dmax / (bmax > 1.0 ? bmax : 1.0);
        if (pyr.change <= pyr.tol || outer >= pyr.max_outer) break;
        // the next solve: the bounds move, rows at a bound move with them, the set stays
        for (int i = tid; i < n; i += BLOCK) {
          const int f = nloc[i];
          if (f < 0) continue;
          const double xf = x[f];
          const double bn = xf > 0.0 ? pyr.mu[idxI[i]] * xf : 0.0;
          const double old = hi[i];
          if (bn == 0.0) { S[i] = 0; Cv[i] = 0.0; lo[i] = 0.0; hi[i] = 0.0; continue; }
          if (old == 0.0) S[i] = 1;                        // released from the pin: 0 is strictly inside
          else if (!S[i]) Cv[i] = Cv[i] < 0.0 ? -bn : bn;
          lo[i] = -bn; hi[i] = bn;
        }
        if (tid == 0) sh.state = 0;
        __syncthreads();
        ++outer;
        again = true;
      }
    } while (again);
  }

  // ---- x_e = A_ee^-1 (b_e - A_ei x_i)   (lcp.cc:317); the factor of A_ee once more (the loop above reused T)
  if (solved && ne > 0) {
    for (int q = tid; q < ne * ne; q += BLOCK) {
      const int rr = q / ne, cc = q - rr * ne;
      if (cc <= rr) T[dtri(rr, cc)] = A[(size_t)idxE[rr] * N + idxE[cc]];
    }
    for (int k = tid; k < ne; k += BLOCK) {
      double s = 0.0;
      const double *row = A + (size_t)idxE[k] * N;
      for (int c = 0; c < ni; ++c) s = __builtin_fma(row[idxI[c]], x[c], s);
      y2[k] = vb[idxE[k]] - s;
    }
    __syncthreads();
    packed_cholesky<BLOCK>(T, ne, y2, &sh.fail);
    packed_back_solve(T, ne, y2);
  }
  MixedSolveResult res;
  res.solved = solved; res.pivots = pivots;
  return res;
}

// the plain form
template <int MAXN, int BLOCK>
__device__ __forceinline__ MixedSolveResult mixed_solve_stage(MixedSolveShared<MAXN> &sh, const MixedSolveLds &L, const double *A, int N,
                                                               const double *vb, const double *vlo, const double *vhi, double *Z,
                                                               double *Lh, int use_bounds, int max_pivots) {
  MixedPyramid<false> none;
  return mixed_solve_stage<MAXN, BLOCK, false>(sh, L, A, N, vb, vlo, vhi, Z, Lh, use_bounds, max_pivots, none);
}

}  // namespace egs
