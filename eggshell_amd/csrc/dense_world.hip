// dense_world.hip -- Ensemble::ComputeVDot (ensembles.cc:498-538) for every ensemble of a world in two launches
// (egs_world_step_dense): the dense J M^-1 J^T of each ensemble, then ONE workgroup per ensemble runs the rest
// without the host: CheckMatrixCondition against kGoodConditionNumber = 1e7 (ensembles.cc:513-521), the Schur
// complement over the equality rows (lcp.cc:286-294), the reference's Murty loop on the inequality rows
// (lcp.cc:157-274, as murty_small_kernel in dense_lcp.hip) and x_e = A_ee^-1 (b_e - A_ei x_i) (lcp.cc:317).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dense_world.h"

namespace egs {

namespace {

__device__ __forceinline__ int dtri(int r, int c) { return r * (r + 1) / 2 + c; }   // c <= r

// Kernel 1: pair (i, j) of ensemble blockIdx.y's constraints -> the 3x3 block of A_e at (3i, 3j), the arithmetic of
// dense_system_kernel (kernels.hip) on the world's blocks.  The lane of pair (i, 0) also gathers constraint i's rows.
__global__ void __launch_bounds__(256) dense_world_system_kernel(DenseWorldArgs a) {
  const int e = blockIdx.y;
  const int c0 = a.cstart[e], m = a.cstart[e + 1] - c0;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)m * m) return;
  const int i = (int)(idx / m), j = (int)(idx % m);
  const int ci = a.cons[c0 + i], cj = a.cons[c0 + j];
  double blk[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int si = 0; si < 2; ++si) {
    const int bi = si ? a.body1[ci] : a.body0[ci];
    if (bi < 0) continue;
    for (int sj = 0; sj < 2; ++sj) {
      const int bj = sj ? a.body1[cj] : a.body0[cj];
      if (bj != bi) continue;
      const double *Ji = (si ? a.J1 : a.J0) + (size_t)ci * 18, *Jj = (sj ? a.J1 : a.J0) + (size_t)cj * 18;
      const double *W = a.Minv + (size_t)bi * 36;
      double t[18];   // W Jj^T, 6x3
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          double v = W[6 * k] * Jj[6 * q];
#pragma unroll
          for (int l = 1; l < 6; ++l) v = __builtin_fma(W[6 * k + l], Jj[6 * q + l], v);
          t[3 * k + q] = v;
        }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          double v = blk[3 * r + q];
#pragma unroll
          for (int k = 0; k < 6; ++k) v = __builtin_fma(Ji[6 * r + k], t[3 * k + q], v);
          blk[3 * r + q] = v;
        }
    }
  }
  const size_t N = (size_t)3 * m;
  double *A = a.ws + a.ws_off[e];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) A[((size_t)3 * i + r) * N + 3 * j + q] = blk[3 * r + q];
  if (j == 0) {
    double *vb = A + dense_ws_vec(N);
    for (int r = 0; r < 3; ++r) {
      const size_t row = (size_t)3 * i + r, src = (size_t)3 * ci + r;
      vb[row] = a.rhs[src];
      vb[N + row] = a.lo[src];
      vb[2 * N + row] = a.hi[src];
      vb[3 * N + row] = a.is_eq[src] ? 1.0 : 0.0;
    }
  }
}

// Kernel 2: one workgroup (BLOCK threads) per ensemble of at most MAXN rows.  A_e, its inverse and the Schur
// complement live in the ensemble's workspace (global memory, cache-resident at these sizes); the Cholesky factors
// (packed lower triangle) and every vector live in LDS.  Every decision is the workgroup's alone, so an ensemble
// gets the same bits whatever else the world holds.
template <int MAXN, int BLOCK>
__global__ void __launch_bounds__(BLOCK) dense_world_fused_kernel(DenseWorldArgs a, const int32_t *list) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double *T = sm;                                   // packed lower triangle: Cholesky factors of A, A_ee, A(S,S)
  double *x = T + MAXN * (MAXN + 1) / 2;
  double *w = x + MAXN, *r = w + MAXN, *Cv = r + MAXN, *lo = Cv + MAXN;
  double *hi = lo + MAXN, *b = hi + MAXN, *y = b + MAXN, *bx = y + MAXN;
  double *bw = bx + MAXN, *y2 = bw + MAXN;
  __shared__ int idx[MAXN], idxE[MAXN], idxI[MAXN];
  __shared__ unsigned char S[MAXN];
  __shared__ int s_first, s_oob, s_wbad, s_ns, s_state, s_fail, s_ne, s_ni, s_badb;
  __shared__ double s_resid2, s_good, s_best, s_diag[2];
  __shared__ double s_red[BLOCK / 64][6];
  const int tid = threadIdx.x;
  const int NONE = 0x7fffffff;
  const int e = list[blockIdx.x];
  const int c0 = a.cstart[e];
  const int N = 3 * (a.cstart[e + 1] - c0);
  double *A = a.ws + a.ws_off[e];
  double *Z = A + (size_t)N * N;
  double *Lh = Z + (size_t)N * N + N;
  const double *vb = A + dense_ws_vec(N), *vlo = vb + N, *vhi = vb + 2 * N, *vc = vb + 3 * N;

  // K partial sums per thread -> the workgroup's sums, the same bits in every thread
  auto block_sum = [&](double *v, int K) {
    for (int k = 0; k < K; ++k)
      for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (BLOCK > 64) {
      if ((tid & 63) == 0)
        for (int k = 0; k < K; ++k) s_red[tid >> 6][k] = v[k];
      __syncthreads();
      for (int k = 0; k < K; ++k) {
        double t = s_red[0][k];
        for (int q = 1; q < BLOCK / 64; ++q) t += s_red[q][k];
        v[k] = t;
      }
      __syncthreads();
    }
  };
  // right-looking Cholesky of the packed n x n triangle in T, in place; yv (may be NULL) rides along as an extra
  // row, so L z = yv is solved by the same column steps.  s_fail = 1 on a non-positive pivot.
  auto cholesky = [&](int n, double *yv) {
    for (int j = 0; j < n; ++j) {
      const double d = T[dtri(j, j)];
      if (!(d > 0.0)) { if (tid == 0) s_fail = 1; }
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
  };
  // L^T v = z for the factor in T, in ONE wavefront (no workgroup barrier per step)
  auto back_solve = [&](int n, double *yv) {
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
  };

  // ---- CheckMatrixCondition (ensembles.cc:513-521): cond_2(A) < 1e7 ?  A is positive definite here or singular.
  if (tid == 0) { s_fail = 0; s_state = 0; s_badb = 0; }
  for (int q = tid; q < N * N; q += BLOCK) {
    const int rr = q / N, cc = q - rr * N;
    if (cc <= rr) T[dtri(rr, cc)] = A[q];
  }
  __syncthreads();
  cholesky(N, nullptr);
  double condition = INFINITY;
  if (!s_fail) {
    if (tid == 0) {
      double mx = 0.0, mn = 1e300;
      for (int k = 0; k < N; ++k) { const double d = T[dtri(k, k)]; mx = d > mx ? d : mx; mn = d < mn ? d : mn; }
      s_diag[0] = mx; s_diag[1] = mn;
    }
    // Z = A^-1 = L^-T L^-1 I, N right-hand sides side by side
    for (int q = tid; q < N * N; q += BLOCK) Z[q] = (q / N == q % N) ? 1.0 : 0.0;
    __syncthreads();
    for (int j = 0; j < N; ++j) {
      const double d = T[dtri(j, j)];
      for (int c = tid; c < N; c += BLOCK) Z[(size_t)j * N + c] /= d;
      __syncthreads();
      for (int q = tid; q < (N - j - 1) * N; q += BLOCK) {
        const int i = j + 1 + q / N, c = q % N;
        Z[(size_t)i * N + c] = __builtin_fma(-T[dtri(i, j)], Z[(size_t)j * N + c], Z[(size_t)i * N + c]);
      }
      __syncthreads();
    }
    for (int j = N - 1; j >= 0; --j) {
      const double d = T[dtri(j, j)];
      for (int c = tid; c < N; c += BLOCK) Z[(size_t)j * N + c] /= d;
      __syncthreads();
      for (int q = tid; q < j * N; q += BLOCK) {
        const int i = q / N, c = q % N;
        Z[(size_t)i * N + c] = __builtin_fma(-T[dtri(j, i)], Z[(size_t)j * N + c], Z[(size_t)i * N + c]);
      }
      __syncthreads();
    }
    // lambda_max by power iteration on A, 1 / lambda_min by power iteration on A^-1, side by side: the start vector
    // and the 60 iterations of dense_condition_estimate (dense_lcp.hip); Rayleigh quotients, both from below
    double *v1 = x, *u1 = w, *v2 = r, *u2 = y;
    for (int i = tid; i < N; i += BLOCK) {
      const double s0 = 1.0 + 0.37 * (double)((unsigned)(i * 2654435761u) >> 22) / 1024.0;
      v1[i] = s0; v2[i] = s0;
    }
    __syncthreads();
    double lmax = 0.0, mu = 0.0;
    for (int it = 0; it < 60; ++it) {
      for (int i = tid; i < N; i += BLOCK) {
        double p = 0.0, q = 0.0;
        const double *ra = A + (size_t)i * N, *rz = Z + (size_t)i * N;
        for (int c = 0; c < N; ++c) { p = __builtin_fma(ra[c], v1[c], p); q = __builtin_fma(rz[c], v2[c], q); }
        u1[i] = p; u2[i] = q;
      }
      __syncthreads();
      double sums[6] = {0, 0, 0, 0, 0, 0};
      for (int i = tid; i < N; i += BLOCK) {
        sums[0] = __builtin_fma(v1[i], v1[i], sums[0]); sums[1] = __builtin_fma(v1[i], u1[i], sums[1]);
        sums[2] = __builtin_fma(u1[i], u1[i], sums[2]); sums[3] = __builtin_fma(v2[i], v2[i], sums[3]);
        sums[4] = __builtin_fma(v2[i], u2[i], sums[4]); sums[5] = __builtin_fma(u2[i], u2[i], sums[5]);
      }
      block_sum(sums, 6);
      lmax = sums[1] / sums[0];
      mu = sums[4] / sums[3];
      const double sc1 = sums[2] > 0.0 ? 1.0 / sqrt(sums[2]) : 0.0, sc2 = sums[5] > 0.0 ? 1.0 / sqrt(sums[5]) : 0.0;
      __syncthreads();
      for (int i = tid; i < N; i += BLOCK) { v1[i] = u1[i] * sc1; v2[i] = u2[i] * sc2; }
      __syncthreads();
    }
    const double pr = s_diag[0] / s_diag[1], est = lmax * mu;
    condition = est > pr * pr ? est : pr * pr;     // two lower bounds: the larger one
  }
  const double cfm = condition < 1e7 ? 0.0 : a.cfm_coeff;
  if (cfm != 0.0)
    for (int i = tid; i < N; i += BLOCK) A[(size_t)i * N + i] += cfm;
  __syncthreads();   // (every thread has read s_fail and A before they change)

  // ---- Lcp::MixedConstraintsSolver (lcp.cc:276-336): partition, Schur complement over the equality rows
  if (tid == 0) {
    int ne = 0, ni = 0;
    for (int i = 0; i < N; ++i) {
      if (vc[i] != 0.0) idxE[ne++] = i;
      else idxI[ni++] = i;
    }
    s_ne = ne; s_ni = ni; s_fail = 0;
  }
  __syncthreads();
  const int ne = s_ne, ni = s_ni, ni1 = ni + 1;
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
    cholesky(ne, nullptr);
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
  const bool box_fix = a.use_bounds != 0;
  for (int k = tid; k < ni; k += BLOCK) {
    lo[k] = box_fix ? vlo[idxI[k]] : 0.0;
    hi[k] = box_fix ? vhi[idxI[k]] : INFINITY;
    if (!(lo[k] < hi[k]) || !(lo[k] <= 0) || !(box_fix ? hi[k] >= 0 : hi[k] > 0)) s_badb = 1;   // lcp.cc:161-164
  }
  __syncthreads();
  const bool schur_failed = s_fail != 0;
  int solved = (!schur_failed && !s_badb) ? 1 : 0;
  int pivots = 0;

  // ---- MurtyPrincipalPivot on lhs (lcp.cc:157-274), the loop of murty_small_kernel
  if (solved && ni > 0) {
    const int n = ni;
    const double *M = Lh;
    const double p2 = pow(2.0, n);
    const int max_iterations = p2 > 1000 ? 1000 : (int)p2;   // lcp.cc:168
    for (int i = tid; i < n; i += BLOCK) {
      S[i] = 1; Cv[i] = lo[i];
      x[i] = 0.0; w[i] = -b[i]; r[i] = -b[i];   // lcp.cc:184-185
      bx[i] = 0.0; bw[i] = -b[i];
    }
    __syncthreads();
    auto check = [&]() {     // CheckMurtySolution (lcp.cc:20-103) + goodness (lcp.cc:107-113)
      if (tid == 0) { s_first = NONE; s_oob = 0; s_wbad = 0; }
      __syncthreads();
      for (int i = tid; i < n; i += BLOCK) {
        const double xi = x[i], wi = w[i];
        bool off;
        if (S[i]) off = (xi < lo[i]) || (xi > hi[i]);
        else off = (Cv[i] == lo[i] && wi < 0) || (Cv[i] == hi[i] && wi > 0);
        if (off) atomicMin(&s_first, i);
        if (xi < lo[i] || xi > hi[i]) s_oob = 1;
        if ((xi == lo[i] && wi < 0) || (xi == hi[i] && wi > 0)) s_wbad = 1;
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
        s_resid2 = res2; s_good = good;
      }
      __syncthreads();
    };
    auto is_solution = [&](double tol) { return s_first == NONE && !s_oob && !s_wbad && sqrt(s_resid2) <= tol; };
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
    if (tid == 0) s_best = s_good;
    __syncthreads();
    int iter = 0;
    bool force = box_fix;
    while (iter < max_iterations) {
      if (!force) {
        if (is_solution(1e-9)) { if (tid == 0) s_state = 1; __syncthreads(); break; }
        if (tid == 0 && s_first != NONE) {             // lcp.cc:36-62: flip the first offender
          const int i = s_first;
          if (S[i]) { S[i] = 0; Cv[i] = (x[i] < lo[i]) ? lo[i] : hi[i]; }
          else S[i] = 1;
        }
        __syncthreads();
      }
      force = false;
      if (tid == 0) {                                  // index list of S
        int ns = 0;
        for (int i = 0; i < n; ++i) if (S[i]) idx[ns++] = i;
        s_ns = ns;
      }
      for (int i = tid; i < n; i += BLOCK) x[i] = S[i] ? 0.0 : Cv[i];   // x = x_clamped
      __syncthreads();
      const int ns = s_ns;
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
      cholesky(ns, y);
      back_solve(ns, y);
      for (int k = tid; k < ns; k += BLOCK) x[idx[k]] = y[k];
      __syncthreads();
      residual_vector();                               // r = M x - b
      for (int i = tid; i < n; i += BLOCK) w[i] = S[i] ? 0.0 : r[i];     // lcp.cc:219-223
      __syncthreads();
      ++pivots;
      check();
      if (s_good > s_best) {                           // lcp.cc:125-137 (uniform: shared value)
        for (int i = tid; i < n; i += BLOCK) { bx[i] = x[i]; bw[i] = w[i]; }
        __syncthreads();
        if (tid == 0) s_best = s_good;
        __syncthreads();
      }
      ++iter;
      if (s_fail) break;
    }
    solved = (s_state == 1);
    if (!solved && !s_fail) {
      // capped: the best-seen iterate (reference rule only), re-checked at the looser 1e-8 (lcp.cc:241-246)
      if (!box_fix) {
        for (int i = tid; i < n; i += BLOCK) { x[i] = bx[i]; w[i] = bw[i]; }
        __syncthreads();
      }
      residual_vector();
      check();
      solved = is_solution(1e-8) ? 1 : 0;
    }
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
    cholesky(ne, y2);
    back_solve(ne, y2);
  }
  if (solved) {     // lambda in the world's order
    for (int k = tid; k < ne; k += BLOCK) {
      const int row = idxE[k];
      a.x[(size_t)3 * a.cons[c0 + row / 3] + row % 3] = y2[k];
    }
    for (int k = tid; k < ni; k += BLOCK) {
      const int row = idxI[k];
      a.x[(size_t)3 * a.cons[c0 + row / 3] + row % 3] = x[k];
    }
  }
  if (tid == 0) {
    DenseEnsStatus st;
    st.condition = condition; st.cfm = cfm; st.ok = solved; st.pivots = pivots;
    a.status[e] = st;
  }
}

__global__ void add_diag_kernel(double *A, int N, double cfm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) A[(size_t)i * N + i] += cfm;
}

__global__ void scatter_rows_kernel(const int32_t *cons_e, int N, const double *xs, double *x) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < N) x[(size_t)3 * cons_e[k / 3] + k % 3] = xs[k];
}

template <int MAXN, int BLOCK>
void launch_fused(const DenseWorldArgs &a, const int32_t *list, int count, hipStream_t s) {
  const size_t lds = (size_t)(MAXN * (MAXN + 1) / 2 + 11 * MAXN) * sizeof(double);
  hipLaunchKernelGGL((dense_world_fused_kernel<MAXN, BLOCK>), dim3(count), dim3(BLOCK), lds, s, a, list);
}

}  // namespace

void launch_dense_world_system(const DenseWorldArgs &a, int n_ens, int max_m, hipStream_t s) {
  const size_t pairs = (size_t)max_m * max_m;
  if (n_ens <= 0 || pairs == 0) return;
  hipLaunchKernelGGL(dense_world_system_kernel, dim3((unsigned)((pairs + 255) / 256), (unsigned)n_ens), dim3(256), 0, s, a);
}

void launch_dense_world_fused(const DenseWorldArgs &a, const int32_t *list, int count, int cls, hipStream_t s) {
  if (count <= 0) return;
  if (cls == 0) launch_fused<32, 64>(a, list, count, s);
  else if (cls == 1) launch_fused<64, 64>(a, list, count, s);
  else launch_fused<112, 256>(a, list, count, s);
}

void launch_dense_world_add_diag(double *A, int N, double cfm, hipStream_t s) {
  if (N <= 0) return;
  hipLaunchKernelGGL(add_diag_kernel, dim3((N + 255) / 256), dim3(256), 0, s, A, N, cfm);
}

void launch_dense_world_scatter(const int32_t *cons_e, int N, const double *xs, double *x, hipStream_t s) {
  if (N <= 0) return;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((N + 255) / 256), dim3(256), 0, s, cons_e, N, xs, x);
}

}  // namespace egs
