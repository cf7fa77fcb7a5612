// dense_world.hip -- Ensemble::ComputeVDot (ensembles.cc:498-538) for every ensemble of a world in two launches
// (egs_world_step_dense): the dense J M^-1 J^T of each ensemble, then ONE workgroup per ensemble runs the rest
// without the host: CheckMatrixCondition against kGoodConditionNumber = 1e7 (ensembles.cc:513-521), the Schur
// complement over the equality rows (lcp.cc:286-294), the reference's Murty loop on the inequality rows
// (lcp.cc:157-274, as murty_small_kernel in dense_murty.hip) and x_e = A_ee^-1 (b_e - A_ei x_i) (lcp.cc:317).
// dense_world_friction_kernel is the same body around the stage's pyramid form (egs_world_set_dense_friction): rows 0
// and 1 of a constraint with mu >= 0 are pyramid rows of its row 2, mu read per gathered constraint.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dense_world.h"
#include "mixed_solve_device.h"

namespace egs {

namespace {

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
struct NoWorldFriction {};

template <int MAXN, int BLOCK, bool PYR, typename Friction>
__device__ __forceinline__ void dense_world_body(double *sm, MixedSolveShared<MAXN> &sh, double (&s_diag)[2], double (&s_red)[BLOCK / 64][6],
                                                 const DenseWorldArgs &a, const int32_t *list, const Friction &fa) {
  const MixedSolveLds L(sm, MAXN);                  // the packed triangle (Cholesky factors of A, A_ee, A(S,S)) and the vectors
  double *T = L.T, *x = L.x, *w = L.w, *r = L.r, *y = L.y, *y2 = L.y2;
  const int tid = threadIdx.x;
  const int e = list[blockIdx.x];
  const int c0 = a.cstart[e];
  const int N = 3 * (a.cstart[e + 1] - c0);
  double *A = a.ws + a.ws_off[e];
  double *Z = A + (size_t)N * N;
  double *Lh = Z + (size_t)N * N + N;
  const double *vb = A + dense_ws_vec(N), *vlo = vb + N, *vhi = vb + 2 * N, *vc = vb + 3 * N;
  if constexpr (PYR) {      // mu per row, in the workspace's x vector (free on the fused path); read after the barriers below
    double *vmu = A + dense_ws_vec(N) + 4 * (size_t)N;
    for (int i = tid; i < N; i += BLOCK) vmu[i] = fa.mu[a.cons[c0 + i / 3]];
  }

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
  // ---- CheckMatrixCondition (ensembles.cc:513-521): cond_2(A) < 1e7 ?  A is positive definite here or singular.
  if (tid == 0) sh.fail = 0;
  for (int q = tid; q < N * N; q += BLOCK) {
    const int rr = q / N, cc = q - rr * N;
    if (cc <= rr) T[dtri(rr, cc)] = A[q];
  }
  __syncthreads();
  packed_cholesky<BLOCK>(T, N, nullptr, &sh.fail);
  double condition = INFINITY;
  if (!sh.fail) {
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
    // and the 60 iterations of dense_condition_estimate (dense_factor.hip); Rayleigh quotients, both from below
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
  __syncthreads();   // (every thread has read sh.fail and A before they change)

  // ---- Lcp::MixedConstraintsSolver (lcp.cc:276-336): the stage mixed_batch_kernel shares (mixed_solve_device.h)
  MixedPyramid<PYR> pyr;
  if constexpr (PYR) {
    const double *vmu = vb + 4 * (size_t)N;
    pyr.nrow = nullptr; pyr.mu = vmu;
    pyr.max_outer = fa.max_outer; pyr.tol = fa.tol;
    pyr.ext = sm + mixed_solve_lds_doubles(MAXN);
    pyr.outer = 0; pyr.change = 0.0;
    mixed_partition(sh, N, [&](int i) { return vc[i] != 0.0 && pyr.normal_of(i) < 0; });     // a pyramid row is an inequality row
  } else {
    mixed_partition(sh, N, [&](int i) { return vc[i] != 0.0; });
  }
  const MixedSolveResult res = mixed_solve_stage<MAXN, BLOCK, PYR>(sh, L, A, N, vb, vlo, vhi, Z, Lh, a.use_bounds, 0, pyr);
  const int ne = sh.ne, ni = sh.ni, solved = res.solved, pivots = res.pivots;
  const int *idxE = sh.idxE, *idxI = sh.idxI;
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
    if constexpr (PYR) {
      DenseFrictionStatus fs;
      fs.change = solved ? pyr.change : 0.0;
      fs.outer = (solved && pyr.outer == 0) ? 1 : pyr.outer;
      fs.converged = (solved && fs.change <= fa.tol) ? 1 : 0;
      fa.status[e] = fs;
    }
  }
}

template <int MAXN, int BLOCK>
__global__ void __launch_bounds__(BLOCK) dense_world_fused_kernel(DenseWorldArgs a, const int32_t *list) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ MixedSolveShared<MAXN> sh;
  __shared__ double s_diag[2];
  __shared__ double s_red[BLOCK / 64][6];
  dense_world_body<MAXN, BLOCK, false>(sm, sh, s_diag, s_red, a, list, NoWorldFriction{});
}

template <int MAXN, int BLOCK>
__global__ void __launch_bounds__(BLOCK) dense_world_friction_kernel(DenseWorldArgs a, const int32_t *list, DenseWorldFriction fa) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ MixedSolveShared<MAXN> sh;
  __shared__ double s_diag[2];
  __shared__ double s_red[BLOCK / 64][6];
  dense_world_body<MAXN, BLOCK, true>(sm, sh, s_diag, s_red, a, list, fa);
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
  const size_t lds = mixed_solve_lds_doubles(MAXN) * sizeof(double);
  hipLaunchKernelGGL((dense_world_fused_kernel<MAXN, BLOCK>), dim3(count), dim3(BLOCK), lds, s, a, list);
}

template <int MAXN, int BLOCK>
void launch_friction(const DenseWorldArgs &a, const DenseWorldFriction &fa, const int32_t *list, int count, hipStream_t s) {
  const size_t lds = mixed_pyramid_lds_doubles(MAXN) * sizeof(double);
  hipLaunchKernelGGL((dense_world_friction_kernel<MAXN, BLOCK>), dim3(count), dim3(BLOCK), lds, s, a, list, fa);
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

void launch_dense_world_friction(const DenseWorldArgs &a, const DenseWorldFriction &fa, const int32_t *list, int count, int cls,
                                 hipStream_t s) {
  if (count <= 0) return;
  if (cls == 0) launch_friction<32, 64>(a, fa, list, count, s);
  else if (cls == 1) launch_friction<64, 64>(a, fa, list, count, s);
  else launch_friction<112, 256>(a, fa, list, count, s);
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
