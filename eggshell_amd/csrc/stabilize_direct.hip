// stabilize_direct.hip -- the direct relaxation route (stabilize_direct.h): per ensemble one workgroup that assembles
// its constraints, tests err_sq, forms the lower triangle of A = J J^T, factorises it by a rank-revealing pivoted
// LDL^T, solves, sums J^T y per body in list order and moves the bodies -- every pass of a fixed constraint list
// inside one launch.  Every order of operations depends on the ensemble's own rows only, so an ensemble of a batch
// ends with the bits a world holding it alone ends with.
#include "stabilize_direct.h"

#include "assemble_device.h"
#include "runtime.h"
#include "stabilize_device.h"

namespace egs {

namespace {

__host__ __device__ constexpr int tri(int r) { return r * (r + 1) / 2; }

// Where a workgroup keeps its ensemble.  A: packed lower triangle, A(r, c) at tri(r) + c; J: constraint i's J0 block at
// 36 i, its J1 block at 36 i + 18; b: err, then the solve's running vector (pivoted order); y: the solution in row
// order; lcol / ccol: the column being eliminated, scaled and unscaled; G, hv: the packed Gram matrix and right-hand
// side of the least-squares completion (direct_factor_solve).
struct DirectMem {
  double *A, *G, *J, *b, *y, *lcol, *ccol, *hv, *red;
  int32_t *perm, *cb0, *cb1, *ipiv;
};

template <int CAP, bool GLOBAL>
__host__ __device__ constexpr size_t direct_lds_bytes() {
  return ((GLOBAL ? 0 : 2 * (size_t)tri(CAP) + 12 * (size_t)CAP) + 5 * (size_t)CAP + 2) * sizeof(double) +
         ((size_t)CAP + 2 * ((size_t)CAP / 3 + 1) + 2) * sizeof(int32_t);
}

template <int CAP, bool GLOBAL>
__device__ __forceinline__ DirectMem direct_carve(double *sm, double *ws, int N) {
  DirectMem M;
  double *v = sm;
  if (GLOBAL) {
    M.A = ws;
    M.G = ws + tri(N);
    M.J = M.G + tri(N);
  } else {
    M.A = sm;
    M.G = sm + tri(CAP);
    M.J = M.G + tri(CAP);
    v = M.J + 12 * CAP;
  }
  M.b = v; M.y = v + CAP; M.lcol = v + 2 * CAP; M.ccol = v + 3 * CAP; M.hv = v + 4 * CAP; M.red = v + 5 * CAP;
  M.perm = reinterpret_cast<int32_t *>(M.red + 2);
  M.cb0 = M.perm + CAP;
  M.cb1 = M.cb0 + (CAP / 3 + 1);
  M.ipiv = M.cb1 + (CAP / 3 + 1);
  return M;
}

// sum of b_i^2 over the N rows: lane l of the first wavefront sums rows l, l + 64, ... in order, then a fixed
// butterfly over the 64 partial sums.  Every thread returns the same value.
__device__ __forceinline__ double direct_err_sq(const DirectMem &M, int N, int t) {
  if (t < 64) {
    double s = 0.0;
    for (int r = t; r < N; r += 64) s += M.b[r] * M.b[r];
    for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
    if (t == 0) M.red[0] = s;
  }
  __syncthreads();
  return M.red[0];
}

// The lower triangle of A = J J^T, one 3x3 block per pair of constraints j <= i; a pair that shares no body gives
// zeros.  Per entry: the term of i's body0, then the term of i's body1.
template <int NT>
__device__ __forceinline__ void direct_system(const DirectMem &M, int me, int t) {
  const int pairs = tri(me);
  for (int idx = t; idx < pairs; idx += NT) {
    int i = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
    while (tri(i + 1) <= idx) ++i;
    while (tri(i) > idx) --i;
    const int j = idx - tri(i);
    const int a0 = M.cb0[i], a1 = M.cb1[i], c0 = M.cb0[j], c1 = M.cb1[j];
    // the side of j that holds i's body0 / body1 (-1: none)
    const int s0 = a0 < 0 ? -1 : a0 == c0 ? 0 : a0 == c1 ? 1 : -1;
    const int s1 = a1 < 0 ? -1 : a1 == c0 ? 0 : a1 == c1 ? 1 : -1;
    const double *Ji = M.J + 36 * i, *Jj = M.J + 36 * j;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (i == j && c > r) continue;
        double s = 0.0;
        if (s0 >= 0) s = dot6p(Ji + 6 * r, Jj + 18 * s0 + 6 * c);
        if (s1 >= 0) s = s + dot6p(Ji + 18 + 6 * r, Jj + 18 * s1 + 6 * c);
        M.A[tri(3 * i + r) + 3 * j + c] = s;
      }
  }
}

// G x = h in place for the packed symmetric positive definite G (n x n): LDL^T without pivoting, h eliminated along
// with it, then the diagonal and backward solves.  x replaces h.
template <int NT, int TX>
__device__ __forceinline__ void direct_spd_solve(const DirectMem &M, int n, int t) {
  double *G = M.G, *h = M.hv;
  for (int k = 0; k < n; ++k) {
    const double d = G[tri(k) + k], hk = h[k];
    for (int i = k + 1 + t; i < n; i += NT) {
      const double c = G[tri(i) + k], l = c / d;
      M.ccol[i] = c;
      M.lcol[i] = l;
      G[tri(i) + k] = l;
      h[i] = h[i] - l * hk;
    }
    __syncthreads();
    for (int i = k + 1 + t / TX; i < n; i += NT / TX) {
      const double l = M.lcol[i];
      double *row = G + tri(i);
      for (int j = k + 1 + t % TX; j <= i; j += TX) row[j] = row[j] - l * M.ccol[j];
    }
    __syncthreads();
  }
  for (int i = t; i < n; i += NT) h[i] = h[i] / G[tri(i) + i];
  __syncthreads();
  for (int k = n - 1; k > 0; --k) {
    const double xk = h[k];
    const double *row = G + tri(k);
    for (int i = t; i < k; i += NT) h[i] = h[i] - row[i] * xk;
    __syncthreads();
  }
}

// In-place LDL^T of the packed A with symmetric diagonal pivoting (largest |diagonal|, lowest index on ties, as
// oracle/lcp_dense.c:14-51), b eliminated along with it, truncated at the first pivot <= rank_tol * |first pivot|;
// then the diagonal and backward solves on the leading rank block.  Leaves y in row order (0 on the rows left) and
// returns the rank.  TX lanes run along a row of the trailing update.
//
// Truncated at rank r < N, the rows left of the eliminated b hold rho = b2 - T b1 (T = L2 L1^-1: the rows left are T
// times the leading ones).  rho = 0 when b is consistent, and then the leading block alone gives J^T y.  Otherwise the
// least-squares correction J^T (J J^T)^+ b -- what the sweep route converges to -- is J^T [y1; 0] with the leading
// block solved for z = L1^-1 b1 + (W^T W)^-1 L2^T rho in place of L1^-1 b1, W = [L1; L2] the N x r unit lower
// trapezoid: the completion below, an r x r positive definite solve.
template <int NT, int TX>
__device__ __forceinline__ int direct_factor_solve(const DirectMem &M, int N, double rank_tol, int t) {
  double *A = M.A, *b = M.b;
  for (int i = t; i < N; i += NT) { M.perm[i] = i; M.y[i] = 0.0; }
  __syncthreads();
  int rank = N;
  double d0 = 0.0;
  for (int k = 0; k < N; ++k) {
    if (t < 64) {   // the pivot: one wavefront, no barrier inside
      double best = -1.0;
      int bi = N;
      for (int i = k + t; i < N; i += 64) {
        const double v = fabs(A[tri(i) + i]);
        if (v > best) { best = v; bi = i; }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
      }
      if (t == 0) M.ipiv[0] = bi < N ? bi : k;   // every diagonal NaN: stay, the test below stops
    }
    __syncthreads();
    const int p = M.ipiv[0];
    if (p != k) {   // symmetric swap of rows / columns k and p > k on the packed triangle
      for (int j = t; j < N; j += NT) {
        int u, v;
        if (j < k) { u = tri(k) + j; v = tri(p) + j; }
        else if (j == k) { u = tri(k) + k; v = tri(p) + p; }
        else if (j < p) { u = tri(j) + k; v = tri(p) + j; }
        else if (j > p) { u = tri(j) + k; v = tri(j) + p; }
        else continue;   // A(p, k) stays
        const double x = A[u];
        A[u] = A[v];
        A[v] = x;
      }
      if (t == 0) {
        const int32_t q = M.perm[k]; M.perm[k] = M.perm[p]; M.perm[p] = q;
        const double x = b[k]; b[k] = b[p]; b[p] = x;
      }
    }
    __syncthreads();
    const double d = A[tri(k) + k];
    if (k == 0) d0 = fabs(d);
    if (!(fabs(d) > rank_tol * d0)) { rank = k; break; }   // uniform: d comes from memory behind a barrier
    const double bk = b[k];
    for (int i = k + 1 + t; i < N; i += NT) {
      const double c = A[tri(i) + k], l = c / d;
      M.ccol[i] = c;
      M.lcol[i] = l;
      A[tri(i) + k] = l;
      b[i] = b[i] - l * bk;
    }
    __syncthreads();
    for (int i = k + 1 + t / TX; i < N; i += NT / TX) {
      const double l = M.lcol[i];
      double *row = A + tri(i);
      for (int j = k + 1 + t % TX; j <= i; j += TX) row[j] = row[j] - l * M.ccol[j];
    }
    __syncthreads();
  }
  if (rank > 0 && rank < N) {
    // h = L2^T rho and G = W^T W, every sum over the rows in ascending order
    for (int j = t; j < rank; j += NT) {
      double hsum = 0.0;
      for (int k = rank; k < N; ++k) hsum += A[tri(k) + j] * b[k];
      M.hv[j] = hsum;
    }
    for (int i = t / TX; i < rank; i += NT / TX)
      for (int j = t % TX; j <= i; j += TX) {
        double g = j == i ? 1.0 : A[tri(i) + j];   // row i of W: W(i, i) = 1
        for (int k = i + 1; k < N; ++k) g += A[tri(k) + i] * A[tri(k) + j];
        M.G[tri(i) + j] = g;
      }
    __syncthreads();
    direct_spd_solve<NT, TX>(M, rank, t);
    for (int i = t; i < rank; i += NT) b[i] = b[i] + M.hv[i];
    __syncthreads();
  }
  for (int i = t; i < rank; i += NT) b[i] = b[i] / A[tri(i) + i];
  __syncthreads();
  for (int k = rank - 1; k > 0; --k) {
    const double zk = b[k];
    const double *row = A + tri(k);
    for (int i = t; i < k; i += NT) b[i] = b[i] - row[i] * zk;
    __syncthreads();
  }
  for (int i = t; i < rank; i += NT) M.y[M.perm[i]] = b[i];
  __syncthreads();
  return rank;
}

template <int NT, int CAP, bool GLOBAL>
__global__ void __launch_bounds__(NT) stab_direct_kernel(StabDirectArgs a, const int32_t *list) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int TX = GLOBAL ? 64 : NT == 64 ? 8 : 16;
  const int e = list[blockIdx.x], t = threadIdx.x;
  if (!a.first && !a.active[e]) return;   // frozen: bodies, steps, err_sq and rank stay as they are
  const int c0 = a.cstart[e], me = a.cstart[e + 1] - c0, N = 3 * me;
  if (N > CAP) return;                    // never listed (the host sorts by size); keeps every index in bounds
  const DirectMem M = direct_carve<CAP, GLOBAL>(sm, GLOBAL ? a.ws + a.ws_off[e] : nullptr, N);
  const int bb = a.bo ? a.bo[e] : 0, nb = (a.bo ? a.bo[e + 1] : a.as.n) - bb;
  for (int i = t; i < me; i += NT) {
    const int c = a.cons[c0 + i];
    M.cb0[i] = a.as.body0[c];
    M.cb1[i] = a.as.body1[c];
  }
  int steps = a.first ? 0 : a.steps[e] + 1;   // the launch before relaxed this ensemble
  int rank = a.first ? 0 : a.rank[e];
  double err_sq;
  bool go;
  for (;;) {
    for (int i = t; i < me; i += NT) {   // J and err at the current body state, assemble_kernel's operations
      if (a.slider && a.as.kind[a.cons[c0 + i]] == 5) continue;   // a slider's block: the pass below
      double j0[18], j1[18], ev[3], lo[3], hi[3], u0[6], u1[6];
      bool eq[3];
      assemble_one(a.as, a.cons[c0 + i], j0, j1, ev, lo, hi, eq, u0, u1);
#pragma unroll
      for (int k = 0; k < 18; ++k) { M.J[36 * i + k] = j0[k]; M.J[36 * i + 18 + k] = j1[k]; }
#pragma unroll
      for (int k = 0; k < 3; ++k) M.b[3 * i + k] = ev[k];
    }
    if (a.limit)   // an active stop: err[2] = sin(theta - limit); a pass of its own, so that the blocks above keep their registers
      for (int i = t; i < me; i += NT) {
        double err2, lo2, hi2;
        if (limit_row(a.as, a.limit, a.cons[c0 + i], err2, lo2, hi2)) M.b[3 * i + 2] = err2;
      }
    if (a.slider)   // the slider blocks, and an active travel stop's err[2] = x - limit: a pass of its own for the same reason
      for (int i = t; i < me; i += NT) {
        const int c = a.cons[c0 + i];
        if (a.as.kind[c] != 5) continue;
        double d[7], j0[18], j1[18], ev[3];
#pragma unroll
        for (int k = 0; k < 7; ++k) d[k] = a.as.data[(size_t)c * 7 + k];
#pragma unroll
        for (int k = 0; k < 18; ++k) { j0[k] = 0.0; j1[k] = 0.0; }
        slider_block(a.as, a.as.body0[c], a.as.body1[c], d, j0, j1, ev);
        double lo2, hi2;
        if (a.travel) slider_stop_row(a.as, a.travel, c, ev[2], lo2, hi2);
#pragma unroll
        for (int k = 0; k < 18; ++k) { M.J[36 * i + k] = j0[k]; M.J[36 * i + 18 + k] = j1[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) M.b[3 * i + k] = ev[k];
      }
    __syncthreads();
    err_sq = direct_err_sq(M, N, t);
    go = err_sq > a.threshold && steps < a.max_steps;   // ensembles.cc:610, 632 (NaN stops)
    if (!go) break;
    direct_system<NT>(M, me, t);
    __syncthreads();
    rank = direct_factor_solve<NT, TX>(M, N, a.rank_tol, t);
    for (int q = t; q < nb; q += NT) {   // J^T y of body q in list order, then its relaxation step
      const int gb = bb + q;
      double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int i = 0; i < me; ++i)
#pragma unroll
        for (int side = 0; side < 2; ++side) {
          if ((side ? M.cb1[i] : M.cb0[i]) != gb) continue;
          const double *J = M.J + 36 * i + 18 * side;
#pragma unroll
          for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) acc[c] += J[6 * r + c] * M.y[3 * i + r];
        }
      stab_relax_body(acc, a.scale, a.h, a.post, a.pos + (size_t)gb * 3, a.R + (size_t)gb * 9, a.v + (size_t)gb * 3,
                      a.w + (size_t)gb * 3);
    }
    __syncthreads();   // the moved bodies are read by the next pass's assembly
    if (!a.loop) break;
    ++steps;
  }
  if (t != 0) return;
  a.steps[e] = steps;
  a.err_sq[e] = err_sq;
  a.rank[e] = rank;
  a.active[e] = go ? 1 : 0;
  if (go) atomicAdd(a.n_active, 1);
}

template <int NT, int CAP, bool GLOBAL>
__global__ void __launch_bounds__(NT) relax_direct_kernel(RelaxDirectArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int TX = GLOBAL ? 64 : NT == 64 ? 8 : 16;
  const int t = threadIdx.x, me = a.m, N = 3 * me;
  if (N > CAP) return;
  const DirectMem M = direct_carve<CAP, GLOBAL>(sm, GLOBAL ? a.ws : nullptr, N);
  for (int i = t; i < me; i += NT) { M.cb0[i] = a.body0[i]; M.cb1[i] = a.body1[i]; }
  for (int k = t; k < 18 * me; k += NT) {
    const int i = k / 18, q = k % 18;
    M.J[36 * i + q] = a.J0[k];
    M.J[36 * i + 18 + q] = a.J1[k];
  }
  for (int r = t; r < N; r += NT) M.b[r] = a.err[r];
  __syncthreads();
  direct_system<NT>(M, me, t);
  __syncthreads();
  const int rank = direct_factor_solve<NT, TX>(M, N, a.rank_tol, t);
  for (int r = t; r < N; r += NT) a.y[r] = M.y[r];
  if (t == 0) *a.rank = rank;
}

template <int NT, int CAP, bool GLOBAL, typename K, typename... ARGS>
void launch_direct(K kernel, int blocks, hipStream_t s, ARGS... args) {
  constexpr size_t lds = direct_lds_bytes<CAP, GLOBAL>();
  if (lds > 48 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(NT), lds, s, args...);
}

}  // namespace

void launch_stab_direct(const StabDirectArgs &a, const int32_t *list, int count, int cls, hipStream_t s) {
  if (count <= 0) return;
  if (cls == 0) launch_direct<64, kDirectSmallRows, false>(stab_direct_kernel<64, kDirectSmallRows, false>, count, s, a, list);
  else if (cls == 1) launch_direct<256, kDirectLdsRows, false>(stab_direct_kernel<256, kDirectLdsRows, false>, count, s, a, list);
  else launch_direct<512, kDirectMaxRows, true>(stab_direct_kernel<512, kDirectMaxRows, true>, count, s, a, list);
}

void launch_relax_direct(const RelaxDirectArgs &a, hipStream_t s) {
  const int cls = direct_class(3 * a.m);
  if (cls == 0) launch_direct<64, kDirectSmallRows, false>(relax_direct_kernel<64, kDirectSmallRows, false>, 1, s, a);
  else if (cls == 1) launch_direct<256, kDirectLdsRows, false>(relax_direct_kernel<256, kDirectLdsRows, false>, 1, s, a);
  else launch_direct<512, kDirectMaxRows, true>(relax_direct_kernel<512, kDirectMaxRows, true>, 1, s, a);
}

}  // namespace egs
