// dense_murty.hip -- Lcp::MurtyPrincipalPivot (lcp.cc:157-274) with the pivot loop's state on the device.
// The reference's single-index principal pivoting verbatim -- S starts all-true, x = 0, w = -b; each iteration flips the
// FIRST offending index (lcp.cc:36-62) and re-solves A(S,S) x_S = b_S from scratch (lcp.cc:202-203): gather + Cholesky +
// a product with L^-T (dense_factor.hip), or a bordered system on the last factor (border_* kernels); the flip decision,
// best-solution memory (lcp.cc:105-137) and the iteration cap min(1000, 2^dim) (lcp.cc:168) are evaluated per pivot from
// a 64-byte record read back from the device (MurtyStep, dense_internal.h).  Up to 112 rows the whole loop runs in one
// workgroup instead (murty_small_kernel).  A(S,S) must be positive definite; otherwise the call reports failure.
#include "dense_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <stdexcept>

namespace egs {

namespace {

// out = M v - sub  (row-major M n x n): one wavefront per row.
__global__ void __launch_bounds__(256) gemv_minus_kernel(const double *M, int n, const double *v, const double *sub,
                                                         double *out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  double s = 0.0;
  for (int c = lane; c < n; c += 64) s = __builtin_fma(M[(size_t)row * n + c], v[c], s);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (lane == 0) out[row] = s - sub[row];
}

// ---- the pivot loop's state lives on the device ----------------------------------------------------------
// Round 2's loop downloaded x and w, chose the flips on the host and uploaded S, C and the index list again: seven
// small pageable copies per pivot, ~0.1 ms of the 0.37 ms a pivot of the N = 2048 problem took.  Now the host sees one
// 64-byte record per pivot (MurtyStep, written straight into pinned host memory) and everything else stays where it is:
//   murty_init_kernel     S = 1, C = lo, x = 0, w = r = -b (lcp.cc:184-185), best-iterate memory
//   murty_prep_kernel     x(!S) = C and b_eff = b - A(:, !S) x(!S)
//   murty_resid_kernel    r = A x - b, w = S ? 0 : r (lcp.cc:219-223)
//   murty_advance_kernel  CheckMurtySolution (lcp.cc:20-103) + best-iterate memory (lcp.cc:125-137) + the flips of the
//                         NEXT pivot (single index, lcp.cc:36-62, or the block rule) + the ascending index list of S
struct MurtyState {       // block-rule and best-iterate memory, device resident
  int best_ninf, patience;
  double best_good;
  int have_best, pad;
};

// guess: the block rule may start from any set.  A row whose bound is 0 on the side b points away from (lo = 0 and
// b <= 0: x = 0, w = -b >= 0 is consistent on its own) starts outside S at that bound instead of inside: on the N = 2048
// problem the first system has 470 rows instead of 985 and the rule needs 6 pivots instead of 8.
__global__ void murty_init_kernel(int n, const double *b, const double *lo, const double *hi, int guess, uint8_t *S, double *Cb, double *x,
                                  double *w, double *r, double *bx, double *bw, MurtyState *st) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) { st->best_ninf = n + 1; st->patience = 10; st->best_good = 0.0; st->have_best = 0; st->pad = 0; }
  if (i < n) {
    const double nb = -b[i];
    const bool at_lo = guess && lo[i] == 0.0 && b[i] <= 0.0, at_hi = guess && !at_lo && hi[i] == 0.0 && b[i] >= 0.0;
    S[i] = (at_lo || at_hi) ? 0 : 1; Cb[i] = at_hi ? hi[i] : lo[i]; x[i] = 0.0; w[i] = nb; r[i] = nb; bx[i] = 0.0; bw[i] = nb;
  }
}

// one wavefront per row: beff = b - A xc (box problems; the reference's own loop drops the term, lcp.cc:199-216),
// x = xc, xc = S ? 0 : C
__global__ void __launch_bounds__(256) murty_prep_kernel(const double *M, int n, const double *b, const uint8_t *S,
                                                         const double *Cb, int box_fix, double *beff, double *x) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  double s = 0.0;
  if (box_fix) {
    for (int c = lane; c < n; c += 64) s = __builtin_fma(M[(size_t)row * n + c], S[c] ? 0.0 : Cb[c], s);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  }
  if (lane == 0) {
    beff[row] = box_fix ? -(s - b[row]) : b[row];
    x[row] = S[row] ? 0.0 : Cb[row];
  }
}

__global__ void __launch_bounds__(256) murty_resid_kernel(const double *M, int n, const double *x, const double *b,
                                                          const uint8_t *S, double *r, double *w) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  double s = 0.0;
  for (int c = lane; c < n; c += 64) s = __builtin_fma(M[(size_t)row * n + c], x[c], s);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (lane == 0) {
    const double rr = s - b[row];
    r[row] = rr;
    w[row] = S[row] ? 0.0 : rr;
  }
}

// mode 0: check only; 1: flip the first offender (the reference's rule); 2: the block rule.  Single workgroup.
__global__ void __launch_bounds__(1024) murty_advance_kernel(int n, const double *x, const double *w, const double *r, uint8_t *S,
                                                             double *Cb, const double *lo, const double *hi, int mode, double tol,
                                                             int keep_best, MurtyState *st, double *bx, double *bw, int *idx,
                                                             const int *fail_a, const int *fail_b, MurtyStep *out,
                                                             const int *pos0, const int *idx0, int n0, int *Dl, int *Rl, int list_cap, int seq) {
  __shared__ int s_first, s_last, s_ninf, s_oob, s_wbad, s_improved, s_all, s_flip, s_flipped;
  __shared__ double s_res[1024], s_good[1024];
  __shared__ unsigned long long s_wave[16];
  const int tid = threadIdx.x;
  if (tid == 0) { s_first = 0x7fffffff; s_last = -1; s_ninf = 0; s_oob = 0; s_wbad = 0; s_flipped = 0; }
  __syncthreads();
  auto offender = [&](int i, double xi, double wi) {
    if (S[i]) return (xi < lo[i]) || (xi > hi[i]);
    return (Cb[i] == lo[i] && wi < 0) || (Cb[i] == hi[i] && wi > 0);
  };
  double res = 0.0, good = 0.0;
  for (int i = tid; i < n; i += 1024) {
    const double xi = x[i], wi = w[i];
    if (offender(i, xi, wi)) { atomicMin(&s_first, i); atomicMax(&s_last, i); atomicAdd(&s_ninf, 1); }
    if (xi < lo[i] || xi > hi[i]) s_oob = 1;
    if ((xi == lo[i] && wi < 0) || (xi == hi[i] && wi > 0)) s_wbad = 1;
    const double d = r[i] - wi;   // (A x - b) - w
    res += d * d;
    if (!(xi > 0)) good += xi;
    if (!(wi > 0)) good += wi;
  }
  s_res[tid] = res; s_good[tid] = good;
  __syncthreads();
  for (int k = 512; k > 0; k >>= 1) {
    if (tid < k) { s_res[tid] += s_res[tid + k]; s_good[tid] += s_good[tid + k]; }
    __syncthreads();
  }
  if (tid == 0) {
    const bool solution = s_first == 0x7fffffff && !s_oob && !s_wbad && sqrt(s_res[0]) <= tol;
    s_improved = keep_best && (!st->have_best || s_good[0] > st->best_good);
    if (s_improved) { st->best_good = s_good[0]; st->have_best = 1; }
    bool all = true;
    int flip = 0;
    if (mode != 0 && !solution && s_first != 0x7fffffff) {
      flip = 1;
      if (mode == 2) {      // every infeasible index while their number keeps falling, else the largest one
        if (s_ninf < st->best_ninf) { st->best_ninf = s_ninf; st->patience = 10; }
        else if (st->patience > 0) --st->patience;
        else all = false;
      }
    }
    s_flip = flip; s_all = all ? 1 : 0;
  }
  __syncthreads();
  if (s_improved) for (int i = tid; i < n; i += 1024) { bx[i] = x[i]; bw[i] = w[i]; }
  if (s_flip) {
    const int one = (mode == 1) ? s_first : (s_all ? -1 : s_last);
    for (int i = tid; i < n; i += 1024) {
      const double xi = x[i];
      const bool mine = one >= 0 ? (i == one) : offender(i, xi, w[i]);
      if (mine) {
        if (S[i]) { S[i] = 0; Cb[i] = (xi < lo[i]) ? lo[i] : hi[i]; }   // lcp.cc:36-62
        else S[i] = 1;
        atomicAdd(&s_flipped, 1);
      }
    }
  }
  __syncthreads();
  // the ascending index list of S, and the difference against the factored base set S0 = idx0[0 .. n0): D = S \ S0,
  // R = S0 \ S, ascending.  Thread t owns a run of consecutive indexes; ONE scan over the packed counts (|S| in the low
  // word, |D| and |R| in 16 bits each: n < 32768 when the base is tracked), inside the wavefronts by shuffles, across them
  // through LDS.  pos0 is never cleared: an entry counts only if idx0 points back at it.
  auto in_base = [&](int i) { const int q = pos0[i]; return q >= 0 && q < n0 && idx0[q] == i; };
  const int per = (n + 1023) / 1024, i0 = tid * per, i1 = min(n, i0 + per);
  unsigned long long mine = 0;
  for (int i = i0; i < i1; ++i) {
    const bool in_s = S[i] != 0;
    mine += in_s ? 1ull : 0ull;
    if (pos0) {
      const bool in0 = in_base(i);
      if (in_s && !in0) mine += 1ull << 32;
      if (!in_s && in0) mine += 1ull << 48;
    }
  }
  unsigned long long incl = mine, total = 0;
  {
    const int lane = tid & 63;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    unsigned long long before = 0;
    for (int k = 0; k < 16; ++k) { if (k < (tid >> 6)) before += s_wave[k]; total += s_wave[k]; }
    incl += before;
  }
  const unsigned long long excl = incl - mine;
  const int ns_total = (int)(total & 0xffffffffull);
  int nd_total = -1, nr_total = -1;
  {
    int pos = (int)(excl & 0xffffffffull);
    for (int i = i0; i < i1; ++i) if (S[i]) idx[pos++] = i;
  }
  if (pos0) {
    nd_total = (int)((total >> 32) & 0xffff); nr_total = (int)(total >> 48);
    if (nd_total + nr_total <= list_cap) {
      int pd = (int)((excl >> 32) & 0xffff), pr = (int)(excl >> 48);
      for (int i = i0; i < i1; ++i) {
        const bool in0 = in_base(i);
        if (S[i] && !in0) Dl[pd++] = i;
        if (!S[i] && in0) Rl[pr++] = i;
      }
    }
  }
  if (tid == 0) {
    out->first_offender = s_first; out->out_of_bounds = s_oob; out->w_bad = s_wbad;
    out->fail = (fail_a ? *fail_a : 0) | (fail_b ? *fail_b : 0);
    out->resid2 = s_res[0]; out->goodness = s_good[0];
    out->ns = ns_total; out->ninf = s_ninf; out->flipped = s_flipped; out->nd = nd_total; out->nr = nr_total;
    __threadfence_system();
    __hip_atomic_store(&out->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- pivots that differ little from a factored one ---------------------------------------------------------
// Block pivoting ends with a few small corrections of S (the N = 2048 problem: 486, 440, 226, 121, 40, 11, 2 flips), the
// reference's single-index rule changes one index per pivot -- and a fresh factorisation costs the same 64-column
// latency chain every time.  With S0 the set of the last factorisation (L and W = L^-T in T, see factor()), D = S \ S0
// and R = S0 \ S, m = |D| + |R| <= 64, the new x solves the bordered system
//     [A00  A0D  E_R] [x0]   [b0]
//     [AD0  ADD   0 ] [xD] = [bD]          (the multipliers mu pin x_R = 0)
//     [E_R'  0    0 ] [mu]   [0 ]
// by block elimination on the old factor:  Y = L^-1 [A0D E_R],  z0 = L^-1 b0,  C = [ADD 0; 0 0] - Y'Y (quasi-definite:
// no pivoting needed),  C zz = [bD; 0] - Y'z0,  x0 = W (z0 - Y zz): two products with W (parallel over all CUs), one
// m x m elimination in one workgroup -- no panel chain.
constexpr int kBorderMax = 64;            // m
constexpr int kBorderStride = 68;         // row stride of U and Y: m + 1 columns (the last is b0 / z0), padded

// U (n0pad x kBorderStride): columns A(S0, D), E_R, b0; rows beyond n0 zero
__global__ void border_build_kernel(const double *A, int n, const double *beff, const int *idx0, int n0, int n0pad, const int *pos0,
                                    const int *Dl, int nd, const int *Rl, int nr, double *U) {
  const int m = nd + nr;
  const size_t total = (size_t)n0pad * kBorderStride;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(e / kBorderStride), j = (int)(e % kBorderStride);
    double v = 0.0;
    if (k < n0) {
      if (j < nd) v = A[(size_t)idx0[k] * n + Dl[j]];
      else if (j < m) v = (pos0[Rl[j - nd]] == k) ? 1.0 : 0.0;
      else if (j == m) v = beff[idx0[k]];
    }
    U[e] = v;
  }
}

// Y = L^-1 U = W'U (W[k][c] = T[ibase + k][c], zero for k > c) in 64 x 64 tiles of W: workgroup (tile (cb, kb <= cb), column
// quarter jq) forms Yp[kb][cb 64 + c][j] = sum over the tile's k of W[k][c] U[k][j] for 17 columns j.  Both operands are
// read along k-major rows and staged in LDS; lane = c, wavefront w takes the columns jq 17 + w, + 4, ... (its U reads are
// wavefront-uniform broadcasts).
constexpr int kBorderJ = kBorderStride / 4;      // 17 columns per quarter
__global__ void __launch_bounds__(256) border_forward_kernel(const double *T, int ld, int ibase, int n0, const double *U, double *Yp,
                                                             int n0pad) {
  __shared__ double sW[NB][NB + 1], sU[NB][kBorderJ + 1];
  int cbi = 0, t = blockIdx.x;      // tile index -> (cb, kb), kb <= cb
  while (t > cbi) { t -= cbi + 1; ++cbi; }
  const int kbi = t, cb = cbi * NB, kb = kbi * NB, j0 = blockIdx.y * kBorderJ;
  for (int e = threadIdx.x; e < NB * NB; e += 256) {
    const int k = e >> 6, c = e & 63;
    sW[k][c] = (kb + k < n0 && kb + k <= cb + c) ? T[(size_t)(ibase + kb + k) * ld + cb + c] : 0.0;
  }
  for (int e = threadIdx.x; e < NB * kBorderJ; e += 256) {
    const int k = e / kBorderJ, j = e % kBorderJ;
    sU[k][j] = U[(size_t)(kb + k) * kBorderStride + j0 + j];
  }
  __syncthreads();
  const int c = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int NJ = (kBorderJ + 3) / 4;      // 5 columns per wavefront (the last wavefronts have 4)
  double acc[NJ];
#pragma unroll
  for (int b = 0; b < NJ; ++b) acc[b] = 0.0;
#pragma unroll 8
  for (int k = 0; k < NB; ++k) {
    const double wv = sW[k][c];
#pragma unroll
    for (int b = 0; b < NJ; ++b) if (w + 4 * b < kBorderJ) acc[b] = __builtin_fma(wv, sU[k][w + 4 * b], acc[b]);
  }
  // out through LDS: a row's 17 columns are contiguous in Yp, a lane's are not
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NJ; ++b) if (w + 4 * b < kBorderJ) sU[c][w + 4 * b] = acc[b];
  __syncthreads();
  double *out = Yp + ((size_t)kbi * n0pad + cb) * kBorderStride + j0;
  for (int e = threadIdx.x; e < NB * kBorderJ; e += 256) {
    const int r = e / kBorderJ, j = e % kBorderJ;
    out[(size_t)r * kBorderStride + j] = sU[r][j];
  }
}

// Y = the sum of its tiles' shares for one 64-row block per workgroup, and the block's share of Y'Y (all m + 1 columns:
// the last row is Y'z0), lower triangle.
__global__ void __launch_bounds__(256) border_gram_kernel(const double *Yp, int n0pad, int n0, int m1, double *Y, double *Cpart) {
  __shared__ double sY[NB][kBorderStride + 1];
  const int cbi = blockIdx.x, cb = cbi * NB;
  {
    // the block's NB x kBorderStride entries are contiguous in every partial copy: element e of thread t is t + 256 i
    constexpr int PER = NB * kBorderStride / 256;      // 17
    double v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) v[i] = 0.0;
    for (int kbi = 0; kbi <= cbi; ++kbi) {
      const double *src = Yp + ((size_t)kbi * n0pad + cb) * kBorderStride;
      double ld_[PER];
#pragma unroll
      for (int i = 0; i < PER; ++i) ld_[i] = src[threadIdx.x + 256 * i];
#pragma unroll
      for (int i = 0; i < PER; ++i) v[i] += ld_[i];
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + 256 * i, c = e / kBorderStride, j = e % kBorderStride;
      const double val = (cb + c < n0 && j < m1) ? v[i] : 0.0;
      Y[(size_t)(cb + c) * kBorderStride + j] = val;
      sY[c][j] = val;
    }
  }
  __syncthreads();
  double *Cp = Cpart + (size_t)cbi * kBorderStride * kBorderStride;
  for (int e = threadIdx.x; e < m1 * m1; e += 256) {
    const int j1 = e / m1, j2 = e % m1;
    double sacc = 0.0;
    if (j2 <= j1) {
#pragma unroll 16
      for (int r = 0; r < NB; ++r) sacc = __builtin_fma(sY[r][j1], sY[r][j2], sacc);
    }
    Cp[j1 * kBorderStride + j2] = sacc;
  }
}

// C zz = g in one workgroup: C = [A(D,D) 0; 0 0] - sum of the blocks' Y'Y, g = [b(D); 0] - Y'z0; symmetric elimination
// without pivoting (C is quasi-definite: the D block positive, the R block negative definite).
__global__ void __launch_bounds__(256) border_small_kernel(const double *Cpart, int nblocks, const double *A, int n, const double *beff,
                                                           const int *Dl, int nd, int m, double *zz, int *fail) {
  __shared__ double M[kBorderMax][kBorderMax + 2];      // augmented with g
  const int tid = threadIdx.x, m1 = m + 1;
  for (int e = tid; e < m * m1; e += 256) {
    const int j1 = e / m1, j2 = e % m1;
    const int hi = j2 == m ? m : (j1 > j2 ? j1 : j2), lo = j2 == m ? j1 : (j1 > j2 ? j2 : j1);      // Cpart holds the lower triangle
    const double *src = Cpart + hi * kBorderStride + lo;
    double sum = 0.0;
    int b = 0;
    for (; b + 4 <= nblocks; b += 4) {
      const double a0 = src[(size_t)b * kBorderStride * kBorderStride], a1 = src[(size_t)(b + 1) * kBorderStride * kBorderStride],
                   a2 = src[(size_t)(b + 2) * kBorderStride * kBorderStride], a3 = src[(size_t)(b + 3) * kBorderStride * kBorderStride];
      sum += a0; sum += a1; sum += a2; sum += a3;
    }
    for (; b < nblocks; ++b) sum += src[(size_t)b * kBorderStride * kBorderStride];
    double c0 = 0.0;
    if (j2 == m) c0 = j1 < nd ? beff[Dl[j1]] : 0.0;
    else if (j1 < nd && j2 < nd) c0 = A[(size_t)Dl[j1] * n + Dl[j2]];
    M[j1][j2] = c0 - sum;
  }
  __syncthreads();
  // Gauss-Jordan: step k clears column k in every other row, so the solution is M[i][m] / M[i][i] at the end.  Row k and
  // column k are only read in step k and every other entry has one writer: in place, one barrier per step.  Thread
  // (i = tid / 4, q = tid % 4) owns the columns j = q, q + 4, ... of row i.
  const int i = tid >> 2, q = tid & 3;
  for (int k = 0; k < m; ++k) {
    const double piv = M[k][k];
    if (tid == 0 && !(fabs(piv) > 0.0)) atomicOr(fail, 1);
    if (i < m && i != k) {
      double rp = __builtin_amdgcn_rcp(piv);      // 1 / piv: hardware estimate + two Newton steps
      rp = __builtin_fma(__builtin_fma(-piv, rp, 1.0), rp, rp);
      rp = __builtin_fma(__builtin_fma(-piv, rp, 1.0), rp, rp);
      const double f = -M[i][k] * rp;
      for (int j = k + 1 + ((q - (k + 1)) & 3); j < m1; j += 4) M[i][j] = __builtin_fma(f, M[k][j], M[i][j]);
    }
    __syncthreads();
  }
  if (tid < m) zz[tid] = M[tid][m] / M[tid][tid];
}

// v = z0 - Y zz (the right-hand side of the product with W), one wavefront per row, and x_D = zz[0 .. nd) into x
__global__ void __launch_bounds__(256) border_v_kernel(const double *Y, int n0pad, int m, const double *zz, double *v, const int *Dl, int nd, double *x) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x < nd) x[Dl[threadIdx.x]] = zz[threadIdx.x];      // nd <= kBorderMax <= 256
  if (row >= n0pad) return;
  const double *y = Y + (size_t)row * kBorderStride;
  double sum = lane < m ? -y[lane] * zz[lane] : 0.0;      // m <= 64
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  if (lane == 0) v[row] = y[m] + sum;
}

// ---- small problems: the whole pivot loop in ONE workgroup ----------------------
// The reference's own ensembles give the dense solver a few dozen rows (Cairn(4): 3 rows per
// contact), where a launch and a read-back per pivot dwarf the arithmetic.  For n <= 112 the
// principal submatrix A(S,S) fits LDS in packed lower-triangular form, so one 256-thread
// workgroup runs the reference's complete loop (lcp.cc:157-274: flip the first offender,
// factor A(S,S) afresh, solve, w, CheckMurtySolution, best-solution memory, iteration cap and
// the final looser check) without the host.  Same decisions as murty_device below.
constexpr int kSmallMurtyMax = 112;

struct SmallMurtyResult {   // written by thread 0 at the end
  int solved;               // a solution at 1e-9 (lcp.cc:196) or, when capped, at 1e-8 (lcp.cc:244-246)
  int pivots;
  int not_spd;              // a principal submatrix had a non-positive pivot
  int pad;
};

__device__ __forceinline__ int tri(int r, int c) { return r * (r + 1) / 2 + c; }   // c <= r

__global__ void __launch_bounds__(256) murty_small_kernel(int n, const double *A, const double *bvec, const double *lo_g,
                                                          const double *hi_g, int box_fix, int max_iterations,
                                                          double *x_out, double *w_out, SmallMurtyResult *res) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double *T = sm;                                   // packed lower triangle of A(S,S), then its Cholesky factor
  double *x = T + kSmallMurtyMax * (kSmallMurtyMax + 1) / 2;
  double *w = x + kSmallMurtyMax, *r = w + kSmallMurtyMax, *Cv = r + kSmallMurtyMax, *lo = Cv + kSmallMurtyMax;
  double *hi = lo + kSmallMurtyMax, *b = hi + kSmallMurtyMax, *y = b + kSmallMurtyMax, *bx = y + kSmallMurtyMax;
  double *bw = bx + kSmallMurtyMax, *y2 = bw + kSmallMurtyMax;
  __shared__ int idx[kSmallMurtyMax];
  __shared__ unsigned char S[kSmallMurtyMax];
  __shared__ int s_first, s_oob, s_wbad, s_ns, s_state, s_fail;   // s_state: 0 run, 1 solved, 2 capped
  __shared__ double s_resid2, s_good, s_best;
  const int tid = threadIdx.x;
  const int NONE = 0x7fffffff;

  for (int i = tid; i < n; i += 256) {
    S[i] = 1; lo[i] = lo_g[i]; hi[i] = hi_g[i]; Cv[i] = lo_g[i]; b[i] = bvec[i];
    x[i] = 0.0; w[i] = -bvec[i]; r[i] = -bvec[i];   // lcp.cc:184-185
    bx[i] = 0.0; bw[i] = -bvec[i];
  }
  if (tid == 0) { s_state = 0; s_fail = 0; }
  __syncthreads();

  // CheckMurtySolution (lcp.cc:20-103) + goodness (lcp.cc:107-113) of the current x, w, r
  auto check = [&]() {
    if (tid == 0) { s_first = NONE; s_oob = 0; s_wbad = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
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
  // (A x)_i with two threads per row (even / odd columns) and four independent chains each;
  // the pair is combined through LDS by the caller
  auto row_times_x = [&](int i, int half) {
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
    const double *row = A + (size_t)i * n;
    int c = half;
    for (; c + 6 < n; c += 8) {
      p0 = __builtin_fma(row[c], x[c], p0);
      p1 = __builtin_fma(row[c + 2], x[c + 2], p1);
      p2 = __builtin_fma(row[c + 4], x[c + 4], p2);
      p3 = __builtin_fma(row[c + 6], x[c + 6], p3);
    }
    for (; c < n; c += 2) p0 = __builtin_fma(row[c], x[c], p0);
    return (p0 + p1) + (p2 + p3);
  };
  // r = A x - b
  auto residual_vector = [&]() {
    const int i = tid >> 1, half = tid & 1;
    double part = 0.0;
    if (i < n) part = row_times_x(i, half);
    if (i < n && half == 1) y2[i] = part;
    __syncthreads();
    if (i < n && half == 0) r[i] = (part + y2[i]) - b[i];
    __syncthreads();
  };

  check();
  if (tid == 0) s_best = s_good;
  __syncthreads();

  int iter = 0, pivots = 0;
  bool force = box_fix != 0;
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
    for (int i = tid; i < n; i += 256) x[i] = S[i] ? 0.0 : Cv[i];   // x = x_clamped
    __syncthreads();
    const int ns = s_ns;
    // right-hand side: b(S), minus A(S,!S) x(!S) for the true box problem (lcp.cc:199-216)
    if (box_fix) {
      residual_vector();                              // r = A x_clamped - b
      for (int k = tid; k < ns; k += 256) y[k] = -r[idx[k]];
    } else {
      for (int k = tid; k < ns; k += 256) y[k] = b[idx[k]];
    }
    for (int e = tid; e < ns * (ns + 1) / 2; e += 256) {             // gather A(S,S), lower triangle
      int rr = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
      while (tri(rr + 1, 0) <= e) ++rr;
      while (tri(rr, 0) > e) --rr;
      const int cc = e - tri(rr, 0);
      T[e] = A[(size_t)idx[rr] * n + idx[cc]];
    }
    __syncthreads();
    // Cholesky, right-looking, in place; y rides along as an extra row, so L z = y is solved by
    // the same column steps.  Two barriers per column: every thread takes the square root of the
    // (not yet overwritten) pivot itself.
    for (int j = 0; j < ns; ++j) {
      const double d = T[tri(j, j)];
      if (!(d > 0.0)) { if (tid == 0) s_fail = 1; }
      const double rt = sqrt(d > 0.0 ? d : 1.0);
      for (int i = j + 1 + tid; i < ns; i += 256) T[tri(i, j)] /= rt;
      if (tid == 255) y[j] /= rt;
      __syncthreads();
      if (tid == 0) T[tri(j, j)] = rt;
      const int tx = tid & 15, ty = tid >> 4;
      for (int i = j + 1 + ty; i < ns; i += 16) {
        const double lij = T[tri(i, j)];
        for (int k = j + 1 + tx; k <= i; k += 16) T[tri(i, k)] = __builtin_fma(-lij, T[tri(k, j)], T[tri(i, k)]);
      }
      {
        const double yj = y[j];
        for (int i = j + 1 + tid; i < ns; i += 256) y[i] = __builtin_fma(-T[tri(i, j)], yj, y[i]);
      }
      __syncthreads();
    }
    // L^T v = z in ONE wavefront (two unknowns per lane), no workgroup barrier per step
    if (tid < 64) {
      for (int j = ns - 1; j >= 0; --j) {
        if (tid == (j & 63)) y[j] = y[j] / T[tri(j, j)];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const double yj = y[j];
        for (int i = tid; i < j; i += 64) y[i] = __builtin_fma(-T[tri(j, i)], yj, y[i]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
    __syncthreads();
    for (int k = tid; k < ns; k += 256) x[idx[k]] = y[k];
    __syncthreads();
    residual_vector();                               // r = A x - b
    for (int i = tid; i < n; i += 256) w[i] = S[i] ? 0.0 : r[i];     // lcp.cc:219-223
    __syncthreads();
    ++pivots;
    check();
    if (s_good > s_best) {                           // lcp.cc:125-137 (uniform: shared value)
      for (int i = tid; i < n; i += 256) { bx[i] = x[i]; bw[i] = w[i]; }
      __syncthreads();
      if (tid == 0) s_best = s_good;
      __syncthreads();
    }
    ++iter;
    if (s_fail) break;
  }
  int solved = (s_state == 1);
  if (!solved && !s_fail) {
    // capped: the best-seen iterate (reference rule only), re-checked at the looser 1e-8 (lcp.cc:241-246)
    if (!box_fix) {
      for (int i = tid; i < n; i += 256) { x[i] = bx[i]; w[i] = bw[i]; }
      __syncthreads();
    }
    residual_vector();
    check();
    solved = is_solution(1e-8) ? 1 : 0;
  }
  for (int i = tid; i < n; i += 256) { x_out[i] = x[i]; w_out[i] = w[i]; }
  if (tid == 0) { res->solved = solved; res->pivots = pivots; res->not_spd = s_fail; res->pad = 0; }
}

}  // namespace

// Murty on (A n x n device, b device).  Mirrors lcp.cc:157-274; box_fix as in
// the oracle (true box problem: solve once before the first check).
//
// block = true is NOT the reference's pivot rule: block principal pivoting
// (Judice & Pires): every infeasible index flips at once while the number of
// infeasibilities keeps falling, with single-index steps (largest index) as the
// safeguard that guarantees termination.  Same unique solution for SPD A, in
// tens of factorisations instead of hundreds -- and no min(1000, 2^n) cap, which
// the reference's single-index rule exhausts for n >~ 600.
// extra_fail: a device flag of the caller's own factorisation, folded into the record's `fail`; after_first_sync: run
// once after the first synchronisation (the caller's deferred checks ride on it instead of synchronising themselves).
bool murty_device(DenseWorkspace &ws, int n, const double *dA, const double *db, const std::vector<double> &lo,
                  const std::vector<double> &hi, bool box_fix, bool block, int max_pivots, double max_seconds, double *dx,
                  double *dw, int *pivots_out, std::string *msg, const int *extra_fail,
                  const std::function<void()> *after_first_sync) {
  hipStream_t s = ws.stream;
  const auto t_start = std::chrono::steady_clock::now();
  for (int i = 0; i < n; ++i)   // lcp.cc:161-164; the box variant also admits hi == 0 (toolkit/lcp.h:129)
    if (!(lo[i] < hi[i]) || !(lo[i] <= 0) || !(box_fix ? hi[i] >= 0 : hi[i] > 0)) { if (msg) *msg = "bounds must satisfy lo <= 0 < hi (lcp.cc:161-164)"; return false; }
  *pivots_out = 0;
  if (n == 0) return true;
  const double p2 = std::pow(2.0, n);
  int max_iterations = block ? 4 * n + 100 : (p2 > 1000 ? 1000 : (int)p2);  // lcp.cc:168
  // the caller's own cap (lcp::Settings::max_iterations, toolkit/lcp.h:161-164): give up and return false
  if (max_pivots > 0 && max_pivots < max_iterations) max_iterations = max_pivots;
  if (n <= kSmallMurtyMax && !block) {   // the whole loop in one workgroup, one read-back
    Buf<double> lo_s(ws, n), hi_s(ws, n);
    Buf<SmallMurtyResult> res_d(ws, 1);
    SmallMurtyResult res{};
    HIPCHK(hipMemcpyAsync(lo_s.p, lo.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(hi_s.p, hi.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    const size_t lds = (size_t)(kSmallMurtyMax * (kSmallMurtyMax + 1) / 2 + 11 * kSmallMurtyMax) * sizeof(double);
    hipLaunchKernelGGL(murty_small_kernel, dim3(1), dim3(256), lds, s, n, dA, db, lo_s.p, hi_s.p, box_fix ? 1 : 0,
                       max_iterations, dx, dw, res_d.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&res, res_d.p, sizeof res, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *pivots_out = res.pivots;
    if (res.not_spd) { if (msg) *msg = "a principal submatrix A(S,S) is not positive definite"; return false; }
    if (!res.solved && msg) *msg = "MurtyPrincipalPivot: iteration cap reached without a sensible solution (lcp.cc:250-252)";
    return res.solved != 0;
  }
  const int npad_max = (n + NB - 1) / NB * NB;
  Buf<double> T(ws, (size_t)(2 * npad_max + 1) * npad_max), lohi_d(ws, 2 * (size_t)n), Cb(ws, n), beff(ws, n), r(ws, n), bx(ws, n), bw(ws, n), xs(ws, npad_max), dinv(ws, (size_t)npad_max * NB);
  Buf<uint8_t> S_d(ws, n);
  Buf<int> idx_d(ws, n), fail_d(ws, 1);
  Buf<MurtyState> st_d(ws, 1);
  // bordered pivots (see border_* kernels): the base set of the last factorisation and the work arrays
  static const bool border_on = [] { const char *e = std::getenv("EGS_DENSE_BORDER"); return !(e && std::atoi(e) == 0); }();
  static const bool start_guess = [] { const char *e = std::getenv("EGS_DENSE_GUESS"); return !(e && std::atoi(e) == 0); }();
  const bool track_base = border_on && n <= 2048;      // (the forward product keeps n / 64 partial copies of Y)
  Buf<int> pos0(ws, track_base ? n : 0), idx0(ws, track_base ? npad_max : 0), Dl(ws, track_base ? kBorderMax : 0), Rl(ws, track_base ? kBorderMax : 0);
  Buf<double> Um(ws, track_base ? (size_t)npad_max * kBorderStride : 0), Ym(ws, track_base ? (size_t)npad_max * kBorderStride : 0),
      Cpart(ws, track_base ? (size_t)(npad_max / NB) * kBorderStride * kBorderStride : 0), zz(ws, track_base ? kBorderStride : 0), vv(ws, track_base ? npad_max : 0),
      Yp(ws, track_base ? (size_t)(npad_max / NB) * npad_max * kBorderStride : 0);
  int base_n0 = -1;      // |S0|, or -1 while nothing is factored
  if (track_base) HIPCHK(hipMemsetAsync(pos0.p, 0xff, (size_t)n * sizeof(int), s));
  const double *lo_d = lohi_d.p, *hi_d = lohi_d.p + n;
  MurtyStep *rec = &pinned_records(ws)->step;
  int seq = rec->seq;      // continues across calls (the record is the workspace's)
  {
    std::vector<double> lohi(2 * (size_t)n);
    std::copy(lo.begin(), lo.end(), lohi.begin());
    std::copy(hi.begin(), hi.end(), lohi.begin() + n);
    HIPCHK(hipMemcpyAsync(lohi_d.p, lohi.data(), 2 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemsetAsync(fail_d.p, 0, sizeof(int), s));
  // x = 0, w = -b, r = A x - b = -b   (lcp.cc:184-185); S = everything, C = lo
  hipLaunchKernelGGL(murty_init_kernel, dim3(grid1(n)), dim3(256), 0, s, n, db, lo_d, hi_d, (block && start_guess) ? 1 : 0, S_d.p, Cb.p, dx,
                     dw, r.p, bx.p, bw.p, st_d.p);
  const int flip_mode = block ? 2 : 1;
  // check the iterate on the device, flip for the next pivot there too, and read the 64-byte record
  auto advance = [&](int mode, double tol, int keep_best) {
    hipLaunchKernelGGL(murty_advance_kernel, dim3(1), dim3(1024), 0, s, n, dx, dw, r.p, S_d.p, Cb.p, lo_d, hi_d, mode, tol, keep_best,
                       st_d.p, bx.p, bw.p, idx_d.p, fail_d.p, extra_fail, rec, track_base ? pos0.p : (const int *)nullptr, idx0.p, base_n0 > 0 ? base_n0 : 0,
                       Dl.p, Rl.p, kBorderMax, ++seq);
    HIPCHK(hipGetLastError());
    // the record is in host-coherent memory and its sequence number is written last: poll it (every later launch is
    // ordered by the stream anyway); fall back to the stream's own completion if it does not show up
    const auto t_poll = std::chrono::steady_clock::now();
    for (unsigned spins = 0; __atomic_load_n(&rec->seq, __ATOMIC_ACQUIRE) != seq; ++spins) {
      if ((spins & 0xfff) == 0xfff && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_poll).count() > 0.05) {
        HIPCHK(hipStreamSynchronize(s));
        if (__atomic_load_n(&rec->seq, __ATOMIC_ACQUIRE) != seq) throw std::runtime_error("dense LCP: the pivot record did not arrive");
        break;
      }
    }
  };
  auto is_solution = [&](double tol) {
    return rec->first_offender == 0x7fffffff && !rec->out_of_bounds && !rec->w_bad && std::sqrt(rec->resid2) <= tol;
  };
  int iter = 0, pivots = 0, bordered = 0;
  bool last_bordered = false, polished = false;
  bool force = box_fix, solved = false, timed_out = false;
  // the start iterate: its goodness opens the best-solution memory; a box problem solves once before the first flip,
  // the reference's loop (lcp.cc:196-198) checks and flips first
  advance(force ? 0 : flip_mode, 1e-9, 1);
  if (after_first_sync) (*after_first_sync)();
  const bool trace = dense_trace();
  auto t_prev = std::chrono::steady_clock::now();
  while (iter < max_iterations && !rec->fail) {
    if (max_seconds > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > max_seconds) {
      timed_out = true;   // lcp::Settings::max_time (toolkit/lcp.h:166-167)
      break;
    }
    // The reference's rule starts from S = everything and moves one index per pivot, so its bordered pivots all stand on
    // the factor of the FIRST set: an accepted x then carries the conditioning of that set (often the whole matrix), not
    // of its own A(S,S) -- on a C5-recipe matrix of 113 rows a backward error of 112 u where a factorisation of the final
    // set gives 1 u.  Such an iterate is solved once more on a fresh factor of its own set before
    // it is accepted; that is no pivot of the rule (S does not change) and is not counted as one.  The block rule's
    // bases lie next to its final set and measure like fresh factors, so it keeps its last bordered pivot.
    const bool polish = !force && !block && last_bordered && !polished && is_solution(1e-9);
    if (!force && !polish && is_solution(1e-9)) { solved = true; break; }
    // (no index to flip but not a solution -- residual / sign checks failed: the reference recomputes with unchanged S,
    //  and so does this)
    force = false;
    polished = polished || polish;
    // new candidate: x(S) = A(S,S)^-1 (b(S) [- A(S,!S) x(!S)])   lcp.cc:199-216
    const int ns = rec->ns;
    const int nspad = (ns + NB - 1) / NB * NB;
    hipLaunchKernelGGL(murty_prep_kernel, dim3((n + 3) / 4), dim3(256), 0, s, dA, n, db, S_d.p, Cb.p, box_fix ? 1 : 0, beff.p, dx);
    const int nd = rec->nd, nr = rec->nr, mb = nd + nr;
    if (track_base && base_n0 > 0 && nd >= 0 && mb <= kBorderMax && ns > 0 && !polish) {
      // a few indexes away from the factored set: the bordered system on the old factor
      const int n0 = base_n0, n0pad = (n0 + NB - 1) / NB * NB, nblocks = n0pad / NB;
      hipLaunchKernelGGL(border_build_kernel, dim3(grid1((size_t)n0pad * kBorderStride)), dim3(256), 0, s, dA, n, beff.p, idx0.p, n0, n0pad,
                         pos0.p, Dl.p, nd, Rl.p, nr, Um.p);
      hipLaunchKernelGGL(border_forward_kernel, dim3(nblocks * (nblocks + 1) / 2, 4), dim3(256), 0, s, T.p, n0pad, n0pad, n0, Um.p, Yp.p, n0pad);
      hipLaunchKernelGGL(border_gram_kernel, dim3(nblocks), dim3(256), 0, s, Yp.p, n0pad, n0, mb + 1, Ym.p, Cpart.p);
      if (mb > 0)
        hipLaunchKernelGGL(border_small_kernel, dim3(1), dim3(256), 0, s, Cpart.p, nblocks, dA, n, beff.p, Dl.p, nd, mb, zz.p, fail_d.p);
      hipLaunchKernelGGL(border_v_kernel, dim3(n0pad / 4), dim3(256), 0, s, Ym.p, n0pad, mb, zz.p, vv.p, Dl.p, nd, dx);
      launch_inverse_rows_solve(ws, T.p, n0pad, n0pad, n0pad, vv.p, n0, idx0.p, dx, S_d.p);
      ++bordered;
      last_bordered = true;
    } else if (ns > 0) {
      last_bordered = false;
      launch_build_pivot(ws, dA, n, idx_d.p, ns, nspad, beff.p, T.p, true, track_base ? pos0.p : nullptr, idx0.p);
      factor(ws, T.p, nspad, 2 * nspad + 1, nspad, fail_d.p, dinv.p, nspad);
      launch_inverse_rows_solve(ws, T.p, nspad, nspad, nspad, T.p + (size_t)2 * nspad * nspad, ns, idx_d.p, dx, nullptr);
      if (track_base) base_n0 = ns;      // (build_pivot_kernel recorded the set: the base of the bordered pivots that may follow)
    }
    // r = A x - b; w(!S) = r.  (The reference, lcp.cc:219-221, uses x(S) only: x(!S) = lo = 0 there, so A x(S) == A x.)
    hipLaunchKernelGGL(murty_resid_kernel, dim3((n + 3) / 4), dim3(256), 0, s, dA, n, dx, db, S_d.p, r.p, dw);
    if (!polish) ++pivots;
    advance(flip_mode, 1e-9, 1);     // lcp.cc:125-137: the best iterate by "goodness" is kept by the kernel
    // resid2 is the squared residual of A(S,S) x(S) = b(S) (w is zero on S, r - w off it): a bordered solve that misses
    // the tolerance a solution must meet anyway is not built upon -- the next pivot factors afresh
    if (last_bordered && !(std::sqrt(rec->resid2) <= 1e-10)) base_n0 = -1;
    if (trace) {
      const auto t_now = std::chrono::steady_clock::now();
      std::fprintf(stderr, "dense trace pivot %d: ns %d of %d (%s, +%d -%d against the factored set), %.3f ms, residual on S %.1e; then %d infeasible, %d flipped\n",
                   pivots, ns, n, polish ? "accepted set factored afresh" : last_bordered ? "bordered" : "factored", nd, nr,
                   std::chrono::duration<double, std::milli>(t_now - t_prev).count(), std::sqrt(rec->resid2), rec->ninf, rec->flipped);
      t_prev = t_now;
    }
    if (!polish) ++iter;
  }
  if (!solved && iter < max_iterations && !timed_out && !rec->fail) solved = is_solution(1e-9);
  if (trace) std::fprintf(stderr, "dense trace: %d pivots, %d of them bordered\n", pivots, bordered);
  *pivots_out = pivots;
  if (rec->fail) { if (msg) *msg = "a principal submatrix A(S,S) is not positive definite"; return false; }
  if (solved) return true;  // x, w hold the solution iterate (== best, see lcp.cc:241)
  // capped: return the best-seen iterate and re-check it with the looser 1e-8 (lcp.cc:241-246)
  if (!box_fix && !block) {
    HIPCHK(hipMemcpyAsync(dx, bx.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(dw, bw.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  hipLaunchKernelGGL(gemv_minus_kernel, dim3((n + 3) / 4), dim3(256), 0, s, dA, n, dx, db, r.p);
  advance(0, 1e-8, 0);
  const bool ok = is_solution(1e-8);
  if (!ok && msg) *msg = "MurtyPrincipalPivot: iteration cap reached without a sensible solution (lcp.cc:250-252)";
  return ok;
}

}  // namespace egs
