// dense_factor.hip -- the one factorisation of the dense direct solvers (dense_lcp.hip, dense_murty.hip) and the
// solves with its factor; all matrices row-major fp64, resident in HBM.
//   * factor(): a blocked right-looking Cholesky of the first `nf` columns of a lower-trapezoid T (extra rows below
//     the square part ride along).  Per 64-column block: chol_diag_kernel (diagonal block and its inverse, in
//     registers), chol_trsm_kernel (panel below = B L11^-T as a matrix product) and chol_update_kernel (trailing
//     T -= P P^T), the last two on the fp64 matrix cores (v_mfma_f64_16x16x4_f64); chol_panel_kernel fuses the three.
//   * launch_back_solve() / launch_inverse_rows_solve(): L^T x = y block by block in one workgroup, or as one product
//     with the rows of L^-T that factor() leaves where the trapezoid held an identity block.
//   * launch_build_pivot() gathers the trapezoid of A(S,S); dense_condition_estimate() is gather, factor, iterations.
#include "dense_internal.h"

#include <limits>
#include <vector>

namespace egs {

namespace {

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double double4_t __attribute__((ext_vector_type(4)));

// the diagonal tile (chol_diag_tile)
constexpr int kTileLs = NB + 2;      // column stride of sL / row stride of sX (doubles)
constexpr int kTileQs = 34;          // row stride of the 32 x 32 scratch
constexpr int kTileLdsDoubles = 2 * NB * kTileLs + 32 * kTileQs + NB;      // sL, sX, sQ, sRv
constexpr int kDiagThreads = 320;
constexpr size_t kDiagLdsBytes = (size_t)(NB * (NB + 2) + kTileLdsDoubles) * sizeof(double);
// the MFMA operands staged in LDS (stage_block)
constexpr int kStageLd = NB + 2;     // doubles; keeps 16-byte alignment of every row start
constexpr int kPanelThreads = 320;   // chol_panel_kernel: four MFMA wavefronts + the inverse wavefront of the diagonal tile

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// 1 / sqrt(d) to within an ulp or two: hardware estimate y, e = 1 - d y^2, then
// y (1 + e/2 + 3 e^2 / 8) (cubic convergence, one short dependent chain).
__device__ __forceinline__ double rsqrt_refined(double d) {
  const double y = __builtin_amdgcn_rsq(d);
  const double e = __builtin_fma(-d * y, y, 1.0);
  const double t = __builtin_fma(0.375, e, 0.5) * e;
  return __builtin_fma(y, t, y);
}

// Workgroup barrier that orders LDS traffic only (__syncthreads() also drains vmcnt, i.e. waits for the
// acknowledgement of the global stores in flight; the column loop below stores one finished column per
// step and has no reason to wait for it).
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ---- the diagonal tile ------------------------------------------------------------------------------------
// L11 = chol(tile) and its inverse for a 64 x 64 tile staged in LDS, one workgroup of five wavefronts.  This is the
// latency chain of the whole factorisation (one tile per 64 columns, nothing else can start before it ends), so it is
// built for few dependent steps rather than for throughput (tools/diag_bench.hip times the variants: 23.4 us for the
// round-2 routine -- one barrier per column, the inverse accumulated by a fifth wavefront with 63 - j multiply-adds
// per column -- against 12.9 us for this one):
//   * wavefronts 0..3, lane i = row i; wavefront w holds the four-column groups g = 4 m + w (16 registers).  The
//     owner of group g reads the 4 x 4 diagonal mini-block out of its lanes once (readlane -> scalar registers),
//     factors it redundantly in every lane and solves its own row against it: no cross-lane traffic inside the four
//     columns.  The four columns go to LDS (column-major sL, every column in its own place: no double buffer), ONE
//     barrier per group, and every wavefront applies the rank-4 update to the groups it holds -- the factored ones too
//     (dead registers; the code stays free of wavefront-dependent branches).  Entries above the diagonal are scratch:
//     nothing masks them and nothing reads them.
//   * wavefront 4, lane c < 16 = column c of the inverse of the current 16 x 16 diagonal block: forward substitution
//     row by row as the columns appear (15 - r multiply-adds per row, in the shadow of the column chain).
//   * afterwards the rest of the inverse by products on the fp64 matrix cores: X(2p+1, 2p) = -X(2p+1, 2p+1) L(2p+1, 2p)
//     X(2p, 2p) for the two 32 x 32 diagonal blocks, then the 32 x 32 block below them the same way.
//   * L (lower triangle) and the inverse (all of it: zero above the diagonal) go to memory at the end, rows coalesced.
// The inverse turns the panel's triangular solve and the diagonal steps of the back substitution into matrix
// products (chol_trsm_kernel, chol_panel_kernel, back_solve_kernel).

__device__ __forceinline__ double4_t mfma_f64(double a, double b, double4_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// sB: the tile, row-major with row stride ldb.  sL, sX: NB * kTileLs doubles each; sQ: 32 * kTileQs; sRv: NB.
// Tout / inv: where L (row stride ld, tile origin already applied) and the inverse (64 x 64, dense) go.
__device__ __forceinline__ void chol_diag_tile(const double *sB, int ldb, double *sL, double *sX, double *sQ, double *sRv, double *Tout,
                                               int ld, double *inv, int *fail) {
  constexpr int GW = 4, NG = NB / GW, MG = NG / 4, LS = kTileLs, XS = kTileLs, QS = kTileQs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < NB * XS; i += blockDim.x) sX[i] = 0.0;      // the inverse is zero above its diagonal blocks
  if (wave < 4) {
    double a[MG][GW];
#pragma unroll
    for (int m = 0; m < MG; ++m)
#pragma unroll
      for (int q = 0; q < GW; ++q) a[m][q] = sB[lane * ldb + GW * (4 * m + wave) + q];
    bool bad = false;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int mo = g >> 2, c0 = GW * g;
      if (wave == (g & 3)) {
        // the mini-block's lower triangle, m[r][c] from lane c0 + r
        const double m00 = readlane_f64(a[mo][0], c0);
        const double m10 = readlane_f64(a[mo][0], c0 + 1), m11 = readlane_f64(a[mo][1], c0 + 1);
        const double m20 = readlane_f64(a[mo][0], c0 + 2), m21 = readlane_f64(a[mo][1], c0 + 2), m22 = readlane_f64(a[mo][2], c0 + 2);
        const double m30 = readlane_f64(a[mo][0], c0 + 3), m31 = readlane_f64(a[mo][1], c0 + 3), m32 = readlane_f64(a[mo][2], c0 + 3),
                     m33 = readlane_f64(a[mo][3], c0 + 3);
        const double r0 = rsqrt_refined(m00);
        const double x0 = a[mo][0] * r0;
        const double l10 = m10 * r0, l20 = m20 * r0, l30 = m30 * r0;
        const double d1 = __builtin_fma(-l10, l10, m11);
        const double r1 = rsqrt_refined(d1);
        const double x1 = __builtin_fma(-x0, l10, a[mo][1]) * r1;
        const double l21 = __builtin_fma(-l20, l10, m21) * r1, l31 = __builtin_fma(-l30, l10, m31) * r1;
        const double d2 = __builtin_fma(-l21, l21, __builtin_fma(-l20, l20, m22));
        const double r2 = rsqrt_refined(d2);
        const double x2 = __builtin_fma(-x1, l21, __builtin_fma(-x0, l20, a[mo][2])) * r2;
        const double l32 = __builtin_fma(-l31, l21, __builtin_fma(-l30, l20, m32)) * r2;
        const double d3 = __builtin_fma(-l32, l32, __builtin_fma(-l31, l31, __builtin_fma(-l30, l30, m33)));
        const double r3 = rsqrt_refined(d3);
        const double x3 = __builtin_fma(-x2, l32, __builtin_fma(-x1, l31, __builtin_fma(-x0, l30, a[mo][3]))) * r3;
        bad |= !(m00 > 0.0) | !(d1 > 0.0) | !(d2 > 0.0) | !(d3 > 0.0);
        sL[(c0 + 0) * LS + lane] = x0; sL[(c0 + 1) * LS + lane] = x1; sL[(c0 + 2) * LS + lane] = x2; sL[(c0 + 3) * LS + lane] = x3;
        if (lane == 0) { sRv[c0] = r0; sRv[c0 + 1] = r1; sRv[c0 + 2] = r2; sRv[c0 + 3] = r3; }
      }
      lds_barrier();
      if (g + 1 < NG) {
        double lrow[GW];
#pragma unroll
        for (int q = 0; q < GW; ++q) lrow[q] = sL[(c0 + q) * LS + lane];
#pragma unroll
        for (int m = mo; m < MG; ++m) {
          const int cg = GW * (4 * m + wave);
#pragma unroll
          for (int q2 = 0; q2 < GW; ++q2) {
            double acc = a[m][q2];
#pragma unroll
            for (int q = 0; q < GW; ++q) acc = __builtin_fma(-lrow[q], sL[(c0 + q) * LS + cg + q2], acc);
            a[m][q2] = acc;
          }
        }
      }
    }
    if (bad && lane == 0) atomicOr(fail, 1);
  } else {
    double acc[16];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      lds_barrier();
#pragma unroll
      for (int q = 0; q < GW; ++q) {
        const int R = GW * g + q, b = R >> 4, r = R & 15;
        if (r == 0) {
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[k] = 0.0;
        }
        if (lane < 16) {
          const double x = (((lane == r) ? 1.0 : 0.0) - acc[r]) * sRv[R];      // lanes c > r: exactly 0
          sX[R * XS + 16 * b + lane] = x;
#pragma unroll
          for (int k2 = r + 1; k2 < 16; ++k2) acc[k2] = __builtin_fma(sL[R * LS + 16 * b + k2], x, acc[k2]);
        }
      }
    }
  }
  lds_barrier();
  // v_mfma_f64_16x16x4_f64 operand maps: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15]; D: col = lane&15, row = (lane>>4) + 4 reg
  const int li = lane & 15, lk = lane >> 4;
  if (wave < 2) {      // X(2p+1, 2p) = -X(2p+1, 2p+1) (L(2p+1, 2p) X(2p, 2p)), p = wave
    const int o = 32 * wave;
    double4_t P = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) P = mfma_f64(sL[(o + 4 * kk + lk) * LS + o + 16 + li], sX[(o + 4 * kk + lk) * XS + o + li], P);
    double *sP = sQ + wave * 16 * QS;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) sP[(lk + 4 * reg) * QS + li] = P[reg];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    double4_t D = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) D = mfma_f64(sX[(o + 16 + li) * XS + o + 16 + 4 * kk + lk], sP[(4 * kk + lk) * QS + li], D);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) sX[(o + 16 + lk + 4 * reg) * XS + o + li] = -D[reg];
  }
  lds_barrier();
  // X_BL = -X_BR (L_BL X_TL) on the 32 x 32 blocks, one 16 x 16 tile per wavefront
  if (wave < 4) {
    const int ti = wave >> 1, tj = wave & 1;
    double4_t Q = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) Q = mfma_f64(sL[(4 * kk + lk) * LS + 32 + 16 * ti + li], sX[(4 * kk + lk) * XS + 16 * tj + li], Q);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) sQ[(16 * ti + lk + 4 * reg) * QS + 16 * tj + li] = Q[reg];
  }
  lds_barrier();
  if (wave < 4) {
    const int ti = wave >> 1, tj = wave & 1;
    double4_t D = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) D = mfma_f64(sX[(32 + 16 * ti + li) * XS + 32 + 4 * kk + lk], sQ[(4 * kk + lk) * QS + 16 * tj + li], D);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) sX[(32 + 16 * ti + lk + 4 * reg) * XS + 16 * tj + li] = -D[reg];
  }
  lds_barrier();
  for (int i = threadIdx.x; i < NB * NB; i += blockDim.x) {
    const int r = i >> 6, c = i & 63;
    inv[i] = sX[r * XS + c];
    if (c <= r) Tout[(size_t)r * ld + c] = sL[c * LS + r];
  }
}

// The tile at (k0, k0) of T: L to Tout (same place), the inverse to inv.
__global__ void __launch_bounds__(kDiagThreads) chol_diag_kernel(const double *T, double *Tout, int ld, int k0, double *inv, int *fail) {
  extern __shared__ __attribute__((aligned(16))) double smem_d[];
  double *sB = smem_d, *sL = sB + NB * (NB + 2), *sX = sL + NB * kTileLs, *sQ = sX + NB * kTileLs, *sRv = sQ + 32 * kTileQs;
  for (int i = threadIdx.x; i < NB * NB; i += blockDim.x) {
    const int r = i >> 6, c = i & 63;
    sB[r * (NB + 2) + c] = T[(size_t)(k0 + r) * ld + k0 + c];
  }
  __syncthreads();
  chol_diag_tile(sB, NB + 2, sL, sX, sQ, sRv, Tout + (size_t)k0 * ld + k0, ld, inv, fail);
}

// A 64 x 64 block of doubles from global memory (row stride ld) into LDS (row stride kStageLd) with 16-byte loads, all
// of a thread's eight loads in flight at once: one memory round trip per operand instead of one per k-step of the MFMA
// loop.  Rows at or beyond `nrows` read as zero.  Threads 0..255: thread t takes row t / 4, columns 16 (t % 4) .. + 15.
__device__ __forceinline__ void stage_block(const double *src, int ld, int row0, int nrows, double *dst) {
  if (threadIdx.x >= 256) return;
  const int r = threadIdx.x >> 2, c = (threadIdx.x & 3) * 16;
  const bool ok = row0 + r < nrows;
  const double *p = src + (size_t)(ok ? row0 + r : 0) * ld + c;
  double v[16];
  if ((((size_t)p) & 15) == 0) {
    double2_t q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = ok ? *reinterpret_cast<const double2_t *>(p + 2 * k) : (double2_t){0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[2 * k] = q[k].x; v[2 * k + 1] = q[k].y; }
  } else {          // an odd leading dimension leaves rows 8-byte aligned only
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = ok ? p[k] : 0.0;
  }
  double *d = dst + r * kStageLd + c;
#pragma unroll
  for (int k = 0; k < 8; ++k) *reinterpret_cast<double2_t *>(d + 2 * k) = (double2_t){v[2 * k], v[2 * k + 1]};
}

// acc[ti][tj] += (rows lr.. of sA) (rows lc.. of sB)^T over K = 64: the 32 x 32 quadrant of one wavefront.
// v_mfma_f64_16x16x4_f64 operand maps: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15];
// D: col = lane&15, row = (lane>>4) + 4*reg.
__device__ __forceinline__ void mfma_quadrant(const double *sA, const double *sB, int lr, int lc, double4_t (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < NB / 4; ++kk) {
    double a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[t] = sA[(lr + 16 * t + li) * kStageLd + 4 * kk + lk];
      b[t] = sB[(lc + 16 * t + li) * kStageLd + 4 * kk + lk];
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
        acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
  }
}

// Panel below the diagonal block: X = B L11^-T = B (L11^-1)^T on the fp64 matrix
// cores, X[r][c] = sum_k B[r][k] Linv[c][k].  One workgroup per 64-row slab,
// each wavefront a 32x32 quadrant; both operands staged in LDS.  B is read from T, X goes to Tout (may be T).
__global__ void __launch_bounds__(256) chol_trsm_kernel(const double *T, double *Tout, int ld, int nrows, int k0, const double *inv, int ibase, int iend) {
  __shared__ __attribute__((aligned(16))) double sA[NB * kStageLd], sBm[NB * kStageLd];
  const int r0 = k0 + NB + blockIdx.x * NB;
  if (r0 >= ibase && r0 < iend && r0 - ibase >= k0 + NB) return;      // identity rows that no panel has reached yet (see factor())
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = (wave >> 1) * 32, lc = (wave & 1) * 32;
  const int li = lane & 15, lk = lane >> 4;
  stage_block(T + k0, ld, r0, nrows, sA);
  stage_block(inv, NB, 0, NB, sBm);
  double4_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
  __syncthreads();
  mfma_quadrant(sA, sBm, lr, lc, acc);
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = r0 + lr + 16 * ti + lk + 4 * reg, c = lc + 16 * tj + li;
        if (r < nrows) Tout[(size_t)r * ld + k0 + c] = acc[ti][tj][reg];
      }
}

// Trailing update on the fp64 matrix cores: for rows r >= k0+64 and columns
// c in [k0+64, ld) with c <= r (lower trapezoid),  T[r][c] -= sum_k P[r][k] P[c][k],
// P = T[:, k0..k0+64).  One workgroup (4 wavefronts) per 64x64 tile; each
// wavefront owns a 32x32 quadrant = 2x2 MFMA tiles, K = 64 in 16 steps of 4; the two 64 x 64 pieces of the panel are
// staged in LDS first (stage_block).
__global__ void __launch_bounds__(256) chol_update_kernel(double *T, int ld, int nrows, int k0) {
  __shared__ __attribute__((aligned(16))) double sA[NB * kStageLd], sBm[NB * kStageLd];
  const int r0 = k0 + NB + blockIdx.y * NB;
  const int c0 = k0 + NB + blockIdx.x * NB;
  if (c0 > r0 + NB - 1) return;  // tile entirely above the diagonal
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = (wave >> 1) * 32, lc = (wave & 1) * 32;
  const int qr = r0 + lr, qc = c0 + lc;
  const int li = lane & 15, lk = lane >> 4;
  double4_t acc[2][2], told[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
  // the tile's old values, requested before the operands: the final T -= acc costs no second round trip
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = qr + 16 * ti + lk + 4 * reg, c = qc + 16 * tj + li;
        told[ti][tj][reg] = (r < nrows && c < ld && c <= r) ? T[(size_t)r * ld + c] : 0.0;
      }
  const bool diag = r0 == c0;
  stage_block(T + k0, ld, r0, nrows, sA);
  if (!diag) stage_block(T + k0, ld, c0, nrows < ld ? nrows : ld, sBm);     // rows of the panel that are columns of the tile
  __syncthreads();
  mfma_quadrant(sA, diag ? sA : sBm, lr, lc, acc);
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = qr + 16 * ti + lk + 4 * reg, c = qc + 16 * tj + li;
        if (r < nrows && c < ld && c <= r) T[(size_t)r * ld + c] = told[ti][tj][reg] - acc[ti][tj][reg];
      }
}

// Solve L^T x = y in one workgroup: L = T[0..nf)[0..nf) lower, y = T[yrow][0..nf),
// inv = the L_kk^-1 blocks chol_diag_kernel left behind.  Blocks from the last to
// the first: x_k = L_kk^-T t_k is a 64x64 product with the stored inverse, then
// the 64-row strip L[k-block][0..k) (contiguous rows, coalesced) is subtracted
// from the remaining right-hand side.
// x is written to out[map ? map[i] : i] for i < nreal (padding rows dropped).
// XS_LDS: the running right-hand side lives in LDS (nf <= kBackSolveLdsRows) instead of global scratch -- every block
// step reads and rewrites it, and a workgroup-visible global round trip costs a microsecond each way.
constexpr int kBackSolveLdsRows = 16384;
template <bool XS_LDS>
__global__ void __launch_bounds__(1024) back_solve_kernel(const double *T, int ld, int nf, int yrow, int nreal,
                                                          const int *map, double *out, double *xs_global /*[nf] scratch*/,
                                                          const double *inv) {
  extern __shared__ __attribute__((aligned(16))) double xs_lds[];
  double *xs = XS_LDS ? xs_lds : xs_global;
  __shared__ double sx[NB];
  __shared__ double red[16][NB];
  __shared__ double redB[1024];
  const int tid = threadIdx.x;
  // with the right-hand side in LDS nothing a step exchanges goes through memory: a barrier that orders LDS only lets
  // the loads requested ahead (next strip, next inverse block) stay in flight across it
  auto step_barrier = [] { if (XS_LDS) lds_barrier(); else __syncthreads(); };
  for (int i = tid; i < nf; i += 1024) xs[i] = T[(size_t)yrow * ld + i];
  __syncthreads();
  // thread (i, part) of the 64 x 16 layout multiplies rows part, part+16, ... of the inverse block;
  // its four entries for the NEXT block are requested before this block's strip update
  const int i = tid & 63, part = tid >> 6;
  double li[4];
  {
    const double *Li = inv + (size_t)((nf - NB) / NB) * NB * NB;
#pragma unroll
    for (int q = 0; q < 4; ++q) li[q] = nf >= NB ? Li[(part + 16 * q) * NB + i] : 0.0;
  }
  for (int kb = nf - NB; kb >= 0; kb -= NB) {
    // The strip L[kb .. kb+64)[0 .. kb) is subtracted from the kb open entries by P threads per column (P rows-parts of
    // R = 64 / P rows, as many as 1024 threads allow); its entries do not depend on x_k, so they are requested now and
    // arrive while x_k = L_kk^-T t_k is formed.
    int P = kb > 0 ? 1024 / kb : 0;      // (0 only for kb = 0: more than 1024 open columns is P = 1 plus the tail loop below)
    P = P >= 16 ? 16 : P >= 8 ? 8 : P >= 4 ? 4 : P >= 2 ? 2 : (kb > 0 ? 1 : 0);
    const int R = P ? NB / P : 0;
    const bool active = P > 0 && tid < P * kb;
    const int c = active ? tid % kb : 0, rp = active ? tid / kb : 0;
    double lv[32];
    const double *strip = T + (size_t)(kb + rp * R) * ld + c;
#pragma unroll
    for (int j = 0; j < 32; ++j) lv[j] = (active && j < R) ? strip[(size_t)j * ld] : 0.0;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) s = __builtin_fma(li[q], xs[kb + part + 16 * q], s);   // Linv[r][i] = 0 for i > r
    red[part][i] = s;
    if (kb >= NB) {
      const double *Ln = inv + (size_t)(kb / NB - 1) * NB * NB;
#pragma unroll
      for (int q = 0; q < 4; ++q) li[q] = Ln[(part + 16 * q) * NB + i];
    }
    step_barrier();
    if (tid < NB) {
      double x = 0.0;
#pragma unroll
      for (int p = 0; p < 16; ++p) x += red[p][tid];
      sx[tid] = x;
      xs[kb + tid] = x;
    }
    step_barrier();
    if (P == 0) continue;      // (kb == 0: nothing left to update; uniform)
    double u = 0.0;
#pragma unroll
    for (int j = 0; j < 32; ++j) if (j < R) u = __builtin_fma(lv[j], sx[rp * R + j], u);
    if (P == 1) {             // more than 512 open columns: one thread per column, the second half of its 64 rows now
      if (active) {
#pragma unroll
        for (int j = 0; j < 32; ++j) lv[j] = strip[(size_t)(32 + j) * ld];
#pragma unroll
        for (int j = 0; j < 32; ++j) u = __builtin_fma(lv[j], sx[32 + j], u);
        xs[c] -= u;
      }
      for (int c2 = tid + 1024; c2 < kb; c2 += 1024) {      // (more than 1024 open columns)
        double y = 0.0;
#pragma unroll 32
        for (int r = 0; r < NB; ++r) y = __builtin_fma(T[(size_t)(kb + r) * ld + c2], sx[r], y);
        xs[c2] -= y;
      }
    } else {
      if (active) redB[rp * kb + c] = u;
      step_barrier();
      if (tid < kb) {
        double y = 0.0;
        for (int p = 0; p < P; ++p) y += redB[p * kb + tid];
        xs[tid] -= y;
      }
    }
    step_barrier();
  }
  for (int i = tid; i < nreal; i += 1024) out[map ? map[i] : i] = xs[i];
}

// Pivot trapezoid: A(S,S) padded with an identity block; then nspad identity rows (they become L^-T, see factor());
// b_eff(S) as last row.
__global__ void build_pivot_kernel(const double *lhs, int n, const int *S, int ns, int nspad, const double *beff,
                                   double *T, int identity_rows, int *pos0, int *idx0) {
  const int ld = nspad, ib = identity_rows ? nspad : 0, rows = nspad + ib + 1;
  if (pos0) {      // this set becomes the base of the bordered pivots (murty_advance_kernel validates pos0 through idx0)
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < (size_t)ns) { pos0[S[k]] = (int)k; idx0[k] = S[k]; }
  }
  const size_t total = (size_t)rows * ld;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(idx / ld), c = (int)(idx % ld);
    double v = 0.0;
    if (r < ns) { if (c < ns) v = lhs[(size_t)S[r] * n + S[c]]; }
    else if (r < nspad) v = (c == r) ? 1.0 : 0.0;
    else if (r < nspad + ib) v = (c == r - nspad) ? 1.0 : 0.0;
    else { if (c < ns) v = beff[S[c]]; }
    T[idx] = v;
  }
}

// x = L^-T z from the rows the factorisation turned into L^-T (factor(), ibase): x_i = sum_{c >= i} Linvt[i][c] z[c],
// z = L^-1 b.  One wavefront per row; x goes to out[map ? map[i] : i] for i < nreal.
// keep: rows whose map[row] has keep == 0 are not written (indexes that left the set since the factorisation).
__global__ void __launch_bounds__(256) inverse_rows_solve_kernel(const double *T, int ld, int nf, int ibase, const double *z, int nreal,
                                                                 const int *map, double *out, const uint8_t *keep) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nreal) return;
  if (keep && !keep[map[row]]) return;
  const double *Li = T + (size_t)(ibase + row) * ld;
  double s0 = 0.0, s1 = 0.0;
  int c = (row & ~63) + lane;      // whole 64-column groups from the one that holds the diagonal
  for (; c + 64 < nf; c += 128) {
    s0 = __builtin_fma(c >= row ? Li[c] : 0.0, z[c], s0);
    s1 = __builtin_fma(Li[c + 64], z[c + 64], s1);
  }
  if (c < nf) s0 = __builtin_fma(c >= row ? Li[c] : 0.0, z[c], s0);
  double sum = s0 + s1;
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  if (lane == 0) out[map ? map[row] : row] = sum;
}

// ---- one launch per panel -------------------------------------------------------------------------------
// The three launches of a panel step (diagonal block -> panel solve -> trailing update) run one after the other and
// the first, a 64-column latency chain in ONE workgroup, takes 20 of the 37 us.  chol_panel_kernel does the panel
// solve AND the trailing update of panel k in one launch, and the workgroup that finishes the NEXT diagonal tile
// factors it on the spot (chol_diag_tile, the algorithm of chol_diag_kernel on a tile staged in LDS), while the other
// workgroups are still updating: per panel one launch whose length is that one workgroup's (update + 20 us).
//   * Every workgroup needs X_r = B_r L^-T and X_c = B_c L^-T of its tile's row blocks; it computes them itself from the
//     unsolved panel (two extra 64^3 MFMA products per tile: the matrix cores are idle anyway) instead of waiting for a
//     panel-solve launch.
//   * Nobody may overwrite the panel while others still read it, so the solved panel X, the factored diagonal blocks
//     and nothing else go to a second array (Tl, same shape); T keeps taking the trailing updates.  After the last panel
//     merge_factor_kernel copies the factored columns back, so every consumer finds L where it always was.

// grid (tc, tr) over the 64 x 64 tiles of the trailing trapezoid of panel k0 (as chol_update_kernel).
// factor_next: the tile (k0 + 64, k0 + 64) is the next diagonal block to factor (k0 + 64 < nf).
__global__ void __launch_bounds__(kPanelThreads) chol_panel_kernel(double *T, double *Tl, int ld, int nrows, int k0, const double *inv_k,
                                                                   double *inv_next, int *fail, int factor_next, int ibase, int iend) {
  extern __shared__ __attribute__((aligned(16))) double smem_d[];
  double *sA = smem_d, *sBm = sA + NB * kStageLd, *sI = sBm + NB * kStageLd;
  double *sQ = sI + NB * kStageLd, *sRv = sQ + 32 * kTileQs;      // scratch of the diagonal tile (with sA and sI)
  const int r0 = k0 + NB + blockIdx.y * NB;
  const int c0 = k0 + NB + blockIdx.x * NB;
  if (c0 > r0 + NB - 1) return;  // tile entirely above the diagonal
  if (r0 >= ibase && r0 < iend && r0 - ibase >= k0 + NB) return;      // identity rows that no panel has reached yet
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool mm = wave < 4;      // the MFMA wavefronts
  const int lr = (wave >> 1) * 32, lc = (wave & 1) * 32;
  const int qr = r0 + lr, qc = c0 + lc;
  const int li = lane & 15, lk = lane >> 4;
  const bool diag = r0 == c0;
  double4_t told[2][2], xr[2][2], xc[2][2], acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      xr[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0}; xc[a][b] = xr[a][b]; acc[a][b] = xr[a][b]; told[a][b] = xr[a][b];
    }
  if (mm) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int r = qr + 16 * ti + lk + 4 * reg, c = qc + 16 * tj + li;
          told[ti][tj][reg] = (r < nrows && c < ld && c <= r) ? T[(size_t)r * ld + c] : 0.0;
        }
  }
  stage_block(T + k0, ld, r0, nrows, sA);
  if (!diag) stage_block(T + k0, ld, c0, nrows < ld ? nrows : ld, sBm);
  stage_block(inv_k, NB, 0, NB, sI);
  __syncthreads();
  // the solved panel rows of this tile: X = B L^-T, X[r][c] = sum_k B[r][k] Linv[c][k]
  if (mm) {
    mfma_quadrant(sA, sI, lr, lc, xr);
    if (!diag) mfma_quadrant(sBm, sI, lr, lc, xc);
  }
  __syncthreads();
  if (mm) {
    // back into LDS as operands of the update; the first tile of every row block also files its X rows in Tl
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int rr = lr + 16 * ti + lk + 4 * reg, cc = lc + 16 * tj + li;
          sA[rr * kStageLd + cc] = xr[ti][tj][reg];
          if (!diag) sBm[rr * kStageLd + cc] = xc[ti][tj][reg];
          if (blockIdx.x == 0 && r0 + rr < nrows) Tl[(size_t)(r0 + rr) * ld + k0 + cc] = xr[ti][tj][reg];
        }
  }
  __syncthreads();
  if (mm) mfma_quadrant(sA, diag ? sA : sBm, lr, lc, acc);
  const bool factor_here = factor_next && diag && blockIdx.x == 0;      // uniform
  if (!factor_here) {
    if (mm) {
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int r = qr + 16 * ti + lk + 4 * reg, c = qc + 16 * tj + li;
            if (r < nrows && c < ld && c <= r) T[(size_t)r * ld + c] = told[ti][tj][reg] - acc[ti][tj][reg];
          }
    }
    return;
  }
  // the next diagonal block: updated tile -> LDS -> L and its inverse
  __syncthreads();
  if (mm) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int rr = lr + 16 * ti + lk + 4 * reg, cc = lc + 16 * tj + li;
          sBm[rr * kStageLd + cc] = told[ti][tj][reg] - acc[ti][tj][reg];
        }
  }
  __syncthreads();
  chol_diag_tile(sBm, kStageLd, sA, sI, sQ, sRv, Tl + (size_t)r0 * ld + r0, ld, inv_next, fail);
}

// the factored columns (and the solved rows below them) back from Tl into T
__global__ void merge_factor_kernel(double *T, const double *Tl, int ld, int nrows, int nf) {
  const size_t total = (size_t)nrows * nf;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(idx / nf), c = (int)(idx % nf);
    if (r >= c) T[(size_t)r * ld + c] = Tl[(size_t)r * ld + c];
  }
}

// max and min of the diagonal of the factor held in T (the first n columns)
__global__ void __launch_bounds__(256) diag_minmax_kernel(const double *T, int ld, int n, double *out) {
  __shared__ double smax[256], smin[256];
  double mx = 0.0, mn = 1e300;
  for (int k = threadIdx.x; k < n; k += 256) {
    const double d = T[(size_t)k * ld + k];
    mx = d > mx ? d : mx;
    mn = d < mn ? d : mn;
  }
  smax[threadIdx.x] = mx; smin[threadIdx.x] = mn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      smax[threadIdx.x] = smax[threadIdx.x + o] > smax[threadIdx.x] ? smax[threadIdx.x + o] : smax[threadIdx.x];
      smin[threadIdx.x] = smin[threadIdx.x + o] < smin[threadIdx.x] ? smin[threadIdx.x + o] : smin[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = smax[0]; out[1] = smin[0]; }
}

// lambda_max(A) by power iteration and 1 / lambda_min(A) by inverse iteration with the blocked Cholesky factor held in
// T (ld = npad, identity padding) and its inverted diagonal blocks: cond_2(A) = lambda_max / lambda_min for a symmetric
// positive definite A -- what the reference reads off a JacobiSVD (utils.cc:256-261: sigma_max / sigma_min).  One
// workgroup, N <= 1024: every vector in LDS, a thread per row for the products, 64-row block steps for the two
// triangular solves.  out[0] = lambda_max estimate, out[1] = 1 / lambda_min estimate (Rayleigh quotients, both from below).
constexpr int kCondMaxRows = 1024;
__global__ void __launch_bounds__(1024) cond_iterations_kernel(const double *A, int N, const double *T, int ld, int npad, const double *inv,
                                                               int iters, double *out) {
  __shared__ double v[kCondMaxRows], u[kCondMaxRows], red[1024], part[16][NB], blk[NB];
  const int tid = threadIdx.x;
  auto dot = [&](const double *a, const double *b) {
    double sacc = 0.0;
    for (int i = tid; i < N; i += 1024) sacc = __builtin_fma(a[i], b[i], sacc);
    red[tid] = sacc;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
  };
  auto start = [&]() {     // a start vector with a component along every eigenvector one can reasonably expect
    for (int i = tid; i < npad; i += 1024) v[i] = i < N ? 1.0 + 0.37 * (double)((unsigned)(i * 2654435761u) >> 22) / 1024.0 : 0.0;
    __syncthreads();
  };
  // ---- lambda_max
  start();
  double lmax = 0.0;
  for (int it = 0; it < iters; ++it) {
    for (int r = tid; r < N; r += 1024) {
      double sacc = 0.0;
      const double *row = A + (size_t)r * N;
      for (int c = 0; c < N; ++c) sacc = __builtin_fma(row[c], v[c], sacc);
      u[r] = sacc;
    }
    __syncthreads();
    const double vv = dot(v, v), vu = dot(v, u), uu = dot(u, u);
    lmax = vu / vv;
    const double sc = uu > 0.0 ? 1.0 / sqrt(uu) : 0.0;
    for (int i = tid; i < N; i += 1024) v[i] = u[i] * sc;
    __syncthreads();
  }
  // ---- 1 / lambda_min: z = A^-1 v = L^-T L^-1 v
  start();
  double mu = 0.0;
  const int i64 = tid & 63, p16 = tid >> 6;
  for (int it = 0; it < iters; ++it) {
    for (int i = tid; i < npad; i += 1024) u[i] = v[i];
    __syncthreads();
    for (int kb = 0; kb < npad; kb += NB) {            // L y = u, block by block: y_kb = Linv_kb u_kb, then the strip below
      const double *Li = inv + (size_t)(kb / NB) * NB * NB;
      double sacc = 0.0;
      for (int c = p16; c < NB; c += 16) sacc = __builtin_fma(Li[i64 * NB + c], u[kb + c], sacc);     // Linv[r][c] = 0 for c > r
      part[p16][i64] = sacc;
      __syncthreads();
      if (tid < NB) {
        double y = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) y += part[q][tid];
        blk[tid] = y;
        u[kb + tid] = y;
      }
      __syncthreads();
      for (int i = kb + NB + tid; i < npad; i += 1024) {
        double y = u[i];
        const double *row = T + (size_t)i * ld + kb;
#pragma unroll 16
        for (int c = 0; c < NB; ++c) y = __builtin_fma(-row[c], blk[c], y);
        u[i] = y;
      }
      __syncthreads();
    }
    for (int kb = npad - NB; kb >= 0; kb -= NB) {      // L^T z = y: z_kb = Linv_kb^T y_kb, then the strip to its left
      const double *Li = inv + (size_t)(kb / NB) * NB * NB;
      double sacc = 0.0;
      for (int r = p16; r < NB; r += 16) sacc = __builtin_fma(Li[r * NB + i64], u[kb + r], sacc);
      part[p16][i64] = sacc;
      __syncthreads();
      if (tid < NB) {
        double z = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) z += part[q][tid];
        blk[tid] = z;
        u[kb + tid] = z;
      }
      __syncthreads();
      for (int c = tid; c < kb; c += 1024) {
        double y = u[c];
#pragma unroll 16
        for (int r = 0; r < NB; ++r) y = __builtin_fma(-T[(size_t)(kb + r) * ld + c], blk[r], y);
        u[c] = y;
      }
      __syncthreads();
    }
    const double vv = dot(v, v), vu = dot(v, u), uu = dot(u, u);
    mu = vu / vv;
    const double sc = uu > 0.0 ? 1.0 / sqrt(uu) : 0.0;
    for (int i = tid; i < npad; i += 1024) v[i] = i < N ? u[i] * sc : 0.0;
    __syncthreads();
  }
  if (tid == 0) { out[0] = lmax; out[1] = mu; }
}

// the diagonal-tile kernel needs 110 KB of LDS: opt in once
void launch_diag(DenseWorkspace &ws, const double *T, double *Tout, int ld, int k0, double *inv, int *fail) {
  if (!ws.diag_lds) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(chol_diag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDiagLdsBytes));
    ws.diag_lds = true;
  }
  hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(kDiagThreads), kDiagLdsBytes, ws.stream, T, Tout, ld, k0, inv, fail);
}

// Blocked Cholesky of the first nf (multiple of 64) columns of T; inv receives
// the nf/64 inverted diagonal blocks (64x64 each).
void factor_launches(DenseWorkspace &ws, double *T, int ld, int nrows, int nf, int *fail, double *inv, int ibase) {
  hipStream_t s = ws.stream;
  const int iend = ibase >= 0 ? ibase + nf : -1;
  if (ibase < 0) ibase = 1 << 30;
  for (int k0 = 0; k0 < nf; k0 += NB) {
    double *inv_k = inv + (size_t)(k0 / NB) * NB * NB;
    launch_diag(ws, T, T, ld, k0, inv_k, fail);
    const int slabs = (nrows - (k0 + NB) + NB - 1) / NB;
    if (slabs > 0) hipLaunchKernelGGL(chol_trsm_kernel, dim3(slabs), dim3(256), 0, s, T, T, ld, nrows, k0, inv_k, ibase, iend);
    const int tr = (nrows - (k0 + NB) + NB - 1) / NB, tc = (ld - (k0 + NB) + NB - 1) / NB;
    if (tr > 0 && tc > 0) hipLaunchKernelGGL(chol_update_kernel, dim3(tc, tr), dim3(256), 0, s, T, ld, nrows, k0);
  }
}

}  // namespace

void launch_back_solve(DenseWorkspace &ws, const double *T, int ld, int nf, int yrow, int nreal, const int *map, double *out, double *xs,
                       const double *inv) {
  hipStream_t s = ws.stream;
  if (nf <= kBackSolveLdsRows) {
    if (!ws.back_solve_lds) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(back_solve_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(kBackSolveLdsRows * sizeof(double))));
      ws.back_solve_lds = true;
    }
    hipLaunchKernelGGL(back_solve_kernel<true>, dim3(1), dim3(1024), (size_t)nf * sizeof(double), s, T, ld, nf, yrow, nreal, map, out, xs, inv);
  } else {
    hipLaunchKernelGGL(back_solve_kernel<false>, dim3(1), dim3(1024), 0, s, T, ld, nf, yrow, nreal, map, out, xs, inv);
  }
}

void launch_build_pivot(DenseWorkspace &ws, const double *lhs, int n, const int *S, int ns, int nspad, const double *beff, double *T, bool identity_rows, int *pos0, int *idx0) {
  const size_t rows = (size_t)(identity_rows ? 2 : 1) * nspad + 1;
  hipLaunchKernelGGL(build_pivot_kernel, dim3(grid1(rows * nspad)), dim3(256), 0, ws.stream, lhs, n, S, ns, nspad, beff, T, identity_rows ? 1 : 0, pos0, idx0);
}

void launch_inverse_rows_solve(DenseWorkspace &ws, const double *T, int ld, int nf, int ibase, const double *z, int nreal, const int *map, double *out, const uint8_t *keep) {
  hipLaunchKernelGGL(inverse_rows_solve_kernel, dim3((nreal + 3) / 4), dim3(256), 0, ws.stream, T, ld, nf, ibase, z, nreal, map, out, keep);
}

// ibase >= 0: rows [ibase, ibase + nf) of T hold an identity block (ibase a multiple of 64, at or below nf).  The panel
// solves turn it into L^-T row by row -- row i is zero left of column i, so a 64-row block of it is skipped until the
// panels reach its columns -- and a solve with the factor becomes ONE matrix-vector product with those rows
// (inverse_rows_solve_kernel) instead of a block-by-block back substitution in a single workgroup, which one CU's
// memory bandwidth bounds (the strips of L are n^2 / 2 doubles: 34 us at n = 512, 105 us at n = 1088).  The extra
// tiles run on other CUs in the shadow of the diagonal tile's chain.
void factor(DenseWorkspace &ws, double *T, int ld, int nrows, int nf, int *fail, double *inv, int ibase) {
  if (nf <= 0) return;
  hipStream_t s = ws.stream;
  static const bool fused = [] { const char *e = std::getenv("EGS_CHOL_FUSED"); return !(e && std::atoi(e) == 0); }();
  if (!fused || nf <= NB) { factor_launches(ws, T, ld, nrows, nf, fail, inv, ibase); return; }
  const int iend = ibase >= 0 ? ibase + nf : -1;
  if (ibase < 0) ibase = 1 << 30;
  const size_t need = (size_t)nrows * ld;
  if (ws.factor_work.cap < need) {      // the second array: grow-only, a quarter of head-room from the start
    if (ws.factor_work.p) HIPCHK(hipStreamSynchronize(s));
    ws.factor_work.release();
    ws.factor_work.alloc(need + need / 4);
  }
  double *Tl = ws.factor_work.p;
  const size_t lds = (size_t)(3 * NB * kStageLd + 32 * kTileQs + NB) * sizeof(double);
  if (!ws.panel_lds) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(chol_panel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ws.panel_lds = true;
  }
  // the first diagonal block has no update before it
  launch_diag(ws, T, Tl, ld, 0, inv, fail);
  for (int k0 = 0; k0 < nf; k0 += NB) {
    double *inv_k = inv + (size_t)(k0 / NB) * NB * NB;
    const int tr = (nrows - (k0 + NB) + NB - 1) / NB, tc = (ld - (k0 + NB) + NB - 1) / NB;
    if (tr > 0 && tc > 0) {
      const int factor_next = (k0 + NB < nf) ? 1 : 0;
      hipLaunchKernelGGL(chol_panel_kernel, dim3(tc, tr), dim3(kPanelThreads), lds, s, T, Tl, ld, nrows, k0, inv_k, inv_k + NB * NB, fail, factor_next, ibase, iend);
    } else {
      // nothing to the right of this panel: only the rows below it are left to solve (k0 + 64 == nf here)
      const int slabs = (nrows - (k0 + NB) + NB - 1) / NB;
      if (slabs > 0) hipLaunchKernelGGL(chol_trsm_kernel, dim3(slabs), dim3(256), 0, s, T, Tl, ld, nrows, k0, inv_k, ibase, iend);
    }
  }
  hipLaunchKernelGGL(merge_factor_kernel, dim3(grid1((size_t)nrows * nf)), dim3(256), 0, s, T, Tl, ld, nrows, nf);
}

double dense_condition_estimate(DenseWorkspace &ws, int N, const double *dA, bool *spd, double *pivot_bound) {
  if (spd) *spd = true;
  if (pivot_bound) *pivot_bound = 1.0;
  if (N == 0) return 1.0;
  hipStream_t s = ws.stream;
  const int npad = (N + NB - 1) / NB * NB;
  Buf<double> T(ws, (size_t)(npad + 1) * npad), dinv(ws, (size_t)npad * NB), zero(ws, N), mm(ws, 4);
  Buf<int> idx_d(ws, N), fail_d(ws, 1);
  std::vector<int> idx(N);
  for (int i = 0; i < N; ++i) idx[i] = i;
  HIPCHK(hipMemcpyAsync(idx_d.p, idx.data(), N * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(zero.p, 0, N * sizeof(double), s));
  HIPCHK(hipMemsetAsync(fail_d.p, 0, sizeof(int), s));
  launch_build_pivot(ws, dA, N, idx_d.p, N, npad, zero.p, T.p, false, nullptr, nullptr);
  factor(ws, T.p, npad, npad + 1, npad, fail_d.p, dinv.p);
  hipLaunchKernelGGL(diag_minmax_kernel, dim3(1), dim3(256), 0, s, T.p, npad, N, mm.p);
  double h[4] = {1, 1, 0, 0};
  int fail = 0;
  HIPCHK(hipMemcpyAsync(h, mm.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&fail, fail_d.p, sizeof fail, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (fail || !(h[1] > 0)) { if (spd) *spd = false; return std::numeric_limits<double>::infinity(); }
  const double r = h[0] / h[1];
  if (pivot_bound) *pivot_bound = r * r;
  if (N > kCondMaxRows) return r * r;      // beyond one workgroup's vectors: the pivot bound (a LOWER bound) is all there is
  // 60 iterations each: the Rayleigh quotients converge like (lambda_2 / lambda_1)^(2k); both approach from below
  hipLaunchKernelGGL(cond_iterations_kernel, dim3(1), dim3(1024), 0, s, dA, N, T.p, npad, npad, dinv.p, 60, mm.p + 2);
  HIPCHK(hipMemcpyAsync(h + 2, mm.p + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const double est = h[2] * h[3];
  return est > r * r ? est : r * r;          // two lower bounds: the larger one
}

}  // namespace egs
