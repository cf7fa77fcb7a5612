// mixed_batch.hip -- Lcp::MixedConstraintsSolver (lcp.cc:276-336) for MANY problems on explicit matrices in one fused
// pipeline (egs_mixed_constraints_solve_batch): what the reference's own test of the function does one problem after
// another (lcp.cc:412-528).  One workgroup per problem of at most 112 rows runs the stage of mixed_solve_device.h --
// the second half of dense_world_fused_kernel -- on the caller's packed matrix and writes x, w, ok and pivots in the
// caller's row order.  Size classes and launch geometry are the world kernel's (dense_world.h).
// mixed_friction_batch_kernel is the same body around the stage's pyramid form (egs_mixed_friction_solve_batch): the rows
// with a normal row are inequality rows whatever C says, and it also writes beta, the solves made and the last change.
#include <hip/hip_runtime.h>

#include <cstring>
#include <stdexcept>
#include <vector>

#include "dense_lcp.h"
#include "dense_world.h"
#include "mixed_solve_device.h"
#include "packed_block.h"
#include "runtime.h"

namespace egs {

namespace {

struct MixedBatchProblem {   // one fused problem, in the packed device block
  int64_t a_off;             // its matrix, in doubles from A
  int64_t v_off;             // its vectors, in rows
  int64_t ws_off;            // its slice of the global workspace, in doubles (the 112-row class only)
  int32_t n, pad;
};
struct MixedBatchOut { int32_t ok, pivots; };

struct MixedBatchArgs {
  const MixedBatchProblem *prob;
  const double *A, *b, *lo, *hi;
  const uint8_t *C;
  double *x, *w;
  MixedBatchOut *out;
  double *ws;
  int32_t use_bounds, max_pivots;
};

struct MixedFrictionOut { int32_t outer, pad; double change; };
struct MixedFrictionArgs {   // the pyramid form's own arguments, packed like the vectors
  const int32_t *nrow;
  const double *mu;
  double *beta;
  MixedFrictionOut *out;
  double tol;
  int32_t max_outer, pad;
};
struct NoFrictionArgs {};

// LDS_WS: Z = L^-1 [A_ei | b_e] and the Schur complement sit in LDS behind the vectors.  ne (ni + 1) + ni^2 =
// ni (n - 1) + n <= n^2 doubles whatever the partition, so MAXN^2 doubles hold both.  Otherwise they sit in the
// problem's n^2-double slice of the workspace.
template <int MAXN, int BLOCK, bool LDS_WS, bool PYR, typename FrictionArgs>
__device__ __forceinline__ void mixed_batch_body(double *sm, MixedSolveShared<MAXN> &sh, const MixedBatchArgs &a, const int32_t *list,
                                                 const FrictionArgs &fa) {
  const MixedSolveLds L(sm, MAXN);
  const int tid = threadIdx.x;
  const int p = list[blockIdx.x];
  const MixedBatchProblem P = a.prob[p];
  const int N = P.n;
  if (N < 1 || N > MAXN) {      // never launched this way (the host sorts by n); no row is touched
    if (tid == 0) { a.out[p].ok = 0; a.out[p].pivots = 0; }
    if constexpr (PYR) {
      if (tid == 0) { fa.out[p].outer = 0; fa.out[p].change = 0.0; }
    }
    return;
  }
  const double *A = a.A + P.a_off;
  const double *vb = a.b + P.v_off, *vlo = a.lo + P.v_off, *vhi = a.hi + P.v_off;
  const uint8_t *vc = a.C + P.v_off;
  MixedPyramid<PYR> pyr;
  constexpr size_t kVectors = PYR ? mixed_pyramid_lds_doubles(MAXN) : mixed_solve_lds_doubles(MAXN);
  if constexpr (PYR) {
    pyr.nrow = fa.nrow + P.v_off; pyr.mu = fa.mu + P.v_off;
    pyr.max_outer = fa.max_outer; pyr.tol = fa.tol;
    pyr.ext = sm + mixed_solve_lds_doubles(MAXN);
    pyr.outer = 0; pyr.change = 0.0;
    const int32_t *nr = pyr.nrow;
    mixed_partition(sh, N, [&](int i) { return vc[i] != 0 && nr[i] < 0; });     // a pyramid row is an inequality row
  } else {
    mixed_partition(sh, N, [&](int i) { return vc[i] != 0; });
  }
  double *Lh = LDS_WS ? sm + kVectors : a.ws + P.ws_off;
  double *Z = Lh + sh.ni * sh.ni;
  const MixedSolveResult res = mixed_solve_stage<MAXN, BLOCK, PYR>(sh, L, A, N, vb, vlo, vhi, Z, Lh, a.use_bounds, a.max_pivots, pyr);
  // x and w in the caller's row order; w = 0 on the equality rows (lcp.cc:332-333).  A failed problem leaves zeros.
  double *xo = a.x + P.v_off, *wo = a.w + P.v_off;
  const int ne = sh.ne, ni = sh.ni;
  for (int k = tid; k < ne; k += BLOCK) {
    const int row = sh.idxE[k];
    xo[row] = res.solved ? L.y2[k] : 0.0;
    wo[row] = 0.0;
  }
  for (int k = tid; k < ni; k += BLOCK) {
    const int row = sh.idxI[k];
    xo[row] = res.solved ? L.x[k] : 0.0;
    wo[row] = res.solved ? L.w[k] : 0.0;
  }
  if (tid == 0) { a.out[p].ok = res.solved; a.out[p].pivots = res.pivots; }
  if constexpr (PYR) {
    // beta: the bound the returned x was solved under, 0 on every plain row and for a failed problem
    double *bo = fa.beta + P.v_off;
    for (int k = tid; k < ne; k += BLOCK) bo[sh.idxE[k]] = 0.0;
    for (int k = tid; k < ni; k += BLOCK) bo[sh.idxI[k]] = (res.solved && pyr.normal_of(sh.idxI[k]) >= 0) ? L.hi[k] : 0.0;
    if (tid == 0) {
      fa.out[p].outer = (res.solved && pyr.outer == 0) ? 1 : pyr.outer;     // no inequality row: the one solve is the Schur stage
      fa.out[p].change = res.solved ? pyr.change : 0.0;
    }
  }
}

template <int MAXN, int BLOCK, bool LDS_WS>
__global__ void __launch_bounds__(BLOCK) mixed_batch_kernel(MixedBatchArgs a, const int32_t *list) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ MixedSolveShared<MAXN> sh;
  mixed_batch_body<MAXN, BLOCK, LDS_WS, false>(sm, sh, a, list, NoFrictionArgs{});
}

template <int MAXN, int BLOCK, bool LDS_WS>
__global__ void __launch_bounds__(BLOCK) mixed_friction_batch_kernel(MixedBatchArgs a, const int32_t *list, MixedFrictionArgs fa) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ MixedSolveShared<MAXN> sh;
  mixed_batch_body<MAXN, BLOCK, LDS_WS, true>(sm, sh, a, list, fa);
}

template <int MAXN, int BLOCK, bool LDS_WS>
void launch_mixed_batch(const MixedBatchArgs &a, const int32_t *list, int count, bool *raised, hipStream_t s) {
  const size_t lds = (mixed_solve_lds_doubles(MAXN) + (LDS_WS ? (size_t)MAXN * MAXN : 0)) * sizeof(double);
  if (lds > 48 * 1024 && !*raised) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(mixed_batch_kernel<MAXN, BLOCK, LDS_WS>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    *raised = true;
  }
  hipLaunchKernelGGL((mixed_batch_kernel<MAXN, BLOCK, LDS_WS>), dim3((unsigned)count), dim3(BLOCK), lds, s, a, list);
  HIPCHK(hipGetLastError());
}

template <int MAXN, int BLOCK, bool LDS_WS>
void launch_mixed_friction_batch(const MixedBatchArgs &a, const MixedFrictionArgs &fa, const int32_t *list, int count, bool *raised,
                                 hipStream_t s) {
  const size_t lds = (mixed_pyramid_lds_doubles(MAXN) + (LDS_WS ? (size_t)MAXN * MAXN : 0)) * sizeof(double);
  if (lds > 48 * 1024 && !*raised) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(mixed_friction_batch_kernel<MAXN, BLOCK, LDS_WS>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    *raised = true;
  }
  hipLaunchKernelGGL((mixed_friction_batch_kernel<MAXN, BLOCK, LDS_WS>), dim3((unsigned)count), dim3(BLOCK), lds, s, a, list, fa);
  HIPCHK(hipGetLastError());
}

}  // namespace

void mixed_constraints_fused(DenseWorkspace &ws, const LaunchHooks &hooks, int count, const int32_t *sel, const int32_t *n,
                             const int64_t *a_off, const int64_t *v_off, const double *A, const double *b, const uint8_t *C,
                             const double *lo, const double *hi, bool use_bounds, int max_pivots, double *x, double *w, int32_t *ok,
                             int32_t *pivots, const MixedFrictionBatch *fr) {
  if (count <= 0) return;
  hipStream_t s = ws.stream;
  // sizes of the packed block: the fused problems one after another, each class's index list
  std::vector<int32_t> cls_list[3];
  size_t at = 0, vt = 0, wt = 0;
  std::vector<MixedBatchProblem> prob((size_t)count);
  for (int f = 0; f < count; ++f) {
    const size_t nk = (size_t)n[sel[f]];
    if (nk < 1 || nk > (size_t)kFusedDenseMax) throw std::invalid_argument("mixed constraints batch: a fused problem has 1 .. 112 rows");
    const int cls = nk <= (size_t)kDenseClassRows[0] ? 0 : nk <= (size_t)kDenseClassRows[1] ? 1 : 2;
    cls_list[cls].push_back(f);
    prob[f] = MixedBatchProblem{(int64_t)at, (int64_t)vt, (int64_t)wt, (int32_t)nk, 0};
    at += nk * nk; vt += nk;
    if (cls == 2) wt += nk * nk;
  }
  // one packed block, the same layout on both sides (packed_block.h).  read back: x w [beta fout] out; uploaded: A b lo
  // hi [mu] prob list [nrow] C; device only: the 112-row class's workspace.  [..]: the pyramid form only.
  const size_t nc = (size_t)count, fv = fr ? vt : 0, fc = fr ? nc : 0;
  PackedBlock blk;
  const auto s_x = blk.add<double>(Zone::Download, vt), s_w = blk.add<double>(Zone::Download, vt), s_beta = blk.add<double>(Zone::Download, fv);
  const auto s_fout = blk.add<MixedFrictionOut>(Zone::Download, fc);
  const auto s_out = blk.add<MixedBatchOut>(Zone::Download, nc);
  const auto s_A = blk.add<double>(Zone::Upload, at, 16), s_b = blk.add<double>(Zone::Upload, vt), s_lo = blk.add<double>(Zone::Upload, vt),
             s_hi = blk.add<double>(Zone::Upload, vt), s_mu = blk.add<double>(Zone::Upload, fv);
  const auto s_prob = blk.add<MixedBatchProblem>(Zone::Upload, nc);
  const auto s_list = blk.add<int32_t>(Zone::Upload, nc), s_nrow = blk.add<int32_t>(Zone::Upload, fv);
  const auto s_C = blk.add<uint8_t>(Zone::Upload, vt);
  const auto s_ws = blk.add<double>(Zone::Scratch, wt, 16);
  char *h = static_cast<char *>(hooks.take(hooks.self, blk.host_bytes()));
  ScopedDevBuf<char> d(blk.total_bytes());
  blk.bind(h, d.p);
  const auto rows = [&](int f) { return (size_t)prob[f].n; };
  const auto entries = [&](int f) { return (size_t)prob[f].n * (size_t)prob[f].n; };
  const auto a_at = [&](int f) { return (size_t)prob[f].a_off; };
  const auto v_at = [&](int f) { return (size_t)prob[f].v_off; };
  gather_ragged(blk.host(s_A), A, count, sel, a_off, entries, a_at);
  gather_ragged(blk.host(s_b), b, count, sel, v_off, rows, v_at);
  gather_ragged(blk.host(s_lo), lo, count, sel, v_off, rows, v_at);
  gather_ragged(blk.host(s_hi), hi, count, sel, v_off, rows, v_at);
  gather_ragged(blk.host(s_C), C, count, sel, v_off, rows, v_at);
  if (fr) {
    gather_ragged(blk.host(s_mu), fr->mu, count, sel, v_off, rows, v_at);
    gather_ragged(blk.host(s_nrow), fr->normal_row, count, sel, v_off, rows, v_at);
  }
  std::copy(prob.begin(), prob.end(), blk.host(s_prob));
  size_t lp = 0;
  for (int c = 0; c < 3; ++c) { std::copy(cls_list[c].begin(), cls_list[c].end(), blk.host(s_list) + lp); lp += cls_list[c].size(); }
  HIPCHK(hipMemcpyAsync(d.p + blk.upload_begin(), h + blk.upload_begin(), blk.upload_end() - blk.upload_begin(), hipMemcpyHostToDevice, s));
  MixedBatchArgs a{};
  a.prob = blk.device(s_prob);
  a.A = blk.device(s_A); a.b = blk.device(s_b); a.lo = blk.device(s_lo); a.hi = blk.device(s_hi);
  a.C = blk.device(s_C);
  a.x = blk.device(s_x); a.w = blk.device(s_w);
  a.out = blk.device(s_out);
  a.ws = blk.device(s_ws);
  a.use_bounds = use_bounds ? 1 : 0; a.max_pivots = max_pivots;
  const int32_t *dlist = blk.device(s_list);
  if (hooks.mark) hooks.mark(hooks.self, true);
  lp = 0;
  if (fr) {
    MixedFrictionArgs fa{};
    fa.nrow = blk.device(s_nrow); fa.mu = blk.device(s_mu); fa.beta = blk.device(s_beta); fa.out = blk.device(s_fout);
    fa.tol = fr->tol; fa.max_outer = fr->max_outer;
    if (!cls_list[0].empty()) launch_mixed_friction_batch<32, 64, true>(a, fa, dlist + lp, (int)cls_list[0].size(), &ws.mixed_friction_lds[0], s);
    lp += cls_list[0].size();
    if (!cls_list[1].empty()) launch_mixed_friction_batch<64, 64, true>(a, fa, dlist + lp, (int)cls_list[1].size(), &ws.mixed_friction_lds[1], s);
    lp += cls_list[1].size();
    if (!cls_list[2].empty()) launch_mixed_friction_batch<112, 256, false>(a, fa, dlist + lp, (int)cls_list[2].size(), &ws.mixed_friction_lds[2], s);
  } else {
    if (!cls_list[0].empty()) launch_mixed_batch<32, 64, true>(a, dlist + lp, (int)cls_list[0].size(), &ws.mixed_batch_lds[0], s);
    lp += cls_list[0].size();
    if (!cls_list[1].empty()) launch_mixed_batch<64, 64, true>(a, dlist + lp, (int)cls_list[1].size(), &ws.mixed_batch_lds[1], s);
    lp += cls_list[1].size();
    if (!cls_list[2].empty()) launch_mixed_batch<112, 256, false>(a, dlist + lp, (int)cls_list[2].size(), &ws.mixed_batch_lds[2], s);
  }
  if (hooks.mark) hooks.mark(hooks.self, false);
  HIPCHK(hipMemcpyAsync(h, d.p, blk.download_bytes(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  scatter_ragged(x, blk.host(s_x), count, sel, v_off, rows, v_at);
  scatter_ragged(w, blk.host(s_w), count, sel, v_off, rows, v_at);
  if (fr && fr->beta) scatter_ragged(fr->beta, blk.host(s_beta), count, sel, v_off, rows, v_at);
  const MixedBatchOut *hout = blk.host(s_out);
  const MixedFrictionOut *hf = blk.host(s_fout);
  for (int f = 0; f < count; ++f) {
    const int k = sel[f];
    ok[k] = hout[f].ok;
    if (pivots) pivots[k] = hout[f].pivots;
    if (fr) { fr->outer[k] = hf[f].outer; fr->change[k] = hf[f].change; }
  }
}

bool mixed_friction_host(DenseWorkspace &ws, int N, const double *A, const double *b, const uint8_t *C, const double *lo,
                         const double *hi, const int32_t *normal_row, const double *mu, int max_pivots, int max_outer, double tol,
                         double *x, double *w, double *beta_out, int *pivots, int *outer, double *change, std::string *msg) {
  std::vector<double> beta((size_t)N, 0.0), next((size_t)N, 0.0), A2, b2, lo2, hi2, x2, w2;
  std::vector<uint8_t> C2;
  std::vector<int> keep;
  *pivots = 0; *outer = 0; *change = 0.0;
  for (int i = 0; i < N; ++i) { x[i] = 0.0; w[i] = 0.0; }
  if (beta_out) std::fill(beta_out, beta_out + N, 0.0);
  for (int k = 1;; ++k) {
    // P(beta^k) without its pinned rows (x = 0 there, so the other rows lose nothing)
    keep.clear();
    for (int i = 0; i < N; ++i)
      if (normal_row[i] < 0 || beta[i] > 0.0) keep.push_back(i);
    const int m = (int)keep.size();
    A2.resize((size_t)m * m); b2.resize(m); lo2.resize(m); hi2.resize(m); x2.assign(m, 0.0); w2.assign(m, 0.0); C2.resize(m);
    for (int r = 0; r < m; ++r) {
      const int i = keep[r];
      const bool pyr = normal_row[i] >= 0;
      for (int c = 0; c < m; ++c) A2[(size_t)r * m + c] = A[(size_t)i * N + keep[c]];
      b2[r] = b[i];
      C2[r] = pyr ? 0 : C[i];
      lo2[r] = pyr ? -beta[i] : lo[i];
      hi2[r] = pyr ? beta[i] : hi[i];
    }
    int piv = 0;
    const bool good = dense_mixed_constraints(ws, m, A2.data(), b2.data(), C2.data(), lo2.data(), hi2.data(), true, false, x2.data(),
                                              w2.data(), &piv, msg, max_pivots, 0.0);
    *pivots += piv;
    *outer = k;
    if (!good) {
      for (int i = 0; i < N; ++i) { x[i] = 0.0; w[i] = 0.0; }
      return false;
    }
    for (int i = 0; i < N; ++i) { x[i] = 0.0; w[i] = 0.0; }
    for (int r = 0; r < m; ++r) { x[keep[r]] = x2[r]; w[keep[r]] = w2[r]; }
    for (int i = 0; i < N; ++i) {
      if (normal_row[i] < 0 || beta[i] > 0.0) continue;
      double s = 0.0;                                   // a pinned row's w = (A x - b)_i
      for (int c = 0; c < N; ++c) s = std::fma(A[(size_t)i * N + c], x[c], s);
      w[i] = s - b[i];
    }
    double dmax = 0.0, bmax = 0.0;
    for (int i = 0; i < N; ++i) {
      next[i] = 0.0;
      if (normal_row[i] < 0) continue;
      const double xf = x[normal_row[i]];
      next[i] = xf > 0.0 ? mu[i] * xf : 0.0;
      dmax = std::fmax(dmax, std::fabs(next[i] - beta[i]));
      bmax = std::fmax(bmax, next[i]);
    }
    *change = dmax / (bmax > 1.0 ? bmax : 1.0);
    if (beta_out) std::copy(beta.begin(), beta.end(), beta_out);
    if (*change <= tol || k >= max_outer) return true;
    beta.swap(next);
  }
}

}  // namespace egs
