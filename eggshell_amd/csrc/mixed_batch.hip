// mixed_batch.hip -- Lcp::MixedConstraintsSolver (lcp.cc:276-336) for MANY problems on explicit matrices in one fused
// pipeline (egs_mixed_constraints_solve_batch): what the reference's own test of the function does one problem after
// another (lcp.cc:412-528).  One workgroup per problem of at most 112 rows runs the stage of mixed_solve_device.h --
// the second half of dense_world_fused_kernel -- on the caller's packed matrix and writes x, w, ok and pivots in the
// caller's row order.  Size classes and launch geometry are the world kernel's (dense_world.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <stdexcept>
#include <vector>

#include "dense_lcp.h"
#include "dense_world.h"
#include "mixed_solve_device.h"
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

// LDS_WS: Z = L^-1 [A_ei | b_e] and the Schur complement sit in LDS behind the vectors.  ne (ni + 1) + ni^2 =
// ni (n - 1) + n <= n^2 doubles whatever the partition, so MAXN^2 doubles hold both.  Otherwise they sit in the
// problem's n^2-double slice of the workspace.
template <int MAXN, int BLOCK, bool LDS_WS>
__global__ void __launch_bounds__(BLOCK) mixed_batch_kernel(MixedBatchArgs a, const int32_t *list) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const MixedSolveLds L(sm, MAXN);
  __shared__ MixedSolveShared<MAXN> sh;
  const int tid = threadIdx.x;
  const int p = list[blockIdx.x];
  const MixedBatchProblem P = a.prob[p];
  const int N = P.n;
  if (N < 1 || N > MAXN) {      // never launched this way (the host sorts by n); no row is touched
    if (tid == 0) { a.out[p].ok = 0; a.out[p].pivots = 0; }
    return;
  }
  const double *A = a.A + P.a_off;
  const double *vb = a.b + P.v_off, *vlo = a.lo + P.v_off, *vhi = a.hi + P.v_off;
  const uint8_t *vc = a.C + P.v_off;
  mixed_partition(sh, N, [&](int i) { return vc[i] != 0; });
  double *Lh = LDS_WS ? sm + mixed_solve_lds_doubles(MAXN) : a.ws + P.ws_off;
  double *Z = Lh + sh.ni * sh.ni;
  const MixedSolveResult res = mixed_solve_stage<MAXN, BLOCK>(sh, L, A, N, vb, vlo, vhi, Z, Lh, a.use_bounds, a.max_pivots);
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

}  // namespace

void mixed_constraints_fused(DenseWorkspace &ws, const LaunchHooks &hooks, int count, const int32_t *sel, const int32_t *n,
                             const int64_t *a_off, const int64_t *v_off, const double *A, const double *b, const uint8_t *C,
                             const double *lo, const double *hi, bool use_bounds, int max_pivots, double *x, double *w, int32_t *ok,
                             int32_t *pivots) {
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
  // one packed block, the same layout on both sides:  x w out | A b lo hi prob list C | workspace (device only)
  // read back: everything before A; uploaded: from A to the end of C
  const auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
  const size_t o_x = 0, o_w = o_x + vt * 8, o_out = o_w + vt * 8, o_A = up16(o_out + (size_t)count * sizeof(MixedBatchOut)),
               o_b = o_A + at * 8, o_lo = o_b + vt * 8, o_hi = o_lo + vt * 8, o_prob = o_hi + vt * 8,
               o_list = o_prob + (size_t)count * sizeof(MixedBatchProblem), o_C = o_list + (size_t)count * 4, o_end = o_C + vt,
               o_ws = up16(o_end), total = o_ws + wt * 8;
  char *h = static_cast<char *>(hooks.take(hooks.self, o_end));
  double *hA = reinterpret_cast<double *>(h + o_A), *hb = reinterpret_cast<double *>(h + o_b), *hlo = reinterpret_cast<double *>(h + o_lo),
         *hhi = reinterpret_cast<double *>(h + o_hi);
  int32_t *hlist = reinterpret_cast<int32_t *>(h + o_list);
  uint8_t *hC = reinterpret_cast<uint8_t *>(h + o_C);
  for (int f = 0; f < count; ++f) {
    const int k = sel[f];
    const size_t nk = (size_t)n[k];
    std::memcpy(hA + prob[f].a_off, A + a_off[k], nk * nk * sizeof(double));
    std::memcpy(hb + prob[f].v_off, b + v_off[k], nk * sizeof(double));
    std::memcpy(hlo + prob[f].v_off, lo + v_off[k], nk * sizeof(double));
    std::memcpy(hhi + prob[f].v_off, hi + v_off[k], nk * sizeof(double));
    std::memcpy(hC + prob[f].v_off, C + v_off[k], nk);
  }
  std::memcpy(h + o_prob, prob.data(), (size_t)count * sizeof(MixedBatchProblem));
  size_t lp = 0;
  for (int c = 0; c < 3; ++c) { std::copy(cls_list[c].begin(), cls_list[c].end(), hlist + lp); lp += cls_list[c].size(); }
  ScopedDevBuf<char> d(total);
  HIPCHK(hipMemcpyAsync(d.p + o_A, h + o_A, o_end - o_A, hipMemcpyHostToDevice, s));
  MixedBatchArgs a{};
  a.prob = reinterpret_cast<MixedBatchProblem *>(d.p + o_prob);
  a.A = reinterpret_cast<double *>(d.p + o_A); a.b = reinterpret_cast<double *>(d.p + o_b);
  a.lo = reinterpret_cast<double *>(d.p + o_lo); a.hi = reinterpret_cast<double *>(d.p + o_hi);
  a.C = reinterpret_cast<uint8_t *>(d.p + o_C);
  a.x = reinterpret_cast<double *>(d.p + o_x); a.w = reinterpret_cast<double *>(d.p + o_w);
  a.out = reinterpret_cast<MixedBatchOut *>(d.p + o_out);
  a.ws = reinterpret_cast<double *>(d.p + o_ws);
  a.use_bounds = use_bounds ? 1 : 0; a.max_pivots = max_pivots;
  const int32_t *dlist = reinterpret_cast<int32_t *>(d.p + o_list);
  if (hooks.mark) hooks.mark(hooks.self, true);
  lp = 0;
  if (!cls_list[0].empty()) launch_mixed_batch<32, 64, true>(a, dlist + lp, (int)cls_list[0].size(), &ws.mixed_batch_lds[0], s);
  lp += cls_list[0].size();
  if (!cls_list[1].empty()) launch_mixed_batch<64, 64, true>(a, dlist + lp, (int)cls_list[1].size(), &ws.mixed_batch_lds[1], s);
  lp += cls_list[1].size();
  if (!cls_list[2].empty()) launch_mixed_batch<112, 256, false>(a, dlist + lp, (int)cls_list[2].size(), &ws.mixed_batch_lds[2], s);
  if (hooks.mark) hooks.mark(hooks.self, false);
  HIPCHK(hipMemcpyAsync(h, d.p, o_out + (size_t)count * sizeof(MixedBatchOut), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const double *hx = reinterpret_cast<const double *>(h + o_x), *hw = reinterpret_cast<const double *>(h + o_w);
  const MixedBatchOut *hout = reinterpret_cast<const MixedBatchOut *>(h + o_out);
  for (int f = 0; f < count; ++f) {
    const int k = sel[f];
    const size_t nk = (size_t)n[k];
    std::memcpy(x + v_off[k], hx + prob[f].v_off, nk * sizeof(double));
    std::memcpy(w + v_off[k], hw + prob[f].v_off, nk * sizeof(double));
    ok[k] = hout[f].ok;
    if (pivots) pivots[k] = hout[f].pivots;
  }
}

}  // namespace egs
