// dense_lcp.hip -- the two dense direct solvers of the reference with the O(n^3) pieces on the GPU:
// Lcp::MixedConstraintsSolver (lcp.cc:276-336) and lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747).  All matrices
// row-major fp64, resident in HBM for the whole call.
//   * Both permute to [E | I], append b as a last row and factor only the E columns (SchurStage): the trailing block IS
//     the Schur complement A_ii - A_ie A_ee^-1 A_ei, the trailing part of the b row IS b_i - A_ie A_ee^-1 b_e, and the
//     b row's E part is L^-1 b_e (lcp.cc:286-294).
//   * The factorisation and the solves with its factor are dense_factor.hip's; the reduced LCP goes to the Murty pivot
//     loop of dense_murty.hip or, in SolveLCP_BoxSchur up to kIncrementalMaxRows bounded rows, to dantzig.hip.
// The reference factors with Eigen's pivoted LDLT / LU inverse; A is required to be symmetric with positive definite
// A_ee and A(S,S) (true for J M^-1 J^T + cfm I and for the reference's own tests); otherwise the call reports failure
// instead of a wrong answer.
#include "dense_internal.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <limits>
#include <stdexcept>

namespace egs {

namespace {

// max |a_ij| and max |a_ij - a_ji| over i > j (non-negative doubles order like
// their bit patterns, so an integer atomicMax does the reduction).
__global__ void __launch_bounds__(256) symmetry_kernel(const double *A, int N, unsigned long long *out /*[2]*/) {
  // 32 x 32 tiles: tile (bi, bj) with bj <= bi is compared with the transpose of tile (bj, bi)
  // staged through LDS, so both reads walk rows
  __shared__ double tT[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  double amax = 0.0, asym = 0.0;
  if (bj <= bi) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
      const int gi = bj * 32 + r, gj = bi * 32 + tx;           // element of the mirror tile
      tT[r][tx] = (gi < N && gj < N) ? A[(size_t)gi * N + gj] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int gi = bi * 32 + r, gj = bj * 32 + tx;
      if (gi < N && gj < N && gj < gi) {
        const double v = A[(size_t)gi * N + gj];
        amax = fmax(amax, fabs(v));
        asym = fmax(asym, fabs(v - tT[tx][r]));
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    amax = fmax(amax, __shfl_down(amax, o, 64));
    asym = fmax(asym, __shfl_down(asym, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    // the maxima only grow: a (possibly stale) plain read that is already >= ours makes the atomic
    // pointless -- almost every wavefront then skips it instead of queueing on two addresses
    const unsigned long long ua = (unsigned long long)__double_as_longlong(amax), us = (unsigned long long)__double_as_longlong(asym);
    if (ua > __hip_atomic_load(&out[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&out[0], ua);
    if (us > __hip_atomic_load(&out[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&out[1], us);
  }
}

// ---- gathers ---------------------------------------------------------------
// Schur-stage trapezoid: rows = nepad + ni + 1, ld = nepad + ni (see header).
// lower_only: A holds a symmetric matrix in its lower triangle and nothing else is read (toolkit/lcp.h:73).
__global__ void build_schur_kernel(const double *A, const double *b, int N, const int *E, int ne, int nepad,
                                   const int *I, int ni, double *T, int lower_only) {
  const int ld = nepad + ni, rows = nepad + ni + 1;
  const size_t total = (size_t)rows * ld;
  auto at = [&](int gr, int gcol) {
    if (lower_only && gcol > gr) { const int t = gr; gr = gcol; gcol = t; }
    return A[(size_t)gr * N + gcol];
  };
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(idx / ld), c = (int)(idx % ld);
    double v = 0.0;
    const int gc = c < ne ? E[c] : (c >= nepad ? I[c - nepad] : -1);
    if (r < ne) { if (gc >= 0 && c < ne) v = at(E[r], gc); }
    else if (r < nepad) v = (c == r) ? 1.0 : 0.0;
    else if (r < nepad + ni) { if (gc >= 0) v = at(I[r - nepad], gc); }
    else { if (gc >= 0) v = b[gc]; }
    T[idx] = v;
  }
}

// lhs (ni x ni, full symmetric) and rhs from the factored trapezoid.
__global__ void extract_schur_kernel(const double *T, int nepad, int ni, double *lhs, double *rhs) {
  const int ld = nepad + ni;
  const size_t total = (size_t)ni * ni;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / ni), j = (int)(idx % ni);
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    lhs[idx] = T[(size_t)(nepad + hi) * ld + nepad + lo];
    if (i == 0) rhs[j] = T[(size_t)(nepad + ni) * ld + nepad + j];
  }
}

// t_k = T[last][k] - sum_j T[nepad+j][k] xi[j]   (k < nepad), in place.  One workgroup per 64
// columns; 16 row groups each sum every 16th row (row reads stay contiguous), then one LDS pass.
__global__ void __launch_bounds__(1024) xe_rhs_kernel(double *T, int nepad, int ni, const double *xi) {
  __shared__ double red[16][64];
  const int ld = nepad + ni;
  const int kk = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + kk;          // nepad is a multiple of 64
  double s0 = 0.0, s1 = 0.0;
  int j = part;
  for (; j + 16 < ni; j += 32) {
    s0 = __builtin_fma(T[(size_t)(nepad + j) * ld + k], xi[j], s0);
    s1 = __builtin_fma(T[(size_t)(nepad + j + 16) * ld + k], xi[j + 16], s1);
  }
  for (; j < ni; j += 16) s0 = __builtin_fma(T[(size_t)(nepad + j) * ld + k], xi[j], s0);
  red[part][kk] = s0 + s1;
  __syncthreads();
  if (part == 0) {
    double sum = 0.0;
#pragma unroll
    for (int p = 0; p < 16; ++p) sum += red[p][kk];
    T[(size_t)(nepad + ni) * ld + k] -= sum;
  }
}

__global__ void scatter_kernel(int n, const int *idx, const double *src, double *dst) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) dst[idx[k]] = src[k];
}

// What both solvers share: the trapezoid [A_ee A_ei; A_ie A_ii; b^T] over E (padded to nepad) and I, its scratch and the
// two runs of launches on it.  Uploads, the reset and read-back of `fail_d` and every synchronisation are the caller's.
struct SchurStage {
  DenseWorkspace &ws;
  const int ne, ni, nepad, ld, rows;
  Buf<double> T, lhs, rhs, xi, wi, xe, xs, dinv;      // lhs, rhs: the reduced LCP; xi, wi: its solution; xe: the E part of x
  Buf<int> fail_d;
  SchurStage(DenseWorkspace &w, int ne_, int ni_)
      : ws(w), ne(ne_), ni(ni_), nepad((ne_ + NB - 1) / NB * NB), ld(nepad + ni_), rows(ld + 1),
        T(w, (size_t)rows * (ld > 0 ? ld : 1)), lhs(w, (size_t)ni_ * ni_), rhs(w, ni_), xi(w, ni_), wi(w, ni_), xe(w, ne_), xs(w, nepad),
        dinv(w, (size_t)nepad * NB), fail_d(w, 1) {}
  // Factor the E columns (lcp.cc:286-294; toolkit/lcp.cc: L L' = Z, Q = L^-1 B'): the trailing block becomes the Schur
  // complement A_ii - A_ie A_ee^-1 A_ei (lhs), the trailing part of the b row b_i - A_ie A_ee^-1 b_e (rhs).
  void eliminate(const double *dA, const double *db, int N, const int *dE, const int *dI, int lower_only) {
    hipStream_t s = ws.stream;
    hipLaunchKernelGGL(build_schur_kernel, dim3(grid1((size_t)rows * ld)), dim3(256), 0, s, dA, db, N, dE, ne, nepad, dI, ni, T.p, lower_only);
    factor(ws, T.p, ld, rows, nepad, fail_d.p, dinv.p);
    if (ni) hipLaunchKernelGGL(extract_schur_kernel, dim3(grid1((size_t)ni * ni)), dim3(256), 0, s, T.p, nepad, ni, lhs.p, rhs.p);
  }
  // xe = A_ee^-1 (b_e - A_ei x_i) = L^-T (L^-1 b_e - (L^-1 A_ei) x_i) from xi   (lcp.cc:317); needs ne > 0
  void back_substitute() {
    hipLaunchKernelGGL(xe_rhs_kernel, dim3(nepad / NB), dim3(1024), 0, ws.stream, T.p, nepad, ni, xi.p);
    launch_back_solve(ws, T.p, ld, nepad, nepad + ni, ne, nullptr, xe.p, xs.p, dinv.p);
  }
};

// The host entry uploads the lower block trapezoids of A first and hands the rest over as `upload_rest`: the Schur stage
// (which reads the lower triangle only) is enqueued before the host pushes the remainder on a second stream, where the
// symmetry check then runs; `side` is that stream.
bool dense_mixed_impl(DenseWorkspace &ws, int N, const double *dA_in, const double *db_in, const uint8_t *C, const double *lo, const double *hi,
                      bool use_bounds, bool block_pivoting, int max_pivots, double max_seconds, double *x, double *w, double *dx_out,
                      int *pivots, std::string *msg, const std::function<void()> *upload_rest, hipStream_t side) {
  if (pivots) *pivots = 0;
  if (N == 0) return true;
  hipStream_t s = ws.stream;
  const auto t_dev0 = std::chrono::steady_clock::now();
  std::vector<int> E, I;
  for (int i = 0; i < N; ++i) (C[i] ? E : I).push_back(i);
  const int ne = (int)E.size(), ni = (int)I.size();
  SchurStage st(ws, ne, ni);
  Buf<int> dEI(ws, N);
  int *const dE_p = dEI.p, *const dI_p = dEI.p + ne;
  struct { const double *p; } dA{dA_in}, db{db_in};
  {
    std::vector<int> EI(E);
    EI.insert(EI.end(), I.begin(), I.end());
    HIPCHK(hipMemcpyAsync(dEI.p, EI.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemsetAsync(st.fail_d.p, 0, sizeof(int), s));
  // A must be symmetric: the factorisations read its lower triangle only.  The verdict (and the Schur factorisation's
  // failure flag) is read at the first synchronisation the pivot loop makes anyway, not at one of its own.
  Buf<unsigned long long> sym_d(ws, 2);
  HostWords *host = &pinned_records(ws)->words;
  auto check_symmetry = [&](hipStream_t q) {
    HIPCHK(hipMemsetAsync(sym_d.p, 0, 2 * sizeof(unsigned long long), q));
    hipLaunchKernelGGL(symmetry_kernel, dim3((N + 31) / 32, (N + 31) / 32), dim3(256), 0, q, dA.p, N, sym_d.p);
    HIPCHK(hipMemcpyAsync(host->sym, sym_d.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
  };
  if (!upload_rest) check_symmetry(s);
  st.eliminate(dA.p, db.p, N, dE_p, dI_p, upload_rest ? 1 : 0);
  HIPCHK(hipMemcpyAsync(&host->fail, st.fail_d.p, sizeof(int), hipMemcpyDeviceToHost, s));
  if (upload_rest) {      // the device is busy with the Schur stage: now the rest of A, then the symmetry check, on the side stream
    (*upload_rest)();
    check_symmetry(side);
  }
  bool schur_failed = false;
  const std::function<void()> deferred = [&]() {     // after any synchronisation that follows the copies above
    if (upload_rest) HIPCHK(hipStreamSynchronize(side));
    double amax, asym;
    std::memcpy(&amax, &host->sym[0], sizeof amax);
    std::memcpy(&asym, &host->sym[1], sizeof asym);
    if (asym > 1e-10 * std::max(amax, 1e-300)) throw std::invalid_argument("A must be symmetric (J M^-1 J^T + cfm I is)");
    if (host->fail) schur_failed = true;
    if (dense_trace())
      std::fprintf(stderr, "dense trace schur: ne %d ni %d, symmetry + factor + first check %.3f ms\n", ne, ni,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_dev0).count());
  };
  // (no inequality rows: nothing synchronises before the final read-back, the checks run there)
  // Murty on the inequality part; the reference calls the no-bounds overload (lcp.cc:298)
  std::vector<double> l2(ni), h2(ni);
  for (int k = 0; k < ni; ++k) { l2[k] = use_bounds ? lo[I[k]] : 0.0; h2[k] = use_bounds ? hi[I[k]] : std::numeric_limits<double>::infinity(); }
  int piv = 0;
  bool deferred_ran = false;
  const std::function<void()> once = [&]() { if (!deferred_ran) { deferred_ran = true; deferred(); } };
  bool ok = true;
  if (ni > 0) {
    ok = murty_device(ws, ni, st.lhs.p, st.rhs.p, l2, h2, use_bounds, block_pivoting, max_pivots, max_seconds, st.xi.p, st.wi.p, &piv, msg,
                      st.fail_d.p, &once);
    once();     // (paths of the pivot loop that return without its first synchronisation hook have synchronised all the same)
    if (schur_failed) { if (msg) *msg = "A_ee is not positive definite"; return false; }
  }
  if (pivots) *pivots = piv;
  if (!ok) return false;
  Buf<double> xw(ws, (size_t)2 * N);      // x and w in the caller's order: one copy back
  std::vector<double> xwh((size_t)2 * N);
  HIPCHK(hipMemsetAsync(xw.p, 0, (size_t)2 * N * sizeof(double), s));     // w = 0 on the equality rows, lcp.cc:332-333
  if (ne) {
    st.back_substitute();
    hipLaunchKernelGGL(scatter_kernel, dim3(grid1(ne)), dim3(256), 0, s, ne, dE_p, st.xe.p, xw.p);
  }
  if (ni) {
    hipLaunchKernelGGL(scatter_kernel, dim3(grid1(ni)), dim3(256), 0, s, ni, dI_p, st.xi.p, xw.p);
    hipLaunchKernelGGL(scatter_kernel, dim3(grid1(ni)), dim3(256), 0, s, ni, dI_p, st.wi.p, xw.p + N);
  }
  HIPCHK(hipMemcpyAsync(xwh.data(), xw.p, (size_t)2 * N * sizeof(double), hipMemcpyDeviceToHost, s));
  if (dx_out) HIPCHK(hipMemcpyAsync(dx_out, xw.p, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, s));   // stays on the device too
  HIPCHK(hipStreamSynchronize(s));
  once();
  if (schur_failed) { if (msg) *msg = "A_ee is not positive definite"; return false; }
  if (x) std::memcpy(x, xwh.data(), (size_t)N * sizeof(double));
  if (w) std::memcpy(w, xwh.data() + N, (size_t)N * sizeof(double));
  return true;
}

}  // namespace

bool dense_mixed_constraints(DenseWorkspace &ws, int N, const double *A, const double *b, const uint8_t *C, const double *lo,
                             const double *hi, bool use_bounds, bool block_pivoting, double *x, double *w, int *pivots,
                             std::string *msg, int max_pivots, double max_seconds) {
  if (pivots) *pivots = 0;
  if (N == 0) return true;
  hipStream_t s = ws.stream;
  const bool trace = dense_trace();
  const auto t_a = std::chrono::steady_clock::now();
  Buf<double> dA(ws, (size_t)N * N), db(ws, N);
  const auto t_b = std::chrono::steady_clock::now();
  // (a pageable source: ROCm 7.2 moves these 33.6 MB in 0.6 ms on MI355X's host; a hand-made threaded staging copy took 0.9).
  // From N = 1024 on the lower block trapezoids go first (62 % of the bytes with four blocks of rows, 0.41 ms) -- all the
  // Schur stage reads -- and the rest follows on a second stream while the device factors.
  const int chunk = N >= 1024 ? ((N / 4 + 63) / 64) * 64 : 0;
  hipStream_t side = nullptr;
  // whatever way this call ends, dA goes back to the scratch cache only after the side stream is done with it
  struct SideGuard {
    hipStream_t *q;
    ~SideGuard() { if (*q) (void)hipStreamSynchronize(*q); }
  } side_guard{&side};
  std::function<void()> rest;
  if (chunk) {
    side = ws.side_stream();
    for (int r0 = 0; r0 < N; r0 += chunk) {
      const int r1 = std::min(N, r0 + chunk);
      HIPCHK(hipMemcpy2DAsync(dA.p + (size_t)r0 * N, (size_t)N * sizeof(double), A + (size_t)r0 * N, (size_t)N * sizeof(double),
                              (size_t)r1 * sizeof(double), (size_t)(r1 - r0), hipMemcpyHostToDevice, s));
    }
    hipEvent_t ev = ws.side_event();
    HIPCHK(hipEventRecord(ev, s));
    HIPCHK(hipStreamWaitEvent(side, ev, 0));      // (the symmetry check on the side stream reads the lower part too)
    rest = [&, chunk, side]() {
      for (int r0 = 0; r0 + chunk < N; r0 += chunk) {
        const int r1 = r0 + chunk;
        HIPCHK(hipMemcpy2DAsync(dA.p + (size_t)r0 * N + r1, (size_t)N * sizeof(double), A + (size_t)r0 * N + r1, (size_t)N * sizeof(double),
                                (size_t)(N - r1) * sizeof(double), (size_t)chunk, hipMemcpyHostToDevice, side));
      }
    };
  } else {
    HIPCHK(hipMemcpyAsync(dA.p, A, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice, s));
  }
  if (trace) {
    HIPCHK(hipStreamSynchronize(s));
    const auto t_c = std::chrono::steady_clock::now();
    std::fprintf(stderr, "dense trace N=%d: alloc %.3f ms, upload %.3f ms\n", N, std::chrono::duration<double, std::milli>(t_b - t_a).count(),
                 std::chrono::duration<double, std::milli>(t_c - t_b).count());
  }
  HIPCHK(hipMemcpyAsync(db.p, b, N * sizeof(double), hipMemcpyHostToDevice, s));
  return dense_mixed_impl(ws, N, dA.p, db.p, C, lo, hi, use_bounds, block_pivoting, max_pivots, max_seconds, x, w, nullptr, pivots, msg,
                          chunk ? &rest : nullptr, side);
}

bool dense_mixed_constraints_device(DenseWorkspace &ws, int N, const double *dA_in, const double *db_in, const uint8_t *C,
                                    const double *lo, const double *hi, bool use_bounds, bool block_pivoting, int max_pivots,
                                    double max_seconds, double *x, double *w, double *dx_out, int *pivots, std::string *msg) {
  return dense_mixed_impl(ws, N, dA_in, db_in, C, lo, hi, use_bounds, block_pivoting, max_pivots, max_seconds, x, w, dx_out, pivots, msg,
                          nullptr, nullptr);
}

// ---- lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747) -------------------------------------------------
namespace {
// A(i <-> j) on the lower triangle only (toolkit/lcp.cc:171-195), host side
void swap_rows_and_columns_lower(double *A, int n, int i, int j) {
  if (i == j) return;
  if (i > j) std::swap(i, j);
  for (int c = 0; c < i; ++c) std::swap(A[(size_t)i * n + c], A[(size_t)j * n + c]);
  for (int r = j + 1; r < n; ++r) std::swap(A[(size_t)r * n + i], A[(size_t)r * n + j]);
  for (int k = i + 1; k < j; ++k) std::swap(A[(size_t)k * n + i], A[(size_t)j * n + k]);
  std::swap(A[(size_t)i * n + i], A[(size_t)j * n + j]);
}
__global__ void symmetrize_lower_kernel(double *A, int n) {    // A(r, c) = A(c, r) for c > r
  const size_t total = (size_t)n * n;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(idx / n), c = (int)(idx % n);
    if (c > r) A[idx] = A[(size_t)c * n + r];
  }
}
}  // namespace

bool box_lcp_schur(DenseWorkspace &ws, int n, double *A, const double *b_arg, const double *lo_arg, const double *hi_arg, int algorithm,
                   int nub_arg, bool q6, int max_steps, double max_seconds, double *x, double *w, int32_t *perm_out, int *nub_out,
                   int *pivots, std::string *msg) {
  if (pivots) *pivots = 0;
  if (n <= 0) throw std::invalid_argument("SolveLCP_BoxSchur: n >= 1");
  if (nub_arg > n) throw std::invalid_argument("SolveLCP_BoxSchur: nub <= n");
  hipStream_t s = ws.stream;
  const double big = std::numeric_limits<double>::max();
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> b(b_arg, b_arg + n), lo(lo_arg, lo_arg + n), hi(hi_arg, hi_arg + n);
  std::vector<int> perm(n);
  for (int i = 0; i < n; ++i) perm[i] = i;
  // the partition of toolkit/lcp.cc:652-683: the unbounded indexes first, A's lower triangle swapped along
  int nub = nub_arg;
  std::vector<std::pair<int, int>> swaps;
  if (nub < 0) {
    nub = 0;
    int nb = n - 1;
    while (true) {
      for (; nub <= nb; ++nub) if (q6 ? (lo[nub] > -big || hi[nub] < -big) : (lo[nub] > -big || hi[nub] < big)) break;
      for (; nb >= nub; --nb) if (q6 ? (lo[nb] <= -big && hi[nb] >= -big) : (lo[nb] <= -big && hi[nb] >= big)) break;
      if (nub > nb) break;
      swaps.emplace_back(nub, nb);
      std::swap(perm[nub], perm[nb]); std::swap(b[nub], b[nb]); std::swap(lo[nub], lo[nb]); std::swap(hi[nub], hi[nb]);
    }
  }
  if (nub_out) *nub_out = nub;
  if (perm_out) for (int k = 0; k < n; ++k) perm_out[k] = perm[k];
  const int ne = nub, ni = n - nub;
  // "infinity" is DBL_MAX or the real one (toolkit/lcp.h:149-150): the inner solvers see the real one
  std::vector<double> l2(ni), h2(ni);
  for (int k = 0; k < ni; ++k) { l2[k] = lo[nub + k] <= -big ? -inf : lo[nub + k]; h2[k] = hi[nub + k] >= big ? inf : hi[nub + k]; }

  Buf<double> dA(ws, (size_t)n * n), db(ws, n);
  if (ne == 0) {
    // entirely an LCP (toolkit/lcp.cc:695-700): the inner solver works on A itself and leaves its pivoting order there
    if (n <= kIncrementalMaxRows) {
      int piv = 0;
      const bool good = box_lcp_incremental(s, algorithm, n, A, b.data(), l2.data(), h2.data(), x, w, nullptr, max_steps, max_seconds, &piv, msg);
      if (pivots) *pivots = piv;
      return good;
    }
    // beyond the incremental solver's reach: block principal pivoting on the symmetric matrix (same solution for SPD A;
    // A is left as it was, NOT in the reference's pivoting order)
    HIPCHK(hipMemcpyAsync(dA.p, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(db.p, b.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(symmetrize_lower_kernel, dim3(grid1((size_t)n * n)), dim3(256), 0, s, dA.p, n);
    Buf<double> dx(ws, n), dw(ws, n);
    int piv = 0;
    const bool good = murty_device(ws, n, dA.p, db.p, l2, h2, true, true, max_steps, max_seconds, dx.p, dw.p, &piv, msg);
    if (pivots) *pivots = piv;
    if (!good) return false;
    HIPCHK(hipMemcpyAsync(x, dx.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(w, dw.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return true;
  }
  // Schur stage on the caller's matrix (lower triangle) read through the permutation: E = perm[0, nub), I = the rest
  HIPCHK(hipMemcpyAsync(dA.p, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(db.p, b_arg, n * sizeof(double), hipMemcpyHostToDevice, s));
  SchurStage st(ws, ne, ni);
  Buf<double> dl2(ws, ni), dh2(ws, ni);
  Buf<int> dE(ws, ne), dI(ws, ni);
  HIPCHK(hipMemcpyAsync(dE.p, perm.data(), ne * sizeof(int), hipMemcpyHostToDevice, s));
  if (ni) HIPCHK(hipMemcpyAsync(dI.p, perm.data() + ne, ni * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(st.fail_d.p, 0, sizeof(int), s));
  st.eliminate(dA.p, db.p, n, dE.p, dI.p, 1);            // L L' = Z, Q = L^-1 B', R = C - Q'Q, rhs = d - B Z^-1 c
  // meanwhile the host applies the partition to the caller's lower triangle, as the reference leaves it
  for (const auto &sw : swaps) swap_rows_and_columns_lower(A, n, sw.first, sw.second);
  int fail = 0;
  HIPCHK(hipMemcpyAsync(&fail, st.fail_d.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (fail) { if (msg) *msg = "the unbounded block Z is not positive definite"; return false; }
  if (ni) {
    int piv = 0;
    bool good;
    if (ni <= kIncrementalMaxRows) {
      HIPCHK(hipMemcpyAsync(dl2.p, l2.data(), ni * sizeof(double), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(dh2.p, h2.data(), ni * sizeof(double), hipMemcpyHostToDevice, s));
      good = box_lcp_incremental_device(s, algorithm, ni, st.lhs.p, st.rhs.p, dl2.p, dh2.p, l2.data(), h2.data(), max_steps, max_seconds,
                                        st.xi.p, st.wi.p, &piv, msg);
    } else {
      good = murty_device(ws, ni, st.lhs.p, st.rhs.p, l2, h2, true, true, max_steps, max_seconds, st.xi.p, st.wi.p, &piv, msg);
    }
    if (pivots) *pivots = piv;
    if (!good) return false;
  }
  // y = Z^-1 (c - B' z) = L^-T (L^-1 c - Q z)
  std::vector<double> xih(ni), wih(ni), xeh(ne);
  st.back_substitute();
  HIPCHK(hipMemcpyAsync(xeh.data(), st.xe.p, ne * sizeof(double), hipMemcpyDeviceToHost, s));
  if (ni) {
    HIPCHK(hipMemcpyAsync(xih.data(), st.xi.p, ni * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(wih.data(), st.wi.p, ni * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  for (int k = 0; k < ne; ++k) { x[perm[k]] = xeh[k]; w[perm[k]] = 0.0; }          // Unpermute (:741-744)
  for (int k = 0; k < ni; ++k) { x[perm[ne + k]] = xih[k]; w[perm[ne + k]] = wih[k]; }
  return true;
}

}  // namespace egs
