// warm_start.hip -- the start of a solve from the previous step's lambda: every new contact looks its nearest old
// contact of the same body pair up (warm_start.h) and takes its rows.  One lane per new contact, no atomics, no
// dependence between lanes; the snapshot that makes the solved list the next step's history; and egs_match_contacts,
// the stand-alone entry over host arrays.
#include "warm_start.h"

#include <vector>

#include "runtime.h"

namespace egs {
namespace {

// (b0, b1) as one ordered key: -1 (the ground) sorts first, as in the collider's list
__device__ __host__ inline uint64_t pair_key(int32_t b0, int32_t b1) {
  return ((uint64_t)(uint32_t)(b0 + 1) << 32) | (uint64_t)(uint32_t)(b1 + 1);
}

// the owner of item i among n_ens ranges off [n_ens + 1]: the last e with off[e] <= i (an empty ensemble shares its
// offset with the next one); one ensemble owns everything
__device__ inline int owner(const int32_t *off, int n_ens, int i) {
  if (n_ens <= 1 || !off) return 0;
  int lo = 0, hi = n_ens;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

template <typename REAL>
__global__ void __launch_bounds__(256) match_contacts_kernel(const MatchArgs<REAL> A) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // the constraint: a joint, or contact c
  if (i >= A.mj + A.m_new) return;
  const int c = i - A.mj;
  const int e = c < 0 ? owner(A.joint_off, A.n_ens, i) : owner(A.new_off, A.n_ens, c);
  REAL out[3] = {REAL(0), REAL(0), REAL(0)};
  int src = -1;
  if (!A.valid[e]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = A.new_rhs[(size_t)i * 3 + r];
    src = -2;
  } else if (c < 0) {   // a joint is permanent: its own previous rows
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = A.old_lambda[(size_t)i * 3 + r];
    src = i;
  } else {
    const uint64_t key = pair_key(A.new_b0[c], A.new_b1[c]);
    const int end = A.old_off ? A.old_off[e + 1] : A.m_old;
    // lower bound of the key in the ensemble's old segment
    int first = A.old_off ? A.old_off[e] : 0, count = end - first;
    while (count > 0) {
      const int step = count >> 1, mid = first + step;
      if (pair_key(A.old_b0[mid], A.old_b1[mid]) < key) { first = mid + 1; count -= step + 1; }
      else count = step;
    }
    const double *pn = A.new_pos + (size_t)c * A.new_stride;
    const double px = pn[0], py = pn[1], pz = pn[2];
    double best = 0.0;
    for (int o = first; o < end && pair_key(A.old_b0[o], A.old_b1[o]) == key; ++o) {
      const double *po = A.old_pos + (size_t)o * A.old_stride;
      const double dx = px - po[0], dy = py - po[1], dz = pz - po[2];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= A.r2 && (src < 0 || d2 < best)) { best = d2; src = o; }   // strict <: a tie keeps the lowest old index
    }
    if (src >= 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) out[r] = A.old_lambda[(size_t)(A.mj + src) * 3 + r];
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) A.x0[(size_t)i * 3 + r] = out[r];
  A.source[i] = src;
  if (A.start) {
    const bool sits_out = A.dt && A.dt[e] == 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) A.start[(size_t)i * 3 + r] = sits_out ? A.new_rhs[(size_t)i * 3 + r] : out[r];
  }
}

// lanes [0, mj + mc): one constraint each; lanes [mj + mc, mj + mc + n_ens): one ensemble's valid flag each
template <typename REAL>
__global__ void __launch_bounds__(256) warm_snapshot_kernel(const SnapshotArgs<REAL> A) {
  const int i = blockIdx.x * 256 + threadIdx.x, m = A.mj + A.mc;
  if (i >= m + A.n_ens) return;
  if (i >= m) {
    const int e = i - m;
    if (!(A.dt && A.dt[e] == 0.0)) A.valid[e] = 1;
    return;
  }
  const int c = i - A.mj;
  const int e = c < 0 ? owner(A.joint_off, A.n_ens, i) : owner(A.contact_off, A.n_ens, c);
  const REAL *from = (A.dt && A.dt[e] == 0.0) ? A.x0 : A.x;
#pragma unroll
  for (int r = 0; r < 3; ++r) A.h_lambda[(size_t)i * 3 + r] = from[(size_t)i * 3 + r];
  if (c >= 0) {
    A.h_b0[c] = A.b0[c];
    A.h_b1[c] = A.b1[c];
#pragma unroll
    for (int k = 0; k < 3; ++k) A.h_pos[(size_t)c * 3 + k] = A.pos[(size_t)c * A.stride + k];
  }
}

// offsets [n_ens + 1] from 0 to m, never falling; b0 / b1 sorted by pair inside every ensemble
bool list_ok(int32_t n_ens, int32_t m, const int32_t *b0, const int32_t *b1, const int32_t *off, bool sorted) {
  if (off[0] != 0 || off[n_ens] != m) return false;
  for (int e = 0; e < n_ens; ++e) {
    if (off[e + 1] < off[e]) return false;
    for (int i = off[e]; i < off[e + 1]; ++i) {
      if (b0[i] < -1 || b1[i] < -1) return false;
      if (sorted && i > off[e] && pair_key(b0[i], b1[i]) < pair_key(b0[i - 1], b1[i - 1])) return false;
    }
  }
  return true;
}

template <typename T>
T *to_device(ScopedDevBuf<T> &d, const T *src, size_t n, hipStream_t s) {
  if (n) HIPCHK(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
  return d.p;
}

}  // namespace

template <typename REAL>
void launch_match_contacts(const MatchArgs<REAL> &a, hipStream_t s) {
  const int lanes = a.mj + a.m_new;
  if (lanes <= 0) return;
  hipLaunchKernelGGL((match_contacts_kernel<REAL>), dim3((lanes + 255) / 256), dim3(256), 0, s, a);
}
template void launch_match_contacts<double>(const MatchArgs<double> &, hipStream_t);
template void launch_match_contacts<float>(const MatchArgs<float> &, hipStream_t);

template <typename REAL>
void launch_warm_snapshot(const SnapshotArgs<REAL> &a, hipStream_t s) {
  const int lanes = a.mj + a.mc + a.n_ens;
  hipLaunchKernelGGL((warm_snapshot_kernel<REAL>), dim3((lanes + 255) / 256), dim3(256), 0, s, a);
}
template void launch_warm_snapshot<double>(const SnapshotArgs<double> &, hipStream_t);
template void launch_warm_snapshot<float>(const SnapshotArgs<float> &, hipStream_t);

}  // namespace egs

using namespace egs;

extern "C" egs_status egs_match_contacts(egs_context *ctx, int32_t n_ens, int32_t m_old, const int32_t *old_b0,
                                         const int32_t *old_b1, const double *old_pos, const double *old_lambda,
                                         const int32_t *old_off, const uint8_t *valid, int32_t m_new, const int32_t *new_b0,
                                         const int32_t *new_b1, const double *new_pos, const double *new_rhs,
                                         const int32_t *new_off, double radius, double *x0, int32_t *source) {
  if (!ctx) return EGS_ERR_INVALID;
  if (n_ens < 1 || m_old < 0 || m_new < 0 || !old_off || !new_off || !valid) return fail(ctx, EGS_ERR_INVALID, "bad sizes / NULL tables");
  if ((m_old > 0 && (!old_b0 || !old_b1 || !old_pos || !old_lambda)) ||
      (m_new > 0 && (!new_b0 || !new_b1 || !new_pos || !new_rhs || !x0 || !source)))
    return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (!(radius >= 0)) return fail(ctx, EGS_ERR_INVALID, "radius must be >= 0");
  if (!list_ok(n_ens, m_old, old_b0, old_b1, old_off, true) || !list_ok(n_ens, m_new, new_b0, new_b1, new_off, false))
    return fail(ctx, EGS_ERR_INVALID, "offsets must run from 0 to m and the old list be ordered by (b0, b1) in every ensemble");
  if (m_new == 0) return EGS_OK;
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t mo = (size_t)m_old, mn = (size_t)m_new, E = (size_t)n_ens;
    ScopedDevBuf<int32_t> d_ob0(mo), d_ob1(mo), d_ooff(E + 1), d_nb0(mn), d_nb1(mn), d_noff(E + 1), d_src(mn);
    ScopedDevBuf<double> d_opos(mo * 3), d_olam(mo * 3), d_npos(mn * 3), d_nrhs(mn * 3), d_x0(mn * 3);
    ScopedDevBuf<uint8_t> d_valid(E);
    MatchArgs<double> a;
    a.n_ens = n_ens; a.m_old = m_old; a.m_new = m_new;
    a.old_b0 = to_device(d_ob0, old_b0, mo, s); a.old_b1 = to_device(d_ob1, old_b1, mo, s);
    a.old_pos = to_device(d_opos, old_pos, mo * 3, s); a.old_lambda = to_device(d_olam, old_lambda, mo * 3, s);
    a.old_off = to_device(d_ooff, old_off, E + 1, s); a.valid = to_device(d_valid, valid, E, s);
    a.new_b0 = to_device(d_nb0, new_b0, mn, s); a.new_b1 = to_device(d_nb1, new_b1, mn, s);
    a.new_pos = to_device(d_npos, new_pos, mn * 3, s); a.new_rhs = to_device(d_nrhs, new_rhs, mn * 3, s);
    a.new_off = to_device(d_noff, new_off, E + 1, s);
    a.r2 = radius * radius;
    a.x0 = d_x0.p; a.source = d_src.p;
    launch_match_contacts(a, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(x0, d_x0.p, mn * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(source, d_src.p, mn * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return EGS_OK;
  });
}
