// dense_internal.h -- for dense_factor.hip (the blocked Cholesky and the solves with its factor), dense_murty.hip (the
// pivot loop) and dense_lcp.hip (the two reference solvers built on them) only.  The units meet in the host calls
// declared here; every kernel is private to its unit.
#pragma once
#include "dense_lcp.h"
#include "runtime.h"

#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace egs {

constexpr int NB = 64;    // block size = wavefront size

// A block of the workspace's cache (DenseWorkspace::take, runtime.h), rounded up to 256 bytes.
template <typename T>
struct Buf {
  DenseWorkspace &ws;
  T *p = nullptr;
  size_t bytes = 0;
  Buf(DenseWorkspace &w, size_t n) : ws(w) {
    if (n) { bytes = ((n * sizeof(T) + 255) / 256) * 256; p = static_cast<T *>(ws.take(bytes)); }
  }
  // a block goes back to the cache while kernels that use it may still be queued: the next taker enqueues on the same
  // context's stream, so the stream's order keeps them apart
  ~Buf() { if (p) ws.give(p, bytes); }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
};

inline int grid1(size_t n, int block = 256) {
  size_t g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// EGS_DENSE_TRACE: timings of the stages and one line per pivot on stderr.  Read on every call, not cached.
inline bool dense_trace() { return std::getenv("EGS_DENSE_TRACE") != nullptr; }

// ---- dense_factor.hip ---------------------------------------------------------------------------------------
// Blocked Cholesky of the first nf (multiple of 64) columns of the lower trapezoid T (nrows x ld); inv receives the
// nf / 64 inverted diagonal blocks.  ibase >= 0: rows [ibase, ibase + nf) hold an identity block and leave as L^-T.
void factor(DenseWorkspace &ws, double *T, int ld, int nrows, int nf, int *fail, double *inv, int ibase = -1);
// L^T x = y, y = row yrow of T; x to out[map ? map[i] : i], i < nreal.  xs: [nf] scratch.
void launch_back_solve(DenseWorkspace &ws, const double *T, int ld, int nf, int yrow, int nreal, const int *map, double *out, double *xs, const double *inv);
// The trapezoid of one pivot: A(S,S) padded to nspad, nspad identity rows if identity_rows, beff(S) as the last row.
void launch_build_pivot(DenseWorkspace &ws, const double *lhs, int n, const int *S, int ns, int nspad, const double *beff, double *T, bool identity_rows, int *pos0, int *idx0);
// x = L^-T z from the identity rows factor() turned into L^-T; keep (may be NULL) masks the rows written.
void launch_inverse_rows_solve(DenseWorkspace &ws, const double *T, int ld, int nf, int ibase, const double *z, int nreal, const int *map, double *out, const uint8_t *keep);

// ---- dense_murty.hip ----------------------------------------------------------------------------------------
struct MurtyStep {        // one per pivot, read by the host after the synchronisation
  int first_offender;     // lowest index that must flip, or INT_MAX
  int out_of_bounds;      // any x < lo or x > hi            (lcp.cc:66)
  int w_bad;              // any w < 0 at x == lo or w > 0 at x == hi  (lcp.cc:72-76)
  int fail;               // a factorisation met a non-positive pivot
  double resid2;          // || A x - (b + w) ||^2           (lcp.cc:81-83)
  double goodness;        // sum of the non-positive x and w (lcp.cc:107-113)
  int ns;                 // |S| after the flips: the size of the next pivot's system
  int ninf;               // number of infeasible indexes before the flips
  int flipped;
  int nd, nr;             // |S \ S0| and |S0 \ S| against the factored base set S0 (-1: not tracked)
  int seq;                // the launch's sequence number, stored last (system scope): the host polls it instead of
                          // waiting for the stream (a completion signal costs ~15 us of host latency per pivot)
};

// The workspace's page-locked records: murty_advance_kernel writes `step` and the host reads it after the sync;
// `words` is the landing area of the deferred checks (a line of its own: the host polls step.seq while copies land here).
struct HostWords { unsigned long long sym[2]; int fail; int pad; };
struct DensePinned { alignas(64) MurtyStep step; alignas(64) HostWords words; };

inline DensePinned *pinned_records(DenseWorkspace &ws) {
  if (!ws.pinned.p) {
    ws.pinned.alloc(1);
    std::memset(ws.pinned.p, 0, sizeof(DensePinned));
  }
  return ws.pinned.p;
}

// Murty's principal pivoting on (A n x n, b), both on the device; x and w to dx, dw.  See dense_murty.hip.
bool murty_device(DenseWorkspace &ws, int n, const double *dA, const double *db, const std::vector<double> &lo, const std::vector<double> &hi,
                  bool box_fix, bool block, int max_pivots, double max_seconds, double *dx, double *dw, int *pivots_out, std::string *msg,
                  const int *extra_fail = nullptr, const std::function<void()> *after_first_sync = nullptr);

}  // namespace egs
