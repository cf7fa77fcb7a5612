// runtime.h -- what every host unit of the C ABI (include/eggshell_amd.h) shares: the context, HIP error handling,
// device and page-locked buffers, the dense solvers' workspace, staged uploads, and the try / catch boundary of an
// entry point.  Internal to the
// library; the plan-inspection entries (plan_debug.cpp) do without it, they make no HIP call.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/eggshell_amd.h"

namespace egs {

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void hip_check(hipError_t e, const char *what) {
  if (e != hipSuccess) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    throw HipError(buf);
  }
}
#define HIPCHK(call) ::egs::hip_check((call), #call)

template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t count = 0, cap = 0;
  // Grow-only: a buffer that is already large enough is kept (a world re-plans
  // on every contact-topology change; hipMalloc/hipFree would dominate that).
  void alloc(size_t n) {
    if (n > cap) {
      const size_t want = p ? n + n / 4 : n;   // head-room only once a buffer has had to grow
      release();
      HIPCHK(hipMalloc(reinterpret_cast<void **>(&p), want * sizeof(T)));
      cap = want;
    }
    count = n;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    count = cap = 0;
  }
  size_t bytes() const { return cap * sizeof(T); }
  ~DevBuf() { release(); }
};

// Sized once, freed at scope exit: the working arrays of one call.  Plain hipMalloc / hipFree on purpose, and it must
// not become stream-ordered or cached: with a stream-ordered pool allocation (hipMallocAsync / hipFreeAsync)
// back-to-back calls that got the same block back saw stale lines of the previous call's matrix on this stack (ROCm
// 7.2; tests/test_gpu_dantzig.py::test_repeated_calls_are_independent).  The Dantzig, batch and fused-Schur paths
// therefore stay on this type and off the block cache of DenseWorkspace.
template <typename T>
struct ScopedDevBuf {
  T *p = nullptr;
  explicit ScopedDevBuf(size_t n) { if (n) HIPCHK(hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T))); }
  ~ScopedDevBuf() { if (p) (void)hipFree(p); }
  ScopedDevBuf(const ScopedDevBuf &) = delete;
  ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
};

// The page-locked counterpart: grow-only, freed with its owner.  The caller sees to it that the stream no longer
// writes to a buffer it regrows.
template <typename T>
struct PinnedBuf {
  T *p = nullptr;
  size_t cap = 0;
  void alloc(size_t n) {
    if (n <= cap) return;
    release();
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&p), n * sizeof(T), hipHostMallocDefault));
    cap = n;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  ~PinnedBuf() { release(); }
};

// What the dense solvers (dense_lcp.hip, dense_factor.hip, dense_murty.hip) keep between calls.  A context owns one:
// everything in it is used only by work enqueued on that context's stream, under that context's device, and all of it
// is created on first use.
struct DensePinned;      // dense_internal.h: the records the device writes for the host (pivot step, deferred checks)
struct DenseWorkspace {
  hipStream_t stream = nullptr;      // the owning context's
  // Device scratch.  A solve takes some twenty-five buffers; hipMalloc + hipFree for each of them (hipFree synchronises
  // the device) cost more than a millisecond per call at N = 2048.  Freed blocks therefore go to a small cache and the
  // next request of at most that size reuses them; the cache holds at most 256 MB (beyond that a released block is
  // really freed).
  struct Block { void *p; size_t bytes; };
  std::vector<Block> free_blocks;
  size_t held = 0;
  void *take(size_t &bytes) {      // in: wanted, out: the block's real size
    int best = -1;
    for (int i = 0; i < (int)free_blocks.size(); ++i)
      if (free_blocks[i].bytes >= bytes && free_blocks[i].bytes <= 2 * bytes + 4096 && (best < 0 || free_blocks[i].bytes < free_blocks[best].bytes)) best = i;
    if (best >= 0) {
      void *p = free_blocks[best].p;
      bytes = free_blocks[best].bytes;
      held -= bytes;
      free_blocks.erase(free_blocks.begin() + best);
      return p;
    }
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {      // no memory while blocks sit idle here: hand them back and try once more
      (void)hipGetLastError();
      drop_blocks();
      HIPCHK(hipMalloc(&p, bytes));
    }
    return p;
  }
  void give(void *p, size_t bytes) {
    if (held + bytes > (size_t(256) << 20)) { (void)hipFree(p); return; }
    free_blocks.push_back({p, bytes});
    held += bytes;
  }
  void drop_blocks() {
    for (auto &b : free_blocks) (void)hipFree(b.p);
    free_blocks.clear();
    held = 0;
  }
  DevBuf<double> factor_work;        // the second array of the fused factorisation, grow-only
  PinnedBuf<DensePinned> pinned;
  // a second stream (and an event) for work that overlaps the main stream's
  hipStream_t side = nullptr;
  hipEvent_t side_done = nullptr;
  hipStream_t side_stream() {
    if (!side) HIPCHK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    return side;
  }
  hipEvent_t side_event() {
    if (!side_done) HIPCHK(hipEventCreateWithFlags(&side_done, hipEventDisableTiming));
    return side_done;
  }
  // the kernels whose dynamic LDS limit has been raised on this context's device
  bool back_solve_lds = false, diag_lds = false, panel_lds = false;
  bool mixed_batch_lds[3] = {false, false, false};      // mixed_batch_kernel, one per size class
  bool mixed_friction_lds[3] = {false, false, false};   // mixed_friction_batch_kernel, likewise
  // with the device set and both streams idle
  void release() {
    drop_blocks();
    factor_work.release();
    pinned.release();
    if (side_done) (void)hipEventDestroy(side_done);
    if (side) (void)hipStreamDestroy(side);
    side_done = nullptr;
    side = nullptr;
  }
  ~DenseWorkspace() { release(); }
};

// Page-locked staging for host->device uploads of plan tables and device->host
// reads of the contact topology: pageable std::vector memory makes every
// hipMemcpyAsync a synchronous bounce through the runtime's own staging buffer.
struct PinnedArena {
  std::vector<std::pair<char *, size_t>> blocks;
  size_t used = 0;   // in blocks.back()
  void *take(size_t bytes) {
    bytes = (bytes + 63) & ~size_t(63);
    if (blocks.empty() || used + bytes > blocks.back().second) {
      const size_t want = std::max(bytes, blocks.empty() ? size_t(1) << 20 : 2 * blocks.back().second);
      char *p = nullptr;
      HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault));
      blocks.emplace_back(p, want);
      used = 0;
    }
    void *r = blocks.back().first + used;
    used += bytes;
    return r;
  }
  // call only when no copy from the arena is in flight: keeps the largest block
  void reset() {
    while (blocks.size() > 1) { (void)hipHostFree(blocks.front().first); blocks.erase(blocks.begin()); }
    used = 0;
  }
  ~PinnedArena() { for (auto &b : blocks) (void)hipHostFree(b.first); }
};

constexpr size_t kEventPairs = 4096;
constexpr uint32_t kSpinLimitDefault = 1u << 22;
// EGS_DEBUG_SPIN_LIMIT=k: bound of the device-side ordering waits (tests force a stall with 1)
inline uint32_t spin_limit() {
  const char *e = std::getenv("EGS_DEBUG_SPIN_LIMIT");
  const long v = e ? std::atol(e) : 0;
  return v > 0 ? (uint32_t)v : kSpinLimitDefault;
}

}  // namespace egs

struct egs_context {
  egs::PinnedArena pinned;
  egs::DenseWorkspace dense;   // (its stream is `stream` below)
  int device = 0;
  int cu_count = 256;   // co-residency caps of the cross-workgroup kernels scale with it
  hipStream_t stream = nullptr;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  std::string error;
  // hipEvent pairs around every solve-kernel launch
  std::vector<hipEvent_t> kev;
  size_t kev_used = 0;
  // egs_solve_blocks is stateless for its caller, but a simulation calls it every step with
  // the same constraint graph: the last problem (schedule + device buffers) is kept and reused
  // when n, m, precision and body0/body1 are unchanged (4.6 -> 0.7 ms per call at C3).
  egs_problem *oneshot = nullptr;
};

namespace egs {

template <typename T>
void upload(DevBuf<T> &d, const T *src, size_t n, hipStream_t s) {
  if (n == 0) return;
  HIPCHK(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));  // src may be a temporary
}

// alloc + copy through the context's pinned arena, without a synchronise; the
// caller synchronises before the arena is reset
template <typename T>
void stage(egs_context *ctx, DevBuf<T> &d, const std::vector<T> &src) {
  d.alloc(src.size());
  if (src.empty()) return;
  const size_t bytes = src.size() * sizeof(T);
  void *h = ctx->pinned.take(bytes);
  std::memcpy(h, src.data(), bytes);
  HIPCHK(hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, ctx->stream));
}

inline egs_status fail(egs_context *ctx, egs_status st, const std::string &msg) {
  if (ctx) ctx->error = msg;
  return st;
}

template <typename F>
egs_status guarded(egs_context *ctx, F &&f) {
  try {
    return f();
  } catch (const HipError &e) {
    return fail(ctx, EGS_ERR_HIP, e.what());
  } catch (const std::invalid_argument &e) {
    return fail(ctx, EGS_ERR_INVALID, e.what());
  } catch (const std::bad_alloc &) {
    return fail(ctx, EGS_ERR_INTERNAL, "host allocation failed");
  } catch (const std::exception &e) {   // std::logic_error from the planner etc.: a library bug, not a HIP failure
    return fail(ctx, EGS_ERR_INTERNAL, e.what());
  }
}

inline void record_kernel_event(egs_context *ctx, bool begin) {
  if (ctx->kev.empty()) return;
  const size_t pair = ctx->kev_used % kEventPairs;
  HIPCHK(hipEventRecord(ctx->kev[2 * pair + (begin ? 0 : 1)], ctx->stream));
  if (!begin) ++ctx->kev_used;
}

}  // namespace egs
