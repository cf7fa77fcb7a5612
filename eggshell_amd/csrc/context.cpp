// context.cpp -- the context entries of the C ABI: egs_default_params, egs_context_*, egs_last_error, the stream
// timer and the per-launch kernel-time events.  A context owns the stream every other unit enqueues on, and with it
// everything that work on that stream uses between calls: the staging arena, the dense workspace, the one-shot problem.
#include "plan.h"
#include "runtime.h"

using namespace egs;

extern "C" {

void egs_default_params(egs_solve_params *p) {
  if (!p) return;
  p->method = EGS_GAUSS_SEIDEL;
  p->max_iters = 500;   // sparse_iterations.cc:19
  p->check_every = 1;
  p->reserved = 0;
  p->omega = 1.5;       // sparse_iterations.cc:15
  p->cfm = 0.0;
  p->tol = 1e-9;        // constants.h:5
}

egs_status egs_context_create(int device_index, egs_context **out) {
  if (!out) return EGS_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return EGS_ERR_NO_DEVICE;
  if (device_index < 0 || device_index >= count) return EGS_ERR_INVALID;
  egs_context *ctx = new (std::nothrow) egs_context;
  if (!ctx) return EGS_ERR_HIP;
  ctx->device = device_index;
  egs_status st = guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(device_index));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_index));
    if (prop.multiProcessorCount > 0) ctx->cu_count = prop.multiProcessorCount;
    set_patch_workgroups(ctx->cu_count);
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->dense.stream = ctx->stream;
    HIPCHK(hipEventCreate(&ctx->t0));
    HIPCHK(hipEventCreate(&ctx->t1));
    ctx->kev.resize(2 * kEventPairs, nullptr);
    for (auto &e : ctx->kev) HIPCHK(hipEventCreate(&e));
    return EGS_OK;
  });
  if (st != EGS_OK) {
    egs_context_destroy(ctx);
    return st;
  }
  *out = ctx;
  return EGS_OK;
}

void egs_context_destroy(egs_context *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->dense.side) (void)hipStreamSynchronize(ctx->dense.side);
  ctx->dense.release();     // while its streams still exist and are idle
  if (ctx->oneshot) { egs_problem_destroy(ctx->oneshot); ctx->oneshot = nullptr; }
  for (auto e : ctx->kev) if (e) (void)hipEventDestroy(e);
  if (ctx->t0) (void)hipEventDestroy(ctx->t0);
  if (ctx->t1) (void)hipEventDestroy(ctx->t1);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char *egs_last_error(const egs_context *ctx) { return ctx ? ctx->error.c_str() : "no context"; }

egs_status egs_context_synchronize(egs_context *ctx) {
  if (!ctx) return EGS_ERR_INVALID;
  return guarded(ctx, [&]() -> egs_status { HIPCHK(hipStreamSynchronize(ctx->stream)); return EGS_OK; });
}

egs_status egs_context_cu_count(const egs_context *ctx, int32_t *cus) {
  if (!ctx || !cus) return EGS_ERR_INVALID;
  *cus = ctx->cu_count;
  return EGS_OK;
}

egs_status egs_timer_start(egs_context *ctx) {
  if (!ctx) return EGS_ERR_INVALID;
  return guarded(ctx, [&]() -> egs_status { HIPCHK(hipEventRecord(ctx->t0, ctx->stream)); return EGS_OK; });
}

egs_status egs_timer_stop(egs_context *ctx, float *elapsed_ms) {
  if (!ctx || !elapsed_ms) return EGS_ERR_INVALID;
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipEventRecord(ctx->t1, ctx->stream));
    HIPCHK(hipEventSynchronize(ctx->t1));
    HIPCHK(hipEventElapsedTime(elapsed_ms, ctx->t0, ctx->t1));
    return EGS_OK;
  });
}

egs_status egs_kernel_time(egs_context *ctx, double *sum_ms, int64_t *launches, int reset) {
  if (!ctx) return EGS_ERR_INVALID;
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const size_t cnt = std::min(ctx->kev_used, kEventPairs);
    double sum = 0;
    for (size_t i = 0; i < cnt; ++i) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, ctx->kev[2 * i], ctx->kev[2 * i + 1]));
      sum += ms;
    }
    if (sum_ms) *sum_ms = sum;
    if (launches) *launches = (int64_t)cnt;
    if (reset) ctx->kev_used = 0;
    return EGS_OK;
  });
}

}  // extern "C"
