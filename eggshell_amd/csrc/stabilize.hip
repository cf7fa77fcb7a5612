// stabilize.hip -- Ensemble::InitStabilize / PostStabilize (ensembles.cc:602-666) for every ensemble of a world
// (egs_world_stabilize): the per-ensemble stopping test and the relaxation step.  The relaxation solve and the
// list-order J^T y are the solve kernels' own (world.cpp drives the loop).
#include "stabilize.h"

#include "stabilize_device.h"

namespace egs {

namespace {

constexpr int kErrThreads = 256;

// One workgroup per ensemble.  err_sq = sum of err_i^2 over the ensemble's rows (its joints, then its contacts, as its
// own constraint list holds them): thread t sums rows t, t + 256, ... in order, then a fixed tree over the 256 partial
// sums.  The order depends on the ensemble's own row count only, so a batch of one and a batch of many give the same bits.
__global__ void __launch_bounds__(kErrThreads) stab_err_kernel(StabErrArgs a) {
  __shared__ double red[kErrThreads];
  const int e = blockIdx.x, t = threadIdx.x;
  if (!a.first && !a.active[e]) return;   // frozen: bodies, contacts, steps and err_sq stay as they are
  const int64_t jb = 3 * (int64_t)a.jo[e], jn = 3 * (int64_t)(a.jo[e + 1] - a.jo[e]);
  const int64_t cb = 3 * ((int64_t)a.mj + a.co[e]), cn = 3 * (int64_t)(a.co[e + 1] - a.co[e]);
  double s = 0.0;
  for (int64_t r = t; r < jn + cn; r += kErrThreads) {
    const double x = a.err[r < jn ? jb + r : cb + (r - jn)];
    s += x * x;
  }
  red[t] = s;
  __syncthreads();
  for (int h = kErrThreads / 2; h > 0; h >>= 1) {
    if (t < h) red[t] = red[t] + red[t + h];
    __syncthreads();
  }
  if (t != 0) return;
  const double err_sq = red[0];
  const int32_t steps = a.first ? 0 : a.steps[e] + 1;   // the relaxation step of the pass before has been taken
  a.steps[e] = steps;
  a.err_sq[e] = err_sq;
  const int32_t go = (err_sq > a.threshold && steps < a.max_steps) ? 1 : 0;   // ensembles.cc:610, 632 (NaN stops)
  a.active[e] = go;
  if (go) atomicAdd(a.n_active, 1);
}

// One thread per body of an active ensemble: v_r = -step_scale J^T y (ensembles.cc:659-666), then
// StepPositions_ExplicitEuler (ensembles.cc:553-561) with advance_kernel's rotation (rotate_by_w, as orc_w_to_R),
// and in POST the velocity add (ensembles.cc:653-658).
__global__ void __launch_bounds__(256) stab_relax_kernel(StabRelaxArgs a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.n) return;
  if (!a.active[a.ens ? a.ens[b] : 0]) return;
  double acc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = a.acc[(size_t)b * 6 + k];
  stab_relax_body(acc, a.scale, a.h, a.post, a.pos + (size_t)b * 3, a.R + (size_t)b * 9, a.v + (size_t)b * 3,
                  a.w + (size_t)b * 3);
}

__global__ void __launch_bounds__(256) stab_seed_running_kernel(int n_ens, const int32_t *active, int32_t *running,
                                                               int32_t *n_running) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_ens || active[e] || !running[e]) return;
  running[e] = 0;
  atomicSub(n_running, 1);
}

}  // namespace

void launch_stab_err(const StabErrArgs &a, int n_ens, hipStream_t s) {
  if (n_ens <= 0) return;
  hipLaunchKernelGGL(stab_err_kernel, dim3(n_ens), dim3(kErrThreads), 0, s, a);
}

void launch_stab_relax(const StabRelaxArgs &a, hipStream_t s) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(stab_relax_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

void launch_stab_seed_running(int n_ens, const int32_t *active, int32_t *running, int32_t *n_running, hipStream_t s) {
  if (n_ens <= 0) return;
  hipLaunchKernelGGL(stab_seed_running_kernel, dim3((n_ens + 255) / 256), dim3(256), 0, s, n_ens, active, running, n_running);
}

}  // namespace egs
