// stabilize.h -- the device half of egs_world_stabilize (Ensemble::InitStabilize / PostStabilize,
// ensembles.cc:602-666, for every ensemble of a world).  stabilize.hip holds the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace egs {

// The stopping test of one pass, one workgroup per ensemble.  Ensemble e's rows are 3 jo[e] .. 3 jo[e+1] (its joints)
// and 3 (mj + co[e]) .. 3 (mj + co[e+1]) (its contacts) of err.  first = 1: every ensemble is evaluated and starts at
// 0 steps; otherwise only the active ones, whose step count grows by one (the pass before relaxed them).  Each
// evaluated ensemble gets err_sq[e] and active[e] = err_sq > threshold && steps < max_steps; *n_active (zeroed by
// the caller) counts the active ones.
struct StabErrArgs {
  const int32_t *jo = nullptr, *co = nullptr;   // [E + 1]
  int32_t mj = 0;
  const double *err = nullptr;                  // [3m]
  int32_t *active = nullptr, *steps = nullptr;  // [E]
  double *err_sq = nullptr;                     // [E]
  int32_t *n_active = nullptr;
  int32_t first = 0, max_steps = 0;
  double threshold = 0.0;
};
void launch_stab_err(const StabErrArgs &a, int n_ens, hipStream_t s);

// One relaxation step of every body whose ensemble (ens[b], ens = NULL: ensemble 0) is active: v_r = scale * acc[b]
// (acc = J^T y in list order), p += h v_r[0:3], R = WtoR(v_r[3:6], h) R; post = 1 also adds v_r to v and w.
struct StabRelaxArgs {
  int32_t n = 0, post = 0;
  const int32_t *ens = nullptr, *active = nullptr;
  const double *acc = nullptr;                  // [n][6]
  double scale = 0.0, h = 0.0;
  double *pos = nullptr, *R = nullptr, *v = nullptr, *w = nullptr;
};
void launch_stab_relax(const StabRelaxArgs &a, hipStream_t s);

// Seeds a batched tolerance-terminated solve (solve.cpp: do_solve_batch) after its test of x0: an ensemble with
// active[e] == 0 stops running and leaves the count n_running (integer atomics only).  It is no longer tested and no
// state of it is selected; the sweeps still cover it, as they cover every ensemble until the last one stops.
void launch_stab_seed_running(int n_ens, const int32_t *active, int32_t *running, int32_t *n_running, hipStream_t s);

}  // namespace egs
