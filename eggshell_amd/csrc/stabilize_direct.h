// stabilize_direct.h -- the direct route of Ensemble::InitStabilize / PostStabilize (egs_world_stabilize_direct) and the
// one-shot relaxation solve (egs_relax_blocks_direct).  One workgroup per ensemble does a whole pass: assembly, the
// stopping test, A = J J^T, a rank-revealing LDL^T, the solve, the list-order J^T y and the relaxation step.
//
// The reference's CalculateVelocityRelaxation (ensembles.cc:659-666) calls ldlt() on J J^T.  Here the factorisation is
// the same LDL^T with symmetric diagonal pivoting (largest |diagonal|, lowest index on ties) but it STOPS at the first
// pivot <= rank_tol * |first pivot| and takes y = 0 on the rows left: with redundant contact points J J^T is singular,
// and dividing by its rounding-noise pivots destroys the correction, while err is consistent, so every solution of the
// system gives the same J^T y.  Where J J^T is positive definite nothing is truncated.  Where err is NOT consistent
// (the contacts of tilted boxes over-determine the bodies) the rows left carry a residual, and a small positive
// definite solve on the truncated factor (stabilize_direct.hip: direct_factor_solve) turns the leading block's
// solution into the least-squares one: J^T y = J^T (J J^T)^+ err, the correction the sweep route converges to.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace egs {

// Size classes by the ensemble's own row count (3 per constraint): one wavefront with everything in LDS; four
// wavefronts with everything in LDS (145 KB: the packed matrix, the completion's Gram matrix and the Jacobian blocks;
// one workgroup per CU); eight wavefronts with both matrices and the Jacobian blocks in a per-ensemble global workspace
// and the vectors in LDS.
constexpr int kDirectSmallRows = 48;
constexpr int kDirectLdsRows = 126;     // the LDS limit: 42 constraints
constexpr int kDirectMaxRows = 1024;    // above: EGS_ERR_UNSUPPORTED
constexpr int kDirectClasses = 3;
inline int direct_class(int rows) { return rows <= kDirectSmallRows ? 0 : rows <= kDirectLdsRows ? 1 : 2; }
// doubles of global workspace an ensemble of `rows` rows needs (0 in the LDS classes): two packed lower triangles
// (A and the completion's Gram matrix) + J0 | J1
inline size_t direct_ws_size(size_t rows) {
  return rows <= (size_t)kDirectLdsRows ? 0 : rows * (rows + 1) + 12 * rows;
}

struct StabDirectArgs {
  AssembleArgs as{};                             // the world problem's body state and constraint list (outputs unused)
  const double *limit = nullptr;                 // the hinge limits' table [as.m][8] (assemble_device.h: limit_row); NULL: off
  bool slider = false;                           // the list holds an EGS_JOINT_SLIDER_AXIS: its blocks get a pass of their own
  const double *travel = nullptr;                // the sliders' travel stops [as.m][2] (assemble_device.h: slider_stop_row); NULL: off
  double *pos = nullptr, *R = nullptr, *v = nullptr, *w = nullptr;   // the same body state, to be moved
  const int32_t *cons = nullptr, *cstart = nullptr;   // ensemble e's constraints, in its own order: cons[cstart[e] .. cstart[e+1])
  const int32_t *bo = nullptr;                   // body offsets [E + 1]; NULL: one ensemble of as.n bodies
  const int64_t *ws_off = nullptr;               // [E] into ws (global class only)
  double *ws = nullptr;
  int32_t *active = nullptr, *steps = nullptr, *rank = nullptr;   // [E]
  double *err_sq = nullptr;                      // [E]
  int32_t *n_active = nullptr;                   // zeroed by the caller; counts the ensembles left active
  // first = 1: every listed ensemble is evaluated and starts at 0 steps; otherwise only the active ones, whose step
  // count grows by one (the launch before relaxed them).  loop = 1: all passes of the call inside this launch (fixed
  // constraint list), every ensemble ends inactive; loop = 0: one pass, an ensemble that relaxed stays active.
  int32_t first = 0, loop = 0, post = 0, max_steps = 0;
  double threshold = 0.0, rank_tol = 0.0, scale = 0.0, h = 0.0;
};
// the ensembles list[0 .. count) (device), all of size class cls
void launch_stab_direct(const StabDirectArgs &a, const int32_t *list, int count, int cls, hipStream_t s);

// One problem, one workgroup: (J J^T) y = err by the same device functions; y [3m] in row order (0 on the rows the
// truncation left), *rank = pivots taken.  ws: direct_ws_size(3m) doubles.  All device pointers.
struct RelaxDirectArgs {
  int32_t m = 0;
  const int32_t *body0 = nullptr, *body1 = nullptr;
  const double *J0 = nullptr, *J1 = nullptr, *err = nullptr;
  double rank_tol = 0.0;
  double *ws = nullptr, *y = nullptr;
  int32_t *rank = nullptr;
};
void launch_relax_direct(const RelaxDirectArgs &a, hipStream_t s);

}  // namespace egs
