// dense_world.h -- Ensemble::ComputeVDot on the reference's live dense path (ensembles.cc:498-538) for every
// ensemble of a world at once (egs_world_step_dense).  dense_world.hip holds the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace egs {

// Ensembles of at most this many rows (3 per constraint) are solved by the fused kernel, one workgroup each;
// larger ones go through the multi-launch path (dense_mixed_constraints_device, dense_lcp.hip).  Size classes: <= 32 and <= 64 rows run on
// one wavefront, <= 112 on four.
constexpr int kDenseClassRows[3] = {32, 64, 112};
constexpr int kFusedDenseMax = 112;

// What one ensemble's solve leaves (one read-back of these per step).
struct DenseEnsStatus {
  double condition;   // estimate of cond_2(J M^-1 J^T); +inf when it is not positive definite
  double cfm;         // what was added to the diagonal: 0 or cfm_coeff (ensembles.cc:513-521)
  int32_t ok;         // 1: Lcp::MixedConstraintsSolver reached a solution
  int32_t pivots;     // principal pivots of the Murty loop
};

// What the pyramid form's fixed-point iteration leaves per ensemble (egs_world_dense_friction_info).
struct DenseFrictionStatus {
  double change;      // the last delta
  int32_t outer;      // solves made
  int32_t converged;  // change <= tol
};

// Per-ensemble workspace of an ensemble of N rows, in doubles from its offset:
//   A [N][N] | Z [N][N] + N (A^-1, then L^-1 [A_ei | b_e]) | lhs [N][N] | b, lo, hi, C (0 / 1), x [N] each.
inline size_t dense_ws_size(size_t N) { return 3 * N * N + 6 * N; }
__host__ __device__ inline size_t dense_ws_vec(size_t N) { return 3 * N * N + N; }   // b; lo, hi, C, x follow at +N each

struct DenseWorldArgs {
  const int32_t *cons;      // constraint indexes of the world, grouped by ensemble, each group in its Ensemble's order
  const int32_t *cstart;    // [E + 1]: ensemble e's constraints are cons[cstart[e] .. cstart[e + 1])
  const int64_t *ws_off;    // [E]: offset of ensemble e's workspace in ws (doubles)
  const int32_t *body0, *body1;
  const double *J0, *J1, *Minv;                 // the world problem's assembled blocks
  const double *rhs, *lo, *hi;                  // its rows
  const uint8_t *is_eq;
  double *ws;
  double *x;                                    // the world's lambda, written in world order
  DenseEnsStatus *status;                       // [E]
  double cfm_coeff;
  int32_t use_bounds;
};

// The pyramid form's own arguments (egs_world_set_dense_friction): the world problem's per-constraint coefficients as
// world_fill_friction leaves them (fp64; < 0: the constraint's rows stay as stored).
struct DenseWorldFriction {
  const double *mu;
  DenseFrictionStatus *status;                  // [E]
  double tol;
  int32_t max_outer, pad;
};

// A_e = J M^-1 J^T of every ensemble (the operation order of dense_system_kernel, without the cfm) and its rows
// gathered into the ensemble's workspace.  Grid: a workgroup row per ensemble, max_m^2 constraint pairs wide.
void launch_dense_world_system(const DenseWorldArgs &a, int n_ens, int max_m, hipStream_t s);
// The fused ComputeVDot of the `count` ensembles list[0 .. count) of size class cls (kDenseClassRows[cls]).
void launch_dense_world_fused(const DenseWorldArgs &a, const int32_t *list, int count, int cls, hipStream_t s);
// The same with the Coulomb pyramid solved by the stage's fixed-point iteration (mixed_solve_device.h); use_bounds is 1.
void launch_dense_world_friction(const DenseWorldArgs &a, const DenseWorldFriction &fa, const int32_t *list, int count, int cls,
                                 hipStream_t s);
// A[i][i] += cfm, i < N
void launch_dense_world_add_diag(double *A, int N, double cfm, hipStream_t s);
// x[3 cons_e[i] + r] = xs[3 i + r]
void launch_dense_world_scatter(const int32_t *cons_e, int N, const double *xs, double *x, hipStream_t s);

}  // namespace egs
