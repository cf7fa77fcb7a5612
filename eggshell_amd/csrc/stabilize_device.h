// stabilize_device.h -- one relaxation step of one body (ensembles.cc:553-561, 653-666), shared by the sweep route's
// stab_relax_kernel (stabilize.hip) and the direct route's fused kernel (stabilize_direct.hip), so both move a body
// with the same operations.
#pragma once
#include "rotation_device.h"

namespace egs {

// v_r = scale * acc (acc = J^T y of the body in list order), p += h v_r[0:3], R = WtoR(v_r[3:6], h) R
// (StepPositions_ExplicitEuler with advance_kernel's rotation); post: v += v_r[0:3], w += v_r[3:6].
__device__ __forceinline__ void stab_relax_body(const double acc[6], double scale, double h, int post, double *pos,
                                                double *R, double *v, double *w) {
  double vr[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) vr[k] = acc[k] * scale;
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[k] = pos[k] + h * vr[k];
  rotate_by_w(vr + 3, h, R);
  if (!post) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = v[k] + vr[k];
    w[k] = w[k] + vr[3 + k];
  }
}

}  // namespace egs
