// rotation_device.h -- R <- WtoR(w, dt) R on the device (utils.cc:82-89: the quaternion of the rotation by |w| dt
// about w, as a matrix), the arithmetic of the CPU oracle's orc_w_to_R and quat_to_R.  Shared by the integrators:
// advance_kernel (StepPositions_ODE, kernels.hip) and stab_relax_body (StepPositions_ExplicitEuler, stabilize_device.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace egs {

__device__ __forceinline__ void rotate_by_w(const double wv[3], double dt, double *R) {
  const double n2 = (wv[0] * wv[0] + wv[1] * wv[1]) + wv[2] * wv[2];
  const double nrm = sqrt(n2);
  double ax[3] = {wv[0], wv[1], wv[2]};
  if (n2 > 0) { ax[0] = wv[0] / nrm; ax[1] = wv[1] / nrm; ax[2] = wv[2] / nrm; }
  const double half = 0.5 * (nrm * dt);
  const double sn = sin(half), cs = cos(half);
  const double qw = cs, qx = sn * ax[0], qy = sn * ax[1], qz = sn * ax[2];
  const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  const double Q[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx,
                       txz - twy, tyz + twx, 1.0 - (txx + tyy)};
  double Ro[9], Rn[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Ro[k] = R[k];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Q[3 * i] * Ro[j] + Q[3 * i + 1] * Ro[3 + j]) + Q[3 * i + 2] * Ro[6 + j];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rn[k];
}

}  // namespace egs
