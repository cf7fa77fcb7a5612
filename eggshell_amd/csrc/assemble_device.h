// assemble_device.h -- K1-K4 for one constraint (joints.cc:3-35, contact.cc:14-117, ensembles.cc:569-570): the
// Jacobian blocks, the error, the bounds and the ODE rhs.  Shared by assemble_kernel (kernels.hip) and the fused
// prologue of step_solve_kernel (step_solve.hip: ASSEMBLE), so both write the same bits.  Operation order mirrors
// oracle/model.c.  Anonymous namespace: one private copy per translation unit.
#pragma once
#include "kernels.h"

namespace egs {
namespace {

__device__ __forceinline__ double d3(const double *a, const double *b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
__device__ __forceinline__ void mv3(const double *A, const double *v, double *o) {
  o[0] = (A[0] * v[0] + A[1] * v[1]) + A[2] * v[2];
  o[1] = (A[3] * v[0] + A[4] * v[1]) + A[5] * v[2];
  o[2] = (A[6] * v[0] + A[7] * v[1]) + A[8] * v[2];
}
__device__ __forceinline__ void mm3(const double *A, const double *B, double *O) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      O[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void crossmat(const double *a, double *m) {  // utils.cc:16-24
  m[0] = 0;     m[1] = -a[2]; m[2] = a[1];
  m[3] = a[2];  m[4] = 0;     m[5] = -a[0];
  m[6] = -a[1]; m[7] = a[0];  m[8] = 0;
}
__device__ __forceinline__ void quat_to_R(double w, double x, double y, double z, double *R) {
  double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  double twx = tx * w, twy = ty * w, twz = tz * w;
  double txx = tx * x, txy = ty * x, txz = tz * x;
  double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}
// utils.cc:233-237 (Eigen FromTwoVectors(a, z).toRotationMatrix()); for the
// antiparallel case see DESIGN.md (deterministic axis instead of Eigen's SVD).
__device__ void align_to_z(const double *a, double *Rout) {
  double v0[3];
  const double na = d3(a, a);
  if (na > 0) { const double s = sqrt(na); v0[0] = a[0] / s; v0[1] = a[1] / s; v0[2] = a[2] / s; }
  else { v0[0] = a[0]; v0[1] = a[1]; v0[2] = a[2]; }
  const double v1[3] = {0.0 / 1.0, 0.0 / 1.0, 1.0 / 1.0};
  double c = d3(v1, v0);
  double qw, q[3];
  if (c < -1.0 + 1e-12) {
    if (c < -1.0) c = -1.0;
    const double ax = fabs(v0[0]), ay = fabs(v0[1]), az = fabs(v0[2]);
    double e[3] = {0, 0, 0};
    if (ax <= ay && ax <= az) e[0] = 1; else if (ay <= az) e[1] = 1; else e[2] = 1;
    double axis[3] = {v0[1] * e[2] - v0[2] * e[1], v0[2] * e[0] - v0[0] * e[2], v0[0] * e[1] - v0[1] * e[0]};
    const double n = sqrt(d3(axis, axis));
    axis[0] /= n; axis[1] /= n; axis[2] /= n;
    const double w2 = (1.0 + c) * 0.5;
    qw = sqrt(w2);
    const double sv = sqrt(1.0 - w2);
    q[0] = axis[0] * sv; q[1] = axis[1] * sv; q[2] = axis[2] * sv;
  } else {
    const double axis[3] = {v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]};
    const double s = sqrt((1.0 + c) * 2.0);
    const double invs = 1.0 / s;
    q[0] = axis[0] * invs; q[1] = axis[1] * invs; q[2] = axis[2] * invs;
    qw = s * 0.5;
  }
  quat_to_R(qw, q[0], q[1], q[2], Rout);
}

__device__ __forceinline__ double dot6p(const double *a, const double *b) {
  return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}

// The angular blocks (EGS_JOINT_LOCK, EGS_JOINT_HINGE_AXIS; eggshell_amd.h has the derivation and DESIGN.md section
// 4k the limits).  The linear columns stay exactly zero on both sides; err is (body0 quantity) - (body1 quantity) and
// d err/dt = J0 s0 + J1 s1 at err = 0, as for the ball joint.  fp64, no contraction, no trigonometric function; the
// operation order below is the one tests/joint_reference.py restates.
//
// LOCK, data = (qw, qx, qy, qz, 0, 0, 0), the unit quaternion of Rref = R0(0)^T R1(0) (R0(0)^T for a world side):
//   Rq = quat_to_R(q);  T = mm3(R0, Rq);  E = mm3(T, R1^T) with R1^T formed by index (a world side: E = T)
//   err = (0.5*(E[7]-E[5]), 0.5*(E[2]-E[6]), 0.5*(E[3]-E[1]))      the axial vector of E, sin(theta) n
//   J0 = [0 | I3], J1 = [0 | -1.0*I3] (zero for a world side); three equality rows, lo = hi = 0
__device__ __forceinline__ void lock_block(const AssembleArgs &A, int b0, int b1, const double *d, double *j0, double *j1,
                                           double *e) {
  double R0[9], Rq[9], T[9], E[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) R0[k] = A.R[(size_t)b0 * 9 + k];
  quat_to_R(d[0], d[1], d[2], d[3], Rq);
  mm3(R0, Rq, T);
#pragma unroll
  for (int r = 0; r < 3; ++r) j0[6 * r + 3 + r] = 1.0;
  if (b1 >= 0) {
    double R1t[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R1t[3 * r + c] = A.R[(size_t)b1 * 9 + 3 * c + r];
    mm3(T, R1t, E);
#pragma unroll
    for (int r = 0; r < 3; ++r) j1[6 * r + 3 + r] = -1.0 * 1.0;
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = T[k];
  }
  e[0] = 0.5 * (E[7] - E[5]);
  e[1] = 0.5 * (E[2] - E[6]);
  e[2] = 0.5 * (E[3] - E[1]);
}
// HINGE_AXIS, data = (a0[3], a1[3], 0): a0 the unit axis in body0's frame, a1 in body1's (the world axis for a world side):
//   s = mv3(R0, a0);  t = mv3(R1, a1) (a world side: a1);  Rn = align_to_z(s), rows (p, q, s^)
//   c = t x s = (t1 s2 - t2 s1, t2 s0 - t0 s2, t0 s1 - t1 s0);  err = (d3(p, c), d3(q, c), 0)
//   J0 = [0 | Rn], J1 = [0 | -1.0*Rn] (zero for a world side)
// Rows 0 and 1 are equality rows; row 2, the axis row, is an inequality row with lo = hi = 0 (the multiplier pinned
// at 0: the hinge turns freely) unless a motor opens its bounds (motor_row below) or a stop is active (limit_row).  t = -s is a false equilibrium
// (c = 0 there too): the linearisation holds for axes less than a right angle apart.
__device__ __forceinline__ void hinge_block(const AssembleArgs &A, int b0, int b1, const double *d, double *j0, double *j1,
                                            double *e) {
  double R0[9], s[3], t[3], Rn[9], c[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R0[k] = A.R[(size_t)b0 * 9 + k];
  mv3(R0, d, s);
  if (b1 >= 0) {
    double R1[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R1[k] = A.R[(size_t)b1 * 9 + k];
    mv3(R1, d + 3, t);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = d[3 + k];
  }
  align_to_z(s, Rn);
  c[0] = t[1] * s[2] - t[2] * s[1];
  c[1] = t[2] * s[0] - t[0] * s[2];
  c[2] = t[0] * s[1] - t[1] * s[0];
  e[0] = d3(Rn, c);
  e[1] = d3(Rn + 3, c);
  e[2] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      j0[6 * r + 3 + k] = Rn[3 * r + k];
      if (b1 >= 0) j1[6 * r + 3 + k] = -1.0 * Rn[3 * r + k];
    }
}

// SLIDER_AXIS (EGS_JOINT_SLIDER_AXIS = 5; a slider is LOCK + SLIDER_AXIS as a hinge is BALL + HINGE_AXIS), data =
// (a0[3], c[3], 0): a0 the unit rail direction in body0's frame; with body1 a body c is a point of the rail in body0's
// frame and the rail's target point is body1's centre, P1 = pos[b1]; with a world side c is the world point the rail
// passes through, P1 = c, and the rail passes through body0's centre.
//   s = mv3(R0, a0);  Rn = align_to_z(s), rows (p, q, s^)
//   two bodies:  ro = mv3(R0, c);  D[k] = (p0[k] + ro[k]) - P1[k]
//   world side:                    D[k] =  p0[k] - c[k]
//   rel[k] = p0[k] - P1[k];  rw = mm3(Rn, crossmat(rel))         row r is (P1 - p0) x Rn_r: the lever arm is body0's alone
//   J0 = [Rn | rw], J1 = [-1.0*Rn | 0] (all zero for a world side);  err = (d3(p, D), d3(q, D), 0)
// Rows 0 and 1 are equality rows; row 2, the rail row, is an inequality row with lo = hi = 0 (the multiplier pinned at
// 0: the slider runs freely) unless a motor opens its bounds (motor_row) or a travel stop is active (slider_stop_row).
// The travel is x = d3(s^, D): d x/dt = row 2 of J0 s0 + J1 s1 at every pose (s is rigid in body0, body1 enters
// through its centre only); rows 0 and 1 are exact at err = 0, as the ball's and the hinge's.
// slider_frame: Rn and D, the part slider_stop_row shares with the block, operation for operation.
__device__ __forceinline__ void slider_frame(const AssembleArgs &A, int b0, int b1, const double *d, double *Rn, double *D,
                                             double *rel) {
  double R0[9], s[3], p0[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R0[k] = A.R[(size_t)b0 * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p0[k] = A.pos[(size_t)b0 * 3 + k];
  mv3(R0, d, s);
  align_to_z(s, Rn);
  if (b1 >= 0) {
    double ro[3];
    mv3(R0, d + 3, ro);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double P1 = A.pos[(size_t)b1 * 3 + k];
      D[k] = (p0[k] + ro[k]) - P1;
      rel[k] = p0[k] - P1;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      D[k] = p0[k] - d[3 + k];
      rel[k] = p0[k] - d[3 + k];
    }
  }
}
__device__ __forceinline__ void slider_block(const AssembleArgs &A, int b0, int b1, const double *d, double *j0, double *j1,
                                             double *e) {
  double Rn[9], D[3], rel[3], cm[9], rw[9];
  slider_frame(A, b0, b1, d, Rn, D, rel);
  crossmat(rel, cm);
  mm3(Rn, cm, rw);
  e[0] = d3(Rn, D);
  e[1] = d3(Rn + 3, D);
  e[2] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      j0[6 * r + k] = Rn[3 * r + k];
      j0[6 * r + 3 + k] = rw[3 * r + k];
      if (b1 >= 0) j1[6 * r + k] = -1.0 * Rn[3 * r + k];
    }
}

// A contact's blocks (contact.cc:14-117, FrictionModel::BOX) as functions of values: no loads.  d = the descriptor
// (point[3], normal[3], depth).  contact_frame: Rn from the normal.  contact_side: side SIDE's block j (all 18 entries)
// from Rn, the point and the body's position.  contact_err: e = err.  contact_blocks: the three together, j0 / j1 zero
// for a side without a body (pos0 / pos1 not read there).  assemble_one_t's contact branch calls the parts where it had
// their code, each side's behind that side's load of pos; the staged prologue of step_solve_face_kernel
// (step_face.hip), which has the values in registers, calls contact_blocks: the same operations in the same order,
// the same bits.
__device__ __forceinline__ void contact_frame(const double *d, double *Rn) { align_to_z(d + 3, Rn); }
template <int SIDE>
__device__ __forceinline__ void contact_side(const double *d, const double *Rn, const double *pos, double *j) {
  double rel[3], cm[9], rw[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) rel[k] = d[k] - pos[k];
  crossmat(rel, cm);
  if (SIDE == 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) cm[k] = -1.0 * cm[k];
  }
  mm3(Rn, cm, rw);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) { j[6 * r + c] = SIDE == 1 ? Rn[3 * r + c] : -Rn[3 * r + c]; j[6 * r + 3 + c] = rw[3 * r + c]; }
}
__device__ __forceinline__ void contact_err(const double *d, double *e) { e[0] = 0.0; e[1] = 0.0; e[2] = -d[6]; }
__device__ __forceinline__ void contact_blocks(const double *d, const double *pos0, const double *pos1, bool has0, bool has1,
                                               double *j0, double *j1, double *e) {
  double Rn[9];
  contact_frame(d, Rn);
#pragma unroll
  for (int k = 0; k < 18; ++k) { j0[k] = 0.0; j1[k] = 0.0; }
  if (has0) contact_side<0>(d, Rn, pos0, j0);
  if (has1) contact_side<1>(d, Rn, pos1, j1);
  contact_err(d, e);
}
// One side's u = v/dt + W f (ensembles.cc:569-570) from values: vw = (v, w) of the body, wf = its M^-1 f_ext.  The
// expression of assemble_one_t's last lines, which keep it in place between their loads (v, the quotient, W f, the
// sum): with W f loaded ahead of the division assemble_kernel<double> takes 132 VGPRs instead of 128 and loses a
// wavefront per SIMD.  tests/test_gpu_step_face_prologue.py holds the two to the same bits.
__device__ __forceinline__ void side_u(const double *vw, const double *wf, double dt, double *u) {
#pragma unroll
  for (int r = 0; r < 6; ++r) u[r] = vw[r] / dt + wf[r];
}

// Constraint i: j0 / j1 (3x6 row-major, zero for a world side), e = err, lo / hi, eq per row (every row of a ball joint
// and of a lock is an equality row, no row of a contact is, a hinge's axis row and a slider's rail row are not) and per side u = v/dt + W f
// (zero for a world side), what the rhs needs.
// EACH: dt is the constraint's own time step, dt_each (constraint_rates); otherwise the launch's A.dt, read where the
// scalar form has always read it.  ANGULAR = false leaves the angular blocks out: the fused prologue of
// step_solve_kernel, which choose_sweep offers lists of contacts only, keeps the code it had.  SLIDER = true adds the
// slider block (kind 5): the forms launched only for a list that holds one, so that every other list runs the code it ran.
template <bool EACH, bool ANGULAR = true, bool SLIDER = false>
__device__ __forceinline__ void assemble_one_t(const AssembleArgs &A, int i, double dt_each, double *j0, double *j1, double *e,
                                               double *lo, double *hi, bool *eq, double *u0, double *u1) {
  const int b0 = A.body0[i], b1 = A.body1[i];
  double d[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) d[k] = A.data[(size_t)i * 7 + k];
#pragma unroll
  for (int k = 0; k < 18; ++k) { j0[k] = 0.0; j1[k] = 0.0; }
  const int kind = A.kind[i];
  if (ANGULAR && kind >= 2) {
    if (kind == 2) lock_block(A, b0, b1, d, j0, j1, e);
    else if (SLIDER && kind == 5) slider_block(A, b0, b1, d, j0, j1, e);
    else hinge_block(A, b0, b1, d, j0, j1, e);
    eq[0] = true; eq[1] = true; eq[2] = kind == 2;
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = 0.0; hi[k] = 0.0; }
  } else if (kind == 0) {  // joints.cc:3-35
    double R0[9], rc0[3], cm[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R0[k] = A.R[(size_t)b0 * 9 + k];
    mv3(R0, d, rc0);
    crossmat(rc0, cm);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      j0[6 * r + r] = 1.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) j0[6 * r + 3 + c] = -1.0 * cm[3 * r + c];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = A.pos[(size_t)b0 * 3 + k] + rc0[k];
    if (b1 >= 0) {
      double R1[9], rc1[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) R1[k] = A.R[(size_t)b1 * 9 + k];
      mv3(R1, d + 3, rc1);
      crossmat(rc1, cm);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        j1[6 * r + r] = -1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) j1[6 * r + 3 + c] = cm[3 * r + c];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) e[k] = (e[k] - A.pos[(size_t)b1 * 3 + k]) - rc1[k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) e[k] = e[k] - d[3 + k];
    }
    eq[0] = true; eq[1] = true; eq[2] = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = 0.0; hi[k] = 0.0; }
  } else {  // contact.cc:14-117, FrictionModel::BOX
    double Rn[9];
    contact_frame(d, Rn);
    if (b0 >= 0) {
      double p[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = A.pos[(size_t)b0 * 3 + k];
      contact_side<0>(d, Rn, p, j0);
    }
    if (b1 >= 0) {
      double p[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = A.pos[(size_t)b1 * 3 + k];
      contact_side<1>(d, Rn, p, j1);
    }
    contact_err(d, e);
    eq[0] = false; eq[1] = false; eq[2] = false;
    lo[0] = -1.0; lo[1] = -1.0; lo[2] = 0.0;
    hi[0] = 1.0; hi[1] = 1.0; hi[2] = INFINITY;
  }
  // rhs = -(erp/dt^2) err - J (v/dt + W f)      ensembles.cc:569-570
#pragma unroll
  for (int r = 0; r < 6; ++r) { u0[r] = 0.0; u1[r] = 0.0; }
  if (b0 >= 0) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double vel = r < 3 ? A.v[(size_t)b0 * 3 + r] : A.w[(size_t)b0 * 3 + r - 3];
      u0[r] = vel / (EACH ? dt_each : A.dt) + A.Wf[(size_t)b0 * 6 + r];
    }
  }
  if (b1 >= 0) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double vel = r < 3 ? A.v[(size_t)b1 * 3 + r] : A.w[(size_t)b1 * 3 + r - 3];
      u1[r] = vel / (EACH ? dt_each : A.dt) + A.Wf[(size_t)b1 * 6 + r];
    }
  }
}
template <bool ANGULAR = true>
__device__ __forceinline__ void assemble_one(const AssembleArgs &A, int i, double *j0, double *j1, double *e, double *lo,
                                             double *hi, bool *eq, double *u0, double *u1) {
  assemble_one_t<false, ANGULAR>(A, i, 0.0, j0, j1, e, lo, hi, eq, u0, u1);
}
// row r of rhs = -(erp/dt^2) err - J (v/dt + W f)      ensembles.cc:569-570
template <bool EACH>
__device__ __forceinline__ double assemble_rhs_t(const AssembleArgs &A, double dt_each, double erp_each, const double *j0,
                                                 const double *j1, const double *e, const double *u0, const double *u1, int r) {
  const double kk = EACH ? -erp_each / dt_each / dt_each : -A.erp / A.dt / A.dt;
  const double ju = dot6p(j0 + 6 * r, u0) + dot6p(j1 + 6 * r, u1);
  return kk * e[r] - ju;
}
// Restitution (egs_problem_set_restitution): the normal row's target t = kk err[2] of contact i, raised to -rest vn / dt
// where the contact approaches faster than vth.  vn: the separating speed of row 2 from the bodies' (v, w), zeros for
// a world side.  Whatever is not a contact (the joints never bounce), a coefficient < 0 and a contact that does not
// trigger return t itself: the stored bits.
template <bool EACH>
__device__ __forceinline__ double restitution_target(const AssembleArgs &A, int i, double dt_each, const double *j0,
                                                     const double *j1, double t) {
  if (A.kind[i] != 1) return t;
  const double rest = A.rest[i];
  if (!(rest >= 0)) return t;
  const int b0 = A.body0[i], b1 = A.body1[i];
  double s0[6], s1[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    s0[r] = b0 >= 0 ? (r < 3 ? A.v[(size_t)b0 * 3 + r] : A.w[(size_t)b0 * 3 + r - 3]) : 0.0;
    s1[r] = b1 >= 0 ? (r < 3 ? A.v[(size_t)b1 * 3 + r] : A.w[(size_t)b1 * 3 + r - 3]) : 0.0;
  }
  const double vn = dot6p(j0 + 12, s0) + dot6p(j1 + 12, s1);
  if (vn < -A.vth) {
    const double b = (-(rest * vn)) / (EACH ? dt_each : A.dt);
    if (b > t) t = b;
  }
  return t;
}
// row 2 of constraint i with restitution (A.rest is set): assemble_rhs_t's, its target raised where the contact bounces
template <bool EACH>
__device__ __forceinline__ double assemble_rhs_bounce_t(const AssembleArgs &A, int i, double dt_each, double erp_each,
                                                        const double *j0, const double *j1, const double *e, const double *u0,
                                                        const double *u1) {
  const double kk = EACH ? -erp_each / dt_each / dt_each : -A.erp / A.dt / A.dt;
  const double ju = dot6p(j0 + 12, u0) + dot6p(j1 + 12, u1);
  return restitution_target<EACH>(A, i, dt_each, j0, j1, kk * e[2]) - ju;
}
// The motor table (egs_problem_set_motors), motor [m][2] = (speed, tau), not NULL: a HINGE_AXIS constraint i with
// tau >= 0 (+inf allowed) gets lo[2] = -tau, hi[2] = +tau and the target t = speed / dt in place of kk err[2] (which
// is 0 for it): rhs2 = t - ju, so that the solve asks for s^ . (w0' - w1') = speed within the torque limit.  Returns
// whether it applied; tau < 0 and every other kind are left as assembled.  A hinge whose stop is active this step
// (limit_row below) is not handed to it: motor and limit share the axis row, and the row is the limit's then.
// SLIDER: a SLIDER_AXIS constraint's rail row likewise, (speed, f) with f the force limit and speed = dx/dt, body0's
// travel relative to body1 along s^; a slider whose travel stop is active (slider_stop_row) is not handed to it.
template <bool EACH, bool SLIDER = false>
__device__ __forceinline__ bool motor_row(const AssembleArgs &A, const double *motor, int i, double dt_each, const double *j0,
                                          const double *j1, const double *u0, const double *u1, double *lo, double *hi,
                                          double &rhs2) {
  if (SLIDER ? (A.kind[i] != 3 && A.kind[i] != 5) : A.kind[i] != 3) return false;
  const double speed = motor[(size_t)i * 2], tau = motor[(size_t)i * 2 + 1];
  if (!(tau >= 0)) return false;
  lo[2] = -tau;
  hi[2] = tau;
  const double t = speed / (EACH ? dt_each : A.dt);
  const double ju = dot6p(j0 + 12, u0) + dot6p(j1 + 12, u1);
  rhs2 = t - ju;
  return true;
}
// The limit table (egs_problem_set_hinge_limits), lim [m][8] = (qw, qx, qy, qz, sin lo, cos lo, sin hi, cos hi), not
// NULL: a HINGE_AXIS constraint i with a stop (a (sin, cos) pair that is not (0, 0)) has its angle read as the lock
// reads its error -- q is the unit quaternion of Rref = R0(0)^T R1(0), which fixes theta = 0 -- and, past a stop, its
// axis row made the one-sided row of that stop.  After the block (s, Rn, err[0..1], J keep their bits):
//   Rq = quat_to_R(q);  T = mm3(R0, Rq);  E = mm3(T, R1^T) with R1^T formed by index (a world side: E = T)
//   ax = (0.5*(E[7]-E[5]), 0.5*(E[2]-E[6]), 0.5*(E[3]-E[1]));  sn = d3(s, ax), s = mv3(R0, a0);  cs = 0.5*(((E[0]+E[4])+E[8]) - 1.0)
//   upper set and sn*(1.0+chi) > shi*(1.0+cs):       err[2] = sn*chi - cs*shi, lo[2] = -inf, hi[2] = 0
//   else lower set and sn*(1.0+clo) < slo*(1.0+cs):  err[2] = sn*clo - cs*slo, lo[2] = 0, hi[2] = +inf
// The comparisons are tan(theta/2) against tan(limit/2), cross-multiplied; err[2] = sin(theta - limit).  The rhs row is
// the ordinary kk err[2] - ju.  err2 / lo2 / hi2: row 2 of err, lo and hi, written only then.  Returns whether a stop is active; then motor_row leaves the row alone for this step.
// Every other kind, a row without a stop and a hinge inside its range are left as assembled.
__device__ __forceinline__ bool limit_row(const AssembleArgs &A, const double *lim, int i, double &err2, double &lo2, double &hi2) {
  if (A.kind[i] != 3) return false;
  const double *L = lim + (size_t)i * 8;
  const double slo = L[4], clo = L[5], shi = L[6], chi = L[7];
  const bool lower = slo != 0.0 || clo != 0.0, upper = shi != 0.0 || chi != 0.0;
  if (!lower && !upper) return false;
  const int b0 = A.body0[i], b1 = A.body1[i];
  double R0[9], a0[3], s[3], Rq[9], T[9], E[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) R0[k] = A.R[(size_t)b0 * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) a0[k] = A.data[(size_t)i * 7 + k];
  mv3(R0, a0, s);
  quat_to_R(L[0], L[1], L[2], L[3], Rq);
  mm3(R0, Rq, T);
  if (b1 >= 0) {
    double R1t[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R1t[3 * r + c] = A.R[(size_t)b1 * 9 + 3 * c + r];
    mm3(T, R1t, E);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = T[k];
  }
  const double ax[3] = {0.5 * (E[7] - E[5]), 0.5 * (E[2] - E[6]), 0.5 * (E[3] - E[1])};
  const double sn = d3(s, ax);
  const double cs = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0);
  if (upper && sn * (1.0 + chi) > shi * (1.0 + cs)) {
    err2 = sn * chi - cs * shi;
    lo2 = -INFINITY;
    hi2 = 0.0;
    return true;
  }
  if (lower && sn * (1.0 + clo) < slo * (1.0 + cs)) {
    err2 = sn * clo - cs * slo;
    lo2 = 0.0;
    hi2 = INFINITY;
    return true;
  }
  return false;
}
// The travel table (egs_problem_set_slider_limits), lim [m][2] = (xlo, xhi), -inf / +inf: no stop on that side, not
// NULL: a SLIDER_AXIS constraint i has its travel x = d3(s^, D) read with the block's own operations (slider_frame) and,
// past a stop, its rail row made the one-sided row of that stop:
//   xhi finite and x > xhi:       err[2] = x - xhi, lo[2] = -inf, hi[2] = 0
//   else xlo finite and x < xlo:  err[2] = x - xlo, lo[2] = 0,    hi[2] = +inf
// The rhs row is the ordinary kk err[2] - ju.  err2 / lo2 / hi2 are written only then.  Returns whether a stop is
// active; then motor_row leaves the row alone for this step.  Every other kind is left as assembled.
__device__ __forceinline__ bool slider_stop_row(const AssembleArgs &A, const double *lim, int i, double &err2, double &lo2,
                                                double &hi2) {
  if (A.kind[i] != 5) return false;
  const double xlo = lim[(size_t)i * 2], xhi = lim[(size_t)i * 2 + 1];
  const bool lower = xlo > -INFINITY, upper = xhi < INFINITY;
  if (!lower && !upper) return false;
  double d[6], Rn[9], D[3], rel[3];
#pragma unroll
  for (int k = 0; k < 6; ++k) d[k] = A.data[(size_t)i * 7 + k];
  slider_frame(A, A.body0[i], A.body1[i], d, Rn, D, rel);
  const double x = d3(Rn + 6, D);
  if (upper && x > xhi) {
    err2 = x - xhi;
    lo2 = -INFINITY;
    hi2 = 0.0;
    return true;
  }
  if (lower && x < xlo) {
    err2 = x - xlo;
    lo2 = 0.0;
    hi2 = INFINITY;
    return true;
  }
  return false;
}
__device__ __forceinline__ double assemble_rhs(const AssembleArgs &A, const double *j0, const double *j1, const double *e,
                                               const double *u0, const double *u1, int r) {
  return assemble_rhs_t<false>(A, 0.0, 0.0, j0, j1, e, u0, u1, r);
}
// the per-ensemble form's dt and erp of constraint i: its ensemble's (the ensemble of its first body)
template <typename RATES>   // (instantiated for EnsembleRates only: the scalar form never calls it)
__device__ __forceinline__ void constraint_rates(const AssembleArgs &A, const RATES &T, int i, double &dt, double &erp) {
  const int b0 = A.body0[i];
  const int en = T.body_ens[b0 >= 0 ? b0 : A.body1[i]];
  dt = T.dt[en];
  erp = T.erp[en];
}

}  // namespace
}  // namespace egs
