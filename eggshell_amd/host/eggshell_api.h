// eggshell_api.h -- host-side C++ adapter: the reference's Body / Constraint /
// Joint / Contact / Ensemble API for the constraint-solve path, unchanged in
// names, argument meaning and result types, with the arithmetic behind
//   sparse::{Jacobi,GaussSeidel,SOR}Iteration   (sparse_iterations.h:26-34)
//   Lcp::MixedConstraintsSolver                 (lcp.h:21-23)
//   Ensemble::Step / StepVelocities_ODE         (ensembles.cc:390-427, 563-575)
// routed to the MI355X library through the C ABI (include/eggshell_amd.h).
// What is mirrored here and from where:
//   Body                body.h:13-96 (state p,v,m,R,w,I; side 0.3)
//   Constraint          constraints.h:14-48
//   Joint, BallAndSocketJoint   joints.h:12-50, joints.cc:3-35
//   ContactGeometry     collision.h:12-27
//   Contact             contact.h:11-56, contact.cc:14-117 (FrictionModel::BOX)
//   Ensemble, Chain     ensembles.h:25-186, ensembles.cc:24-87,156-171,202-239,
//                       429-443, 563-591, 668-707
// Error convention differs on purpose: the reference Panics (_exit(1)); these
// functions throw egs::Error carrying the C ABI status and message.
#ifndef EGGSHELL_API_H
#define EGGSHELL_API_H

#include <array>
#include <cmath>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/eggshell_amd.h"
#include "eigen_lite.h"

namespace egs {
struct Error : std::runtime_error {
  int status;
  Error(int st, const std::string &msg) : std::runtime_error(msg), status(st) {}
};
// Process-wide context on device 0 (created on first use).
egs_context *DefaultContext();
}  // namespace egs

// utils.h
Matrix3d CrossMat(const Vector3d &a);                      // utils.cc:16-24
Matrix3d AlignVectors(const Vector3d &a, const Vector3d &b);  // utils.cc:233-237
Matrix3d WtoR(const Vector3d &w, double dt);               // utils.cc:82-89 (as a matrix)

class Body {  // body.h:13-96
 public:
  Body() : m_(1.0), R_(Matrix3d::Identity()) { I_ = CalculateInertia(m_); }
  Body(const Vector3d &p, const Vector3d &v, const Matrix3d &R, const Vector3d &w)
      : p_(p), v_(v), m_(1.0), R_(R), w_(w) { I_ = CalculateInertia(m_); }
  Body(const Vector3d &p, const Vector3d &v, double m, const Matrix3d &R, const Vector3d &w, const Matrix3d &I)
      : p_(p), v_(v), m_(m), R_(R), w_(w), I_(I) {}
  const Vector3d &p() const { return p_; }
  const Vector3d &v() const { return v_; }
  double m() const { return m_; }
  const Matrix3d &R() const { return R_; }
  const Vector3d &w_g() const { return w_; }
  const Matrix3d &I_b() const { return I_; }
  Matrix3d I_g() const { return R_ * I_ * R_.transpose(); }
  void SetP(const Vector3d &p) { p_ = p; }
  void SetV(const Vector3d &v) { v_ = v; }
  void SetR(const Matrix3d &R) { R_ = R; }
  void SetW_GlobalFrame(const Vector3d &w) { w_ = w; }
  // body.h:60: `enum struct BodyType { Box = 0 }` with the TODO "move this to a subclass when there are different
  // types of Bodies".  Sphere is not in the reference: a ball of the given radius and mass, I = (2/5) m r^2 * 1,
  // collided as a sphere on the device (EGS_SHAPE_SPHERE; its side lengths are the diameter three times).
  // Capsule is not in the reference either: radius, tip-to-tip length > 2 radius, its axis the body's z axis (column 2
  // of R), collided as a capsule on the device (EGS_SHAPE_CAPSULE; side lengths (2 radius, 2 radius, length)).  It has
  // a uniform solid capsule's inertia: a cylinder of height H = length - 2 radius and two hemispheres, the mass split
  // by volume into m_c and m_s,  I_zz = m_c r^2 / 2 + (2/5) m_s r^2,
  // I_xx = I_yy = m_c (H^2 / 12 + r^2 / 4) + m_s (2 r^2 / 5 + H^2 / 4 + 3 H r / 8).
  // That is not a multiple of the identity: under the default frozen inertia (quirk Q5: M^-1 and the external force
  // are taken at Init() and kept) a tumbling capsule keeps the world-frame inertia it had at Init().
  // Ensemble::SetLiveInertia(true) is the remedy: M^-1 and the gyroscopic torque then follow the body.
  enum struct BodyType { Box = 0, Sphere, Capsule };
  static Body Sphere(const Vector3d &p, const Vector3d &v, double radius, double m = 1.0) {
    Body b(p, v, m, Matrix3d::Identity(), Vector3d::Zero(), Matrix3d::Identity() * (0.4 * m * radius * radius));
    b.type_ = BodyType::Sphere;
    b.radius_ = radius;
    return b;
  }
  static Body Capsule(const Vector3d &p, const Vector3d &v, double radius, double length, double m = 1.0);
  BodyType type() const { return type_; }
  double radius() const { return radius_; }   // 0 for a box
  double length() const { return length_; }   // tip to tip; 0 unless a capsule
  Vector3d GetSideLengths() const {           // body.h:91 for a box
    if (type_ == BodyType::Capsule) return Vector3d(2 * radius_, 2 * radius_, length_);
    return type_ == BodyType::Sphere ? Vector3d(2 * radius_, 2 * radius_, 2 * radius_) : Vector3d(0.3, 0.3, 0.3);
  }

 private:
  Vector3d p_, v_;
  double m_;
  Matrix3d R_;
  Vector3d w_;
  Matrix3d I_;
  BodyType type_ = BodyType::Box;
  double radius_ = 0.0, length_ = 0.0;
  Matrix3d CalculateInertia(double m) const;  // body.cc:19-36
};

class Constraint {  // constraints.h:14-48
 public:
  Constraint(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1)
      : i0_(i0), i1_(i1), b0_(std::move(b0)), b1_(std::move(b1)) {}
  virtual ~Constraint() = default;
  virtual VectorXd ComputeError() const = 0;
  virtual void ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *constraint_type, VectorXd *constraint_lo,
                        VectorXd *constraint_hi) const = 0;
  // Device-assembly descriptor (egs_constraint_kind + 7 doubles); returns false
  // for constraint types the library cannot assemble itself (then the solver
  // falls back to flattening ComputeJ on the host, entry 1).
  virtual bool Describe(int32_t *kind, double data[7]) const { (void)kind; (void)data; return false; }
  // Get the global frame constraint position (constraints.h:38-39).
  virtual Vector3d GetConstraintPosition() const = 0;
  // Not in the reference: false for a constraint that acts on orientations only (AngularLockJoint, HingeAxisJoint).
  // It has no position, so the closeness scans (CheckAndCorrectEnsembleState, the contact pruning) pass it over.
  virtual bool HasPosition() const { return true; }
  int i0_ = -1;
  int i1_ = -1;

 protected:
  const std::shared_ptr<Body> b0_;
  const std::shared_ptr<Body> b1_;
};

class Joint : public Constraint {  // joints.h:12-28
 public:
  Joint(std::shared_ptr<Body> b0, int i0, const Vector3d &c0, const Vector3d &c1)
      : Constraint(std::move(b0), i0, nullptr, -1), c0_(c0), c1_(c1) {}
  Joint(std::shared_ptr<Body> b0, int i0, const Vector3d &c0, std::shared_ptr<Body> b1, int i1, const Vector3d &c1)
      : Constraint(std::move(b0), i0, std::move(b1), i1), c0_(c0), c1_(c1) {}

 protected:
  Vector3d c0_, c1_;
};

class BallAndSocketJoint : public Joint {  // joints.h:31-50
 public:
  using Joint::Joint;
  VectorXd ComputeError() const override;                                   // joints.cc:3-11
  void ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *constraint_type, VectorXd *constraint_lo,
                VectorXd *constraint_hi) const override;                    // joints.cc:13-35
  bool Describe(int32_t *kind, double data[7]) const override;
  Vector3d GetConstraintPosition() const override;                          // joints.cc:57-75
};

// Not in the reference, whose joints.h announces a "library of all joint types" and holds the ball joint alone: the
// two angular blocks of the library (EGS_JOINT_LOCK, EGS_JOINT_HINGE_AXIS; include/eggshell_amd.h has the formulas).
// Beside a BallAndSocketJoint on the same two bodies they make a weld and a hinge (Ensemble::AddWeld / AddHinge).
// b1 = nullptr, i1 = -1: to the world.  ComputeError / ComputeJ follow the device's operation order.
class AngularLockJoint : public Joint {
 public:
  // holds the relative orientation the two bodies have now
  AngularLockJoint(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1);
  VectorXd ComputeError() const override;                                   // the axial vector of R0 Rq R1^T: sin(theta) n
  void ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *constraint_type, VectorXd *constraint_lo,
                VectorXd *constraint_hi) const override;                    // [0 | I], [0 | -I]; three equality rows
  bool Describe(int32_t *kind, double data[7]) const override;
  Vector3d GetConstraintPosition() const override { return Vector3d::Zero(); }
  bool HasPosition() const override { return false; }

 private:
  double q_[4];   // (w, x, y, z) of R0(0)^T R1(0)
};

class HingeAxisJoint : public Joint {
 public:
  // axis_world: the hinge axis at the bodies' current pose (any length > 0)
  HingeAxisJoint(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &axis_world);
  VectorXd ComputeError() const override;                                   // (p . c, q . c, 0), c = t x s
  void ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *constraint_type, VectorXd *constraint_lo,
                VectorXd *constraint_hi) const override;                    // [0 | Rn], [0 | -Rn]; the axis row an inequality row
  bool Describe(int32_t *kind, double data[7]) const override;
  Vector3d GetConstraintPosition() const override { return Vector3d::Zero(); }
  bool HasPosition() const override { return false; }
  // the motor (egs_problem_set_motors): the solve asks for axis . (w0' - w1') = speed within +-max_torque (+inf
  // allowed); max_torque < 0: no motor, the hinge turns freely
  void SetMotor(double speed, double max_torque) { speed_ = speed; tau_ = max_torque; }
  double motor_speed() const { return speed_; }
  double motor_torque() const { return tau_; }
  // The angle limits (egs_problem_set_hinge_limits), in radians: theta, body0's turn relative to body1 about the axis
  // since the joint was built, is kept within [lo, hi]; -INFINITY / +INFINITY: no stop on that side.  Past a stop the
  // axis row is that stop's one-sided row for the step and the motor leaves it alone.  lo <= hi, a finite limit inside
  // (-pi, pi): Ensemble::SetHingeLimits checks them.
  void SetLimits(double lo, double hi) { limit_lo_ = lo; limit_hi_ = hi; }
  double limit_lo() const { return limit_lo_; }
  double limit_hi() const { return limit_hi_; }
  bool has_limits() const { return std::isfinite(limit_lo_) || std::isfinite(limit_hi_); }
  // the row of the limit table: (qw, qx, qy, qz, sin lo, cos lo, sin hi, cos hi), a missing stop as (0, 0)
  void LimitRow(double row[8]) const;
  // theta now, by atan2 on the host from the sine and cosine the device forms: for read-out only
  double Angle() const;

 private:
  // (sin theta, cos theta) in the device's operation order (assemble_device.h: limit_row)
  void SinCos(double *sn, double *cs) const;
  // +1: past the upper stop, -1: past the lower, 0: neither, by the device's half-angle comparison; *err2 = sin(theta - limit)
  int ActiveStop(double *err2) const;
  Vector3d a0_, a1_;   // the unit axis in body0's frame and in body1's (the world's for a world side)
  double q_[4];        // (w, x, y, z) of R0(0)^T R1(0): theta = 0
  double speed_ = 0.0, tau_ = -1.0;
  double limit_lo_ = -INFINITY, limit_hi_ = INFINITY;
};

// The slider block of the library (EGS_JOINT_SLIDER_AXIS; include/eggshell_amd.h has the formulas).  Beside an
// AngularLockJoint on the same two bodies it makes a slider, a general prismatic joint (Ensemble::AddSlider).  The rail
// is rigid in body0; with a body on side 1 it is held to body1's centre, to the world it passes through body0's
// centre and the world point c.  ComputeError / ComputeJ follow the device's operation order.
class SliderAxisJoint : public Joint {
 public:
  // axis_world: the rail direction at the bodies' current pose (any length > 0); the travel x is 0 now
  SliderAxisJoint(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &axis_world);
  VectorXd ComputeError() const override;                                   // (p . D, q . D, 0 or x - stop)
  void ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *constraint_type, VectorXd *constraint_lo,
                VectorXd *constraint_hi) const override;                    // [Rn | rw], [-Rn | 0]; the rail row an inequality row
  bool Describe(int32_t *kind, double data[7]) const override;
  Vector3d GetConstraintPosition() const override { return Vector3d::Zero(); }
  bool HasPosition() const override { return false; }                       // pruning stays with the ball joints
  // the motor (egs_problem_set_motors): the solve asks for dx/dt = speed within +-max_force (+inf allowed);
  // max_force < 0: no motor, the slider runs freely
  void SetMotor(double speed, double max_force) { speed_ = speed; force_ = max_force; }
  double motor_speed() const { return speed_; }
  double motor_force() const { return force_; }
  // The travel stops (egs_problem_set_slider_limits): x is kept within [lo, hi]; -INFINITY / +INFINITY: no stop on that
  // side.  Past a stop the rail row is that stop's one-sided row for the step and the motor leaves it alone.
  void SetLimits(double lo, double hi) { limit_lo_ = lo; limit_hi_ = hi; }
  double limit_lo() const { return limit_lo_; }
  double limit_hi() const { return limit_hi_; }
  bool has_limits() const { return std::isfinite(limit_lo_) || std::isfinite(limit_hi_); }
  // x now: body0's travel relative to body1 along the rail, 0 where the joint was built (the device's operations)
  double Position() const;

 private:
  // Rn (rows p, q, s^), D and rel = p0 - P1 in the device's operation order (assemble_device.h: slider_frame)
  void Frame(Matrix3d *Rn, Vector3d *D, Vector3d *rel) const;
  // +1: past the upper stop, -1: past the lower, 0: neither; *err2 = x - stop
  int ActiveStop(double *err2) const;
  Vector3d a0_, c_;   // the unit rail direction in body0's frame; the rail's point (body0's frame; the world's for a world side)
  double speed_ = 0.0, force_ = -1.0;
  double limit_lo_ = -INFINITY, limit_hi_ = INFINITY;
};

struct ContactGeometry {  // collision.h:12-27
  Vector3d position, normal;
  double depth = 0;
  ContactGeometry() {}
  ContactGeometry(const Vector3d &p, const Vector3d &n, double d) : position(p), normal(n), depth(d) {}
};

class Contact : public Constraint {  // contact.h:11-56
 public:
  // contact.h:21-25.  The reference implements BOX alone (tangential rows bounded by the constant 1, contact.cc:103-113)
  // and leaves the other three with empty bodies; COULOMB_PYRAMID is built here (Ensemble::SetFriction), NO_FRICTION
  // and INFINITE are not.
  enum struct FrictionModel { NO_FRICTION, INFINITE, BOX, COULOMB_PYRAMID };
  Contact(std::shared_ptr<Body> b, int index, const ContactGeometry &cg)
      : Constraint(nullptr, -1, std::move(b), index), cg_(cg) {}
  Contact(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const ContactGeometry &cg)
      : Constraint(std::move(b0), i0, std::move(b1), i1), cg_(cg) {}
  VectorXd ComputeError() const override;                                   // contact.cc:14-22
  void ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *C, VectorXd *x_lo, VectorXd *x_hi) const override;  // :38-117
  bool Describe(int32_t *kind, double data[7]) const override;
  Vector3d GetConstraintPosition() const override { return cg_.position; }  // contact.cc:166-168

 private:
  const ContactGeometry cg_;
};

typedef std::vector<std::shared_ptr<Body>> ComponentsList;     // ensembles.h:19-22
typedef std::vector<std::shared_ptr<Joint>> JointsList;
typedef std::vector<std::shared_ptr<Contact>> ContactsList;
typedef std::vector<std::shared_ptr<Constraint>> ConstraintsList;

namespace sparse {  // sparse_iterations.h:13-34
// on an explicit matrix (sparse_iterations.h:13-24, sparse_iterations.cc:72-144): the 2-argument forms treat every
// row as an equality, the 5-argument forms project the rows with C = false onto [x_lo, x_hi]
VectorXd JacobiIteration(const MatrixXd &A, const VectorXd &b);
VectorXd JacobiIteration(const MatrixXd &A, const VectorXd &b, const ArrayXb &C, const VectorXd &x_lo, const VectorXd &x_hi);
VectorXd GaussSeidelIteration(const MatrixXd &A, const VectorXd &b);
VectorXd GaussSeidelIteration(const MatrixXd &A, const VectorXd &b, const ArrayXb &C, const VectorXd &x_lo, const VectorXd &x_hi);
VectorXd SORIteration(const MatrixXd &A, const VectorXd &b);
VectorXd SORIteration(const MatrixXd &A, const VectorXd &b, const ArrayXb &C, const VectorXd &x_lo, const VectorXd &x_hi);
// The same on many independent systems in one library call (egs_dense_iterate_batch: one upload, a workgroup per
// system, one read-back), named like lcp::SolveLCPBatch: x[k] is, bit for bit, what the call above returns for A[k],
// b[k] (and C[k], x_lo[k], x_hi[k]).  Sizes may differ from system to system (0..1024 rows); GetLastSolve() reports the
// last system's count and residual.
std::vector<VectorXd> JacobiIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b);
std::vector<VectorXd> JacobiIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b, const std::vector<ArrayXb> &C,
                                           const std::vector<VectorXd> &x_lo, const std::vector<VectorXd> &x_hi);
std::vector<VectorXd> GaussSeidelIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b);
std::vector<VectorXd> GaussSeidelIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b, const std::vector<ArrayXb> &C,
                                                const std::vector<VectorXd> &x_lo, const std::vector<VectorXd> &x_hi);
std::vector<VectorXd> SORIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b);
std::vector<VectorXd> SORIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b, const std::vector<ArrayXb> &C,
                                        const std::vector<VectorXd> &x_lo, const std::vector<VectorXd> &x_hi);
// matrix-free, on an ensemble's constraints (sparse_iterations.h:26-34)
VectorXd JacobiIteration(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &rhs,
                         double cfm = 0.0);
VectorXd GaussSeidelIteration(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &rhs,
                              double cfm = 0.0);
VectorXd SORIteration(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &rhs,
                      double cfm = 0.0);
// sparse_iterations_utils.cc:697-720
void ConstructMixedConstraints(const ConstraintsList &constraints, ArrayXb *C, VectorXd *x_lo, VectorXd *x_hi);
// The matrix-free products (sparse_iterations_utils.h:60-109, sparse_iterations_utils.cc:427-695):
// strict lower / strict upper / diagonal parts of (J M^-1 J^T) x and the full product with
// epsilon on the diagonal.  Same names, arguments and defaults; O(m) on the GPU
// (egs_matvec_blocks) instead of the reference's O(m^2) pair loops.
VectorXd CalculateSparseDx(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &x,
                           double epsilon = 0.0, double scale = 1.0);
VectorXd CalculateSparseLx(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &x,
                           double epsilon_diagonal = 0.0, double scale_diagonal = 1.0);
VectorXd CalculateSparseUx(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &x,
                           double epsilon_diagonal = 0.0, double scale_diagonal = 1.0);
VectorXd CalculateSparseLxUx(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &x,
                             double epsilon_diagonal = 0.0, double scale_diagonal = 1.0);
VectorXd CalculateSparseLxDx(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &x,
                             double epsilon_diagonal = 0.0, double scale_diagonal = 1.0);
VectorXd CalculateSparseUxDx(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &x,
                             double epsilon_diagonal = 0.0, double scale_diagonal = 1.0);
VectorXd CalculateSparseJMJtX(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &x,
                              double epsilon_diagonal = 0.0);
// Iteration count and residual of the most recent *Iteration call (the
// reference prints the count to stdout, sparse_iterations.cc:223-224).
struct LastSolve { int iterations; double residual; int n_islands, n_tiles, n_global; };
LastSolve GetLastSolve();
}  // namespace sparse

namespace Lcp {  // lcp.h:21-23
bool MixedConstraintsSolver(const MatrixXd &A, const VectorXd &b, const ArrayXb &C, const VectorXd &x_lo,
                            const VectorXd &x_hi, VectorXd &x, VectorXd &w);
// The same on many independent problems in one library call (egs_mixed_constraints_solve_batch: problems of up to 112
// rows fused, one upload, a workgroup per problem, one read-back; larger ones one after another inside the call), named
// like lcp::SolveLCPBatch and sparse::*IterationBatch: what the reference's own test of the function does one problem
// after another (lcp.cc:412-528).  Returns MixedConstraintsSolver's bool per problem; (*x)[k] and (*w)[k] are its x and w
// for A[k], b[k], C[k] (the bounds are ignored as there, quirk Q3).  Sizes may differ from problem to problem (0 rows
// included).  A mismatched argument throws egs::Error(EGS_ERR_INVALID).
std::vector<bool> MixedConstraintsSolverBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b,
                                              const std::vector<ArrayXb> &C, const std::vector<VectorXd> &x_lo,
                                              const std::vector<VectorXd> &x_hi, std::vector<VectorXd> *x, std::vector<VectorXd> *w);
}

// toolkit/lcp.h:104-174 -- the "adjacent" solver family the north star names
// (lcp::SolveLCP; not linked into eggshell).  Box LCP
// A x = b + w with lo <= 0 <= hi.  What is kept of the contract:
//   * the dispatch of toolkit/lcp.cc:752-785, including its two refusals (Schur complement
//     or Cottle-Dantzig without box_lcp: the reference Panics, here egs::Error / EGS_ERR_INVALID);
//   * only the LOWER TRIANGLE of A is ever read or written (toolkit/lcp.h:73; the reference's tests hand
//     over lower triangles, toolkit/lcp.cc:808, 880-881, 913, 957, 1109-1110);
//   * schur_complement (the default): SolveLCP_BoxSchur (toolkit/lcp.cc:627-747) on the device
//     (egs_box_lcp_schur): unbounded rows (lo = -inf or -DBL_MAX and hi = +inf or DBL_MAX) come first by
//     its two-pointer partition, Z = L L', R = C - B Z^-1 B', the box LCP on R by SolveLCP_BoxMurty /
//     SolveLCP_BoxDantzig (Settings::algorithm), back-substitution; A IS PERMUTED IN PLACE as the reference
//     leaves it (the partition; plus the inner solver's pivoting order when no row is unbounded, :695-700);
//     quirk Q6 (toolkit/lcp.cc:664, 669 test `hi < -DBL_MAX`, so a row with lo = -inf and a
//     FINITE hi is classed unbounded) is reproduced when reference_quirks is set;
//   * max_iterations and max_time: the solve gives up and returns false (toolkit/lcp.h:161-167); the device
//     loops also carry a cap of their own (20 n + 1000 steps) where the reference would loop for ever;
//   * box_lcp = false: lo = 0, hi = +inf whatever the vectors hold (toolkit/lcp.h:152-154).
//   * schur_complement = false (toolkit/lcp.cc:768-781): algorithm = COTTLE_DANTZIG runs SolveLCP_BoxDantzig
//     and algorithm = MURTY runs SolveLCP_BoxMurty / SolveLCP_Murty on a LinearReducer themselves on the
//     device (egs_box_lcp_batch: the incremental Cholesky factor of AddCholeskyRow / SwapCholeskyRows,
//     toolkit/lcp.cc:91-157), and A's lower triangle is permuted in place by their pivoting order, as in
//     the reference.
// What differs, by design: a bounded part beyond 1024 rows goes through block principal
// pivoting with a single-index safeguard (fresh blocked factorisations on the matrix cores; same unique
// solution), so there A is left in BoxSchur's order or untouched instead of carrying the pivoting order of
// the inner solver.
namespace lcp {
enum Algorithm { MURTY, COTTLE_DANTZIG };
struct Settings {
  Algorithm algorithm = MURTY;
  bool box_lcp = true;
  bool schur_complement = true;
  int max_iterations = __INT_MAX__;
  double max_time = __DBL_MAX__;
  bool reference_quirks = false;   // not in the reference: reproduce Q6 (see above)
};
int LastSolvePivots();             // principal pivots of the most recent SolveLCP
bool SolveLCP(const Settings &settings, MatrixXd &A, const VectorXd &b, const VectorXd &lo, const VectorXd &hi,
              VectorXd *x, VectorXd *w);
// SolveLCP on many independent problems in one library call, with the same dispatch and refusals applied to the
// whole batch: default settings -> egs_box_lcp_schur_batch (problems of up to 96 rows fused into one launch, a
// workgroup per problem; larger ones one after another inside the call), schur_complement = false ->
// egs_box_lcp_batch.  Each (*A)[k] is left as SolveLCP leaves it; returns SolveLCP's bool per problem.
std::vector<bool> SolveLCPBatch(const Settings &settings, std::vector<MatrixXd> *A, const std::vector<VectorXd> &b,
                                const std::vector<VectorXd> &lo, const std::vector<VectorXd> &hi, std::vector<VectorXd> *x,
                                std::vector<VectorXd> *w);
}  // namespace lcp

// Not in the reference: ray casts against the ground and the bodies (egs_cast_rays; the rules are stated above it in
// eggshell_amd.h).  dir is not normalised: t is in its units.  body >= 0 attaches the ray to that component of its
// ensemble: origin and dir are then in the component's frame and the component itself is not tested.
struct Ray {
  Vector3d origin, dir;
  double tmax = std::numeric_limits<double>::infinity();
  int body = -1;
};
// body: -2 no hit, -1 the ground, else the component's index in its ensemble.  t = tmax on a miss; normal = 0 on a miss
// and where the origin is inside the solid (t = 0).  point = the world-frame origin + t x the world-frame dir, the
// origin itself on a miss.
struct RayHit {
  int body;
  double t;
  Vector3d normal, point;
};

class Ensemble {  // ensembles.h:25-186
 public:
  virtual ~Ensemble();
  virtual void Init();                                                   // ensembles.cc:24-29
  enum struct Integrator { EXPLICIT_EULER = 0, OPEN_DYNAMICS_ENGINE, IMPLICIT_MIDPOINT };
  // Step with the switch the reference left open (kSparseImplementation,
  // ensembles.cc:17-21) turned on: contacts as given (UpdateContacts is
  // the caller's until the collision row is built), velocities by the
  // matrix-free projected SOR on the GPU, positions by the midpoint rule.
  virtual void Step(double dt, Integrator g = Integrator::OPEN_DYNAMICS_ENGINE);
  // When Ensemble is first initialized, check for position errors, correct them
  // with StepPositionRelaxation (ensembles.cc:602-622); PostStabilize brings
  // positions AND velocities back to the constraint manifold (ensembles.cc:624-646).
  void InitStabilize();
  void PostStabilize(int max_steps = 500);
  // How CalculateVelocityRelaxation solves (J J^T) y = err.  Sweep (the default): the matrix-free SOR sweep.  Direct:
  // egs_relax_blocks_direct, the pivoted LDL^T the reference's ldlt() is, truncated at the first pivot
  // <= 1e-10 * |first pivot| (J J^T is singular with redundant contact points; J^T y is the same for every solution).
  enum struct RelaxationSolver { Sweep = 0, Direct };
  void SetRelaxationSolver(RelaxationSolver solver) { relaxation_solver_ = solver; }
  int last_relaxation_rank = -1;         // rank of the last Direct solve (-1: none yet)
  // M^-1 and the external force / torque vector: as Init() left them (quirk Q5) -- with SetLiveInertia(true) and a
  // device world, what the device holds for the bodies' current state, read back on demand.
  const MatrixXd &M_inverse() const { PullLiveMass(); return M_inverse_; }
  const VectorXd &external_force_torque() const { PullLiveMass(); return external_force_torque_; }
  // Not in the reference, off by default (Q5 stays the default): M^-1's angular blocks and the gyroscopic torque follow
  // the bodies (egs_world_set_live_inertia, with every Body's I_b()): each Step recomputes, from the R and w it starts
  // from, what Init() would compute at that state, for every Body whose I_b() is not a multiple of the identity.  The
  // device step does it on the device; the explicit paths (use_device_step = false, use_dense_solver, caller-supplied
  // contacts) on the host before StepVelocities_ODE, by Init()'s own code.  Turning it off freezes both at the state of
  // the last step.
  void SetLiveInertia(bool on);
  bool live_inertia() const { return live_inertia_; }
  const ConstraintsList constraints() const { return CombineConstraintsLists(); }
  const ComponentsList &components() const { return components_; }
  void SetContacts(const ContactsList &c) { contacts_ = c; }
  // Find all contacts between Bodies or between Body and ground, clear and
  // update contacts_ (ensembles.cc:445-480), then drop contacts closer than
  // 1e-6 to an earlier contact of the same pair (ensembles.cc:308-328): on the GPU.
  void UpdateContacts();
  // Rays against the ground and the components as they are now.  While the ensemble steps on the device and the Body
  // objects still hold what the last step left there, the table goes to the device world and is cast against the state
  // it holds (egs_world_set_rays, sent again only when the rays change; egs_world_cast_rays): no body state crosses.
  // Otherwise -- before the first Step, on the explicit paths, after a Body was edited -- the stateless entry on the
  // components' current poses (egs_cast_rays).  Both give the same bits.  Throws egs::Error(EGS_ERR_INVALID) as the
  // entries refuse: a non-finite or zero ray, tmax < 0, a body index out of range.
  std::vector<RayHit> CastRays(const std::vector<Ray> &rays);
  RayHit CastRay(const Vector3d &origin, const Vector3d &dir, double tmax = std::numeric_limits<double>::infinity());
  // Check whether there exist constraint pairs that are too close to each other (ensembles.cc:241-329):
  // conflicting joints between one pair of components are an error (the reference Panics; here
  // egs::Error with EGS_ERR_INVALID), a contact closer than 1e-6 to a joint or to an earlier contact
  // of the same pair is dropped.
  void CheckAndCorrectEnsembleState();
  bool use_device_step = true;   // false: the explicit UpdateContacts / StepVelocities_ODE / StepPositions_ODE calls
  // true: StepVelocities_ODE goes through the reference's LIVE dense path on the device (ComputeVDot,
  // ensembles.cc:498-538: dense J M^-1 J^T, condition check, conditional cfm, Lcp::MixedConstraintsSolver)
  // instead of the matrix-free sweeps; implies the explicit Step path.
  bool use_dense_solver = false;
  double last_condition_estimate = 0;
  bool detect_contacts = true;   // Step() calls UpdateContacts() as the reference does (ensembles.cc:393)
  const VectorXd GetVelocities() const;                                  // ensembles.cc:429-436
  VectorXd ComputePositionConstraintError() const;                       // ensembles.cc:156-171
  // solver parameters (compile-time constants in the reference)
  egs_solve_params solver_params;
  double cfm_coeff = 0.01;                                               // kCfmCoeff, ensembles.cc:14
  // Not in the reference, off by default: the device step's sweeps start from the previous step's lambda instead of
  // rhs (egs_world_set_warm_start: a contact takes the rows of the nearest previous contact of its body pair within
  // match_radius, metres, world frame; a joint its own).  The history lives with the device world: a step after
  // which no Body was touched continues it (the state is then not pushed again), a step after an edited Body, an
  // edited joint or a stabilise call starts from rhs as ever.  Throws egs::Error(EGS_ERR_INVALID) if radius < 0.
  void SetWarmStart(bool on, double match_radius = 0.01);
  // Not in the reference (Contact::FrictionModel::COULOMB_PYRAMID has empty bodies there), off by default: BOX is the
  // reference's model; COULOMB_PYRAMID bounds every contact's two tangential multipliers by +-mu times its normal
  // multiplier in the device step's sweeps (egs_world_set_friction).  Throws egs::Error: EGS_ERR_UNSUPPORTED for
  // NO_FRICTION and INFINITE, EGS_ERR_INVALID for a pyramid with mu < 0 or NaN.  A pyramid ensemble steps on the
  // device only: Step throws EGS_ERR_UNSUPPORTED where it would take the explicit or the dense path -- the dense path
  // unless SetDenseFriction has allowed it.
  void SetFriction(Contact::FrictionModel model, double mu = 0);
  // Not in the reference either, off by default: restitution (egs_world_set_restitution, egs_problem_set_restitution).
  // A contact approaching faster than `threshold` (m/s, >= 0) separates at e times its approach speed, with the
  // Baumgarte velocity as the floor; joints never bounce; e > 1 is allowed; e < 0 turns it off.  Takes effect in
  // every step that assembles on the device (the device world, and the per-step device problem with or without
  // use_dense_solver); a step whose rows the host assembles (a constraint the device cannot describe) throws
  // egs::Error(EGS_ERR_UNSUPPORTED) while it is on.  Throws egs::Error(EGS_ERR_INVALID): e NaN or infinite, threshold
  // < 0, NaN or infinite.
  void SetRestitution(double e, double threshold = 0.0);
  // Not in the reference: a weld and a hinge between components b0 (index i0) and b1 (i1; nullptr and -1: the world),
  // each a BallAndSocketJoint at anchor_world plus an angular block captured from the current pose (AngularLockJoint;
  // HingeAxisJoint about axis_world).  Both return the index of the angular joint in the ensemble's joints; call them
  // before Init().  SetHingeMotor drives the hinge at that index: speed rad/s about the axis (body0 relative to
  // body1) within +-max_torque, +inf allowed; max_torque < 0 removes the motor.  Throws egs::Error(EGS_ERR_INVALID)
  // for an index that is no hinge, a NaN or an infinite speed.  A hinge without a motor, or with max_torque = 0,
  // steps through the sweeps only: with use_dense_solver the library's EGS_ERR_UNSUPPORTED is thrown.
  int AddWeld(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &anchor_world);
  int AddHinge(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &anchor_world,
               const Vector3d &axis_world);
  void SetHingeMotor(int index, double speed, double max_torque);
  // Angle limits of the hinge at that index (HingeAxisJoint::SetLimits): lo <= theta <= hi in radians, -INFINITY /
  // +INFINITY for no stop; they reach the device with the next step.  Throws egs::Error(EGS_ERR_INVALID) for an index
  // that is no hinge, a NaN, lo > hi, or a finite |angle| >= pi.  An ensemble with a limited hinge does not step with
  // use_dense_solver (EGS_ERR_UNSUPPORTED from the library).  HingeAngle: theta of that hinge now (host, atan2).
  void SetHingeLimits(int index, double lo, double hi);
  double HingeAngle(int index) const;
  // A slider between b0 and b1 (nullptr, -1: the world) along axis_world at the current pose: an AngularLockJoint plus
  // a SliderAxisJoint whose rail point is chosen so that the travel x is 0 now.  Returns the slider's index; call it
  // before Init.  SetSliderMotor: dx/dt = speed within +-max_force (< 0: off).  SetSliderLimits: lo <= x <= hi,
  // -INFINITY / +INFINITY for no stop; both reach the device with the next step and throw egs::Error(EGS_ERR_INVALID)
  // for an index that is no slider, a NaN, an infinite speed, lo > hi, lo = +INFINITY or hi = -INFINITY.  An ensemble
  // with a free or a stopped slider does not step with use_dense_solver (EGS_ERR_UNSUPPORTED from the library).
  // SliderPosition: x of that slider now (host).
  int AddSlider(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &axis_world);
  void SetSliderMotor(int index, double speed, double max_force);
  void SetSliderLimits(int index, double lo, double hi);
  double SliderPosition(int index) const;
  const JointsList &joints() const { return joints_; }
  double restitution() const { return restitution_; }
  double restitution_threshold() const { return restitution_vth_; }
  // The pyramid on the dense direct solver, opt-in (egs_problem_set_dense_friction / egs_world_set_dense_friction):
  // after SetDenseFriction(max_outer > 0, tol) a COULOMB_PYRAMID ensemble with use_dense_solver steps instead of
  // throwing -- the fixed-point iteration on the tangential bounds, at most max_outer solves, stopping change tol --
  // and this ensemble's dense steps honour the stored bounds (use_bounds = 1, which the pyramid needs), whatever its
  // friction model.  last_dense_outer / last_dense_converged tell how the last such step ended; not converging is no
  // error.  max_outer = 0 switches it off again.  Throws egs::Error(EGS_ERR_INVALID): max_outer < 0, tol < 0 or NaN.
  void SetDenseFriction(int max_outer = 32, double tol = 1e-10);
  int dense_friction_outer() const { return dense_fric_outer_; }
  double dense_friction_tol() const { return dense_fric_tol_; }
  int last_dense_outer = 0;
  bool last_dense_converged = true;
  Contact::FrictionModel friction_model() const { return friction_model_; }
  double friction_mu() const { return friction_mu_; }
  bool warm_start() const { return warm_start_; }
  double warm_start_radius() const { return warm_radius_; }
  VectorXd last_lambda;
  int last_stabilize_steps = 0;

 protected:
  Ensemble();
  int n_ = 0;
  ComponentsList components_;
  JointsList joints_;
  ContactsList contacts_;
  mutable MatrixXd M_inverse_;               // (mutable: PullLiveMass)
  mutable VectorXd external_force_torque_;

 private:
  friend class EnsembleGroup;
  // SetLiveInertia: asked for; what the device world was last told; the world that last stepped this ensemble with live
  // inertia on (its own, or an EnsembleGroup's: not owned), the offset of its first body there and that world's bodies
  bool live_inertia_ = false, world_live_ = false;
  egs_world *live_world_ = nullptr;
  int live_offset_ = 0, live_total_ = 0;
  static bool IsMultipleOfIdentity(const Matrix3d &I);
  std::vector<double> BodyInertias() const;       // [n][9], every Body's I_b()
  void RefreshLiveMassOnHost();                   // Init()'s two arrays at the current state, skipped bodies left alone
  void PullLiveMass() const;                      // live inertia on and a device world: both arrays from egs_world_get_mass
  void ConstructMassInertiaMatrixInverse();                              // ensembles.cc:202-212
  void InitializeExternalForceTorqueVector();                            // ensembles.cc:214-222
  ConstraintsList CombineConstraintsLists() const;                       // ensembles.cc:234-239
  void UpdateComponentsVelocities(const VectorXd &v);                    // ensembles.cc:438-443
  VectorXd StepVelocities_ODE(double dt, const VectorXd &v, double error_reduction_param = 0.2);  // :563-575
  void StepPositions_ODE(double dt, const VectorXd &v, const VectorXd &v_new);                    // :577-591
  bool StepOnDevice(double dt);
  // egs_shape per component; empty when every Body is a box (the library then takes its all-box launches).  Shapes
  // go to the device with the side lengths (frozen at Init(), Q5) and with every UpdateContacts().  An ensemble with a sphere or a capsule
  // needs the device's detection: Step throws egs::Error(EGS_ERR_UNSUPPORTED) with detect_contacts = false.
  std::vector<int32_t> Shapes() const;
  // -step_scale * J^T (J J^T)^-1 err (ensembles.cc:659-666); the SPD(-semidefinite)
  // solve runs matrix-free on the GPU: the same projected sweep with M^-1 = I and
  // every row an equality.
  VectorXd CalculateVelocityRelaxation(double step_scale) const;
  void StepPositions_ExplicitEuler(double dt, const VectorXd &v);          // ensembles.cc:553-561
  void StepPositionRelaxation(double dt, double step_scale = 0.2);         // ensembles.cc:648-651
  void StepPostStabilization(double dt, double step_scale = 0.2);          // ensembles.cc:653-658
  RelaxationSolver relaxation_solver_ = RelaxationSolver::Sweep;
  egs_world *world_ = nullptr;
  int world_joints_ = -1;
  std::vector<int32_t> world_jb0_, world_jb1_;   // the joints the device world holds
  std::vector<double> world_jdata_;
  std::vector<int32_t> world_jkind_;             // ... their kinds and their motors ([joints][2], (0, -1): none)
  std::vector<double> world_jmotor_;
  std::vector<double> world_jlimit_;             // ... and their limit rows ([joints][8]; empty: none sent)
  std::vector<double> world_jtravel_;            // ... and the sliders' travel stops ([joints][2]; empty: none sent)
  bool warm_start_ = false, world_warm_ = false;   // asked for; what the device world was last told
  double warm_radius_ = 0.0, world_warm_radius_ = 0.0;
  Contact::FrictionModel friction_model_ = Contact::FrictionModel::BOX;
  double friction_mu_ = 0.0, world_friction_ = -1.0;   // asked for; the coefficient the device world was last told (< 0: box)
  int dense_fric_outer_ = 0;                     // SetDenseFriction (0: off)
  double dense_fric_tol_ = 0.0;
  bool problem_friction_ = false;                // the cached device problem holds friction coefficients
  double restitution_ = -1.0, restitution_vth_ = 0.0;   // asked for (< 0: off) ...
  double world_restitution_ = -1.0, world_restitution_vth_ = 0.0;   // ... and what the device world was last told
  bool problem_restitution_ = false;             // the cached device problem holds restitution coefficients
  double device_friction() const { return friction_model_ == Contact::FrictionModel::COULOMB_PYRAMID ? friction_mu_ : -1.0; }
  std::vector<double> world_state_;              // pos, R, v, w as pulled after the last device step (warm start only)
  std::vector<double> ray_pose_;                 // pos, R as pulled after the last device step: what the world's rays would see
  std::vector<double> world_rays_;               // the ray table the device world holds (origin, dir, tmax, body per ray)
  egs_problem *problem_ = nullptr;
  std::vector<int32_t> plan_b0_, plan_b1_;   // topology the cached device problem was planned for
};

class Chain : public Ensemble {  // ensembles.h:188-198, ensembles.cc:668-707
 public:
  Chain(int num_links, const Vector3d &anchor_position);
};

// ensembles.h:191-200, ensembles.cc:708-728: num_rocks boxes (m = 1, I = 0.1 I3) suspended at random
// positions inside the bounds with random rotations, velocities (|v_k| <= 1) and spins.  The
// reference draws from Eigen's Random (std::rand); so does this, through the same formulas
// (Vector3d::Random: 2 rand()/RAND_MAX - 1 per coefficient; Quaterniond::UnitRandom), so the
// scenario family is the reference's -- not its exact numbers, which depend on Eigen's call order.
class Cairn : public Ensemble {
 public:
  Cairn(int num_rocks, const std::array<double, 2> &x_bound, const std::array<double, 2> &y_bound,
        const std::array<double, 2> &z_bound);

 private:
  const double max_init_v_ = 1;
  const double max_init_w_ = 1;
};

// The frame of model.cc:37-70 -- SimulationStep() calls Step() on every Ensemble in turn -- as ONE batched device world
// (egs_world_create_batch): Step does for every member what Ensemble::Step does for one on the device, with member i
// stepped by dt[i] (egs_world_step_each; egs_world_step_dense_each when the members have use_dense_solver set), erp 0.2
// as in Ensemble::Step.  After it every member's Body objects, contacts and last_lambda hold, bit for bit, what the
// member's own Step(dt[i]) leaves (sweeps; the dense members: what a world of their own leaves after
// egs_world_step_dense).  dt[i] = 0: member i sits the step out, nothing of it changes.
//   - The members may differ in SetFriction: member i's contacts take its model and coefficient (egs_world_set_friction).
//   - The members may differ in SetRestitution's coefficient (egs_world_set_restitution); those that have it on must
//     agree in the threshold, of which the world has one.
//   - The members may differ in SetLiveInertia: the state is per body (egs_world_set_live_inertia; the bodies of a member
//     with it off are sent as the identity, which the device skips).
//   - The members must agree in solver_params, cfm_coeff, use_dense_solver, detect_contacts, SetWarmStart and SetDenseFriction, and each must be able to
//     take the device step (joints that Describe themselves, no caller-supplied contacts); the list may not be empty or
//     hold a pointer twice: the constructor throws egs::Error(EGS_ERR_INVALID) naming the offending member.
//   - The members are not owned and must outlive the group; Init() them before the first Step (M^-1, the external
//     force and the box sizes are sent once, quirk Q5).  A member may still be stepped on its own between group steps:
//     its Body objects are the interface, they are pushed before and pulled after every step.  Joints are re-sent
//     when edited.
class EnsembleGroup {
 public:
  explicit EnsembleGroup(std::vector<Ensemble *> members);
  ~EnsembleGroup();
  EnsembleGroup(const EnsembleGroup &) = delete;
  EnsembleGroup &operator=(const EnsembleGroup &) = delete;
  void Step(const std::vector<double> &dt);   // dt[i] = 0: member i sits out; Integrator::OPEN_DYNAMICS_ENGINE
  void Step(double dt);                       // every member
  // how many ensembles the group's device world holds (0 before the first Step) and how many worlds it has made
  int world_ensembles() const;
  int worlds_created() const { return worlds_created_; }
  // rays[i]: member i's rays, body indices in member i's own numbering; the result likewise.  One table and one launch on
  // the group's world while every member's Body objects hold what the last group Step left there; otherwise each member
  // casts for itself (Ensemble::CastRays).
  std::vector<std::vector<RayHit>> CastRays(const std::vector<std::vector<Ray>> &rays);

 private:
  std::vector<Ensemble *> members_;
  std::vector<int32_t> off_;                  // [E + 1] member i's bodies in the world
  egs_world *world_ = nullptr;
  int worlds_created_ = 0;
  bool joints_sent_ = false;
  std::vector<int32_t> world_jb0_, world_jb1_;   // the joints the device world holds
  std::vector<double> world_jdata_;
  std::vector<int32_t> world_jkind_;             // ... their kinds and their motors, re-sent with them
  std::vector<double> world_jmotor_;
  std::vector<double> world_jlimit_;             // ... and their limit rows ([joints][8]; empty: none sent)
  std::vector<double> world_jtravel_;            // ... and the sliders' travel stops ([joints][2]; empty: none sent)
  bool world_warm_ = false;                      // what the device world was last told (the members' SetWarmStart)
  double world_warm_radius_ = 0.0;
  std::vector<double> world_friction_;           // ... and the members' friction coefficients (empty: never told)
  std::vector<double> world_restitution_;        // ... their restitution coefficients and the threshold
  double world_restitution_vth_ = 0.0;
  std::vector<char> world_live_;                 // ... and the members' SetLiveInertia (empty: never told, all off)
  std::vector<double> world_state_;              // pos, R, v, w as pulled after the last step (warm start only)
  std::vector<double> ray_pose_;                 // pos, R as pulled after the last step: what the world's rays would see
  std::vector<double> world_rays_;               // the ray table the world holds (origin, dir, tmax, body, ensemble per ray)
};

#endif
