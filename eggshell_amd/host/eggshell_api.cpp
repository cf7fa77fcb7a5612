// eggshell_api.cpp -- see eggshell_api.h.  Host C++ only; all heavy arithmetic
// goes through the C ABI to the HIP library.  There is no CPU solver here: if
// the library cannot reach a GPU the calls throw egs::Error.
#include "eggshell_api.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>

namespace egs {
egs_context *DefaultContext() {
  static egs_context *ctx = nullptr;
  static std::once_flag once;
  static egs_status st = EGS_OK;
  std::call_once(once, [] { st = egs_context_create(0, &ctx); });
  if (!ctx) throw Error(st, "egs_context_create failed: no usable MI355X (there is no CPU fallback)");
  return ctx;
}
static void check(egs_status st) {
  if (st != EGS_OK) throw Error(st, egs_last_error(DefaultContext()));
}
// pos, R, v, w of every body as one array, and whether a gathered state is that array bit for bit (SetWarmStart:
// a state nobody touched since the last device step is not pushed again)
static void keep_state(std::vector<double> &kept, const std::vector<double> &pos, const std::vector<double> &R,
                       const std::vector<double> &v, const std::vector<double> &w) {
  kept.clear();
  for (const std::vector<double> *a : {&pos, &R, &v, &w}) kept.insert(kept.end(), a->begin(), a->end());
}
static bool same_state(const std::vector<double> &kept, const std::vector<double> &pos, const std::vector<double> &R,
                       const std::vector<double> &v, const std::vector<double> &w) {
  if (kept.empty() || kept.size() != pos.size() + R.size() + v.size() + w.size()) return false;
  size_t at = 0;
  for (const std::vector<double> *a : {&pos, &R, &v, &w}) {
    if (!a->empty() && std::memcmp(kept.data() + at, a->data(), a->size() * sizeof(double)) != 0) return false;
    at += a->size();
  }
  return true;
}
}  // namespace egs

// ---- utils ---------------------------------------------------------------
Matrix3d CrossMat(const Vector3d &a) {  // utils.cc:16-24
  Matrix3d m;
  m(0, 1) = -a(2); m(0, 2) = a(1);
  m(1, 0) = a(2);  m(1, 2) = -a(0);
  m(2, 0) = -a(1); m(2, 1) = a(0);
  return m;
}

static Matrix3d QuatToR(double w, double x, double y, double z) {
  double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
  double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  Matrix3d R;
  R(0, 0) = 1.0 - (tyy + tzz); R(0, 1) = txy - twz;         R(0, 2) = txz + twy;
  R(1, 0) = txy + twz;         R(1, 1) = 1.0 - (txx + tzz); R(1, 2) = tyz - twx;
  R(2, 0) = txz - twy;         R(2, 1) = tyz + twx;         R(2, 2) = 1.0 - (txx + tyy);
  return R;
}

Matrix3d AlignVectors(const Vector3d &a, const Vector3d &b) {  // utils.cc:233-237
  auto normalized = [](const Vector3d &v) { double n2 = v.dot(v); return n2 > 0 ? v / std::sqrt(n2) : v; };
  Vector3d v0 = normalized(a), v1 = normalized(b);
  double c = v1.dot(v0);
  if (c < -1.0 + 1e-12) {  // deterministic axis instead of Eigen's SVD
    if (c < -1.0) c = -1.0;
    double ax = std::fabs(v0[0]), ay = std::fabs(v0[1]), az = std::fabs(v0[2]);
    Vector3d e = (ax <= ay && ax <= az) ? Vector3d(1, 0, 0) : (ay <= az ? Vector3d(0, 1, 0) : Vector3d(0, 0, 1));
    Vector3d axis = v0.cross(e);
    axis = axis / axis.norm();
    double w2 = (1.0 + c) * 0.5, sv = std::sqrt(1.0 - w2);
    return QuatToR(std::sqrt(w2), axis[0] * sv, axis[1] * sv, axis[2] * sv);
  }
  Vector3d axis = v0.cross(v1);
  double s = std::sqrt((1.0 + c) * 2.0), invs = 1.0 / s;
  return QuatToR(s * 0.5, axis[0] * invs, axis[1] * invs, axis[2] * invs);
}

Matrix3d WtoR(const Vector3d &w, double dt) {  // utils.cc:82-89
  double n2 = w.dot(w), nrm = std::sqrt(n2);
  Vector3d ax = n2 > 0 ? w / nrm : w;
  double half = 0.5 * (nrm * dt), s = std::sin(half), c = std::cos(half);
  return QuatToR(c, s * ax[0], s * ax[1], s * ax[2]);
}

Matrix3d Body::CalculateInertia(double m) const {  // body.cc:19-36
  Vector3d s = GetSideLengths();
  Matrix3d I;
  I(0, 0) = m / 12 * (s[1] * s[1] + s[2] * s[2]);
  I(1, 1) = m / 12 * (s[0] * s[0] + s[2] * s[2]);
  I(2, 2) = m / 12 * (s[0] * s[0] + s[1] * s[1]);
  return I;
}

// Not in the reference.  A uniform solid capsule about its centre, axis z: the cylinder (m_c) and the two
// hemispheres (m_s together) share the mass by volume, pi r^2 H : (4/3) pi r^3.
Body Body::Capsule(const Vector3d &p, const Vector3d &v, double radius, double length, double m) {
  if (!(radius > 0) || !(length > 2 * radius) || !std::isfinite(length))
    throw egs::Error(EGS_ERR_INVALID, "Body::Capsule: length is tip to tip and must exceed 2 radius > 0 (a capsule "
                                      "with length == 2 radius is a Body::Sphere)");
  const double r = radius, H = length - 2 * radius;
  const double vc = M_PI * r * r * H, vs = 4.0 / 3.0 * M_PI * r * r * r;
  const double mc = m * vc / (vc + vs), ms = m * vs / (vc + vs);
  Matrix3d I = Matrix3d::Identity();
  I(0, 0) = I(1, 1) = mc * (H * H / 12 + r * r / 4) + ms * (0.4 * r * r + H * H / 4 + 0.375 * H * r);
  I(2, 2) = mc * r * r / 2 + 0.4 * ms * r * r;
  Body b(p, v, m, Matrix3d::Identity(), Vector3d::Zero(), I);
  b.type_ = BodyType::Capsule;
  b.radius_ = radius;
  b.length_ = length;
  return b;
}

// ---- joints.cc -----------------------------------------------------------
static VectorXd ToX(const Vector3d &v) { VectorXd x(3); for (int k = 0; k < 3; ++k) x(k) = v[k]; return x; }

VectorXd BallAndSocketJoint::ComputeError() const {  // joints.cc:3-11
  if (b1_ == nullptr) return ToX(b0_->p() + b0_->R() * c0_ - c1_);
  return ToX(b0_->p() + b0_->R() * c0_ - b1_->p() - b1_->R() * c1_);
}

static void SetBlock(MatrixXd *J, const Matrix3d &lin, const Matrix3d &ang) {
  J->resize(3, 6);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) { (*J)(r, c) = lin(r, c); (*J)(r, 3 + c) = ang(r, c); }
}

void BallAndSocketJoint::ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *ct, VectorXd *lo, VectorXd *hi) const {
  SetBlock(J_b0, Matrix3d::Identity(), -1.0 * CrossMat(b0_->R() * c0_));  // joints.cc:21-22
  if (b1_ == nullptr) SetBlock(J_b1, Matrix3d::Zero(), Matrix3d::Zero());
  else SetBlock(J_b1, -1.0 * Matrix3d::Identity(), CrossMat(b1_->R() * c1_));
  ct->resize(3); lo->resize(3); hi->resize(3);
  for (int k = 0; k < 3; ++k) (*ct)(k) = 1;  // joints.cc:31-34
}

bool BallAndSocketJoint::Describe(int32_t *kind, double data[7]) const {
  *kind = EGS_JOINT_BALL;
  for (int k = 0; k < 3; ++k) { data[k] = c0_[k]; data[3 + k] = c1_[k]; }
  data[6] = 0;
  return true;
}

Vector3d BallAndSocketJoint::GetConstraintPosition() const {  // joints.cc:57-75
  const Vector3d p0 = b0_->p() + b0_->R() * c0_;
  if (b1_ == nullptr) return p0;
  return (p0 + (b1_->p() + b1_->R() * c1_)) / 2;
}

// ---- the angular blocks (not in the reference; the device's operation order, assemble_device.h) --------------
static Matrix3d QuatToR(const double q[4]) {   // utils.cc's quaternion matrix in the library's order (quat_to_R)
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  Matrix3d R;
  R.d[0] = 1.0 - (tyy + tzz); R.d[1] = txy - twz;         R.d[2] = txz + twy;
  R.d[3] = txy + twz;         R.d[4] = 1.0 - (txx + tzz); R.d[5] = tyz - twx;
  R.d[6] = txz - twy;         R.d[7] = tyz + twx;         R.d[8] = 1.0 - (txx + tyy);
  return R;
}

// a unit quaternion of the rotation matrix, by the largest of the four squared components
static void RToQuat(const Matrix3d &R, double q[4]) {
  const double t = R(0, 0) + R(1, 1) + R(2, 2);
  const double c[4] = {1 + t, 1 + 2 * R(0, 0) - t, 1 + 2 * R(1, 1) - t, 1 + 2 * R(2, 2) - t};
  int k = 0;
  for (int i = 1; i < 4; ++i) if (c[i] > c[k]) k = i;
  const double s = 2.0 * std::sqrt(c[k]);
  if (k == 0) { q[0] = s / 4; q[1] = (R(2, 1) - R(1, 2)) / s; q[2] = (R(0, 2) - R(2, 0)) / s; q[3] = (R(1, 0) - R(0, 1)) / s; }
  else if (k == 1) { q[0] = (R(2, 1) - R(1, 2)) / s; q[1] = s / 4; q[2] = (R(0, 1) + R(1, 0)) / s; q[3] = (R(0, 2) + R(2, 0)) / s; }
  else if (k == 2) { q[0] = (R(0, 2) - R(2, 0)) / s; q[1] = (R(0, 1) + R(1, 0)) / s; q[2] = s / 4; q[3] = (R(1, 2) + R(2, 1)) / s; }
  else { q[0] = (R(1, 0) - R(0, 1)) / s; q[1] = (R(0, 2) + R(2, 0)) / s; q[2] = (R(1, 2) + R(2, 1)) / s; q[3] = s / 4; }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] /= n;
}

static void AngularRows(ArrayXb *ct, VectorXd *lo, VectorXd *hi, bool axis_row_is_equality) {
  ct->resize(3); lo->resize(3); hi->resize(3);
  (*ct)(0) = 1; (*ct)(1) = 1; (*ct)(2) = axis_row_is_equality ? 1 : 0;
}

AngularLockJoint::AngularLockJoint(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1)
    : Joint(std::move(b0), i0, Vector3d::Zero(), std::move(b1), i1, Vector3d::Zero()) {
  const Matrix3d R0t = b0_->R().transpose();
  RToQuat(b1_ == nullptr ? R0t : R0t * b1_->R(), q_);
}

VectorXd AngularLockJoint::ComputeError() const {
  const Matrix3d T = b0_->R() * QuatToR(q_);
  const Matrix3d E = b1_ == nullptr ? T : T * b1_->R().transpose();
  return ToX(Vector3d(0.5 * (E.d[7] - E.d[5]), 0.5 * (E.d[2] - E.d[6]), 0.5 * (E.d[3] - E.d[1])));
}

void AngularLockJoint::ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *ct, VectorXd *lo, VectorXd *hi) const {
  SetBlock(J_b0, Matrix3d::Zero(), Matrix3d::Identity());
  if (b1_ == nullptr) SetBlock(J_b1, Matrix3d::Zero(), Matrix3d::Zero());
  else SetBlock(J_b1, Matrix3d::Zero(), -1.0 * Matrix3d::Identity());
  AngularRows(ct, lo, hi, true);
}

bool AngularLockJoint::Describe(int32_t *kind, double data[7]) const {
  *kind = EGS_JOINT_LOCK;
  for (int k = 0; k < 4; ++k) data[k] = q_[k];
  data[4] = data[5] = data[6] = 0;
  return true;
}

HingeAxisJoint::HingeAxisJoint(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &axis_world)
    : Joint(std::move(b0), i0, Vector3d::Zero(), std::move(b1), i1, Vector3d::Zero()) {
  if (!(axis_world.norm() > 0)) throw egs::Error(EGS_ERR_INVALID, "HingeAxisJoint: the axis must not vanish");
  const Vector3d a = axis_world / axis_world.norm();
  a0_ = b0_->R().transpose() * a;
  a0_ = a0_ / a0_.norm();
  a1_ = b1_ == nullptr ? a : b1_->R().transpose() * a;
  a1_ = a1_ / a1_.norm();
  const Matrix3d R0t = b0_->R().transpose();
  RToQuat(b1_ == nullptr ? R0t : R0t * b1_->R(), q_);
}

void HingeAxisJoint::SinCos(double *sn, double *cs) const {
  const Vector3d s = b0_->R() * a0_;
  const Matrix3d T = b0_->R() * QuatToR(q_);
  const Matrix3d E = b1_ == nullptr ? T : T * b1_->R().transpose();
  const Vector3d ax(0.5 * (E.d[7] - E.d[5]), 0.5 * (E.d[2] - E.d[6]), 0.5 * (E.d[3] - E.d[1]));
  *sn = s.dot(ax);
  *cs = 0.5 * (((E.d[0] + E.d[4]) + E.d[8]) - 1.0);
}

void HingeAxisJoint::LimitRow(double row[8]) const {
  for (int k = 0; k < 4; ++k) row[k] = q_[k];
  row[4] = std::isfinite(limit_lo_) ? std::sin(limit_lo_) : 0.0;
  row[5] = std::isfinite(limit_lo_) ? std::cos(limit_lo_) : 0.0;
  row[6] = std::isfinite(limit_hi_) ? std::sin(limit_hi_) : 0.0;
  row[7] = std::isfinite(limit_hi_) ? std::cos(limit_hi_) : 0.0;
}

double HingeAxisJoint::Angle() const {
  double sn, cs;
  SinCos(&sn, &cs);
  return std::atan2(sn, cs);
}

int HingeAxisJoint::ActiveStop(double *err2) const {
  *err2 = 0.0;
  if (!has_limits()) return 0;
  double L[8], sn, cs;
  LimitRow(L);
  SinCos(&sn, &cs);
  const double slo = L[4], clo = L[5], shi = L[6], chi = L[7];
  const bool lower = slo != 0.0 || clo != 0.0, upper = shi != 0.0 || chi != 0.0;
  if (upper && sn * (1.0 + chi) > shi * (1.0 + cs)) { *err2 = sn * chi - cs * shi; return 1; }
  if (lower && sn * (1.0 + clo) < slo * (1.0 + cs)) { *err2 = sn * clo - cs * slo; return -1; }
  return 0;
}

VectorXd HingeAxisJoint::ComputeError() const {
  const Vector3d s = b0_->R() * a0_;
  const Vector3d t = b1_ == nullptr ? a1_ : b1_->R() * a1_;
  const Matrix3d Rn = AlignVectors(s, Vector3d(0, 0, 1));
  const Vector3d c = t.cross(s);
  double err2;
  ActiveStop(&err2);   // 0 unless a stop is active: then sin(theta - limit)
  return ToX(Vector3d(Vector3d(Rn.d[0], Rn.d[1], Rn.d[2]).dot(c), Vector3d(Rn.d[3], Rn.d[4], Rn.d[5]).dot(c), err2));
}

void HingeAxisJoint::ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *ct, VectorXd *lo, VectorXd *hi) const {
  const Matrix3d Rn = AlignVectors(b0_->R() * a0_, Vector3d(0, 0, 1));
  SetBlock(J_b0, Matrix3d::Zero(), Rn);
  if (b1_ == nullptr) SetBlock(J_b1, Matrix3d::Zero(), Matrix3d::Zero());
  else SetBlock(J_b1, Matrix3d::Zero(), -1.0 * Rn);
  AngularRows(ct, lo, hi, false);
  double err2;
  const int stop = ActiveStop(&err2);   // an active stop's row is the limit's for the step: the motor leaves it alone
  if (stop > 0) { (*lo)(2) = -INFINITY; (*hi)(2) = 0.0; }
  else if (stop < 0) { (*lo)(2) = 0.0; (*hi)(2) = INFINITY; }
  else if (tau_ >= 0) { (*lo)(2) = -tau_; (*hi)(2) = tau_; }
}

bool HingeAxisJoint::Describe(int32_t *kind, double data[7]) const {
  *kind = EGS_JOINT_HINGE_AXIS;
  for (int k = 0; k < 3; ++k) { data[k] = a0_[k]; data[3 + k] = a1_[k]; }
  data[6] = 0;
  return true;
}

SliderAxisJoint::SliderAxisJoint(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &axis_world)
    : Joint(std::move(b0), i0, Vector3d::Zero(), std::move(b1), i1, Vector3d::Zero()) {
  if (!(axis_world.norm() > 0)) throw egs::Error(EGS_ERR_INVALID, "SliderAxisJoint: the rail direction must not vanish");
  const Vector3d a = axis_world / axis_world.norm();
  a0_ = b0_->R().transpose() * a;
  a0_ = a0_ / a0_.norm();
  // x = 0 now: the rail's point is body1's centre (in body0's frame), or body0's own centre for a world side
  c_ = b1_ == nullptr ? b0_->p() : b0_->R().transpose() * (b1_->p() - b0_->p());
}

void SliderAxisJoint::Frame(Matrix3d *Rn, Vector3d *D, Vector3d *rel) const {
  const Vector3d s = b0_->R() * a0_;
  *Rn = AlignVectors(s, Vector3d(0, 0, 1));
  const Vector3d p0 = b0_->p();
  if (b1_ != nullptr) {
    const Vector3d ro = b0_->R() * c_, P1 = b1_->p();
    for (int k = 0; k < 3; ++k) { (*D)[k] = (p0[k] + ro[k]) - P1[k]; (*rel)[k] = p0[k] - P1[k]; }
  } else {
    for (int k = 0; k < 3; ++k) { (*D)[k] = p0[k] - c_[k]; (*rel)[k] = p0[k] - c_[k]; }
  }
}

double SliderAxisJoint::Position() const {
  Matrix3d Rn;
  Vector3d D, rel;
  Frame(&Rn, &D, &rel);
  return Vector3d(Rn.d[6], Rn.d[7], Rn.d[8]).dot(D);
}

int SliderAxisJoint::ActiveStop(double *err2) const {
  *err2 = 0.0;
  if (!has_limits()) return 0;
  const double x = Position();
  if (limit_hi_ < INFINITY && x > limit_hi_) { *err2 = x - limit_hi_; return 1; }
  if (limit_lo_ > -INFINITY && x < limit_lo_) { *err2 = x - limit_lo_; return -1; }
  return 0;
}

VectorXd SliderAxisJoint::ComputeError() const {
  Matrix3d Rn;
  Vector3d D, rel;
  Frame(&Rn, &D, &rel);
  double err2;
  ActiveStop(&err2);   // 0 unless a stop is active: then x - stop
  return ToX(Vector3d(Vector3d(Rn.d[0], Rn.d[1], Rn.d[2]).dot(D), Vector3d(Rn.d[3], Rn.d[4], Rn.d[5]).dot(D), err2));
}

void SliderAxisJoint::ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *ct, VectorXd *lo, VectorXd *hi) const {
  Matrix3d Rn;
  Vector3d D, rel;
  Frame(&Rn, &D, &rel);
  SetBlock(J_b0, Rn, Rn * CrossMat(rel));   // row r of the angular part: (P1 - p0) x Rn_r, the lever arm on body0 alone
  if (b1_ == nullptr) SetBlock(J_b1, Matrix3d::Zero(), Matrix3d::Zero());
  else SetBlock(J_b1, -1.0 * Rn, Matrix3d::Zero());
  AngularRows(ct, lo, hi, false);
  double err2;
  const int stop = ActiveStop(&err2);   // an active stop's row is the stop's for the step: the motor leaves it alone
  if (stop > 0) { (*lo)(2) = -INFINITY; (*hi)(2) = 0.0; }
  else if (stop < 0) { (*lo)(2) = 0.0; (*hi)(2) = INFINITY; }
  else if (force_ >= 0) { (*lo)(2) = -force_; (*hi)(2) = force_; }
}

bool SliderAxisJoint::Describe(int32_t *kind, double data[7]) const {
  *kind = EGS_JOINT_SLIDER_AXIS;
  for (int k = 0; k < 3; ++k) { data[k] = a0_[k]; data[3 + k] = c_[k]; }
  data[6] = 0;
  return true;
}

// [joints][2] = (speed, tau) of a joint list, (0, -1) for whatever is no motored hinge or slider; returns whether any is driven
static bool JointMotors(const JointsList &joints, std::vector<double> *motor) {
  bool any = false;
  motor->assign(2 * joints.size(), 0.0);
  for (size_t j = 0; j < joints.size(); ++j) {
    (*motor)[2 * j + 1] = -1.0;
    if (const auto *sl = dynamic_cast<const SliderAxisJoint *>(joints[j].get())) {
      if (!(sl->motor_force() >= 0)) continue;
      (*motor)[2 * j] = sl->motor_speed(); (*motor)[2 * j + 1] = sl->motor_force();
      any = true;
      continue;
    }
    const auto *h = dynamic_cast<const HingeAxisJoint *>(joints[j].get());
    if (!h || !(h->motor_torque() >= 0)) continue;
    (*motor)[2 * j] = h->motor_speed(); (*motor)[2 * j + 1] = h->motor_torque();
    any = true;
  }
  return any;
}

// [joints][8], the limit rows of a joint list, zeros for whatever is no limited hinge; returns whether any hinge has a stop
static bool JointLimits(const JointsList &joints, std::vector<double> *lim) {
  bool any = false;
  lim->assign(8 * joints.size(), 0.0);
  for (size_t j = 0; j < joints.size(); ++j) {
    const auto *h = dynamic_cast<const HingeAxisJoint *>(joints[j].get());
    if (!h || !h->has_limits()) continue;
    h->LimitRow(lim->data() + 8 * j);
    any = true;
  }
  return any;
}

// [joints][2], the travel stops of a joint list, (-inf, +inf) for whatever is no limited slider; returns whether any slider has a stop
static bool JointTravel(const JointsList &joints, std::vector<double> *lim) {
  bool any = false;
  lim->assign(2 * joints.size(), INFINITY);
  for (size_t j = 0; j < joints.size(); ++j) {
    (*lim)[2 * j] = -INFINITY;
    const auto *sl = dynamic_cast<const SliderAxisJoint *>(joints[j].get());
    if (!sl || !sl->has_limits()) continue;
    (*lim)[2 * j] = sl->limit_lo(); (*lim)[2 * j + 1] = sl->limit_hi();
    any = true;
  }
  return any;
}

int Ensemble::AddSlider(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &axis_world) {
  auto slider = std::make_shared<SliderAxisJoint>(b0, i0, b1, i1, axis_world);   // (throws before anything is added)
  joints_.push_back(std::make_shared<AngularLockJoint>(b0, i0, b1, i1));
  joints_.push_back(slider);
  return (int)joints_.size() - 1;
}

void Ensemble::SetSliderMotor(int index, double speed, double max_force) {
  auto *s = index >= 0 && index < (int)joints_.size() ? dynamic_cast<SliderAxisJoint *>(joints_[index].get()) : nullptr;
  if (!s) throw egs::Error(EGS_ERR_INVALID, "SetSliderMotor: joint " + std::to_string(index) + " is not a slider");
  if (speed != speed || std::isinf(speed) || max_force != max_force)
    throw egs::Error(EGS_ERR_INVALID, "SetSliderMotor: the speed must be finite and the force limit a number");
  s->SetMotor(speed, max_force);
}

void Ensemble::SetSliderLimits(int index, double lo, double hi) {
  auto *s = index >= 0 && index < (int)joints_.size() ? dynamic_cast<SliderAxisJoint *>(joints_[index].get()) : nullptr;
  if (!s) throw egs::Error(EGS_ERR_INVALID, "SetSliderLimits: joint " + std::to_string(index) + " is not a slider");
  if (lo != lo || hi != hi || lo > hi || lo == INFINITY || hi == -INFINITY)
    throw egs::Error(EGS_ERR_INVALID, "SetSliderLimits: the limits must be numbers with lo <= hi; -INFINITY / +INFINITY mean no stop");
  s->SetLimits(lo, hi);
}

double Ensemble::SliderPosition(int index) const {
  const auto *s = index >= 0 && index < (int)joints_.size() ? dynamic_cast<const SliderAxisJoint *>(joints_[index].get()) : nullptr;
  if (!s) throw egs::Error(EGS_ERR_INVALID, "SliderPosition: joint " + std::to_string(index) + " is not a slider");
  return s->Position();
}

int Ensemble::AddWeld(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &anchor_world) {
  const Vector3d c0 = b0->R().transpose() * (anchor_world - b0->p());
  if (b1 == nullptr) joints_.push_back(std::make_shared<BallAndSocketJoint>(b0, i0, c0, anchor_world));
  else joints_.push_back(std::make_shared<BallAndSocketJoint>(b0, i0, c0, b1, i1, b1->R().transpose() * (anchor_world - b1->p())));
  joints_.push_back(std::make_shared<AngularLockJoint>(b0, i0, b1, i1));
  return (int)joints_.size() - 1;
}

int Ensemble::AddHinge(std::shared_ptr<Body> b0, int i0, std::shared_ptr<Body> b1, int i1, const Vector3d &anchor_world,
                       const Vector3d &axis_world) {
  auto hinge = std::make_shared<HingeAxisJoint>(b0, i0, b1, i1, axis_world);   // (throws before anything is added)
  const Vector3d c0 = b0->R().transpose() * (anchor_world - b0->p());
  if (b1 == nullptr) joints_.push_back(std::make_shared<BallAndSocketJoint>(b0, i0, c0, anchor_world));
  else joints_.push_back(std::make_shared<BallAndSocketJoint>(b0, i0, c0, b1, i1, b1->R().transpose() * (anchor_world - b1->p())));
  joints_.push_back(hinge);
  return (int)joints_.size() - 1;
}

void Ensemble::SetHingeMotor(int index, double speed, double max_torque) {
  auto *h = index >= 0 && index < (int)joints_.size() ? dynamic_cast<HingeAxisJoint *>(joints_[index].get()) : nullptr;
  if (!h) throw egs::Error(EGS_ERR_INVALID, "SetHingeMotor: joint " + std::to_string(index) + " is not a hinge");
  if (speed != speed || std::isinf(speed) || max_torque != max_torque)
    throw egs::Error(EGS_ERR_INVALID, "SetHingeMotor: the speed must be finite and the torque limit a number");
  h->SetMotor(speed, max_torque);
}

void Ensemble::SetHingeLimits(int index, double lo, double hi) {
  auto *h = index >= 0 && index < (int)joints_.size() ? dynamic_cast<HingeAxisJoint *>(joints_[index].get()) : nullptr;
  if (!h) throw egs::Error(EGS_ERR_INVALID, "SetHingeLimits: joint " + std::to_string(index) + " is not a hinge");
  if (lo != lo || hi != hi || lo > hi) throw egs::Error(EGS_ERR_INVALID, "SetHingeLimits: the limits must be numbers with lo <= hi");
  const double pi = 3.14159265358979323846;
  if ((std::isfinite(lo) && std::fabs(lo) >= pi) || (std::isfinite(hi) && std::fabs(hi) >= pi) || lo == INFINITY || hi == -INFINITY)
    throw egs::Error(EGS_ERR_INVALID, "SetHingeLimits: a finite limit lies inside (-pi, pi); -INFINITY / +INFINITY mean no stop");
  h->SetLimits(lo, hi);
}

double Ensemble::HingeAngle(int index) const {
  const auto *h = index >= 0 && index < (int)joints_.size() ? dynamic_cast<const HingeAxisJoint *>(joints_[index].get()) : nullptr;
  if (!h) throw egs::Error(EGS_ERR_INVALID, "HingeAngle: joint " + std::to_string(index) + " is not a hinge");
  return h->Angle();
}

// ---- contact.cc ----------------------------------------------------------
VectorXd Contact::ComputeError() const {  // contact.cc:14-22
  VectorXd e(3);
  e(2) = -cg_.depth;
  return e;
}

void Contact::ComputeJ(MatrixXd *J_b0, MatrixXd *J_b1, ArrayXb *C, VectorXd *x_lo, VectorXd *x_hi) const {
  Matrix3d R = AlignVectors(cg_.normal, Vector3d(0, 0, 1));  // contact.cc:53-54
  if (b0_ == nullptr) SetBlock(J_b0, Matrix3d::Zero(), Matrix3d::Zero());
  else SetBlock(J_b0, R * (-1.0 * Matrix3d::Identity()), R * CrossMat(cg_.position - b0_->p()));
  if (b1_ == nullptr) SetBlock(J_b1, Matrix3d::Zero(), Matrix3d::Zero());
  else SetBlock(J_b1, R * Matrix3d::Identity(), R * (-1.0 * CrossMat(cg_.position - b1_->p())));
  C->resize(3); x_lo->resize(3); x_hi->resize(3);  // FrictionModel::BOX, contact.cc:103-113
  (*x_lo)(0) = -1; (*x_lo)(1) = -1; (*x_lo)(2) = 0;
  (*x_hi)(0) = 1; (*x_hi)(1) = 1; (*x_hi)(2) = std::numeric_limits<double>::infinity();
}

bool Contact::Describe(int32_t *kind, double data[7]) const {
  *kind = EGS_CONTACT_BOX;
  for (int k = 0; k < 3; ++k) { data[k] = cg_.position[k]; data[3 + k] = cg_.normal[k]; }
  data[6] = cg_.depth;
  return true;
}

// ---- flattening: ConstraintsList -> the arrays of entry 1 -------------------
namespace {
struct Flat {
  int n = 0, m = 0;
  std::vector<double> Minv, J0, J1, lo, hi;
  std::vector<int32_t> body0, body1;
  std::vector<uint8_t> is_eq;
};

Flat Flatten(const ConstraintsList &constraints, const MatrixXd &M_inverse) {
  Flat f;
  f.n = M_inverse.rows() / 6;
  f.m = (int)constraints.size();
  f.Minv.resize((size_t)f.n * 36);
  for (int b = 0; b < f.n; ++b)  // only block<6,6>(6b,6b) is ever read
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) f.Minv[(size_t)b * 36 + 6 * r + c] = M_inverse(6 * b + r, 6 * b + c);
  f.J0.assign((size_t)f.m * 18, 0.0); f.J1.assign((size_t)f.m * 18, 0.0);
  f.lo.resize((size_t)f.m * 3); f.hi.resize((size_t)f.m * 3); f.is_eq.resize((size_t)f.m * 3);
  f.body0.resize(f.m); f.body1.resize(f.m);
  for (int i = 0; i < f.m; ++i) {  // m ComputeJ calls (the reference makes O(m^2) per pass)
    MatrixXd j0, j1; ArrayXb ct; VectorXd lo, hi;
    constraints[i]->ComputeJ(&j0, &j1, &ct, &lo, &hi);
    if (j0.rows() != 3 || ct.size() != 3)
      throw egs::Error(EGS_ERR_INVALID, "only 3-row constraints are supported (joints.cc:18, contact.cc:103)");
    f.body0[i] = constraints[i]->i0_; f.body1[i] = constraints[i]->i1_;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 6; ++c) { f.J0[(size_t)i * 18 + 6 * r + c] = j0(r, c); f.J1[(size_t)i * 18 + 6 * r + c] = j1(r, c); }
      f.lo[(size_t)i * 3 + r] = lo(r); f.hi[(size_t)i * 3 + r] = hi(r); f.is_eq[(size_t)i * 3 + r] = ct(r) ? 1 : 0;
    }
  }
  return f;
}

sparse::LastSolve g_last = {0, 0.0, 0, 0, 0};

VectorXd Iterate(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &rhs, double cfm,
                 egs_method method) {
  if (constraints.empty()) return VectorXd(0);  // sparse_iterations.cc:152-154
  Flat f = Flatten(constraints, M_inverse);
  if (rhs.size() != 3 * f.m) throw egs::Error(EGS_ERR_INVALID, "rhs size != 3 * constraints");
  egs_solve_params prm;
  egs_default_params(&prm);  // 500 sweeps, tol 1e-9, omega 1.5: sparse_iterations.cc:15-19
  prm.method = method;
  prm.cfm = cfm;
  egs_solve_stats st;
  VectorXd x(3 * f.m);
  egs::check(egs_solve_blocks(egs::DefaultContext(), f.n, f.Minv.data(), f.m, f.body0.data(), f.body1.data(),
                              f.J0.data(), f.J1.data(), f.is_eq.data(), f.lo.data(), f.hi.data(), rhs.data(), &prm,
                              EGS_F64, x.data(), &st));
  g_last = {st.iterations, st.residual, st.n_islands, st.n_tiles, st.n_global};
  return x;
}
}  // namespace

VectorXd sparse::JacobiIteration(const ConstraintsList &c, const MatrixXd &M, const VectorXd &rhs, double cfm) {
  return Iterate(c, M, rhs, cfm, EGS_JACOBI);
}
VectorXd sparse::GaussSeidelIteration(const ConstraintsList &c, const MatrixXd &M, const VectorXd &rhs, double cfm) {
  return Iterate(c, M, rhs, cfm, EGS_GAUSS_SEIDEL);
}
VectorXd sparse::SORIteration(const ConstraintsList &c, const MatrixXd &M, const VectorXd &rhs, double cfm) {
  return Iterate(c, M, rhs, cfm, EGS_SOR);
}
sparse::LastSolve sparse::GetLastSolve() { return g_last; }

// ---- the same three on an explicit matrix (sparse_iterations.cc:72-144, 229-267) ----------------
namespace {
VectorXd IterateDense(const MatrixXd &A, const VectorXd &b, const ArrayXb *C, const VectorXd *x_lo, const VectorXd *x_hi, int method) {
  // CHECK(A.rows() == A.cols() && A.rows() == b.size()) (:77): the reference Panics
  if (A.rows() != A.cols() || A.rows() != b.size()) throw egs::Error(EGS_ERR_INVALID, "BaseIteration: A must be square, b of its size");
  if (C && (C->size() != b.size() || x_lo->size() != b.size() || x_hi->size() != b.size()))
    throw egs::Error(EGS_ERR_INVALID, "BaseIteration: C, x_lo, x_hi of b's size");
  const int n = b.size();
  VectorXd x(n);
  if (n == 0) return x;                            // :79-81
  egs_solve_params prm;
  egs_default_params(&prm);                       // omega 1.5, 500 sweeps, tol 1e-9: sparse_iterations.cc:15-19, constants.h:5
  prm.method = method;
  egs_solve_stats st;
  egs_status rc = egs_dense_iterate(egs::DefaultContext(), n, A.data(), b.data(), C ? C->data() : nullptr, C ? x_lo->data() : nullptr,
                                    C ? x_hi->data() : nullptr, &prm, x.data(), &st);
  if (rc != EGS_OK) throw egs::Error(rc, egs_last_error(egs::DefaultContext()));
  g_last = sparse::LastSolve{st.iterations, st.residual, 0, 0, 0};
  return x;
}
}  // namespace
VectorXd sparse::JacobiIteration(const MatrixXd &A, const VectorXd &b) { return IterateDense(A, b, nullptr, nullptr, nullptr, EGS_JACOBI); }
VectorXd sparse::JacobiIteration(const MatrixXd &A, const VectorXd &b, const ArrayXb &C, const VectorXd &lo, const VectorXd &hi) {
  return IterateDense(A, b, &C, &lo, &hi, EGS_JACOBI);
}
VectorXd sparse::GaussSeidelIteration(const MatrixXd &A, const VectorXd &b) { return IterateDense(A, b, nullptr, nullptr, nullptr, EGS_GAUSS_SEIDEL); }
VectorXd sparse::GaussSeidelIteration(const MatrixXd &A, const VectorXd &b, const ArrayXb &C, const VectorXd &lo, const VectorXd &hi) {
  return IterateDense(A, b, &C, &lo, &hi, EGS_GAUSS_SEIDEL);
}
VectorXd sparse::SORIteration(const MatrixXd &A, const VectorXd &b) { return IterateDense(A, b, nullptr, nullptr, nullptr, EGS_SOR); }
VectorXd sparse::SORIteration(const MatrixXd &A, const VectorXd &b, const ArrayXb &C, const VectorXd &lo, const VectorXd &hi) {
  return IterateDense(A, b, &C, &lo, &hi, EGS_SOR);
}

// ---- ... and on many explicit matrices in one library call (egs_dense_iterate_batch) -------------
namespace {
std::vector<VectorXd> IterateDenseBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b, const std::vector<ArrayXb> *C,
                                        const std::vector<VectorXd> *x_lo, const std::vector<VectorXd> *x_hi, int method) {
  const size_t count = A.size();
  if (b.size() != count || (C && (C->size() != count || x_lo->size() != count || x_hi->size() != count)))
    throw egs::Error(EGS_ERR_INVALID, "IterationBatch: one A, b (and C, x_lo, x_hi) per problem");
  std::vector<int32_t> n(count);
  size_t rows = 0, entries = 0;
  for (size_t k = 0; k < count; ++k) {
    // CHECK(A.rows() == A.cols() && A.rows() == b.size()) (:77), per problem
    if (A[k].rows() != A[k].cols() || A[k].rows() != b[k].size()) throw egs::Error(EGS_ERR_INVALID, "BaseIteration: A must be square, b of its size");
    if (C && ((*C)[k].size() != b[k].size() || (*x_lo)[k].size() != b[k].size() || (*x_hi)[k].size() != b[k].size()))
      throw egs::Error(EGS_ERR_INVALID, "BaseIteration: C, x_lo, x_hi of b's size");
    n[k] = b[k].size();
    rows += (size_t)n[k]; entries += (size_t)n[k] * n[k];
  }
  std::vector<double> pA(entries), pb(rows), plo(C ? rows : 0), phi(C ? rows : 0), px(rows);
  std::vector<uint8_t> pC(C ? rows : 0);
  size_t at = 0, vt = 0;
  for (size_t k = 0; k < count; ++k) {
    const size_t nk = (size_t)n[k];
    std::copy(A[k].data(), A[k].data() + nk * nk, pA.begin() + at);
    std::copy(b[k].data(), b[k].data() + nk, pb.begin() + vt);
    if (C) {
      std::copy((*C)[k].data(), (*C)[k].data() + nk, pC.begin() + vt);
      std::copy((*x_lo)[k].data(), (*x_lo)[k].data() + nk, plo.begin() + vt);
      std::copy((*x_hi)[k].data(), (*x_hi)[k].data() + nk, phi.begin() + vt);
    }
    at += nk * nk; vt += nk;
  }
  egs_solve_params prm;
  egs_default_params(&prm);                       // omega 1.5, 500 sweeps, tol 1e-9: sparse_iterations.cc:15-19, constants.h:5
  prm.method = method;
  std::vector<int32_t> its(count);
  std::vector<double> res(count);
  egs_status rc = egs_dense_iterate_batch(egs::DefaultContext(), (int32_t)count, n.data(), pA.data(), pb.data(), C ? pC.data() : nullptr,
                                          C ? plo.data() : nullptr, C ? phi.data() : nullptr, &prm, px.data(), its.data(), res.data(), nullptr);
  if (rc != EGS_OK) throw egs::Error(rc, egs_last_error(egs::DefaultContext()));
  std::vector<VectorXd> x(count);
  vt = 0;
  for (size_t k = 0; k < count; ++k) {
    x[k].resize(n[k]);
    std::copy(px.begin() + vt, px.begin() + vt + n[k], x[k].data());
    vt += (size_t)n[k];
  }
  if (count) g_last = sparse::LastSolve{its[count - 1], res[count - 1], 0, 0, 0};   // of the last problem
  return x;
}
}  // namespace
std::vector<VectorXd> sparse::JacobiIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b) {
  return IterateDenseBatch(A, b, nullptr, nullptr, nullptr, EGS_JACOBI);
}
std::vector<VectorXd> sparse::JacobiIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b, const std::vector<ArrayXb> &C,
                                                   const std::vector<VectorXd> &lo, const std::vector<VectorXd> &hi) {
  return IterateDenseBatch(A, b, &C, &lo, &hi, EGS_JACOBI);
}
std::vector<VectorXd> sparse::GaussSeidelIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b) {
  return IterateDenseBatch(A, b, nullptr, nullptr, nullptr, EGS_GAUSS_SEIDEL);
}
std::vector<VectorXd> sparse::GaussSeidelIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b, const std::vector<ArrayXb> &C,
                                                        const std::vector<VectorXd> &lo, const std::vector<VectorXd> &hi) {
  return IterateDenseBatch(A, b, &C, &lo, &hi, EGS_GAUSS_SEIDEL);
}
std::vector<VectorXd> sparse::SORIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b) {
  return IterateDenseBatch(A, b, nullptr, nullptr, nullptr, EGS_SOR);
}
std::vector<VectorXd> sparse::SORIterationBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b, const std::vector<ArrayXb> &C,
                                                const std::vector<VectorXd> &lo, const std::vector<VectorXd> &hi) {
  return IterateDenseBatch(A, b, &C, &lo, &hi, EGS_SOR);
}

// ---- sparse_iterations_utils.cc:427-695 ------------------------------------------
namespace {
VectorXd Product(const ConstraintsList &constraints, const MatrixXd &M_inverse, const VectorXd &x, int32_t parts,
                 double eps, double scale) {
  if (constraints.empty()) return VectorXd(0);
  Flat f = Flatten(constraints, M_inverse);
  if (x.size() != 3 * f.m) throw egs::Error(EGS_ERR_INVALID, "x size != 3 * constraints");
  VectorXd y(3 * f.m);
  egs::check(egs_matvec_blocks(egs::DefaultContext(), f.n, f.Minv.data(), f.m, f.body0.data(), f.body1.data(), f.J0.data(),
                               f.J1.data(), parts, eps, scale, EGS_F64, x.data(), y.data()));
  return y;
}
}  // namespace

VectorXd sparse::CalculateSparseDx(const ConstraintsList &c, const MatrixXd &M, const VectorXd &x, double epsilon, double scale) {
  return Product(c, M, x, EGS_MV_DIAG, epsilon, scale);
}
VectorXd sparse::CalculateSparseLx(const ConstraintsList &c, const MatrixXd &M, const VectorXd &x, double, double) {
  return Product(c, M, x, EGS_MV_LOWER, 0.0, 1.0);   // epsilon / scale unused (sparse_iterations_utils.h:69-71)
}
VectorXd sparse::CalculateSparseUx(const ConstraintsList &c, const MatrixXd &M, const VectorXd &x, double, double) {
  return Product(c, M, x, EGS_MV_UPPER, 0.0, 1.0);
}
VectorXd sparse::CalculateSparseLxUx(const ConstraintsList &c, const MatrixXd &M, const VectorXd &x, double, double) {
  return Product(c, M, x, EGS_MV_LOWER | EGS_MV_UPPER, 0.0, 1.0);
}
VectorXd sparse::CalculateSparseLxDx(const ConstraintsList &c, const MatrixXd &M, const VectorXd &x, double eps, double scale) {
  return Product(c, M, x, EGS_MV_LOWER | EGS_MV_DIAG, eps, scale);
}
VectorXd sparse::CalculateSparseUxDx(const ConstraintsList &c, const MatrixXd &M, const VectorXd &x, double eps, double scale) {
  return Product(c, M, x, EGS_MV_UPPER | EGS_MV_DIAG, eps, scale);
}
VectorXd sparse::CalculateSparseJMJtX(const ConstraintsList &c, const MatrixXd &M, const VectorXd &x, double eps) {
  return Product(c, M, x, EGS_MV_FULL, eps, 1.0);
}

void sparse::ConstructMixedConstraints(const ConstraintsList &constraints, ArrayXb *C, VectorXd *x_lo,
                                       VectorXd *x_hi) {  // sparse_iterations_utils.cc:697-720
  const int m = (int)constraints.size();
  C->resize(3 * m); x_lo->resize(3 * m); x_hi->resize(3 * m);
  for (int i = 0; i < m; ++i) {
    MatrixXd j0, j1; ArrayXb ct; VectorXd lo, hi;
    constraints[i]->ComputeJ(&j0, &j1, &ct, &lo, &hi);
    for (int r = 0; r < 3; ++r) { (*C)(3 * i + r) = ct(r); (*x_lo)(3 * i + r) = lo(r); (*x_hi)(3 * i + r) = hi(r); }
  }
}

bool Lcp::MixedConstraintsSolver(const MatrixXd &A, const VectorXd &b, const ArrayXb &C, const VectorXd &x_lo,
                                 const VectorXd &x_hi, VectorXd &x, VectorXd &w) {  // lcp.cc:276-336
  const int N = b.size();
  if (A.rows() != N || A.cols() != N || C.size() != N) throw egs::Error(EGS_ERR_INVALID, "dimension mismatch");
  x.resize(N); w.resize(N);
  int32_t ok = 0, pivots = 0;
  egs_status st = egs_mixed_constraints_solve(egs::DefaultContext(), N, A.data(), b.data(), C.data(), x_lo.data(),
                                              x_hi.data(), /*use_bounds=*/0, x.data(), w.data(), &ok, &pivots);
  if (st != EGS_OK && st != EGS_ERR_LCP_FAILED) egs::check(st);
  return ok != 0;
}

std::vector<bool> Lcp::MixedConstraintsSolverBatch(const std::vector<MatrixXd> &A, const std::vector<VectorXd> &b,
                                                   const std::vector<ArrayXb> &C, const std::vector<VectorXd> &x_lo,
                                                   const std::vector<VectorXd> &x_hi, std::vector<VectorXd> *x,
                                                   std::vector<VectorXd> *w) {  // lcp.cc:276-336, per problem
  const size_t count = A.size();
  if (!x || !w || b.size() != count || C.size() != count || x_lo.size() != count || x_hi.size() != count)
    throw egs::Error(EGS_ERR_INVALID, "MixedConstraintsSolverBatch: one A, b, C, x_lo and x_hi per problem");
  std::vector<int32_t> n(count);
  size_t rows = 0, entries = 0;
  for (size_t k = 0; k < count; ++k) {
    const auto N = b[k].size();
    if (A[k].rows() != N || A[k].cols() != N || C[k].size() != N || x_lo[k].size() != N || x_hi[k].size() != N)
      throw egs::Error(EGS_ERR_INVALID, "MixedConstraintsSolverBatch: dimension mismatch");
    n[k] = (int32_t)N;
    rows += (size_t)N; entries += (size_t)N * N;
  }
  std::vector<double> pA(entries), pb(rows), plo(rows), phi(rows), px(rows), pw(rows);
  std::vector<uint8_t> pC(rows);
  size_t at = 0, vt = 0;
  for (size_t k = 0; k < count; ++k) {
    const size_t nk = (size_t)n[k];
    std::copy(A[k].data(), A[k].data() + nk * nk, pA.begin() + at);
    std::copy(b[k].data(), b[k].data() + nk, pb.begin() + vt);
    std::copy(C[k].data(), C[k].data() + nk, pC.begin() + vt);
    std::copy(x_lo[k].data(), x_lo[k].data() + nk, plo.begin() + vt);
    std::copy(x_hi[k].data(), x_hi[k].data() + nk, phi.begin() + vt);
    at += nk * nk; vt += nk;
  }
  std::vector<int32_t> ok(count), pivots(count);
  egs::check(egs_mixed_constraints_solve_batch(egs::DefaultContext(), (int32_t)count, n.data(), pA.data(), pb.data(), pC.data(),
                                               plo.data(), phi.data(), /*use_bounds=*/0, /*max_pivots=*/0, px.data(), pw.data(),
                                               ok.data(), pivots.data()));
  x->assign(count, VectorXd());
  w->assign(count, VectorXd());
  std::vector<bool> good(count);
  vt = 0;
  for (size_t k = 0; k < count; ++k) {
    (*x)[k].resize(n[k]); (*w)[k].resize(n[k]);
    std::copy(px.begin() + vt, px.begin() + vt + n[k], (*x)[k].data());
    std::copy(pw.begin() + vt, pw.begin() + vt + n[k], (*w)[k].data());
    good[k] = ok[k] != 0;
    vt += (size_t)n[k];
  }
  return good;
}

// ---- ensembles.cc ----------------------------------------------------------
Ensemble::Ensemble() {
  egs_default_params(&solver_params);
  solver_params.method = EGS_SOR;
}
Ensemble::~Ensemble() {
  if (problem_) egs_problem_destroy(problem_);
  if (world_) egs_world_destroy(world_);
}

void Ensemble::Init() {  // ensembles.cc:24-29
  if (live_world_ == world_) live_world_ = nullptr;
  if (world_) { egs_world_destroy(world_); world_ = nullptr; }   // M^-1 / f_ext are re-sent to a fresh world
  ray_pose_.clear(); world_rays_.clear();                        // ... which holds no rays and no poses yet
  ConstructMassInertiaMatrixInverse();
  InitializeExternalForceTorqueVector();
  VectorXd err = ComputePositionConstraintError();  // CheckInitialConditions, :224-232
  for (int k = 0; k < err.size(); ++k)
    if (!(std::fabs(err(k)) <= 1e-9)) throw egs::Error(EGS_ERR_INVALID, "Check initial conditions failed.");
  CheckAndCorrectEnsembleState();                   // ensembles.cc:28
}

void Ensemble::ConstructMassInertiaMatrixInverse() {  // ensembles.cc:202-212
  M_inverse_ = MatrixXd::Zero(n_ * 6, n_ * 6);
  for (int i = 0; i < n_; ++i) {
    const auto &b = components_.at(i);
    Matrix3d Iinv = b->I_g().inverse();
    for (int k = 0; k < 3; ++k) M_inverse_(6 * i + k, 6 * i + k) = 1.0 / b->m();
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) M_inverse_(6 * i + 3 + r, 6 * i + 3 + c) = Iinv(r, c);
  }
}

void Ensemble::InitializeExternalForceTorqueVector() {  // ensembles.cc:214-222
  external_force_torque_ = VectorXd::Zero(n_ * 6);
  const Vector3d g(0, 0, -9.8);  // constants.h:8
  for (int i = 0; i < n_; ++i) {
    const auto &b = components_.at(i);
    Vector3d tq = ((-1.0 * CrossMat(b->w_g())) * b->I_g()) * b->w_g();
    for (int k = 0; k < 3; ++k) {
      external_force_torque_(6 * i + k) = b->m() * g[k];
      external_force_torque_(6 * i + 3 + k) = tq[k];
    }
  }
}

// ---- live inertia (SetLiveInertia) ------------------------------------------------------------------------------------
bool Ensemble::IsMultipleOfIdentity(const Matrix3d &I) {   // the device's skip rule (egs_problem_set_live_inertia)
  return I.d[1] == 0 && I.d[2] == 0 && I.d[3] == 0 && I.d[5] == 0 && I.d[6] == 0 && I.d[7] == 0 && I.d[0] == I.d[4] &&
         I.d[0] == I.d[8];
}

std::vector<double> Ensemble::BodyInertias() const {
  std::vector<double> Ib((size_t)n_ * 9);
  for (int i = 0; i < n_; ++i)
    for (int k = 0; k < 9; ++k) Ib[(size_t)i * 9 + k] = components_[i]->I_b().d[k];
  return Ib;
}

void Ensemble::RefreshLiveMassOnHost() {   // what the device's refresh does, by the code of Init() (ensembles.cc:202-222)
  for (int i = 0; i < n_; ++i) {
    const auto &b = components_.at(i);
    if (IsMultipleOfIdentity(b->I_b())) continue;
    Matrix3d Iinv = b->I_g().inverse();
    Vector3d tq = ((-1.0 * CrossMat(b->w_g())) * b->I_g()) * b->w_g();
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) M_inverse_(6 * i + 3 + r, 6 * i + 3 + c) = Iinv(r, c);
      external_force_torque_(6 * i + 3 + r) = tq[r];
    }
  }
}

void Ensemble::PullLiveMass() const {
  if (!live_inertia_ || !live_world_) return;
  std::vector<double> Minv((size_t)live_total_ * 36), fext((size_t)live_total_ * 6);
  egs::check(egs_world_get_mass(live_world_, Minv.data(), fext.data()));
  for (int i = 0; i < n_; ++i) {
    const size_t g = (size_t)(live_offset_ + i);
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) M_inverse_(6 * i + r, 6 * i + c) = Minv[g * 36 + 6 * r + c];
      external_force_torque_(6 * i + r) = fext[g * 6 + r];
    }
  }
}

void Ensemble::SetLiveInertia(bool on) {
  if (!on && live_inertia_) PullLiveMass();   // frozen from here on at what the last step used
  live_inertia_ = on;
  if (!on) live_world_ = nullptr;
}

ConstraintsList Ensemble::CombineConstraintsLists() const {  // ensembles.cc:234-239
  ConstraintsList c;
  c.insert(c.end(), joints_.begin(), joints_.end());
  c.insert(c.end(), contacts_.begin(), contacts_.end());
  return c;
}

VectorXd Ensemble::ComputePositionConstraintError() const {  // ensembles.cc:156-171
  ConstraintsList cs = CombineConstraintsLists();
  VectorXd e(3 * (int)cs.size());
  for (size_t i = 0; i < cs.size(); ++i) {
    VectorXd ei = cs[i]->ComputeError();
    for (int k = 0; k < 3; ++k) e(3 * (int)i + k) = ei(k);
  }
  return e;
}

const VectorXd Ensemble::GetVelocities() const {  // ensembles.cc:429-436
  VectorXd v(n_ * 6);
  for (int i = 0; i < n_; ++i)
    for (int k = 0; k < 3; ++k) { v(6 * i + k) = components_[i]->v()[k]; v(6 * i + 3 + k) = components_[i]->w_g()[k]; }
  return v;
}

void Ensemble::UpdateComponentsVelocities(const VectorXd &v) {  // ensembles.cc:438-443
  for (int i = 0; i < n_; ++i) {
    components_[i]->SetV(Vector3d(v(6 * i), v(6 * i + 1), v(6 * i + 2)));
    components_[i]->SetW_GlobalFrame(Vector3d(v(6 * i + 3), v(6 * i + 4), v(6 * i + 5)));
  }
}

// ensembles.cc:563-575 with the sparse switch on.  If every constraint can
// describe itself the whole velocity step (assembly, rhs, solve, v update) runs
// on the GPU (entry 2); otherwise ComputeJ is flattened on the host (entry 1).
VectorXd Ensemble::StepVelocities_ODE(double dt, const VectorXd &v, double erp) {
  ConstraintsList cs = CombineConstraintsLists();
  const int m = (int)cs.size();
  if (m == 0) {  // ensembles.cc:504-505: v_dot = M^-1 f
    VectorXd v_new(n_ * 6);
    for (int i = 0; i < n_; ++i)
      for (int r = 0; r < 6; ++r) {
        double s = 0;
        for (int c = 0; c < 6; ++c) s += M_inverse_(6 * i + r, 6 * i + c) * external_force_torque_(6 * i + c);
        v_new(6 * i + r) = v(6 * i + r) + dt * s;
      }
    UpdateComponentsVelocities(v_new);
    return v_new;
  }
  std::vector<int32_t> kind(m), b0(m), b1(m);
  std::vector<double> data((size_t)m * 7);
  bool describable = true;
  for (int i = 0; i < m; ++i) {
    b0[i] = cs[i]->i0_; b1[i] = cs[i]->i1_;
    describable = describable && cs[i]->Describe(&kind[i], &data[(size_t)i * 7]);
  }
  egs_solve_params prm = solver_params;
  prm.cfm = cfm_coeff;
  VectorXd v_new(n_ * 6);
  if (describable) {
    if (!problem_ || b0 != plan_b0_ || b1 != plan_b1_) {  // re-plan only when the contact topology changed
      if (problem_) egs_problem_destroy(problem_);
      problem_ = nullptr;
      egs::check(egs_problem_create(egs::DefaultContext(), n_, m, b0.data(), b1.data(), EGS_F64, &problem_));
      plan_b0_ = b0; plan_b1_ = b1;
      problem_friction_ = false;
      problem_restitution_ = false;
    }
    std::vector<double> pos((size_t)n_ * 3), R((size_t)n_ * 9), vl((size_t)n_ * 3), w((size_t)n_ * 3), Minv((size_t)n_ * 36);
    for (int i = 0; i < n_; ++i) {
      for (int k = 0; k < 3; ++k) { pos[3 * i + k] = components_[i]->p()[k]; vl[3 * i + k] = v(6 * i + k); w[3 * i + k] = v(6 * i + 3 + k); }
      for (int k = 0; k < 9; ++k) R[9 * i + k] = components_[i]->R().d[k];
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) Minv[(size_t)i * 36 + 6 * r + c] = M_inverse_(6 * i + r, 6 * i + c);
    }
    egs::check(egs_problem_set_state(problem_, pos.data(), R.data(), vl.data(), w.data(), Minv.data(), external_force_torque_.data()));
    egs::check(egs_problem_set_constraints(problem_, kind.data(), data.data()));
    bool hinges = false;
    for (int i = 0; i < m; ++i) hinges = hinges || kind[i] == EGS_JOINT_HINGE_AXIS || kind[i] == EGS_JOINT_SLIDER_AXIS;   // (a slider's rail row likewise)
    if (hinges) {   // the joints come first in cs: their motors, then no motor for the contacts
      std::vector<double> motor;
      if (JointMotors(joints_, &motor)) {
        motor.resize(2 * (size_t)m, -1.0);
        egs::check(egs_problem_set_motors(problem_, motor.data()));
      }
      std::vector<double> lim;
      if (JointLimits(joints_, &lim)) {   // likewise their limit rows, zeros for the contacts
        lim.resize(8 * (size_t)m, 0.0);
        egs::check(egs_problem_set_hinge_limits(problem_, lim.data()));
      }
      std::vector<double> travel;
      if (JointTravel(joints_, &travel)) {   // ... and the sliders' stops, (-inf, +inf) for the contacts
        travel.resize(2 * (size_t)m, INFINITY);
        for (size_t i = joints_.size(); i < (size_t)m; ++i) travel[2 * i] = -INFINITY;
        egs::check(egs_problem_set_slider_limits(problem_, travel.data()));
      }
    }
    if (restitution_ >= 0) {   // every contact the coefficient, every joint -1
      std::vector<double> rest((size_t)m);
      for (int i = 0; i < m; ++i) rest[i] = kind[i] == EGS_CONTACT_BOX ? restitution_ : -1.0;
      egs::check(egs_problem_set_restitution(problem_, rest.data(), restitution_vth_));
      problem_restitution_ = true;
    } else if (problem_restitution_) {
      egs::check(egs_problem_set_restitution(problem_, nullptr, 0.0));
      problem_restitution_ = false;
    }
    egs_solve_stats st;
    if (use_dense_solver) {   // ComputeVDot (ensembles.cc:498-538) on the device
      const bool pyramid = friction_model_ == Contact::FrictionModel::COULOMB_PYRAMID;   // (Step let it through: SetDenseFriction)
      if (pyramid) {   // every contact its coefficient, every joint -1
        std::vector<double> mu((size_t)m);
        for (int i = 0; i < m; ++i) mu[i] = dynamic_cast<const Contact *>(cs[i].get()) ? friction_mu_ : -1.0;
        egs::check(egs_problem_set_friction(problem_, mu.data()));
        problem_friction_ = true;
      } else if (problem_friction_) {
        egs::check(egs_problem_set_friction(problem_, nullptr));
        problem_friction_ = false;
      }
      egs::check(egs_problem_set_dense_friction(problem_, dense_fric_outer_, dense_fric_tol_));
      egs::check(egs_problem_assemble(problem_, dt, erp));
      egs::check(egs_problem_dense_condition(problem_, 0.0, &last_condition_estimate));
      const double cfm = last_condition_estimate < 1e7 ? 0.0 : cfm_coeff;   // kGoodConditionNumber, constants.h:12
      int32_t ok = 0, pivots = 0;
      // a hinge's axis row is a box row: an ensemble that holds one steps with the stored bounds
      egs_status rc = egs_problem_step_dense(problem_, dt, erp, cfm, /*use_bounds=*/dense_fric_outer_ > 0 || hinges ? 1 : 0, &ok, &pivots);
      if (rc != EGS_OK || !ok)   // the reference Panics here (ensembles.cc:531-534)
        throw egs::Error(rc != EGS_OK ? rc : EGS_ERR_LCP_FAILED,
                         rc == EGS_ERR_INVALID || rc == EGS_ERR_UNSUPPORTED ? egs_last_error(egs::DefaultContext())
                                               : "Lcp::MixedConstraintsSolver exited without reaching a solution.");
      last_dense_outer = 1; last_dense_converged = true;
      if (pyramid) {
        int32_t outer = 0, conv = 0;
        egs::check(egs_problem_dense_friction_info(problem_, &outer, &conv, nullptr));
        last_dense_outer = outer; last_dense_converged = conv != 0;
      }
    } else
    egs::check(egs_problem_step(problem_, dt, erp, &prm, &st));
    last_lambda.resize(3 * m);
    egs::check(egs_problem_get_lambda(problem_, last_lambda.data()));
    egs::check(egs_problem_get_velocity(problem_, v_new.data()));
  } else {
    if (restitution_ >= 0)
      throw egs::Error(EGS_ERR_UNSUPPORTED, "SetRestitution takes effect where the device assembles: not with a "
                                            "constraint the device cannot describe");
    Flat f = Flatten(cs, M_inverse_);
    VectorXd err = ComputePositionConstraintError();
    VectorXd rhs(3 * m);
    const double k = -erp / dt / dt;
    auto u_of = [&](int b, double *u) {
      for (int r = 0; r < 6; ++r) {
        double s = 0;
        for (int c = 0; c < 6; ++c) s += M_inverse_(6 * b + r, 6 * b + c) * external_force_torque_(6 * b + c);
        u[r] = v(6 * b + r) / dt + s;
      }
    };
    for (int i = 0; i < m; ++i) {
      double u0[6] = {0}, u1[6] = {0};
      if (f.body0[i] >= 0) u_of(f.body0[i], u0);
      if (f.body1[i] >= 0) u_of(f.body1[i], u1);
      for (int r = 0; r < 3; ++r) {
        double ju = 0;
        for (int c = 0; c < 6; ++c) ju += f.J0[(size_t)i * 18 + 6 * r + c] * u0[c] + f.J1[(size_t)i * 18 + 6 * r + c] * u1[c];
        rhs(3 * i + r) = k * err(3 * i + r) - ju;
      }
    }
    egs_solve_stats st;
    last_lambda.resize(3 * m);
    egs::check(egs_solve_blocks(egs::DefaultContext(), f.n, f.Minv.data(), f.m, f.body0.data(), f.body1.data(), f.J0.data(),
                                f.J1.data(), f.is_eq.data(), f.lo.data(), f.hi.data(), rhs.data(), &prm, EGS_F64,
                                last_lambda.data(), &st));
    std::vector<double> g((size_t)n_ * 6);
    for (int i = 0; i < n_ * 6; ++i) g[i] = external_force_torque_(i);
    for (int i = 0; i < m; ++i)
      for (int side = 0; side < 2; ++side) {
        const int b = side ? f.body1[i] : f.body0[i];
        if (b < 0) continue;
        const double *J = (side ? f.J1.data() : f.J0.data()) + (size_t)i * 18;
        for (int c = 0; c < 6; ++c)
          for (int r = 0; r < 3; ++r) g[(size_t)b * 6 + c] += J[6 * r + c] * last_lambda(3 * i + r);
      }
    for (int b = 0; b < n_; ++b)
      for (int r = 0; r < 6; ++r) {
        double s = 0;
        for (int c = 0; c < 6; ++c) s += M_inverse_(6 * b + r, 6 * b + c) * g[(size_t)b * 6 + c];
        v_new(6 * b + r) = v(6 * b + r) + dt * s;
      }
  }
  UpdateComponentsVelocities(v_new);
  return v_new;
}

void Ensemble::StepPositions_ODE(double dt, const VectorXd &v, const VectorXd &v_new) {  // ensembles.cc:577-591
  for (int i = 0; i < n_; ++i) {
    Vector3d vm, wm;
    for (int k = 0; k < 3; ++k) { vm[k] = (v(6 * i + k) + v_new(6 * i + k)) / 2.0; wm[k] = (v(6 * i + 3 + k) + v_new(6 * i + 3 + k)) / 2.0; }
    components_[i]->SetP(components_[i]->p() + dt * vm);
    components_[i]->SetR(WtoR(wm, dt) * components_[i]->R());
  }
}

std::vector<int32_t> Ensemble::Shapes() const {
  std::vector<int32_t> shape;
  for (int i = 0; i < n_; ++i)
    if (components_[i]->type() != Body::BodyType::Box) {
      if (shape.empty()) shape.assign((size_t)n_, EGS_SHAPE_BOX);
      shape[(size_t)i] = components_[i]->type() == Body::BodyType::Sphere ? EGS_SHAPE_SPHERE : EGS_SHAPE_CAPSULE;
    }
  return shape;
}

void Ensemble::UpdateContacts() {  // ensembles.cc:445-480 (+ :308-328)
  contacts_.clear();
  if (n_ == 0) return;
  std::vector<double> pos((size_t)n_ * 3), R((size_t)n_ * 9), side((size_t)n_ * 3);
  for (int i = 0; i < n_; ++i) {
    const Vector3d sl = components_[i]->GetSideLengths();
    for (int k = 0; k < 3; ++k) { pos[3 * i + k] = components_[i]->p()[k]; side[3 * i + k] = sl[k]; }
    for (int k = 0; k < 9; ++k) R[9 * i + k] = components_[i]->R().d[k];
  }
  const int cap = 64 * n_ + 64;
  std::vector<int32_t> b0(cap), b1(cap);
  std::vector<double> data((size_t)cap * 7);
  int32_t m = 0;
  // The reference's Step prunes right after detection (CheckAndCorrectEnsembleState, ensembles.cc:394):
  // contact-vs-contact always, joint-vs-contact for the joints between the same two components.  Joints
  // that can describe themselves are pruned against on the device, the others on the host below.
  std::vector<int32_t> jb0, jb1;
  std::vector<double> jdata;
  std::vector<std::shared_ptr<Joint>> host_joints;
  for (const auto &j : joints_) {
    if (j->i0_ < 0 || j->i1_ < 0) continue;   // the pair scan never visits the ground (quirk Q4)
    if (!j->HasPosition()) continue;          // an angular block prunes nothing
    int32_t kind = 0;
    double d7[7];
    if (j->Describe(&kind, d7)) { jb0.push_back(j->i0_); jb1.push_back(j->i1_); jdata.insert(jdata.end(), d7, d7 + 7); }
    else host_joints.push_back(j);
  }
  const std::vector<int32_t> shape = Shapes();   // empty: all boxes, egs_update_contacts_joints itself
  egs::check(egs_update_contacts_shapes(egs::DefaultContext(), n_, pos.data(), R.data(), side.data(), (int32_t)jb0.size(),
                                        jb0.data(), jb1.data(), jdata.data(), shape.empty() ? nullptr : shape.data(), cap, &m,
                                        b0.data(), b1.data(), data.data()));
  for (int k = 0; k < m; ++k) {
    const double *d = &data[(size_t)k * 7];
    ContactGeometry cg(Vector3d(d[0], d[1], d[2]), Vector3d(d[3], d[4], d[5]), d[6]);
    bool keep = true;
    for (const auto &j : host_joints) {        // ensembles.cc:296-306, kMinConstraintDistance = 1e-6
      const bool same_pair = (j->i0_ == b0[k] && j->i1_ == b1[k]) || (j->i0_ == b1[k] && j->i1_ == b0[k]);
      if (same_pair && (j->GetConstraintPosition() - cg.position).norm() < 1e-6) keep = false;
    }
    if (!keep) continue;
    if (b0[k] < 0) contacts_.push_back(std::make_shared<Contact>(components_[b1[k]], b1[k], cg));
    else contacts_.push_back(std::make_shared<Contact>(components_[b0[k]], b0[k], components_[b1[k]], b1[k], cg));
  }
}

namespace {

// pos [n][3] | R [n][9] of the components, the layout of ray_pose_
void AppendPose(const ComponentsList &cs, std::vector<double> *pos, std::vector<double> *R) {
  for (const auto &c : cs) {
    for (int k = 0; k < 3; ++k) pos->push_back(c->p()[k]);
    for (int k = 0; k < 9; ++k) R->push_back(c->R().d[k]);
  }
}

bool SamePose(const std::vector<double> &kept, const std::vector<double> &pos, const std::vector<double> &R) {
  return !kept.empty() && kept.size() == pos.size() + R.size() &&
         std::memcmp(kept.data(), pos.data(), pos.size() * sizeof(double)) == 0 &&
         std::memcmp(kept.data() + pos.size(), R.data(), R.size() * sizeof(double)) == 0;
}

// the arrays of the ray entries; body_offset shifts the attached rays' indices (a group's world)
struct RayArrays {
  std::vector<double> origin, dir, tmax;
  std::vector<int32_t> body;
  void Add(const Ray &r, int body_offset) {
    for (int k = 0; k < 3; ++k) { origin.push_back(r.origin[k]); dir.push_back(r.dir[k]); }
    tmax.push_back(r.tmax);
    body.push_back(r.body >= 0 ? r.body + body_offset : r.body);
  }
  // one flat key: the table a world holds is sent again only when this changes
  std::vector<double> Key(const std::vector<int32_t> *ens = nullptr) const {
    std::vector<double> k(origin);
    k.insert(k.end(), dir.begin(), dir.end());
    k.insert(k.end(), tmax.begin(), tmax.end());
    k.insert(k.end(), body.begin(), body.end());
    if (ens) k.insert(k.end(), ens->begin(), ens->end());
    return k;
  }
};

bool SameKey(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

// The hit of ray r in its ensemble's numbering; the point from the world-frame ray, formed as the device forms it.
RayHit MakeHit(const Ray &r, const ComponentsList &cs, int32_t body, int body_offset, double t, const double *n) {
  Vector3d o = r.origin, d = r.dir;
  if (r.body >= 0) {
    const Matrix3d &R = cs[(size_t)r.body]->R();
    const Vector3d c = cs[(size_t)r.body]->p();
    o = Vector3d(c[0] + ((R.d[0] * r.origin[0] + R.d[1] * r.origin[1]) + R.d[2] * r.origin[2]),
                 c[1] + ((R.d[3] * r.origin[0] + R.d[4] * r.origin[1]) + R.d[5] * r.origin[2]),
                 c[2] + ((R.d[6] * r.origin[0] + R.d[7] * r.origin[1]) + R.d[8] * r.origin[2]));
    d = Vector3d((R.d[0] * r.dir[0] + R.d[1] * r.dir[1]) + R.d[2] * r.dir[2], (R.d[3] * r.dir[0] + R.d[4] * r.dir[1]) + R.d[5] * r.dir[2],
                 (R.d[6] * r.dir[0] + R.d[7] * r.dir[1]) + R.d[8] * r.dir[2]);
  }
  RayHit h;
  h.body = body >= 0 ? body - body_offset : body;
  h.t = t;
  h.normal = Vector3d(n[0], n[1], n[2]);
  h.point = body == -2 ? o : Vector3d(o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]);
  return h;
}

}  // namespace

std::vector<RayHit> Ensemble::CastRays(const std::vector<Ray> &rays) {
  const size_t nr = rays.size();
  std::vector<RayHit> out;
  if (nr == 0) return out;
  RayArrays a;
  for (const Ray &r : rays) {
    if (r.body < -1 || r.body >= n_) throw egs::Error(EGS_ERR_INVALID, "Ensemble::CastRays: a ray's body is not a component");
    a.Add(r, 0);
  }
  std::vector<double> pos, R;
  AppendPose(components_, &pos, &R);
  std::vector<int32_t> hit(nr);
  std::vector<double> t(nr), normal(3 * nr);
  if (world_ && SamePose(ray_pose_, pos, R)) {   // the device holds these very poses: nothing but the rays goes up
    const std::vector<double> key = a.Key();
    if (!SameKey(key, world_rays_)) {
      world_rays_.clear();
      egs::check(egs_world_set_rays(world_, (int32_t)nr, nullptr, a.body.data(), a.origin.data(), a.dir.data(), a.tmax.data()));
      world_rays_ = key;
    }
    int32_t got = 0;
    egs::check(egs_world_cast_rays(world_, (int32_t)nr, &got, hit.data(), t.data(), normal.data()));
  } else {
    std::vector<double> side;
    for (const auto &c : components_) {
      const Vector3d sl = c->GetSideLengths();
      for (int k = 0; k < 3; ++k) side.push_back(sl[k]);
    }
    const std::vector<int32_t> shape = Shapes();
    egs::check(egs_cast_rays(egs::DefaultContext(), n_, pos.data(), R.data(), side.data(), shape.empty() ? nullptr : shape.data(),
                             (int32_t)nr, a.body.data(), a.origin.data(), a.dir.data(), a.tmax.data(), hit.data(), t.data(),
                             normal.data()));
  }
  for (size_t i = 0; i < nr; ++i) out.push_back(MakeHit(rays[i], components_, hit[i], 0, t[i], &normal[3 * i]));
  return out;
}

RayHit Ensemble::CastRay(const Vector3d &origin, const Vector3d &dir, double tmax) {
  Ray r;
  r.origin = origin; r.dir = dir; r.tmax = tmax;
  return CastRays({r})[0];
}

// ensembles.cc:241-329.  UpdateContacts already returns a pruned contact list (the device does the
// contact-vs-contact and joint-vs-contact passes in the reference's order), so what is left for
// caller-supplied contacts (SetContacts) is the same scan on the host, and the joint-vs-joint check.
void Ensemble::CheckAndCorrectEnsembleState() {
  if (M_inverse_.rows() != 6 * n_ || M_inverse_.cols() != 6 * n_) throw egs::Error(EGS_ERR_INVALID, "M_inverse_ dimensions are incorrect.");
  if (external_force_torque_.size() != 6 * n_) throw egs::Error(EGS_ERR_INVALID, "external_force_torque_ dimensions are incorrect.");
  auto key_of = [](int a, int b) { return a < b ? std::make_pair(a, b) : std::make_pair(b, a); };
  auto close = [](const Constraint &c1, const Constraint &c2) {   // CheckConstraintPair, ensembles.cc:376-388
    if (!c1.HasPosition() || !c2.HasPosition()) return false;      // an angular block is close to nothing
    return (c1.GetConstraintPosition() - c2.GetConstraintPosition()).norm() < 1e-6;
  };
  // joint vs joint: conflict or overconstraint -> the reference Panics (ensembles.cc:280-289)
  for (size_t a = 0; a < joints_.size(); ++a)
    for (size_t b = a + 1; b < joints_.size(); ++b) {
      if (joints_[a]->i0_ < 0 || joints_[a]->i1_ < 0) continue;   // pairs 0 <= i < j only (quirk Q4)
      if (key_of(joints_[a]->i0_, joints_[a]->i1_) != key_of(joints_[b]->i0_, joints_[b]->i1_)) continue;
      if (close(*joints_[a], *joints_[b]))
        throw egs::Error(EGS_ERR_INVALID, "Joint constraints between components " + std::to_string(key_of(joints_[a]->i0_, joints_[a]->i1_).first) +
                                              " and " + std::to_string(key_of(joints_[a]->i0_, joints_[a]->i1_).second) +
                                              " conflict or cause overconstraint.");
    }
  // joint vs contact, then contact vs contact (the later one goes), pair by pair (the reference's
  // pairwise maps, ensembles.cc:331-374); erased in descending order
  std::map<std::pair<int, int>, std::vector<int>> pair_joints, pair_contacts;
  for (size_t j = 0; j < joints_.size(); ++j)
    if (joints_[j]->i0_ >= 0 && joints_[j]->i1_ >= 0) pair_joints[key_of(joints_[j]->i0_, joints_[j]->i1_)].push_back((int)j);
  for (size_t c = 0; c < contacts_.size(); ++c)
    if (contacts_[c]->i0_ >= 0 && contacts_[c]->i1_ >= 0) pair_contacts[key_of(contacts_[c]->i0_, contacts_[c]->i1_)].push_back((int)c);
  std::vector<char> drop(contacts_.size(), 0);
  for (const auto &pc : pair_contacts) {
    const auto pj = pair_joints.find(pc.first);
    for (size_t a = 0; a < pc.second.size(); ++a) {
      const int c = pc.second[a];
      if (pj != pair_joints.end())
        for (int j : pj->second) if (close(*joints_[j], *contacts_[c])) drop[c] = 1;
      for (size_t e = 0; e < a; ++e)   // every earlier contact of the pair takes part, dropped or not (ensembles.cc:308-322)
        if (close(*contacts_[pc.second[e]], *contacts_[c])) drop[c] = 1;
    }
  }
  for (size_t c = contacts_.size(); c-- > 0;)
    if (drop[c]) contacts_.erase(contacts_.begin() + (long)c);
}

// The whole Step through egs_world (include/eggshell_amd.h): possible when every
// permanent constraint can describe itself (ball joints) -- contacts always can.
// Body objects are the interface, so their state is pushed before and pulled
// after the step; inside the step nothing but the contact topology leaves the GPU.
void Ensemble::SetWarmStart(bool on, double match_radius) {
  if (on && !(match_radius >= 0)) throw egs::Error(EGS_ERR_INVALID, "SetWarmStart: match_radius must be >= 0");
  warm_start_ = on;
  warm_radius_ = on ? match_radius : 0.0;
}

void Ensemble::SetFriction(Contact::FrictionModel model, double mu) {
  if (model != Contact::FrictionModel::BOX && model != Contact::FrictionModel::COULOMB_PYRAMID)
    throw egs::Error(EGS_ERR_UNSUPPORTED, "SetFriction: NO_FRICTION and INFINITE have empty bodies in the reference (contact.cc:150-152) "
                                          "and are not built; BOX and COULOMB_PYRAMID are");
  if (model == Contact::FrictionModel::COULOMB_PYRAMID && !(mu >= 0))
    throw egs::Error(EGS_ERR_INVALID, "SetFriction: COULOMB_PYRAMID needs mu >= 0");
  friction_model_ = model;
  friction_mu_ = model == Contact::FrictionModel::COULOMB_PYRAMID ? mu : 0.0;
}

void Ensemble::SetRestitution(double e, double threshold) {
  if (e != e || std::isinf(e)) throw egs::Error(EGS_ERR_INVALID, "SetRestitution: e must be finite");
  if (!(threshold >= 0) || std::isinf(threshold))
    throw egs::Error(EGS_ERR_INVALID, "SetRestitution: threshold must be finite and >= 0");
  restitution_ = e >= 0 ? e : -1.0;
  restitution_vth_ = threshold;
}

void Ensemble::SetDenseFriction(int max_outer, double tol) {
  if (max_outer < 0) throw egs::Error(EGS_ERR_INVALID, "SetDenseFriction: max_outer must be >= 0");
  if (!(tol >= 0)) throw egs::Error(EGS_ERR_INVALID, "SetDenseFriction: tol must be >= 0");
  dense_fric_outer_ = max_outer;
  dense_fric_tol_ = max_outer > 0 ? tol : 0.0;
}

bool Ensemble::StepOnDevice(double dt) {
  if (!use_device_step || use_dense_solver) return false;
  const int mj = (int)joints_.size();
  std::vector<int32_t> jb0(mj), jb1(mj), jkind(mj);
  std::vector<double> jdata((size_t)mj * 7), jmotor, jlimit, jtravel;
  for (int i = 0; i < mj; ++i) {
    jb0[i] = joints_[i]->i0_; jb1[i] = joints_[i]->i1_;
    if (!joints_[i]->Describe(&jkind[i], &jdata[(size_t)i * 7])) return false;
  }
  const bool motors = JointMotors(joints_, &jmotor);
  if (!JointLimits(joints_, &jlimit)) jlimit.clear();
  if (!JointTravel(joints_, &jtravel)) jtravel.clear();
  if (!detect_contacts && !contacts_.empty()) return false;   // caller-supplied contacts: use the explicit path
  egs_context *ctx = egs::DefaultContext();
  const bool first = !world_;
  if (!world_) {
    egs::check(egs_world_create(ctx, n_, EGS_F64, &world_));
    world_joints_ = -1;
  }
  std::vector<double> pos((size_t)n_ * 3), R((size_t)n_ * 9), vl((size_t)n_ * 3), w((size_t)n_ * 3), Minv((size_t)n_ * 36),
      side((size_t)n_ * 3);
  for (int i = 0; i < n_; ++i) {
    const Vector3d sl = components_[i]->GetSideLengths();
    for (int k = 0; k < 3; ++k) {
      pos[3 * i + k] = components_[i]->p()[k]; vl[3 * i + k] = components_[i]->v()[k];
      w[3 * i + k] = components_[i]->w_g()[k]; side[3 * i + k] = sl[k];
    }
    for (int k = 0; k < 9; ++k) R[9 * i + k] = components_[i]->R().d[k];
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) Minv[(size_t)i * 36 + 6 * r + c] = M_inverse_(6 * i + r, 6 * i + c);
  }
  if (first || warm_start_ != world_warm_ || (warm_start_ && warm_radius_ != world_warm_radius_)) {
    egs::check(egs_world_set_warm_start(world_, warm_start_ ? 1 : 0, warm_radius_));
    world_warm_ = warm_start_; world_warm_radius_ = warm_radius_;
    world_state_.clear();
  }
  if (first) world_friction_ = -1.0;   // a fresh world has the reference's box
  if (const double mu = device_friction(); mu != world_friction_) {
    egs::check(egs_world_set_friction(world_, 1, &mu));
    world_friction_ = mu;
  }
  if (first) { world_restitution_ = -1.0; world_restitution_vth_ = 0.0; }   // a fresh world has none
  if (restitution_ != world_restitution_ || (restitution_ >= 0 && restitution_vth_ != world_restitution_vth_)) {
    egs::check(egs_world_set_restitution(world_, 1, &restitution_, restitution_vth_));
    world_restitution_ = restitution_; world_restitution_vth_ = restitution_vth_;
  }
  // M^-1, the external force and the box sizes are frozen at Init() (Q5): sent once.  With warm start on, a state
  // that is still what the last step left on the device is not pushed again: a push drops the world's history.
  if (!(warm_start_ && egs::same_state(world_state_, pos, R, vl, w)))
    egs::check(egs_world_set_bodies(world_, pos.data(), R.data(), vl.data(), w.data(), first ? Minv.data() : nullptr,
                                    first ? external_force_torque_.data() : nullptr, first ? side.data() : nullptr));
  if (first) world_live_ = false;   // a fresh world has live inertia off
  if (live_inertia_ != world_live_) {
    const std::vector<double> Ib = BodyInertias();
    egs::check(egs_world_set_live_inertia(world_, live_inertia_ ? Ib.data() : nullptr, nullptr));
    world_live_ = live_inertia_;
  }
  live_world_ = live_inertia_ ? world_ : nullptr; live_offset_ = 0; live_total_ = n_;
  if (first)
    if (const std::vector<int32_t> shape = Shapes(); !shape.empty()) egs::check(egs_world_set_shapes(world_, shape.data()));
  // joints are permanent in the reference (ensembles.cc:331-334); a caller that edits them all the same
  // (same count, other bodies or anchors) must not step against the stale device copy
  if (world_joints_ != mj || jb0 != world_jb0_ || jb1 != world_jb1_ || jdata != world_jdata_ || jkind != world_jkind_) {
    egs::check(egs_world_set_joints_kinds(world_, mj, jkind.data(), jb0.data(), jb1.data(), jdata.data()));
    world_joints_ = mj;
    world_jb0_ = jb0; world_jb1_ = jb1; world_jdata_ = jdata; world_jkind_ = jkind;
    world_jmotor_.assign(2 * (size_t)mj, 0.0);
    for (int i = 0; i < mj; ++i) world_jmotor_[2 * (size_t)i + 1] = -1.0;
    world_jlimit_.clear();   // ... and no limits
    world_jtravel_.clear();
  }
  if (jmotor != world_jmotor_) {
    egs::check(egs_world_set_joint_motors(world_, motors ? jmotor.data() : nullptr));
    world_jmotor_ = jmotor;
  }
  if (jlimit != world_jlimit_) {
    egs::check(egs_world_set_joint_limits(world_, jlimit.empty() ? nullptr : jlimit.data()));
    world_jlimit_ = jlimit;
  }
  if (jtravel != world_jtravel_) {
    egs::check(egs_world_set_slider_limits(world_, jtravel.empty() ? nullptr : jtravel.data()));
    world_jtravel_ = jtravel;
  }
  egs_solve_params prm = solver_params;
  prm.cfm = cfm_coeff;
  egs_solve_stats st;
  world_state_.clear();   // (a step that throws leaves no state to trust)
  ray_pose_.clear();
  egs::check(egs_world_step(world_, dt, /*erp=*/0.2, &prm, detect_contacts ? 1 : 0, &st));
  egs::check(egs_world_get_bodies(world_, pos.data(), R.data(), vl.data(), w.data()));
  if (warm_start_) egs::keep_state(world_state_, pos, R, vl, w);
  ray_pose_ = pos;
  ray_pose_.insert(ray_pose_.end(), R.begin(), R.end());
  for (int i = 0; i < n_; ++i) {
    components_[i]->SetP(Vector3d(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]));
    components_[i]->SetV(Vector3d(vl[3 * i], vl[3 * i + 1], vl[3 * i + 2]));
    components_[i]->SetW_GlobalFrame(Vector3d(w[3 * i], w[3 * i + 1], w[3 * i + 2]));
    Matrix3d Rm;
    for (int k = 0; k < 9; ++k) Rm.d[k] = R[9 * i + k];
    components_[i]->SetR(Rm);
  }
  int32_t mcons = 0, mc = 0, replans = 0;
  egs::check(egs_world_info(world_, &mcons, &mc, &replans));
  contacts_.clear();
  if (mc > 0) {   // the contact list the step used (for constraints(), Draw(), ...)
    std::vector<int32_t> b0(mc), b1(mc);
    std::vector<double> data((size_t)mc * 7);
    int32_t got = 0;
    egs::check(egs_world_get_contacts(world_, mc, &got, b0.data(), b1.data(), data.data()));
    for (int k = 0; k < mc; ++k) {
      const double *d = &data[(size_t)k * 7];
      ContactGeometry cg(Vector3d(d[0], d[1], d[2]), Vector3d(d[3], d[4], d[5]), d[6]);
      if (b0[k] < 0) contacts_.push_back(std::make_shared<Contact>(components_[b1[k]], b1[k], cg));
      else contacts_.push_back(std::make_shared<Contact>(components_[b0[k]], b0[k], components_[b1[k]], b1[k], cg));
    }
  }
  last_lambda.resize(3 * mcons);
  if (mcons > 0) {
    int32_t rows = 0;
    egs::check(egs_world_get_lambda(world_, 3 * mcons, &rows, last_lambda.data()));
  }
  return true;
}

void Ensemble::Step(double dt, Integrator g) {  // ensembles.cc:390-427
  // The reference cannot complete a step with either of the other two: IMPLICIT_MIDPOINT Panics outright
  // (ensembles.cc:403-405) and EXPLICIT_EULER reaches ComputeJDotV_Joints(), whose first statement is a Panic
  // (ensembles.cc:94-97). There is no behaviour to reproduce, so both are refused with the reference's reason.
  if (g == Integrator::IMPLICIT_MIDPOINT)
    throw egs::Error(EGS_ERR_UNSUPPORTED,
                     "Implicit midpoint integrator is not properly implemented and tested (ensembles.cc:403-405)");
  if (g != Integrator::OPEN_DYNAMICS_ENGINE)
    throw egs::Error(EGS_ERR_UNSUPPORTED,
                     "Integrator::EXPLICIT_EULER panics in the reference (ComputeJDotV_Joints, ensembles.cc:94-97); "
                     "only Integrator::OPEN_DYNAMICS_ENGINE completes a step");
  if (!detect_contacts && !Shapes().empty())
    throw egs::Error(EGS_ERR_UNSUPPORTED, "an ensemble with a Sphere or a Capsule steps on contacts the device detects: not with "
                                          "detect_contacts = false");
  if (StepOnDevice(dt)) return;   // collide -> solve -> integrate in one resident pipeline
  if (friction_model_ == Contact::FrictionModel::COULOMB_PYRAMID) {
    bool dense = use_dense_solver && dense_fric_outer_ > 0;      // SetDenseFriction: the dense step solves the pyramid
    if (dense) {
      int32_t kind = 0;
      double d[7];
      for (const auto &j : joints_) dense = dense && j->Describe(&kind, d);
    }
    if (!dense)
      throw egs::Error(EGS_ERR_UNSUPPORTED, "COULOMB_PYRAMID steps on the device only: not with use_device_step = false, "
                                            "use_dense_solver, caller-supplied contacts or a joint the device cannot take");
  }
  if (live_inertia_) {   // the explicit paths read the host's arrays: bring them to the state this step starts from
    live_world_ = nullptr;   // (no device world holds newer ones after this step)
    RefreshLiveMassOnHost();
  }
  const VectorXd v = GetVelocities();
  if (detect_contacts) UpdateContacts();
  CheckAndCorrectEnsembleState();   // ensembles.cc:394
  VectorXd v_new = StepVelocities_ODE(dt, v);
  StepPositions_ODE(dt, v, v_new);
}

// ---- EnsembleGroup: the frame (model.cc:37-70) through one batched world ------------------------------------------
EnsembleGroup::EnsembleGroup(std::vector<Ensemble *> members) : members_(std::move(members)) {
  if (members_.empty()) throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup: no members");
  const Ensemble *first = members_[0];
  for (size_t i = 0; i < members_.size(); ++i) {
    const Ensemble *m = members_[i];
    const std::string who = "EnsembleGroup: member " + std::to_string(i);
    if (!m) throw egs::Error(EGS_ERR_INVALID, who + " is a null pointer");
    for (size_t k = 0; k < i; ++k)
      if (members_[k] == m) throw egs::Error(EGS_ERR_INVALID, who + " is member " + std::to_string(k) + " again");
    const egs_solve_params &a = first->solver_params, &b = m->solver_params;
    if (a.method != b.method || a.max_iters != b.max_iters || a.check_every != b.check_every || a.omega != b.omega ||
        a.cfm != b.cfm || a.tol != b.tol)
      throw egs::Error(EGS_ERR_INVALID, who + " differs from member 0 in solver_params");
    if (m->cfm_coeff != first->cfm_coeff) throw egs::Error(EGS_ERR_INVALID, who + " differs from member 0 in cfm_coeff");
    if (m->use_dense_solver != first->use_dense_solver)
      throw egs::Error(EGS_ERR_INVALID, who + " differs from member 0 in use_dense_solver");
    if (m->detect_contacts != first->detect_contacts)
      throw egs::Error(EGS_ERR_INVALID, who + " differs from member 0 in detect_contacts");
    if (m->warm_start_ != first->warm_start_ || m->warm_radius_ != first->warm_radius_)
      throw egs::Error(EGS_ERR_INVALID, who + " differs from member 0 in SetWarmStart");
    if (m->dense_fric_outer_ != first->dense_fric_outer_ || m->dense_fric_tol_ != first->dense_fric_tol_)
      throw egs::Error(EGS_ERR_INVALID, who + " differs from member 0 in SetDenseFriction");
    int32_t kind = 0;
    double data[7];
    for (size_t j = 0; j < m->joints_.size(); ++j)
      if (!m->joints_[j]->Describe(&kind, data))
        throw egs::Error(EGS_ERR_INVALID, who + ": joint " + std::to_string(j) + " cannot describe itself to the device");
    if (!m->detect_contacts && !m->contacts_.empty())
      throw egs::Error(EGS_ERR_INVALID, who + " carries caller-supplied contacts (detect_contacts = false)");
  }
}

EnsembleGroup::~EnsembleGroup() {
  for (Ensemble *m : members_)
    if (world_ && m->live_world_ == world_) m->live_world_ = nullptr;
  if (world_) egs_world_destroy(world_);
}

int EnsembleGroup::world_ensembles() const {
  const int32_t E = (int32_t)members_.size();
  return world_ && egs_world_batch_info(world_, E, nullptr, nullptr, nullptr, nullptr) == EGS_OK ? E : 0;
}

void EnsembleGroup::Step(double dt) { Step(std::vector<double>(members_.size(), dt)); }

void EnsembleGroup::Step(const std::vector<double> &dt) {
  const size_t E = members_.size();
  if (dt.size() != E)
    throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup::Step: " + std::to_string(dt.size()) + " time steps for " +
                                          std::to_string(E) + " members");
  egs_context *ctx = egs::DefaultContext();
  const bool first = !world_;
  if (first) {
    std::vector<int32_t> nb(E);
    for (size_t i = 0; i < E; ++i) nb[i] = members_[i]->n_;
    off_.assign(E + 1, 0);
    egs::check(egs_world_create_batch(ctx, (int32_t)E, nb.data(), EGS_F64, &world_, off_.data()));
    ++worlds_created_;
    joints_sent_ = false;
  }
  const size_t n = (size_t)off_[E];
  std::vector<double> pos(n * 3), R(n * 9), vl(n * 3), w(n * 3), Minv(first ? n * 36 : 0), side(first ? n * 3 : 0),
      fext(first ? n * 6 : 0);
  std::vector<int32_t> jb0, jb1, jkind;
  std::vector<double> jdata, jmotor, jlimit, jtravel;
  bool motors = false, hinges = false, limits = false, travels = false;
  for (size_t i = 0; i < E; ++i)
    for (const auto &j : members_[i]->joints_) hinges = hinges || dynamic_cast<const HingeAxisJoint *>(j.get()) != nullptr || dynamic_cast<const SliderAxisJoint *>(j.get()) != nullptr;
  for (size_t i = 0; i < E; ++i) {
    const Ensemble *m = members_[i];
    const size_t o = (size_t)off_[i];
    if (m->n_ != off_[i + 1] - off_[i])
      throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup: member " + std::to_string(i) + " changed its number of bodies");
    if (!m->detect_contacts && !m->Shapes().empty())
      throw egs::Error(EGS_ERR_UNSUPPORTED, "EnsembleGroup: member " + std::to_string(i) + " holds a Sphere or a Capsule and steps on contacts "
                                                "the device detects: not with detect_contacts = false");
    for (int b = 0; b < m->n_; ++b) {
      const Body &body = *m->components_[b];
      const size_t g = o + (size_t)b;
      for (int k = 0; k < 3; ++k) {
        pos[3 * g + k] = body.p()[k]; vl[3 * g + k] = body.v()[k]; w[3 * g + k] = body.w_g()[k];
      }
      for (int k = 0; k < 9; ++k) R[9 * g + k] = body.R().d[k];
      if (!first) continue;
      const Vector3d sl = body.GetSideLengths();
      for (int k = 0; k < 3; ++k) side[3 * g + k] = sl[k];
      for (int k = 0; k < 6; ++k) fext[6 * g + k] = m->external_force_torque_(6 * b + k);
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) Minv[g * 36 + 6 * r + c] = m->M_inverse_(6 * b + r, 6 * b + c);
    }
    for (size_t j = 0; j < m->joints_.size(); ++j) {   // the world's joints: member by member, global body indices
      int32_t kind = 0;
      double d[7];
      if (!m->joints_[j]->Describe(&kind, d))
        throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup: member " + std::to_string(i) + ": joint " + std::to_string(j) +
                                              " cannot describe itself to the device");
      const int a = m->joints_[j]->i0_, b = m->joints_[j]->i1_;
      jb0.push_back(a >= 0 ? a + (int32_t)o : -1);
      jb1.push_back(b >= 0 ? b + (int32_t)o : -1);
      jdata.insert(jdata.end(), d, d + 7);
      jkind.push_back(kind);
    }
    std::vector<double> own;
    motors = JointMotors(m->joints_, &own) || motors;
    jmotor.insert(jmotor.end(), own.begin(), own.end());
    limits = JointLimits(m->joints_, &own) || limits;
    jlimit.insert(jlimit.end(), own.begin(), own.end());
    travels = JointTravel(m->joints_, &own) || travels;
    jtravel.insert(jtravel.end(), own.begin(), own.end());
  }
  if (!limits) jlimit.clear();
  if (!travels) jtravel.clear();
  const Ensemble *lead = members_[0];
  for (size_t i = 1; i < E; ++i)   // (the constructor's check, again: SetWarmStart may have been called since)
    if (members_[i]->warm_start_ != lead->warm_start_ || members_[i]->warm_radius_ != lead->warm_radius_)
      throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup: member " + std::to_string(i) + " differs from member 0 in SetWarmStart");
  for (size_t i = 1; i < E; ++i)
    if (members_[i]->dense_fric_outer_ != lead->dense_fric_outer_ || members_[i]->dense_fric_tol_ != lead->dense_fric_tol_)
      throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup: member " + std::to_string(i) + " differs from member 0 in SetDenseFriction");
  const bool warm = lead->warm_start_ && !lead->use_dense_solver;
  if (first || warm != world_warm_ || (warm && lead->warm_radius_ != world_warm_radius_)) {
    egs::check(egs_world_set_warm_start(world_, warm ? 1 : 0, lead->warm_radius_));
    world_warm_ = warm; world_warm_radius_ = lead->warm_radius_;
    world_state_.clear();
  }
  {   // the members' friction, each its own (a fresh world has the reference's box everywhere)
    std::vector<double> mu(E);
    for (size_t i = 0; i < E; ++i) mu[i] = members_[i]->device_friction();
    if (first) world_friction_.assign(E, -1.0);
    if (mu != world_friction_) {
      egs::check(egs_world_set_friction(world_, (int32_t)E, mu.data()));
      world_friction_ = mu;
    }
  }
  {   // the members' restitution: each its own coefficient, one threshold among those that have it on
    std::vector<double> rest(E);
    double vth = 0.0;
    bool any = false;
    for (size_t i = 0; i < E; ++i) {
      rest[i] = members_[i]->restitution_;
      if (rest[i] < 0) continue;
      if (any && members_[i]->restitution_vth_ != vth)
        throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup: member " + std::to_string(i) + " differs in SetRestitution's threshold");
      vth = members_[i]->restitution_vth_;
      any = true;
    }
    if (first) { world_restitution_.assign(E, -1.0); world_restitution_vth_ = 0.0; }
    if (rest != world_restitution_ || (any && vth != world_restitution_vth_)) {
      egs::check(egs_world_set_restitution(world_, (int32_t)E, rest.data(), vth));
      world_restitution_ = rest; world_restitution_vth_ = vth;
    }
  }
  // M^-1, the external force and the box sizes are frozen at Init() (Q5): sent once.  With warm start on, a state
  // that is still what the last step left on the device is not pushed again: a push drops the world's history.
  if (!(warm && egs::same_state(world_state_, pos, R, vl, w)))
    egs::check(egs_world_set_bodies(world_, pos.data(), R.data(), vl.data(), w.data(), first ? Minv.data() : nullptr,
                                    first ? fext.data() : nullptr, first ? side.data() : nullptr));
  {   // the members' live inertia, each its own: the bodies of a member with it off go as the identity, which is skipped
    std::vector<char> live(E);
    bool any = false;
    for (size_t i = 0; i < E; ++i) { live[i] = members_[i]->live_inertia_ ? 1 : 0; any = any || live[i]; }
    if (first) world_live_.assign(E, 0);
    if (live != world_live_) {
      std::vector<double> Ib(n * 9, 0.0);
      for (size_t g = 0; g < n; ++g) Ib[9 * g] = Ib[9 * g + 4] = Ib[9 * g + 8] = 1.0;
      for (size_t i = 0; i < E; ++i) {
        if (!live[i]) continue;
        const std::vector<double> own = members_[i]->BodyInertias();
        std::copy(own.begin(), own.end(), Ib.begin() + 9 * (size_t)off_[i]);
      }
      egs::check(egs_world_set_live_inertia(world_, any ? Ib.data() : nullptr, nullptr));
      world_live_ = live;
    }
    for (size_t i = 0; i < E; ++i) {
      Ensemble *m = members_[i];
      if (live[i]) { m->live_world_ = world_; m->live_offset_ = off_[i]; m->live_total_ = (int)n; }
      else if (m->live_world_ == world_) m->live_world_ = nullptr;
    }
  }
  if (first) {   // the members' shapes, with the side lengths; none sent when every Body of every member is a box
    std::vector<int32_t> shape(n, EGS_SHAPE_BOX);
    bool any = false;
    for (size_t i = 0; i < E; ++i) {
      const std::vector<int32_t> s = members_[i]->Shapes();
      if (!s.empty()) { std::copy(s.begin(), s.end(), shape.begin() + off_[i]); any = true; }
    }
    if (any) egs::check(egs_world_set_shapes(world_, shape.data()));
  }
  world_state_.clear();
  ray_pose_.clear();
  if (!joints_sent_ || jb0 != world_jb0_ || jb1 != world_jb1_ || jdata != world_jdata_ || jkind != world_jkind_) {   // re-sent when edited
    egs::check(egs_world_set_joints_kinds(world_, (int32_t)jb0.size(), jkind.data(), jb0.data(), jb1.data(), jdata.data()));
    joints_sent_ = true;
    world_jb0_ = jb0; world_jb1_ = jb1; world_jdata_ = jdata; world_jkind_ = jkind;
    world_jmotor_.assign(2 * jb0.size(), 0.0);   // a new joint list has no motors
    for (size_t j = 0; j < jb0.size(); ++j) world_jmotor_[2 * j + 1] = -1.0;
    world_jlimit_.clear();   // ... and no limits
    world_jtravel_.clear();
  }
  if (jmotor != world_jmotor_) {   // ... and the motors with them
    egs::check(egs_world_set_joint_motors(world_, motors ? jmotor.data() : nullptr));
    world_jmotor_ = jmotor;
  }
  if (jlimit != world_jlimit_) {   // ... and the limits
    egs::check(egs_world_set_joint_limits(world_, jlimit.empty() ? nullptr : jlimit.data()));
    world_jlimit_ = jlimit;
  }
  if (jtravel != world_jtravel_) {   // ... and the sliders' stops
    egs::check(egs_world_set_slider_limits(world_, jtravel.empty() ? nullptr : jtravel.data()));
    world_jtravel_ = jtravel;
  }
  const std::vector<double> erp(E, 0.2);   // error_reduction_param of StepVelocities_ODE, as in Ensemble::Step
  if (lead->use_dense_solver) {
    egs::check(egs_world_set_dense_friction(world_, lead->dense_fric_outer_, lead->dense_fric_tol_));
    egs::check(egs_world_step_dense_each(world_, (int32_t)E, dt.data(), erp.data(), lead->cfm_coeff,
                                         /*use_bounds=*/lead->dense_fric_outer_ > 0 || hinges ? 1 : 0, lead->detect_contacts ? 1 : 0, nullptr));
    std::vector<int32_t> outer(E), conv(E);
    egs::check(egs_world_dense_friction_info(world_, (int32_t)E, outer.data(), conv.data(), nullptr));
    for (size_t i = 0; i < E; ++i) { members_[i]->last_dense_outer = outer[i]; members_[i]->last_dense_converged = conv[i] != 0; }
  } else {
    egs_solve_params prm = lead->solver_params;
    prm.cfm = lead->cfm_coeff;
    egs_solve_stats st;
    egs::check(egs_world_step_each(world_, (int32_t)E, dt.data(), erp.data(), &prm, lead->detect_contacts ? 1 : 0, &st));
  }
  egs::check(egs_world_get_bodies(world_, pos.data(), R.data(), vl.data(), w.data()));
  if (warm) egs::keep_state(world_state_, pos, R, vl, w);
  ray_pose_ = pos;
  ray_pose_.insert(ray_pose_.end(), R.begin(), R.end());
  int32_t mcons = 0, mc = 0, replans = 0;
  egs::check(egs_world_info(world_, &mcons, &mc, &replans));
  std::vector<int32_t> jo(E + 1), co(E + 1), cb0((size_t)mc), cb1((size_t)mc);
  std::vector<double> cdata((size_t)mc * 7), lambda((size_t)mcons * 3);
  egs::check(egs_world_batch_info(world_, (int32_t)E, jo.data(), co.data(), nullptr, nullptr));
  if (mc > 0) {
    int32_t got = 0;
    egs::check(egs_world_get_contacts(world_, mc, &got, cb0.data(), cb1.data(), cdata.data()));
  }
  if (mcons > 0) {
    int32_t rows = 0;
    egs::check(egs_world_get_lambda(world_, 3 * mcons, &rows, lambda.data()));
  }
  const int mj = jo[E];
  for (size_t i = 0; i < E; ++i) {
    Ensemble *m = members_[i];
    if (dt[i] == 0) continue;   // sat out: its bodies, contacts and last_lambda stay as they are
    const int o = off_[i];
    for (int b = 0; b < m->n_; ++b) {
      const size_t g = (size_t)(o + b);
      m->components_[b]->SetP(Vector3d(pos[3 * g], pos[3 * g + 1], pos[3 * g + 2]));
      m->components_[b]->SetV(Vector3d(vl[3 * g], vl[3 * g + 1], vl[3 * g + 2]));
      m->components_[b]->SetW_GlobalFrame(Vector3d(w[3 * g], w[3 * g + 1], w[3 * g + 2]));
      Matrix3d Rm;
      for (int k = 0; k < 9; ++k) Rm.d[k] = R[9 * g + k];
      m->components_[b]->SetR(Rm);
    }
    m->contacts_.clear();   // the member's slice of the contact list the step used, in its own numbering
    for (int k = co[i]; k < co[i + 1]; ++k) {
      const double *d = &cdata[(size_t)k * 7];
      const ContactGeometry cg(Vector3d(d[0], d[1], d[2]), Vector3d(d[3], d[4], d[5]), d[6]);
      const int a = cb0[k] >= 0 ? cb0[k] - o : -1, b = cb1[k] - o;
      if (a < 0) m->contacts_.push_back(std::make_shared<Contact>(m->components_[b], b, cg));
      else m->contacts_.push_back(std::make_shared<Contact>(m->components_[a], a, m->components_[b], b, cg));
    }
    const int rj = 3 * (jo[i + 1] - jo[i]), rc = 3 * (co[i + 1] - co[i]);   // its joints' rows, then its contacts'
    m->last_lambda.resize(rj + rc);
    for (int r = 0; r < rj; ++r) m->last_lambda(r) = lambda[(size_t)(3 * jo[i] + r)];
    for (int r = 0; r < rc; ++r) m->last_lambda(rj + r) = lambda[(size_t)(3 * (mj + co[i]) + r)];
  }
}

std::vector<std::vector<RayHit>> EnsembleGroup::CastRays(const std::vector<std::vector<Ray>> &rays) {
  const size_t E = members_.size();
  if (rays.size() != E)
    throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup::CastRays: " + std::to_string(rays.size()) + " ray lists for " +
                                          std::to_string(E) + " members");
  std::vector<std::vector<RayHit>> out(E);
  std::vector<double> pos, R;
  for (const Ensemble *m : members_) AppendPose(m->components_, &pos, &R);
  if (!world_ || !SamePose(ray_pose_, pos, R)) {   // the world does not hold these poses: each member for itself
    for (size_t i = 0; i < E; ++i) out[i] = members_[i]->CastRays(rays[i]);
    return out;
  }
  RayArrays a;
  std::vector<int32_t> ens;
  for (size_t i = 0; i < E; ++i)
    for (const Ray &r : rays[i]) {
      if (r.body < -1 || r.body >= members_[i]->n_)
        throw egs::Error(EGS_ERR_INVALID, "EnsembleGroup::CastRays: a ray's body is not a component of member " + std::to_string(i));
      a.Add(r, off_[i]);
      ens.push_back((int32_t)i);
    }
  const size_t nr = ens.size();
  if (nr == 0) return out;
  const std::vector<double> key = a.Key(&ens);
  if (!SameKey(key, world_rays_)) {
    world_rays_.clear();
    egs::check(egs_world_set_rays(world_, (int32_t)nr, ens.data(), a.body.data(), a.origin.data(), a.dir.data(), a.tmax.data()));
    world_rays_ = key;
  }
  std::vector<int32_t> hit(nr);
  std::vector<double> t(nr), normal(3 * nr);
  int32_t got = 0;
  egs::check(egs_world_cast_rays(world_, (int32_t)nr, &got, hit.data(), t.data(), normal.data()));
  size_t at = 0;
  for (size_t i = 0; i < E; ++i)
    for (const Ray &r : rays[i]) {
      out[i].push_back(MakeHit(r, members_[i]->components_, hit[at], off_[i], t[at], &normal[3 * at]));
      ++at;
    }
  return out;
}

Chain::Chain(int num_links, const Vector3d &anchor) {  // ensembles.cc:668-707
  if (num_links <= 0) throw egs::Error(EGS_ERR_INVALID, "num_links > 0");
  n_ = num_links;
  const double az = 0.95531661812451, ax = M_PI / 4;
  double qz_w = std::cos(az / 2), qz_z = std::sin(az / 2), qx_w = std::cos(ax / 2), qx_x = std::sin(ax / 2);
  Matrix3d R = QuatToR(qz_w * qx_w, qz_w * qx_x, qz_z * qx_x, qz_z * qx_w);
  for (int i = 0; i < n_; ++i) {
    Vector3d p(std::sqrt(3.0) * 0.3 * i + anchor[0], 0 + anchor[1], 0 + anchor[2]);
    components_.push_back(std::make_shared<Body>(p, Vector3d::Zero(), R, Vector3d::Zero()));
  }
  const Vector3d c1(0.15, -0.15, 0.15), c2(-0.15, 0.15, -0.15);
  for (int i = 0; i < n_ - 1; ++i)
    joints_.push_back(std::make_shared<BallAndSocketJoint>(components_[i], i, c1, components_[i + 1], i + 1, c2));
  joints_.push_back(std::make_shared<BallAndSocketJoint>(components_[0], 0, Vector3d::Zero(), components_[0]->p()));
}

// ---- Cairn (ensembles.cc:708-728) ------------------------------------------------
namespace {
double Rand01() { return double(std::rand()) / double(RAND_MAX); }          // Eigen internal::random<double>(0, 1)
double RandPm1() { return -1.0 + 2.0 * Rand01(); }                          // ... (-1, 1): Vector3d::Random() per coefficient
Vector3d RandomVector() { double a = RandPm1(), b = RandPm1(), c = RandPm1(); return Vector3d(a, b, c); }
}  // namespace

Cairn::Cairn(int num_rocks, const std::array<double, 2> &xb, const std::array<double, 2> &yb, const std::array<double, 2> &zb) {
  if (num_rocks < 0) throw egs::Error(EGS_ERR_INVALID, "num_rocks >= 0");
  n_ = num_rocks;
  const Matrix3d I = Matrix3d::Identity() * 0.1;
  for (int i = 0; i < num_rocks; ++i) {
    // RandomPosition, utils.cc:26-38
    Vector3d u = (RandomVector() + Vector3d(1, 1, 1)) / 2;
    Vector3d p(u[0] * std::fabs(xb[1] - xb[0]) + std::min(xb[0], xb[1]), u[1] * std::fabs(yb[1] - yb[0]) + std::min(yb[0], yb[1]),
               u[2] * std::fabs(zb[1] - zb[0]) + std::min(zb[0], zb[1]));
    // RandomRotationViaQuaternion -> Quaterniond::UnitRandom (utils.cc:52-55)
    const double u1 = Rand01(), u2 = 2 * M_PI * Rand01(), u3 = 2 * M_PI * Rand01();
    const double a = std::sqrt(1 - u1), b = std::sqrt(u1);
    const Matrix3d R = QuatToR(a * std::sin(u2), a * std::cos(u2), b * std::sin(u3), b * std::cos(u3));
    const Vector3d v = RandomVector() * max_init_v_, w = RandomVector() * max_init_w_;   // utils.cc:40-48
    components_.push_back(std::make_shared<Body>(p, v, 1.0, R, w, I));
  }
}
