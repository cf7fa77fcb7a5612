// joint_host_check -- the host-only side of the angular joints (AngularLockJoint, HingeAxisJoint, Ensemble::AddWeld /
// AddHinge / SetHingeMotor: ComputeError, ComputeJ, Describe) exercised without a device, as a stand-alone program that
// tests/test_joint_reference_cpu.py builds with -fsanitize=address,undefined and runs on the CPU.  It checks what the
// classes promise -- err = 0 at the captured pose, err = sin(theta) n after a known turn, d err/dt = J0 s0 + J1 s1 by a
// central difference, unit descriptors, the motor's bounds -- and exits non-zero on the first miss.
#include <cmath>
#include <cstdio>
#include <memory>

#include "eggshell_api.h"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

Matrix3d Rodrigues(const Vector3d &axis, double angle) {
  const Vector3d n = axis / axis.norm();
  Matrix3d K;
  K(0, 1) = -n[2]; K(0, 2) = n[1]; K(1, 0) = n[2]; K(1, 2) = -n[0]; K(2, 0) = -n[1]; K(2, 1) = n[0];
  const Matrix3d K2 = K * K;
  Matrix3d R = Matrix3d::Identity();
  for (int k = 0; k < 9; ++k) R.d[k] += std::sin(angle) * K.d[k] + (1 - std::cos(angle)) * K2.d[k];
  return R;
}

class Scene : public Ensemble {
 public:
  std::shared_ptr<Body> Add(const Body &b) {
    components_.push_back(std::make_shared<Body>(b));
    n_ = (int)components_.size();
    return components_.back();
  }
};

double max_abs(const VectorXd &v) {
  double m = 0;
  for (int i = 0; i < v.size(); ++i) m = std::fmax(m, std::fabs(v(i)));
  return m;
}

// central difference of the joint's error while both bodies turn with w0 / w1, against J0 (0, w0) + J1 (0, w1)
void rate_check(const Joint &j, Body &a, Body *b, const Vector3d &w0, const Vector3d &w1, const char *what) {
  MatrixXd J0, J1;
  ArrayXb ct;
  VectorXd lo, hi;
  j.ComputeJ(&J0, &J1, &ct, &lo, &hi);
  const double h = 1e-6;
  const Matrix3d Ra = a.R(), Rb = b ? b->R() : Matrix3d::Identity();
  VectorXd e[2];
  for (int s = 0; s < 2; ++s) {
    const double t = s ? h : -h;
    a.SetR(Rodrigues(w0, t * w0.norm()) * Ra);
    if (b) b->SetR(Rodrigues(w1, t * w1.norm()) * Rb);
    e[s] = j.ComputeError();
  }
  a.SetR(Ra);
  if (b) b->SetR(Rb);
  const int rows = ct(2) ? 3 : 2;   // a hinge's axis row carries no error
  for (int r = 0; r < rows; ++r) {
    double want = 0;
    for (int c = 0; c < 3; ++c) want += J0(r, 3 + c) * w0[c] + (b ? J1(r, 3 + c) * w1[c] : 0.0);
    for (int c = 0; c < 3; ++c) expect(J0(r, c) == 0.0 && J1(r, c) == 0.0, "linear columns are zero");
    expect(std::fabs((e[1](r) - e[0](r)) / (2 * h) - want) < 1e-8, what);
  }
}

}  // namespace

int main() {
  const Vector3d w0(0.3, -0.7, 0.5), w1(-0.2, 0.4, 0.9);
  for (int world = 0; world < 2; ++world) {
    Scene s;
    auto a = s.Add(Body(Vector3d(0.5, 0, 2), Vector3d::Zero(), Rodrigues(Vector3d(1, 2, 3), 0.7), Vector3d::Zero()));
    auto b = world ? nullptr : s.Add(Body(Vector3d(1.1, 0, 2), Vector3d::Zero(), Rodrigues(Vector3d(-2, 1, 0.5), 1.9), Vector3d::Zero()));
    const int wi = s.AddWeld(a, 0, b, world ? -1 : 1, Vector3d(0.8, 0, 2));
    const int hi_ = s.AddHinge(a, 0, b, world ? -1 : 1, Vector3d(0.8, 0, 2), Vector3d(0, 3, 4));
    expect(wi == 1 && hi_ == 3 && s.joints().size() == 4, "AddWeld / AddHinge return the angular joint's index");
    const Joint &lock = *s.joints()[wi], &hinge = *s.joints()[hi_];
    expect(!lock.HasPosition() && !hinge.HasPosition() && s.joints()[0]->HasPosition(), "HasPosition");
    expect(max_abs(lock.ComputeError()) < 1e-15 && max_abs(hinge.ComputeError()) < 1e-15, "err = 0 at the captured pose");
    expect(max_abs(s.joints()[0]->ComputeError()) < 1e-15, "the weld's anchor holds at the captured pose");
    int32_t kind = -1;
    double d[7];
    expect(lock.Describe(&kind, d) && kind == EGS_JOINT_LOCK, "the lock describes itself");
    expect(std::fabs(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] - 1.0) <= 1e-12 && d[4] == 0 && d[5] == 0 && d[6] == 0, "unit quaternion");
    expect(hinge.Describe(&kind, d) && kind == EGS_JOINT_HINGE_AXIS, "the hinge describes itself");
    expect(std::fabs(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - 1.0) <= 1e-12 && std::fabs(d[3] * d[3] + d[4] * d[4] + d[5] * d[5] - 1.0) <= 1e-12, "unit axes");
    rate_check(lock, *a, b.get(), w0, w1, "lock: d err/dt = J0 s0 + J1 s1");
    rate_check(hinge, *a, b.get(), w0, w1, "hinge: d err/dt = J0 s0 + J1 s1");
    // a known turn of body 0: 0.05 rad about n
    const Vector3d n = Vector3d(2, 3, 6) / 7.0;
    const Matrix3d Ra = a->R();
    a->SetR(Rodrigues(n, 0.05) * Ra);
    const VectorXd e = lock.ComputeError();
    for (int k = 0; k < 3; ++k) expect(std::fabs(e(k) - std::sin(0.05) * n[k]) < 1e-15, "lock: err = sin(theta) n");
    a->SetR(Ra);
    // the motor's bounds
    MatrixXd J0, J1;
    ArrayXb ct;
    VectorXd lo, hi;
    hinge.ComputeJ(&J0, &J1, &ct, &lo, &hi);
    expect(ct(0) && ct(1) && !ct(2) && lo(2) == 0 && hi(2) == 0, "a free hinge pins its axis row");
    s.SetHingeMotor(hi_, 1.5, 4.0);
    hinge.ComputeJ(&J0, &J1, &ct, &lo, &hi);
    expect(lo(2) == -4.0 && hi(2) == 4.0 && lo(0) == 0 && hi(1) == 0, "the motor opens the axis row");
    bool threw = false;
    try { s.SetHingeMotor(wi, 1.0, 1.0); } catch (const egs::Error &err) { threw = err.status == EGS_ERR_INVALID; }
    expect(threw, "SetHingeMotor refuses a joint that is no hinge");
    threw = false;
    try { s.SetHingeMotor(hi_, std::nan(""), 1.0); } catch (const egs::Error &err) { threw = err.status == EGS_ERR_INVALID; }
    expect(threw, "SetHingeMotor refuses a NaN speed");
    lock.ComputeJ(&J0, &J1, &ct, &lo, &hi);
    expect(ct(0) && ct(1) && ct(2) && J0(0, 3) == 1.0 && J0(1, 4) == 1.0 && J0(2, 5) == 1.0, "lock: [0 | I]");
    expect(world ? J1(0, 3) == 0.0 : J1(0, 3) == -1.0, "lock: [0 | -I] or nothing for the world");
  }
  std::printf(failures ? "joint_host_check: %d failed\n" : "joint_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
