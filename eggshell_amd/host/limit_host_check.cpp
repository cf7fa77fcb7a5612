// limit_host_check -- the host-only side of the hinge angle limits (HingeAxisJoint::SetLimits / LimitRow / Angle,
// ComputeError and ComputeJ under a stop, Ensemble::SetHingeLimits / HingeAngle) exercised without a device, as a
// stand-alone program that tests/test_limit_reference_cpu.py builds with -fsanitize=address,undefined and runs on the
// CPU.  It checks what the classes promise -- theta = 0 at the captured pose, theta after a known turn, the table row,
// err[2] = sin(theta - limit) and one-sided bounds past a stop, the motor's row inside the range, the refusals -- and
// exits non-zero on the first miss.
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

bool refuses(Scene &s, int index, double lo, double hi) {
  try { s.SetHingeLimits(index, lo, hi); } catch (const egs::Error &err) { return err.status == EGS_ERR_INVALID; }
  return false;
}

}  // namespace

int main() {
  const Vector3d axis(0, 3, 4);
  for (int world = 0; world < 2; ++world) {
    Scene s;
    auto a = s.Add(Body(Vector3d(0.5, 0, 2), Vector3d::Zero(), Rodrigues(Vector3d(1, 2, 3), 0.7), Vector3d::Zero()));
    auto b = world ? nullptr : s.Add(Body(Vector3d(1.1, 0, 2), Vector3d::Zero(), Rodrigues(Vector3d(-2, 1, 0.5), 1.9), Vector3d::Zero()));
    const int wi = s.AddWeld(a, 0, b, world ? -1 : 1, Vector3d(0.8, 0, 2));
    const int h = s.AddHinge(a, 0, b, world ? -1 : 1, Vector3d(0.8, 0, 2), axis);
    auto *hinge = dynamic_cast<HingeAxisJoint *>(s.joints()[h].get());
    expect(hinge != nullptr && !hinge->has_limits(), "a new hinge has no limits");
    expect(std::fabs(s.HingeAngle(h)) < 1e-15, "theta = 0 at the captured pose");
    double row[8];
    hinge->LimitRow(row);
    expect(std::fabs(row[0] * row[0] + row[1] * row[1] + row[2] * row[2] + row[3] * row[3] - 1.0) <= 1e-12, "unit quaternion");
    expect(row[4] == 0 && row[5] == 0 && row[6] == 0 && row[7] == 0, "no stop: (0, 0) pairs");
    s.SetHingeLimits(h, -0.3, 0.5);
    hinge->LimitRow(row);
    expect(row[4] == std::sin(-0.3) && row[5] == std::cos(-0.3) && row[6] == std::sin(0.5) && row[7] == std::cos(0.5), "the table's pairs");
    s.SetHingeLimits(h, -INFINITY, 0.5);
    hinge->LimitRow(row);
    expect(row[4] == 0 && row[5] == 0 && row[6] == std::sin(0.5) && hinge->has_limits(), "a one-sided table");
    s.SetHingeLimits(h, -0.3, 0.5);
    // known turns of body 0 about the axis (both bodies together: theta stays)
    const Matrix3d Ra = a->R();
    MatrixXd J0, J1;
    ArrayXb ct;
    VectorXd lo, hi;
    for (double th : {0.2, 0.7, -0.45, 3.0, -3.0}) {
      a->SetR(Rodrigues(axis, th) * Ra);
      expect(std::fabs(s.HingeAngle(h) - th) < 4e-15, "theta after a known turn");
      const VectorXd e = hinge->ComputeError();
      hinge->ComputeJ(&J0, &J1, &ct, &lo, &hi);
      expect(std::fabs(e(0)) < 1e-15 && std::fabs(e(1)) < 1e-15 && !ct(2), "the axes stay aligned; the axis row is no equality row");
      if (th > 0.5) {
        expect(std::fabs(e(2) - std::sin(th - 0.5)) < 4e-15 && lo(2) == -INFINITY && hi(2) == 0.0, "past the upper stop");
      } else if (th < -0.3) {
        expect(std::fabs(e(2) - std::sin(th + 0.3)) < 4e-15 && lo(2) == 0.0 && hi(2) == INFINITY, "past the lower stop");
      } else {
        expect(e(2) == 0.0 && lo(2) == 0.0 && hi(2) == 0.0, "inside the range: the free hinge's row");
      }
    }
    // the motor and the limit share the row
    s.SetHingeMotor(h, 1.5, 4.0);
    a->SetR(Rodrigues(axis, 0.2) * Ra);
    hinge->ComputeJ(&J0, &J1, &ct, &lo, &hi);
    expect(lo(2) == -4.0 && hi(2) == 4.0, "inside the range the motor opens the row");
    a->SetR(Rodrigues(axis, 0.7) * Ra);
    hinge->ComputeJ(&J0, &J1, &ct, &lo, &hi);
    expect(lo(2) == -INFINITY && hi(2) == 0.0 && hinge->ComputeError()(2) > 0, "past a stop the row is the limit's");
    if (b) {   // both bodies turned alike: theta does not move
      const Matrix3d Rb = b->R();
      b->SetR(Rodrigues(axis, 0.7) * Rb);
      expect(std::fabs(s.HingeAngle(h)) < 4e-15, "theta is relative");
      b->SetR(Rb);
    }
    a->SetR(Ra);
    // the refusals leave the limits as they were
    expect(refuses(s, wi, -0.1, 0.1) && refuses(s, -1, -0.1, 0.1) && refuses(s, 99, -0.1, 0.1), "an index that is no hinge");
    expect(refuses(s, h, 0.2, 0.1), "lo > hi");
    expect(refuses(s, h, -4.0, 0.1) && refuses(s, h, -0.1, 3.141592653589793), "a finite |angle| >= pi");
    expect(refuses(s, h, std::nan(""), 0.1) && refuses(s, h, INFINITY, INFINITY) && refuses(s, h, -INFINITY, -INFINITY), "NaN or a stop at infinity");
    expect(hinge->limit_lo() == -0.3 && hinge->limit_hi() == 0.5, "refusals change nothing");
    bool threw = false;
    try { s.HingeAngle(wi); } catch (const egs::Error &err) { threw = err.status == EGS_ERR_INVALID; }
    expect(threw, "HingeAngle refuses a joint that is no hinge");
    s.SetHingeLimits(h, -INFINITY, INFINITY);
    expect(!hinge->has_limits(), "both infinite: no limits");
  }
  std::printf(failures ? "limit_host_check: %d failed\n" : "limit_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
