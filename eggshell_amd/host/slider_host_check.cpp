// slider_host_check -- the host-only side of the slider joints (SliderAxisJoint's ComputeError, ComputeJ, Describe and
// Position, Ensemble::AddSlider / SetSliderMotor / SetSliderLimits / SliderPosition) exercised without a device, as a
// stand-alone program that tests/test_slider_reference_cpu.py builds with -fsanitize=address,undefined and runs on the
// CPU.  It checks what the classes promise -- x = 0 and err = 0 at the captured pose, x after a known travel, err after a
// known offset across the rail, the descriptor, the block's zero net force and torque, err[2] = x - stop and one-sided
// bounds past a stop, the motor's row inside the range, the refusals -- and exits non-zero on the first miss.
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

bool refuses_limits(Scene &s, int index, double lo, double hi) {
  try { s.SetSliderLimits(index, lo, hi); } catch (const egs::Error &err) { return err.status == EGS_ERR_INVALID; }
  return false;
}
bool refuses_motor(Scene &s, int index, double speed, double force) {
  try { s.SetSliderMotor(index, speed, force); } catch (const egs::Error &err) { return err.status == EGS_ERR_INVALID; }
  return false;
}

}  // namespace

int main() {
  const Vector3d axis(0, 3, 4), rail = axis / axis.norm();
  const Vector3d side = Vector3d(1, 0, 0);   // across the rail
  for (int world = 0; world < 2; ++world) {
    Scene s;
    auto a = s.Add(Body(Vector3d(0.5, 0, 2), Vector3d::Zero(), Rodrigues(Vector3d(1, 2, 3), 0.7), Vector3d::Zero()));
    auto b = world ? nullptr : s.Add(Body(Vector3d(1.1, 0.4, 2.3), Vector3d::Zero(), Rodrigues(Vector3d(-2, 1, 0.5), 1.9), Vector3d::Zero()));
    const int j = s.AddSlider(a, 0, b, world ? -1 : 1, axis);
    auto *slider = dynamic_cast<SliderAxisJoint *>(s.joints()[j].get());
    expect(slider != nullptr && !slider->has_limits() && slider->motor_force() < 0, "a new slider has no limits and no motor");
    expect(dynamic_cast<AngularLockJoint *>(s.joints()[j - 1].get()) != nullptr, "AddSlider puts a lock in front of the slider");
    expect(std::fabs(s.SliderPosition(j)) < 1e-15, "x = 0 at the captured pose");
    int32_t kind = -1;
    double d[7];
    expect(slider->Describe(&kind, d) && kind == EGS_JOINT_SLIDER_AXIS && kind == 5 && d[6] == 0, "the descriptor's kind");
    expect(std::fabs(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - 1.0) <= 1e-12, "a unit rail direction");
    const Vector3d back = a->R() * Vector3d(d[0], d[1], d[2]);
    expect((back - rail).norm() < 1e-15, "a0 is the rail direction in body0's frame");
    MatrixXd J0, J1;
    ArrayXb ct;
    VectorXd lo, hi;
    const Vector3d pa = a->p();
    for (double x : {0.0, 0.3, -1.25}) {
      for (double off : {0.0, 0.02}) {
        a->SetP(pa + x * rail + off * side);
        expect(std::fabs(s.SliderPosition(j) - x) < 4e-15, "x after a known travel");
        const VectorXd e = slider->ComputeError();
        slider->ComputeJ(&J0, &J1, &ct, &lo, &hi);
        expect(std::fabs(std::sqrt(e(0) * e(0) + e(1) * e(1)) - off) < 4e-15 && e(2) == 0.0, "err is the offset across the rail");
        expect(ct(0) && ct(1) && !ct(2) && lo(2) == 0.0 && hi(2) == 0.0, "two equality rows and a pinned rail row");
        // no net force, no net torque about the origin for lambda = (1, -2, 3)
        const double lam[3] = {1.0, -2.0, 3.0};
        Vector3d f0 = Vector3d::Zero(), t0 = Vector3d::Zero(), f1 = Vector3d::Zero(), t1 = Vector3d::Zero();
        for (int r = 0; r < 3; ++r)
          for (int k = 0; k < 3; ++k) {
            f0[k] += J0(r, k) * lam[r]; t0[k] += J0(r, 3 + k) * lam[r];
            f1[k] += J1(r, k) * lam[r]; t1[k] += J1(r, 3 + k) * lam[r];
          }
        if (b) {
          expect((f0 + f1).norm() == 0.0, "no net force");
          expect((t0 + t1 + a->p().cross(f0) + b->p().cross(f1)).norm() < 1e-13, "no net torque: the lever arm is body0's alone");
        } else {
          expect(f1.norm() == 0.0 && t1.norm() == 0.0, "a world side has no block");
        }
      }
    }
    // stops, and the motor beside them
    s.SetSliderLimits(j, -0.2, 0.5);
    expect(slider->has_limits() && slider->limit_lo() == -0.2 && slider->limit_hi() == 0.5, "the limits are kept");
    s.SetSliderMotor(j, 1.5, 4.0);
    for (double x : {0.1, 0.7, -0.45}) {
      a->SetP(pa + x * rail);
      const VectorXd e = slider->ComputeError();
      slider->ComputeJ(&J0, &J1, &ct, &lo, &hi);
      if (x > 0.5) expect(std::fabs(e(2) - (x - 0.5)) < 4e-15 && lo(2) == -INFINITY && hi(2) == 0.0, "past the upper stop the row is the stop's");
      else if (x < -0.2) expect(std::fabs(e(2) - (x + 0.2)) < 4e-15 && lo(2) == 0.0 && hi(2) == INFINITY, "past the lower stop the row is the stop's");
      else expect(e(2) == 0.0 && lo(2) == -4.0 && hi(2) == 4.0, "inside the range the motor opens the row");
    }
    if (b) {   // both bodies moved alike: x does not move
      const Vector3d pb = b->p();
      a->SetP(pa + 0.3 * rail);
      b->SetP(pb + 0.3 * rail);
      expect(std::fabs(s.SliderPosition(j)) < 4e-15, "x is relative");
      b->SetP(pb);
    }
    a->SetP(pa);
    // the refusals leave everything as it was
    expect(refuses_limits(s, j - 1, -0.1, 0.1) && refuses_limits(s, -1, -0.1, 0.1) && refuses_limits(s, 99, -0.1, 0.1), "an index that is no slider");
    expect(refuses_limits(s, j, 0.2, 0.1), "lo > hi");
    expect(refuses_limits(s, j, std::nan(""), 0.1) && refuses_limits(s, j, INFINITY, INFINITY) && refuses_limits(s, j, -INFINITY, -INFINITY),
           "NaN or a stop at infinity");
    expect(refuses_motor(s, j - 1, 1.0, 1.0) && refuses_motor(s, j, std::nan(""), 1.0) && refuses_motor(s, j, INFINITY, 1.0) &&
           refuses_motor(s, j, 1.0, std::nan("")), "the motor's refusals");
    expect(slider->limit_lo() == -0.2 && slider->limit_hi() == 0.5 && slider->motor_speed() == 1.5 && slider->motor_force() == 4.0,
           "refusals change nothing");
    bool threw = false;
    try { s.SliderPosition(j - 1); } catch (const egs::Error &err) { threw = err.status == EGS_ERR_INVALID; }
    expect(threw, "SliderPosition refuses a joint that is no slider");
    s.SetSliderLimits(j, -INFINITY, INFINITY);
    expect(!slider->has_limits(), "both infinite: no limits");
    threw = false;
    try { s.AddSlider(a, 0, b, world ? -1 : 1, Vector3d::Zero()); } catch (const egs::Error &err) { threw = err.status == EGS_ERR_INVALID; }
    expect(threw && (int)s.joints().size() == j + 1, "a vanishing rail direction adds nothing");
  }
  std::printf(failures ? "slider_host_check: %d failed\n" : "slider_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
