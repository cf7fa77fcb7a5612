// tumble_demo -- a free brick through the adapter, for tests/test_gpu_adapter_live.py: one box of sides 0.1 x 0.3 x 0.6,
// mass 1 (I_b = diag(0.0375, 0.030833.., 0.008333..)), no gravity, no constraints, Step(1e-3) on the device world.
//   tumble_demo           four JSON lines, Ensemble::SetLiveInertia on and off for each of two starts:
//       "random": a fixed rotation that is no symmetry of the brick, w = (1, 2, 3), 1000 steps -- the largest
//                 |L - L0| / |L0| of the world angular momentum L = I_g w and the relative change of the kinetic energy;
//       "intermediate": R = 1, 5 rad/s about the intermediate axis (y) and 0.05 rad/s about the other two, 4000 steps --
//                 the steps at which the body-frame w_y first and next changes sign (-1: it never does).  A real brick
//                 flips (the tennis-racket effect); with M^-1 and the gyroscopic torque frozen at Init (quirk Q5) it
//                 does not.
//   tumble_demo --explicit   the same four lines through the explicit path of Ensemble::Step (use_device_step = false): a
//                         body without constraints is stepped on the host there (v_dot = M^-1 f), no device needed
//   tumble_demo --minv    the random start with live inertia on, one Step: R after it and the angular 3x3 of M_inverse()
//                         and the torque rows of external_force_torque(), read back from the device, one JSON line
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "eggshell_api.h"

namespace {

const double kDt = 1e-3;

Matrix3d BrickInertia() {
  const double a = 0.1, b = 0.3, c = 0.6, m = 1.0;
  Matrix3d I = Matrix3d::Zero();
  I(0, 0) = m * (b * b + c * c) / 12.0;
  I(1, 1) = m * (a * a + c * c) / 12.0;
  I(2, 2) = m * (a * a + b * b) / 12.0;
  return I;
}

Matrix3d FixedRotation() {   // the unit quaternion along (0.5, 0.1, -0.7, 0.5)
  double w = 0.5, x = 0.1, y = -0.7, z = 0.5;
  const double s = std::sqrt(w * w + x * x + y * y + z * z);
  w /= s; x /= s; y /= s; z /= s;
  Matrix3d R;
  R(0, 0) = 1 - 2 * (y * y + z * z); R(0, 1) = 2 * (x * y - w * z);     R(0, 2) = 2 * (x * z + w * y);
  R(1, 0) = 2 * (x * y + w * z);     R(1, 1) = 1 - 2 * (x * x + z * z); R(1, 2) = 2 * (y * z - w * x);
  R(2, 0) = 2 * (x * z - w * y);     R(2, 1) = 2 * (y * z + w * x);     R(2, 2) = 1 - 2 * (x * x + y * y);
  return R;
}

class FreeBrick : public Ensemble {
 public:
  FreeBrick(const Matrix3d &R, const Vector3d &w) {
    n_ = 1;
    components_.push_back(std::make_shared<Body>(Vector3d(0, 0, 10), Vector3d::Zero(), 1.0, R, w, BrickInertia()));
    detect_contacts = false;
  }
  void Init() override {
    Ensemble::Init();
    for (int k = 0; k < 3; ++k) external_force_torque_(k) = 0.0;   // no gravity: the linear rows stay the caller's
  }
};

Vector3d Momentum(const Body &b) { return b.I_g() * b.w_g(); }

void random_run(bool live, bool on_device) {
  FreeBrick brick(FixedRotation(), Vector3d(1, 2, 3));
  brick.Init();
  brick.use_device_step = on_device;
  brick.SetLiveInertia(live);
  const Body &b = *brick.components()[0];
  const Vector3d L0 = Momentum(b);
  const double E0 = 0.5 * b.w_g().dot(L0);
  double drift = 0;
  for (int s = 0; s < 1000; ++s) {
    brick.Step(kDt);
    drift = std::fmax(drift, (Momentum(b) - L0).norm() / L0.norm());
  }
  const double E1 = 0.5 * b.w_g().dot(Momentum(b));
  std::printf("{\"start\": \"random\", \"live\": %d, \"steps\": 1000, \"L_drift\": %.17g, \"energy_change\": %.17g}\n", live ? 1 : 0,
              drift, std::fabs(E1 - E0) / E0);
}

void intermediate_run(bool live, bool on_device) {
  FreeBrick brick(Matrix3d::Identity(), Vector3d(0.05, 5, 0.05));
  brick.Init();
  brick.use_device_step = on_device;
  brick.SetLiveInertia(live);
  const Body &b = *brick.components()[0];
  const Vector3d L0 = Momentum(b);
  int flip[2] = {-1, -1}, nflip = 0;
  double last = 5, drift = 0;
  for (int s = 1; s <= 4000; ++s) {
    brick.Step(kDt);
    const double wy = (b.R().transpose() * b.w_g())[1];
    if (wy * last < 0 && nflip < 2) flip[nflip++] = s;
    if (wy != 0) last = wy;
    drift = std::fmax(drift, (Momentum(b) - L0).norm() / L0.norm());
  }
  std::printf("{\"start\": \"intermediate\", \"live\": %d, \"steps\": 4000, \"flip_step\": %d, \"second_flip_step\": %d, \"L_drift\": %.17g}\n",
              live ? 1 : 0, flip[0], flip[1], drift);
}

int minv() {
  FreeBrick brick(FixedRotation(), Vector3d(1, 2, 3));
  brick.Init();
  brick.SetLiveInertia(true);
  brick.Step(kDt);
  const Body &b = *brick.components()[0];
  const MatrixXd &M = brick.M_inverse();
  const VectorXd &f = brick.external_force_torque();
  std::printf("{\"R\": [");
  for (int k = 0; k < 9; ++k) std::printf("%s%.17g", k ? ", " : "", b.R().d[k]);
  std::printf("], \"w\": [%.17g, %.17g, %.17g], \"Minv_angular\": [", b.w_g()[0], b.w_g()[1], b.w_g()[2]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) std::printf("%s%.17g", r + c ? ", " : "", M(3 + r, 3 + c));
  std::printf("], \"inv_mass\": %.17g, \"torque\": [%.17g, %.17g, %.17g], \"force\": [%.17g, %.17g, %.17g]}\n", M(0, 0), f(3), f(4),
              f(5), f(0), f(1), f(2));
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "--minv") == 0) return minv();
    const bool on_device = !(argc > 1 && std::strcmp(argv[1], "--explicit") == 0);
    for (const bool live : {true, false}) random_run(live, on_device);
    for (const bool live : {true, false}) intermediate_run(live, on_device);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "tumble_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
