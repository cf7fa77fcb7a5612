// hinge_demo -- welds and hinges through the adapter, for tests/test_gpu_adapter_joints.py.  One JSON line per scene:
//   door    a box on one hinge to the world about the horizontal y axis, its centre 0.5 m from the axis, released at
//           rest and swinging under gravity for 200 steps: the largest constrained angular velocity across the axis
//           (rows 0 and 1 of the hinge's Jacobian times w), the largest hinge and anchor error, the largest solve
//           residual allowed (tol), the swing reached
//   motor   the same door with SetHingeMotor(1 rad/s, 20 N m): the speed about the axis after 50 steps and the axis
//           row's multiplier then (below the limit: the motor holds its speed against gravity)
//   beam    two boxes 0.6 m apart welded to each other and the first to the world, 200 steps under gravity: how far the
//           relative orientation and the tip have moved, the largest error of the four joints
//   hinge_demo --dense-free   a free hinge with use_dense_solver: prints the status the step threw (EGS_ERR_UNSUPPORTED)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "eggshell_api.h"

namespace {

const double kDt = 5e-3, kTol = 1e-10;

class Scene : public Ensemble {
 public:
  std::shared_ptr<Body> Add(const Body &b) {
    components_.push_back(std::make_shared<Body>(b));
    n_ = (int)components_.size();
    return components_.back();
  }
};

void solver(Scene &s) {
  s.solver_params.method = EGS_SOR;
  s.solver_params.omega = 1.2;
  s.solver_params.max_iters = 5000;
  s.solver_params.tol = kTol;
  s.cfm_coeff = 0.0;
  s.detect_contacts = false;   // nothing touches: the bodies hang 2 m above the plate
}

double max_abs(const VectorXd &v, int rows) {
  double m = 0;
  for (int i = 0; i < rows; ++i) m = std::fmax(m, std::fabs(v(i)));
  return m;
}

// rows 0 and 1 of the hinge's body-0 Jacobian times the body's angular velocity: what the hinge holds at zero
double across(const Constraint &hinge, const Body &b) {
  MatrixXd J0, J1;
  ArrayXb ct;
  VectorXd lo, hi;
  hinge.ComputeJ(&J0, &J1, &ct, &lo, &hi);
  double worst = 0;
  for (int r = 0; r < 2; ++r) {
    double s = 0;
    for (int c = 0; c < 3; ++c) s += J0(r, 3 + c) * b.w_g()[c];
    worst = std::fmax(worst, std::fabs(s));
  }
  return worst;
}

int door(bool motor) {
  Scene s;
  auto b = s.Add(Body(Vector3d(0.5, 0, 2), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
  const int h = s.AddHinge(b, 0, nullptr, -1, Vector3d(0, 0, 2), Vector3d(0, 1, 0));
  if (motor) s.SetHingeMotor(h, 1.0, 20.0);
  s.Init();
  solver(s);
  double off = 0, err = 0, swing = 0;
  const int steps = motor ? 50 : 200;
  for (int k = 0; k < steps; ++k) {
    s.Step(kDt);
    off = std::fmax(off, across(*s.joints()[h], *b));
    err = std::fmax(err, std::fmax(max_abs(s.joints()[h]->ComputeError(), 2), max_abs(s.joints()[h - 1]->ComputeError(), 3)));
    swing = std::fmax(swing, std::fabs(b->p()[2] - 2.0));
  }
  if (motor)
    std::printf("{\"scene\": \"motor\", \"speed\": 1.0, \"tau\": 20.0, \"w_axis\": %.17g, \"lambda_axis\": %.17g, \"across\": %.17g, "
                "\"max_err\": %.17g, \"tol\": %.17g, \"dt\": %.17g}\n", b->w_g()[1], s.last_lambda(3 * h + 2), off, err, kTol, kDt);
  else
    std::printf("{\"scene\": \"door\", \"across\": %.17g, \"max_err\": %.17g, \"swing\": %.17g, \"w_axis\": %.17g, \"lambda_axis\": %.17g, "
                "\"tol\": %.17g, \"dt\": %.17g}\n", off, err, swing, b->w_g()[1], s.last_lambda(3 * h + 2), kTol, kDt);
  return 0;
}

int beam() {
  Scene s;
  auto a = s.Add(Body(Vector3d(0.3, 0, 2), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
  auto b = s.Add(Body(Vector3d(0.9, 0, 2), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
  s.AddWeld(a, 0, nullptr, -1, Vector3d(0, 0, 2));
  s.AddWeld(a, 0, b, 1, Vector3d(0.6, 0, 2));
  s.Init();
  solver(s);
  double twist = 0, err = 0;
  for (int k = 0; k < 200; ++k) {
    s.Step(kDt);
    const Matrix3d rel = a->R().transpose() * b->R();
    for (int i = 0; i < 9; ++i) twist = std::fmax(twist, std::fabs(rel.d[i] - (i % 4 == 0 ? 1.0 : 0.0)));
    for (const auto &j : s.joints()) err = std::fmax(err, max_abs(j->ComputeError(), 3));
  }
  std::printf("{\"scene\": \"beam\", \"twist\": %.17g, \"max_err\": %.17g, \"tip_sag\": %.17g, \"joints\": %d, \"tol\": %.17g, \"dt\": %.17g}\n",
              twist, err, 2.0 - b->p()[2], (int)s.joints().size(), kTol, kDt);
  return 0;
}

int dense_free() {
  Scene s;
  auto b = s.Add(Body(Vector3d(0.5, 0, 2), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
  s.AddHinge(b, 0, nullptr, -1, Vector3d(0, 0, 2), Vector3d(0, 1, 0));
  s.Init();
  solver(s);
  s.use_dense_solver = true;
  try {
    s.Step(kDt);
    std::printf("{\"scene\": \"dense-free\", \"refused\": 0}\n");
    return 1;
  } catch (const egs::Error &err) {
    std::printf("{\"scene\": \"dense-free\", \"refused\": %d, \"names_hinge\": %d}\n", err.status, std::strstr(err.what(), "hinge") ? 1 : 0);
    return err.status == EGS_ERR_UNSUPPORTED ? 0 : 1;
  }
}

}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "--dense-free") == 0) return dense_free();
    return door(false) + door(true) + beam();
  } catch (const std::exception &err) {
    std::fprintf(stderr, "hinge_demo: %s\n", err.what());
    return 1;
  }
}
