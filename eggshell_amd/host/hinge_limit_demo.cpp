// hinge_limit_demo -- hinge angle limits through the adapter (Ensemble::SetHingeLimits / HingeAngle), for
// tests/test_gpu_adapter_limits.py.  One JSON line per scene, both on hinge_demo's door (a box on one hinge to the world
// about the horizontal y axis, its centre 0.5 m from the axis, released at rest; gravity turns it towards +theta):
//   door    limits (-inf, 0.4): 200 steps.  The largest angle HingeAngle reported and the step it was first over the
//           stop, the angle and the speed about the axis at the end, the angle of the centre about the anchor then (from
//           the body's position, not from the joint), the axis row's multiplier of the last step over the stop, the
//           largest hinge and anchor error
//   motor   SetHingeMotor(1 rad/s, 20 N m) and limits (-inf, 0.3): 150 steps.  Speed, angle and multiplier at step 40
//           (inside the range: the motor holds its speed), the largest angle, angle and speed at the end (stalled)
//   hinge_limit_demo --dense   a limited hinge with use_dense_solver: prints the status the step threw (EGS_ERR_UNSUPPORTED)
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
  s.detect_contacts = false;   // nothing touches: the door hangs 2 m above the plate
}

double max_abs(const VectorXd &v, int rows) {
  double m = 0;
  for (int i = 0; i < rows; ++i) m = std::fmax(m, std::fabs(v(i)));
  return m;
}

int door(bool motor) {
  const double hi = motor ? 0.3 : 0.4;
  const int steps = motor ? 150 : 200, mid = 40;
  Scene s;
  auto b = s.Add(Body(Vector3d(0.5, 0, 2), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
  const int h = s.AddHinge(b, 0, nullptr, -1, Vector3d(0, 0, 2), Vector3d(0, 1, 0));
  if (motor) s.SetHingeMotor(h, 1.0, 20.0);
  s.SetHingeLimits(h, -INFINITY, hi);
  s.Init();
  solver(s);
  double err = 0, max_angle = -10, lambda_stop = 0, w_mid = 0, angle_mid = 0, lambda_mid = 0;
  int first_over = -1;
  for (int k = 0; k < steps; ++k) {
    const bool over = s.HingeAngle(h) > hi;   // the pose this step assembles at
    s.Step(kDt);
    if (over) lambda_stop = s.last_lambda(3 * h + 2);
    err = std::fmax(err, std::fmax(max_abs(s.joints()[h]->ComputeError(), 2), max_abs(s.joints()[h - 1]->ComputeError(), 3)));
    const double angle = s.HingeAngle(h);
    max_angle = std::fmax(max_angle, angle);
    if (first_over < 0 && angle > hi) first_over = k;
    if (k == mid) { w_mid = b->w_g()[1]; angle_mid = angle; lambda_mid = s.last_lambda(3 * h + 2); }
  }
  const double from_position = std::atan2(2.0 - b->p()[2], b->p()[0]);
  std::printf("{\"scene\": \"%s\", \"hi\": %.17g, \"max_angle\": %.17g, \"first_over\": %d, \"angle_end\": %.17g, \"w_axis_end\": %.17g, "
              "\"angle_from_position\": %.17g, \"lambda_stop\": %.17g, \"max_err\": %.17g, \"speed\": 1.0, \"tau\": 20.0, \"w_axis_mid\": %.17g, "
              "\"angle_mid\": %.17g, \"lambda_mid\": %.17g, \"arm\": 0.5, \"tol\": %.17g, \"dt\": %.17g}\n",
              motor ? "motor" : "door", hi, max_angle, first_over, s.HingeAngle(h), b->w_g()[1], from_position, lambda_stop, err, w_mid,
              angle_mid, lambda_mid, kTol, kDt);
  return 0;
}

int dense() {
  Scene s;
  auto b = s.Add(Body(Vector3d(0.5, 0, 2), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
  const int h = s.AddHinge(b, 0, nullptr, -1, Vector3d(0, 0, 2), Vector3d(0, 1, 0));
  s.SetHingeMotor(h, 1.0, 20.0);   // (the axis row would be a box row: it is the stop that is refused)
  s.SetHingeLimits(h, -0.3, 0.3);
  s.Init();
  solver(s);
  s.use_dense_solver = true;
  try {
    s.Step(kDt);
    std::printf("{\"scene\": \"dense\", \"refused\": 0}\n");
    return 1;
  } catch (const egs::Error &err) {
    std::printf("{\"scene\": \"dense\", \"refused\": %d, \"names_hinge\": %d}\n", err.status, std::strstr(err.what(), "hinge") ? 1 : 0);
    return err.status == EGS_ERR_UNSUPPORTED ? 0 : 1;
  }
}

}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "--dense") == 0) return dense();
    return door(false) + door(true);
  } catch (const std::exception &err) {
    std::fprintf(stderr, "hinge_limit_demo: %s\n", err.what());
    return 1;
  }
}
