// slider_demo -- slider joints through the adapter (Ensemble::AddSlider / SetSliderMotor / SetSliderLimits /
// SliderPosition), for tests/test_gpu_adapter_sliders.py.  One JSON line per scene, both on one box on a rail to the
// world (a unit box, the vertical rail through its centre, x = 0 where it starts), with gravity pressing it into the
// stop it meets; every step a tolerance-terminated solve (tol 1e-10):
//   lift    the rail direction -z (x grows as the lift is lowered), SetSliderMotor(0.5 m/s, 50 N) and limits
//           (-inf, 0.1): 140 steps.  Speed along the rail, travel and multiplier at step 20 (inside the range: the motor
//           holds its speed against gravity), the largest travel and the step it was first over the stop, travel and
//           speed at the end (stalled), the rail row's multiplier of the last step over the stop
//   drawer  the rail direction +z, no motor, limits (-0.05, +inf): released at rest, 200 steps.  The smallest travel
//           SliderPosition reported and the step it was first under the stop, travel and speed at the end, the travel read from the body's centre
//           then (not from the joint), the multiplier of the last step under the stop, the largest lock and rail error
//   slider_demo --dense   a free slider with use_dense_solver: prints the status the step threw (EGS_ERR_UNSUPPORTED)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "eggshell_api.h"

namespace {

const double kDt = 5e-3, kTol = 1e-10, kZ0 = 2.0, kMass = 1.0;

Body Box(const Vector3d &p) { return Body(p, Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()); }

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
  s.detect_contacts = false;   // nothing touches: the box rides 2 m above the plate
}

double max_abs(const VectorXd &v, int rows) {
  double m = 0;
  for (int i = 0; i < rows; ++i) m = std::fmax(m, std::fabs(v(i)));
  return m;
}

int rail(bool lift) {
  const double stop = lift ? 0.1 : -0.05;
  const int steps = lift ? 140 : 200, mid = 20;
  const Vector3d dir = lift ? Vector3d(0, 0, -1) : Vector3d(0, 0, 1), start(0.25, -0.5, kZ0);
  Scene s;
  auto b = s.Add(Box(start));
  const int j = s.AddSlider(b, 0, nullptr, -1, dir);
  if (lift) { s.SetSliderMotor(j, 0.5, 50.0); s.SetSliderLimits(j, -INFINITY, stop); }
  else s.SetSliderLimits(j, stop, INFINITY);
  s.Init();
  solver(s);
  double err = 0, extreme = 0, lambda_stop = 0, v_mid = 0, x_mid = 0, lambda_mid = 0, x0 = s.SliderPosition(j);
  int first_over = -1;
  for (int k = 0; k < steps; ++k) {
    const double before = s.SliderPosition(j);   // the pose this step assembles at
    const bool over = lift ? before > stop : before < stop;
    s.Step(kDt);
    if (over) lambda_stop = s.last_lambda(3 * j + 2);
    err = std::fmax(err, std::fmax(max_abs(s.joints()[j]->ComputeError(), 2), max_abs(s.joints()[j - 1]->ComputeError(), 3)));
    const double x = s.SliderPosition(j);
    extreme = lift ? std::fmax(extreme, x) : std::fmin(extreme, x);
    if (first_over < 0 && (lift ? x > stop : x < stop)) first_over = k;
    if (k == mid) { v_mid = dir.dot(b->v()); x_mid = x; lambda_mid = s.last_lambda(3 * j + 2); }
  }
  std::printf("{\"scene\": \"%s\", \"stop\": %.17g, \"extreme\": %.17g, \"first_over\": %d, \"x_start\": %.17g, \"x_end\": %.17g, \"v_end\": %.17g, "
              "\"x_from_position\": %.17g, \"lambda_stop\": %.17g, \"max_err\": %.17g, \"speed\": 0.5, \"force\": 50.0, \"v_mid\": %.17g, "
              "\"x_mid\": %.17g, \"lambda_mid\": %.17g, \"mass\": %.17g, \"g_along\": %.17g, \"steps\": %d, \"tol\": %.17g, \"dt\": %.17g}\n",
              lift ? "lift" : "drawer", stop, extreme, first_over, x0, s.SliderPosition(j), dir.dot(b->v()), dir.dot(b->p() - start), lambda_stop, err, v_mid,
              x_mid, lambda_mid, kMass, std::fabs(dir[2]), steps, kTol, kDt);
  return 0;
}

int dense() {
  Scene s;
  auto b = s.Add(Box(Vector3d(0.25, -0.5, kZ0)));
  s.AddSlider(b, 0, nullptr, -1, Vector3d(0, 0, 1));   // free: its rail row is pinned at lo = hi = 0
  s.Init();
  solver(s);
  s.use_dense_solver = true;
  try {
    s.Step(kDt);
    std::printf("{\"scene\": \"dense\", \"refused\": 0}\n");
    return 1;
  } catch (const egs::Error &err) {
    std::printf("{\"scene\": \"dense\", \"refused\": %d, \"names_slider\": %d}\n", err.status, std::strstr(err.what(), "slider") ? 1 : 0);
    return err.status == EGS_ERR_UNSUPPORTED ? 0 : 1;
  }
}

}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "--dense") == 0) return dense();
    return rail(true) + rail(false);
  } catch (const std::exception &err) {
    std::fprintf(stderr, "slider_demo: %s\n", err.what());
    return 1;
  }
}
