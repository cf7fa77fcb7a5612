// sphere_demo -- Body::Sphere through the adapter, for tests/test_gpu_adapter_spheres.py.  One JSON line:
//   "ball_ground"   a ball (r = 0.15, m = 1) dropped from 1 cm above the ground, 20 x Step(5e-3)
//   "ball_on_cube"  a 0.3 cube 1 mm in the ground with the ball 1 mm in its top face and 2 cm off its axis, 10 x Step(5e-3)
//   "group"         an EnsembleGroup of a two-ball ensemble and a two-cube ensemble, 10 x group.Step(5e-3), against
//                   identical copies stepped on their own: the largest absolute difference in any body (0 expected)
// Each scene lists what it sent (side lengths, shapes, M^-1 blocks, external force) and what it holds after the last
// step (p, R, v, w per body, the contact list, lambda), so the test can run the same bodies through the C ABI.
// SOR(1.5), at most 500 sweeps to 1e-9, cfm 0.01, erp 0.2 (Ensemble::Step's).
//   sphere_demo --refuse   a sphere ensemble with detect_contacts = false: prints the refusal, exits 0 if refused
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>

#include "eggshell_api.h"

namespace {

const double kDt = 5e-3, kRadius = 0.15;

class Scene : public Ensemble {
 public:
  void Add(const Body &b) { components_.push_back(std::make_shared<Body>(b)); n_ = (int)components_.size(); }
  const VectorXd &f_ext() const { return external_force_torque_; }
  void Setup() {
    Init();
    solver_params.method = EGS_SOR;
    solver_params.omega = 1.5;
    solver_params.max_iters = 500;
    solver_params.tol = 1e-9;
    solver_params.check_every = 1;
    cfm_coeff = 0.01;
  }
};

Body Cube(double x, double z) { return Body(Vector3d(x, 0, z), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()); }
Body Ball(double x, double y, double z) { return Body::Sphere(Vector3d(x, y, z), Vector3d::Zero(), kRadius, 1.0); }

void list(const char *name, int count, const std::function<double(int)> &at, const char *tail) {
  std::printf("\"%s\": [", name);
  for (int k = 0; k < count; ++k) std::printf("%s%.17g", k ? ", " : "", at(k));
  std::printf("]%s", tail);
}

void print_sent(const Scene &s) {
  const int n = (int)s.components().size();
  list("side", 3 * n, [&](int k) { return s.components()[k / 3]->GetSideLengths()[k % 3]; }, ", ");
  list("shape", n, [&](int k) { return s.components()[k]->type() == Body::BodyType::Sphere ? 1.0 : 0.0; }, ", ");
  list("Minv", 36 * n, [&](int k) { const int b = k / 36, r = (k % 36) / 6, c = k % 6; return s.M_inverse()(6 * b + r, 6 * b + c); }, ", ");
  list("f_ext", 6 * n, [&](int k) { return s.f_ext()(k); }, ", ");
}

void print_state(const Scene &s) {
  const int n = (int)s.components().size();
  list("p", 3 * n, [&](int k) { return s.components()[k / 3]->p()[k % 3]; }, ", ");
  list("R", 9 * n, [&](int k) { return s.components()[k / 9]->R().d[k % 9]; }, ", ");
  list("v", 3 * n, [&](int k) { return s.components()[k / 3]->v()[k % 3]; }, ", ");
  list("w", 3 * n, [&](int k) { return s.components()[k / 3]->w_g()[k % 3]; }, ", ");
  const ConstraintsList cs = s.constraints();
  list("contact_b0", (int)cs.size(), [&](int k) { return (double)cs[k]->i0_; }, ", ");
  list("contact_b1", (int)cs.size(), [&](int k) { return (double)cs[k]->i1_; }, ", ");
  list("contact_pos", 3 * (int)cs.size(), [&](int k) { return cs[k / 3]->GetConstraintPosition()[k % 3]; }, ", ");
  list("lambda", (int)s.last_lambda.size(), [&](int k) { return s.last_lambda(k); }, "");
}

void run(const char *name, Scene &s, int steps, const char *tail) {
  std::printf("\"%s\": {\"steps\": %d, ", name, steps);
  list("p0", 3 * (int)s.components().size(), [&](int k) { return s.components()[k / 3]->p()[k % 3]; }, ", ");
  s.Setup();
  print_sent(s);
  for (int k = 0; k < steps; ++k) s.Step(kDt);
  print_state(s);
  std::printf("}%s", tail);
}

void fill_balls(Scene &s) { s.Add(Ball(0, 0, kRadius - 1e-3)); s.Add(Ball(2 * kRadius - 1e-3, 0, kRadius - 1e-3)); }
void fill_cubes(Scene &s) { s.Add(Cube(0, 0.149)); s.Add(Cube(0.299, 0.149)); }

double diff(const Scene &a, const Scene &b) {
  double d = 0;
  for (size_t i = 0; i < a.components().size(); ++i) {
    const Body &x = *a.components()[i], &y = *b.components()[i];
    for (int k = 0; k < 3; ++k)
      d = std::fmax(d, std::fmax(std::fabs(x.p()[k] - y.p()[k]), std::fmax(std::fabs(x.v()[k] - y.v()[k]), std::fabs(x.w_g()[k] - y.w_g()[k]))));
    for (int k = 0; k < 9; ++k) d = std::fmax(d, std::fabs(x.R().d[k] - y.R().d[k]));
  }
  if (a.last_lambda.size() != b.last_lambda.size()) return INFINITY;
  for (int k = 0; k < (int)a.last_lambda.size(); ++k) d = std::fmax(d, std::fabs(a.last_lambda(k) - b.last_lambda(k)));
  return d;
}

int refuse() {
  Scene s;
  s.Add(Ball(0, 0, kRadius));
  s.Setup();
  s.detect_contacts = false;
  try {
    s.Step(kDt);
  } catch (const egs::Error &e) {
    std::printf("{\"refused\": %d, \"message\": \"%s\"}\n", e.status, e.what());
    return e.status == EGS_ERR_UNSUPPORTED ? 0 : 1;
  }
  std::printf("{\"refused\": 0}\n");
  return 1;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "--refuse") == 0) return refuse();
    std::printf("{");
    Scene ground;
    ground.Add(Ball(0, 0, kRadius + 0.01));
    run("ball_ground", ground, 20, ", ");
    Scene stack;
    stack.Add(Cube(0, 0.149));
    stack.Add(Ball(0.02, 0, 0.299 + kRadius - 1e-3));
    run("ball_on_cube", stack, 10, ", ");
    Scene balls, cubes, balls_alone, cubes_alone;
    fill_balls(balls); fill_cubes(cubes); fill_balls(balls_alone); fill_cubes(cubes_alone);
    for (Scene *s : {&balls, &cubes, &balls_alone, &cubes_alone}) s->Setup();
    EnsembleGroup group({&balls, &cubes});
    double d = 0;
    int contacts_balls = 0, contacts_cubes = 0, first_balls = 0;
    for (int k = 0; k < 10; ++k) {
      group.Step(kDt);
      balls_alone.Step(kDt);
      cubes_alone.Step(kDt);
      d = std::fmax(d, std::fmax(diff(balls, balls_alone), diff(cubes, cubes_alone)));
      contacts_balls = (int)balls.constraints().size();
      contacts_cubes = (int)cubes.constraints().size();
      if (k == 0) first_balls = contacts_balls;   // the balls start 1 mm into each other and are pushed apart
    }
    std::printf("\"group\": {\"steps\": 10, \"max_abs_diff\": %.17g, \"contacts_balls\": %d, \"contacts_cubes\": %d, "
                "\"contacts_balls_alone\": %d, \"contacts_cubes_alone\": %d, \"world_ensembles\": %d, \"contacts_balls_first\": %d}}\n",
                d, contacts_balls, contacts_cubes, (int)balls_alone.constraints().size(), (int)cubes_alone.constraints().size(),
                group.world_ensembles(), first_balls);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "sphere_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
