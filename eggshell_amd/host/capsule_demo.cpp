// capsule_demo -- Body::Capsule through the adapter, for tests/test_gpu_adapter_capsules.py.  One JSON line:
//   "lying"     a capsule (r = 0.1, length = 0.6, m = 2) turned to lie along x, 1 mm in the ground, 200 x Step(5e-3)
//   "on_cube"   a 0.3 cube 1 mm in the ground with the same capsule lying 1 mm in its top face, 10 x Step(5e-3)
// Each scene lists what it sent (side lengths, shapes, M^-1 blocks, external force, starting p and R) and what it holds
// after the last step (p, R, v, w per body, the contact list, lambda), so the test can run the same bodies through the
// C ABI.  SOR(1.5), at most 500 sweeps to 1e-9, cfm 0.01, erp 0.2 (Ensemble::Step's).
//   capsule_demo --refuse   Body::Capsule with length == 2 radius: prints the refusal, exits 0 if refused
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>

#include "eggshell_api.h"

namespace {

const double kDt = 5e-3, kRadius = 0.1, kLength = 0.6, kMass = 2.0;

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
Body Log(double x, double z) {   // the body's z axis (the capsule's) turned onto the world's x axis
  Body b = Body::Capsule(Vector3d(x, 0, z), Vector3d::Zero(), kRadius, kLength, kMass);
  Matrix3d R = Matrix3d::Identity();
  R(0, 0) = 0; R(0, 2) = 1; R(2, 0) = -1; R(2, 2) = 0;
  b.SetR(R);
  return b;
}

void list(const char *name, int count, const std::function<double(int)> &at, const char *tail) {
  std::printf("\"%s\": [", name);
  for (int k = 0; k < count; ++k) std::printf("%s%.17g", k ? ", " : "", at(k));
  std::printf("]%s", tail);
}

void print_sent(const Scene &s) {
  const int n = (int)s.components().size();
  list("side", 3 * n, [&](int k) { return s.components()[k / 3]->GetSideLengths()[k % 3]; }, ", ");
  list("shape", n, [&](int k) { return (double)(int)s.components()[k]->type(); }, ", ");
  list("mass", n, [&](int k) { return s.components()[k]->m(); }, ", ");
  list("I_body", 9 * n, [&](int k) { return s.components()[k / 9]->I_b().d[k % 9]; }, ", ");
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
  list("R0", 9 * (int)s.components().size(), [&](int k) { return s.components()[k / 9]->R().d[k % 9]; }, ", ");
  s.Setup();
  print_sent(s);
  for (int k = 0; k < steps; ++k) s.Step(kDt);
  print_state(s);
  std::printf("}%s", tail);
}

int refuse() {
  try {
    Body b = Body::Capsule(Vector3d(0, 0, 1), Vector3d::Zero(), kRadius, 2 * kRadius);
    (void)b;
  } catch (const egs::Error &e) {
    std::printf("{\"refused\": %d, \"message\": \"%s\"}\n", e.status, e.what());
    return e.status == EGS_ERR_INVALID ? 0 : 1;
  }
  std::printf("{\"refused\": 0}\n");
  return 1;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "--refuse") == 0) return refuse();
    std::printf("{");
    Scene lying;
    lying.Add(Log(0, kRadius - 1e-3));
    run("lying", lying, 200, ", ");
    Scene stack;
    stack.Add(Cube(0, 0.149));
    stack.Add(Log(0, 0.299 + kRadius - 1e-3));
    run("on_cube", stack, 10, "}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "capsule_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
