// friction_demo -- the tilted-gravity cube through the adapter, for tests/test_gpu_friction.py: one 0.3 cube of mass 1
// resting on the ground with its bottom corners `depth` below it (the collider reports vertices with z < 0), gravity
// tilted by theta with tan theta = 0.5, one Step(1e-3) of 500 sweeps at cfm 0.
//   friction_demo [mu = 0.2] [method = 1: GS | 2: SOR(1.5)] [depth = 1e-6]
//       Ensemble::SetFriction(COULOMB_PYRAMID, mu); one JSON line: the velocity after the step and Coulomb's:
//       the normal force is N = m (g cos theta + erp depth / dt^2) (the step also pushes the penetration out, erp 0.2),
//       so v_x = dt (g sin theta - mu N / m) if that is positive and 0 otherwise, v_z = erp depth / dt, the rest 0.
//   friction_demo --box      the same step with the reference's friction box: it saturates at 1 per contact
//   friction_demo --refuse   SetFriction(NO_FRICTION), SetFriction(INFINITE), a negative mu and a pyramid ensemble
//                            with use_dense_solver: prints the four refusals, exits 0 if all were refused
//   friction_demo --dense    the cube at mu 0.2 and 0.8 with use_dense_solver after SetDenseFriction(32, 1e-10), cfm 0.01
//                            (the four redundant contacts make J M^-1 J^T singular, so the cfm rule adds it): per mu one
//                            JSON line with the velocity, Coulomb's, outer and converged
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "eggshell_api.h"

namespace {

const double kG = 9.81, kTan = 0.5, kDt = 1e-3;

class TiltedCube : public Ensemble {
 public:
  explicit TiltedCube(double depth) {
    n_ = 1;
    components_.push_back(std::make_shared<Body>(Vector3d(0, 0, 0.15 - depth), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
  }
  void Init() override {
    Ensemble::Init();
    const double th = std::atan(kTan), m = components_[0]->m();
    external_force_torque_ = VectorXd::Zero(6);
    external_force_torque_(0) = m * kG * std::sin(th);
    external_force_torque_(2) = -m * kG * std::cos(th);
  }
};

int refuse() {
  int refused = 0;
  auto attempt = [&](const char *what, auto &&f) {
    try {
      f();
      std::printf("{\"case\": \"%s\", \"refused\": 0}\n", what);
    } catch (const egs::Error &e) {
      std::printf("{\"case\": \"%s\", \"refused\": %d, \"message\": \"%s\"}\n", what, e.status, e.what());
      ++refused;
    }
  };
  TiltedCube cube(1e-6);
  cube.Init();
  attempt("no_friction", [&] { cube.SetFriction(Contact::FrictionModel::NO_FRICTION); });
  attempt("infinite", [&] { cube.SetFriction(Contact::FrictionModel::INFINITE); });
  attempt("negative_mu", [&] { cube.SetFriction(Contact::FrictionModel::COULOMB_PYRAMID, -0.5); });
  cube.SetFriction(Contact::FrictionModel::COULOMB_PYRAMID, 0.5);
  cube.use_dense_solver = true;
  attempt("dense", [&] { cube.Step(kDt); });
  return refused == 4 ? 0 : 1;
}

int dense() {
  const double depth = 1e-6;
  for (const double mu : {0.2, 0.8}) {
    TiltedCube cube(depth);
    cube.Init();
    cube.cfm_coeff = 0.01;
    cube.use_dense_solver = true;
    cube.SetFriction(Contact::FrictionModel::COULOMB_PYRAMID, mu);
    cube.SetDenseFriction(32, 1e-10);
    cube.Step(kDt);
    const Body &b = *cube.components()[0];
    const double th = std::atan(kTan), erp = 0.2;
    const double normal = kG * std::cos(th) + erp * depth / (kDt * kDt);
    const double slide = kDt * (kG * std::sin(th) - mu * normal);
    std::printf("{\"mu\": %.17g, \"depth\": %.17g, \"contacts\": %d, \"v\": [%.17g, %.17g, %.17g], \"w\": [%.17g, %.17g, %.17g], "
                "\"coulomb_vx\": %.17g, \"coulomb_vz\": %.17g, \"outer\": %d, \"converged\": %d}\n",
                mu, depth, (int)cube.constraints().size(), b.v()[0], b.v()[1], b.v()[2], b.w_g()[0], b.w_g()[1], b.w_g()[2],
                slide > 0 ? slide : 0.0, erp * depth / kDt, cube.last_dense_outer, cube.last_dense_converged ? 1 : 0);
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "--refuse") == 0) return refuse();
    if (argc > 1 && std::strcmp(argv[1], "--dense") == 0) return dense();
    const bool box = argc > 1 && std::strcmp(argv[1], "--box") == 0;
    if (box) { --argc; ++argv; }
    const double mu = argc > 1 ? std::atof(argv[1]) : 0.2;
    const int method = argc > 2 ? std::atoi(argv[2]) : 1;
    const double depth = argc > 3 ? std::atof(argv[3]) : 1e-6;
    TiltedCube cube(depth);
    cube.Init();
    cube.solver_params.method = method;
    cube.solver_params.omega = 1.5;
    cube.solver_params.max_iters = 500;
    cube.solver_params.tol = 0.0;
    cube.cfm_coeff = 0.0;
    if (!box) cube.SetFriction(Contact::FrictionModel::COULOMB_PYRAMID, mu);
    cube.Step(kDt);
    const Body &b = *cube.components()[0];
    const double th = std::atan(kTan), erp = 0.2;
    const double normal = kG * std::cos(th) + erp * depth / (kDt * kDt);
    const double slide = kDt * (kG * std::sin(th) - mu * normal);
    std::printf("{\"mu\": %.17g, \"method\": %d, \"depth\": %.17g, \"box\": %d, \"contacts\": %d, "
                "\"v\": [%.17g, %.17g, %.17g], \"w\": [%.17g, %.17g, %.17g], \"coulomb_vx\": %.17g, \"coulomb_vz\": %.17g}\n",
                mu, method, depth, box ? 1 : 0, (int)cube.constraints().size(), b.v()[0], b.v()[1], b.v()[2], b.w_g()[0],
                b.w_g()[1], b.w_g()[2], slide > 0 ? slide : 0.0, erp * depth / kDt);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "friction_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
