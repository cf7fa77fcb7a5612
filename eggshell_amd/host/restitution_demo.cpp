// restitution_demo -- a dropped Body::Sphere and a dropped flat cube through the adapter, for
// tests/test_gpu_adapter_restitution.py: each alone in its ensemble, released at rest 5 cm above the plate,
// Ensemble::SetRestitution(e, threshold), Step(5e-3) until it has come back up and turned round again.
//   restitution_demo [e = 0.8] [threshold = 0.1]
//       one JSON line per body: the normal speed before and after the impact step (the first step that turns a falling
//       body round), the contacts and the largest multiplier of that step, the height after it, and the next apex;
//       e < 0: restitution off, the body stops dead and "impact_step" is -1
//   restitution_demo --refuse   a NaN coefficient and a negative threshold: prints the two refusals, exits 0 if both
//                               were refused
// The ball's one normal row stands alone, so it is solved exactly (GS, cfm 0); the cube's four share one body and take
// the usual cfm 0.01 (SOR, 60 sweeps).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "eggshell_api.h"

namespace {

const double kDt = 5e-3, kRadius = 0.15, kDrop = 0.05;

class Scene : public Ensemble {
 public:
  void Add(const Body &b) { components_.push_back(std::make_shared<Body>(b)); n_ = (int)components_.size(); }
};

void drop(const char *name, Scene &s, double e, double threshold) {
  if (e >= 0) s.SetRestitution(e, threshold);
  int impact_step = -1, contacts = 0;
  double before = 0, after = 0, z_after = 0, apex = 0, lam = 0;
  for (int k = 0; k < 400; ++k) {
    const double v0 = s.components()[0]->v()[2];
    s.Step(kDt);
    const Body &b = *s.components()[0];
    if (impact_step < 0) {
      if (!(v0 < 0 && b.v()[2] > 0 && !s.constraints().empty())) continue;
      impact_step = k; before = v0; after = b.v()[2]; z_after = apex = b.p()[2];
      contacts = (int)s.constraints().size();
      for (int i = 0; i < (int)s.last_lambda.size(); ++i) lam = std::fmax(lam, std::fabs(s.last_lambda(i)));
      if (e < 0) break;   // the Baumgarte velocity alone: no flight to follow
      continue;
    }
    apex = std::fmax(apex, b.p()[2]);
    if (b.v()[2] <= 0) break;
  }
  std::printf("{\"body\": \"%s\", \"e\": %.17g, \"threshold\": %.17g, \"impact_step\": %d, \"contacts\": %d, \"before\": %.17g, "
              "\"after\": %.17g, \"lambda_max\": %.17g, \"z_after\": %.17g, \"apex\": %.17g, \"dt\": %.17g}\n",
              name, e, threshold, impact_step, contacts, before, after, lam, z_after, apex, kDt);
}

int refuse() {
  int refused = 0;
  Scene s;
  s.Add(Body::Sphere(Vector3d(0, 0, kRadius), Vector3d::Zero(), kRadius, 1.0));
  s.Init();
  for (int k = 0; k < 2; ++k) {
    try {
      if (k == 0) s.SetRestitution(std::nan(""), 0.0);
      else s.SetRestitution(0.5, -1.0);
      std::printf("{\"case\": %d, \"refused\": 0}\n", k);
    } catch (const egs::Error &err) {
      std::printf("{\"case\": %d, \"refused\": %d}\n", k, err.status);
      ++refused;
    }
  }
  return refused == 2 && s.restitution() < 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc > 1 && std::strcmp(argv[1], "--refuse") == 0) return refuse();
    const double e = argc > 1 ? std::atof(argv[1]) : 0.8;
    const double threshold = argc > 2 ? std::atof(argv[2]) : 0.1;
    {
      Scene ball;
      ball.Add(Body::Sphere(Vector3d(0, 0, kRadius + kDrop), Vector3d::Zero(), kRadius, 1.0));
      ball.Init();
      ball.solver_params.method = EGS_GAUSS_SEIDEL;
      ball.solver_params.max_iters = 4;
      ball.solver_params.tol = 0.0;
      ball.cfm_coeff = 0.0;
      drop("sphere", ball, e, threshold);
    }
    {
      Scene cube;
      cube.Add(Body(Vector3d(0, 0, 0.15 + kDrop), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
      cube.Init();
      cube.solver_params.method = EGS_SOR;
      cube.solver_params.omega = 1.5;
      cube.solver_params.max_iters = 60;
      cube.solver_params.tol = 0.0;
      cube.cfm_coeff = 0.01;
      drop("cube", cube, e, threshold);
    }
  } catch (const std::exception &err) {
    std::fprintf(stderr, "restitution_demo: %s\n", err.what());
    return 1;
  }
  return 0;
}
