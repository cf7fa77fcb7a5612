// relax_direct_demo -- Ensemble::SetRelaxationSolver for tests/test_gpu_world_stabilize_direct.py: the bent Chain(4) of
// adapter_demo through InitStabilize and PostStabilize twice, once with the default Sweep relaxation solve and once
// with Direct (egs_relax_blocks_direct).  Every number is printed with 17 significant digits, one line per array:
// "<sweep|direct>_<stab|post>_<p|v|steps|rank> values...".
#include <cstdio>

#include "eggshell_api.h"

namespace {

void print(const char *tag, const char *what, const VectorXd &v) {
  std::printf("%s_%s", tag, what);
  for (int i = 0; i < v.size(); ++i) std::printf(" %.17g", v(i));
  std::printf("\n");
}

VectorXd positions(const Ensemble &e) {
  VectorXd p(12);
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 3; ++k) p(3 * i + k) = e.components()[i]->p()[k];
  return p;
}

void run(const char *tag, Ensemble::RelaxationSolver solver) {
  Chain bent(4, Vector3d(0, 0, 2));
  bent.Init();
  bent.SetRelaxationSolver(solver);
  for (int i = 1; i < 4; ++i) {
    const Vector3d p = bent.components()[i]->p();
    bent.components()[i]->SetP(p + Vector3d(0.01 * i, -0.02 * i, 0.015 * i));
  }
  bent.InitStabilize();
  print(tag, "stab_p", positions(bent));
  std::printf("%s_stab_steps %d\n", tag, bent.last_stabilize_steps);
  for (int i = 1; i < 4; ++i) {
    const Vector3d p = bent.components()[i]->p();
    bent.components()[i]->SetP(p + Vector3d(-0.02, 0.01 * i, 0.0));
    bent.components()[i]->SetV(Vector3d(0.1, 0.0, -0.2));
  }
  bent.PostStabilize();
  print(tag, "post_p", positions(bent));
  print(tag, "post_v", bent.GetVelocities());
  std::printf("%s_post_steps %d\n", tag, bent.last_stabilize_steps);
  std::printf("%s_rank %d\n", tag, bent.last_relaxation_rank);
}

}  // namespace

int main() {
  try {
    run("sweep", Ensemble::RelaxationSolver::Sweep);
    run("direct", Ensemble::RelaxationSolver::Direct);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "relax_direct_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
