// frame_demo -- the reference's frame (model.cc:37-70: SimulationStep() steps the hanging chain with kSimTimeStep and the
// cairn with kSimTimeStep * 5) run twice, for tests/test_gpu_adapter_group.py:
//   separate: chain.Step(1e-3) five times and cairn.Step(5e-3) once per frame, each Ensemble on a world of its own;
//   group:    an identically seeded second copy through one EnsembleGroup, group.Step({1e-3, 5e-3}) and then four
//             times group.Step({1e-3, 0}) per frame: one batched world, the cairn sitting four sub-steps out.
// Setup as in model.cc:73-100: srand(seed); Chain(10, (2, 2, 1)) and Cairn(4, {-0.2, 0.2}, {-0.2, 0.2}, {1, 8}), Init() on
// both and cairn.InitStabilize().
//   frame_demo [frames = 3] [seed = 1]   one JSON line: the largest absolute difference between the two runs over every
//                                        frame's p, R, v, w of all bodies and last_lambda (it must be exactly 0), the
//                                        contact counts of both runs per frame, the group's world
//   frame_demo --mismatch                a group of two members that differ in cfm_coeff: prints the refusal, exits 0
//   frame_demo --warm [frames] [seed]    the same two runs with SetWarmStart(true, 0.01) on every Ensemble, and a third,
//                                        cold copy stepped like the separate one: "differs_from_cold" counts the frames
//                                        whose cairn lambda is not the cold run's (the history is in use)
//   frame_demo --warm-mismatch           a group whose members differ in SetWarmStart: prints the refusal, exits 0
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "eggshell_api.h"

namespace {

struct Scene {
  std::unique_ptr<Chain> chain;
  std::unique_ptr<Cairn> cairn;
  explicit Scene(unsigned seed) {
    std::srand(seed);
    chain.reset(new Chain(10, Vector3d(2, 2, 1)));
    cairn.reset(new Cairn(4, {-0.2, 0.2}, {-0.2, 0.2}, {1, 8}));
    chain->Init();
    cairn->Init();
    cairn->InitStabilize();
  }
};

// NaN counts as a difference of infinity: two runs that agree hold no NaN in different places
void widen(double a, double b, double *diff) {
  if (a == b) return;
  const double d = std::fabs(a - b);
  if (!(d <= *diff)) *diff = std::isnan(d) ? INFINITY : d;
}

void compare(const Ensemble &a, const Ensemble &b, double *diff) {
  const ComponentsList &ca = a.components(), &cb = b.components();
  if (ca.size() != cb.size()) { *diff = INFINITY; return; }
  for (size_t i = 0; i < ca.size(); ++i) {
    for (int k = 0; k < 3; ++k) {
      widen(ca[i]->p()[k], cb[i]->p()[k], diff);
      widen(ca[i]->v()[k], cb[i]->v()[k], diff);
      widen(ca[i]->w_g()[k], cb[i]->w_g()[k], diff);
    }
    for (int k = 0; k < 9; ++k) widen(ca[i]->R().d[k], cb[i]->R().d[k], diff);
  }
  if (a.last_lambda.size() != b.last_lambda.size()) { *diff = INFINITY; return; }
  for (int k = 0; k < a.last_lambda.size(); ++k) widen(a.last_lambda(k), b.last_lambda(k), diff);
}

void print_list(const char *name, const std::vector<int> &v) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", v[i]);
  std::printf("]");
}

int mismatch(bool warm) {
  Scene s(1);
  if (warm) s.cairn->SetWarmStart(true, 0.01);
  else s.cairn->cfm_coeff = 0.02;
  try {
    EnsembleGroup group({s.chain.get(), s.cairn.get()});
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
    if (argc > 1 && std::strcmp(argv[1], "--mismatch") == 0) return mismatch(false);
    if (argc > 1 && std::strcmp(argv[1], "--warm-mismatch") == 0) return mismatch(true);
    const bool warm = argc > 1 && std::strcmp(argv[1], "--warm") == 0;
    if (warm) { --argc; ++argv; }
    const int frames = argc > 1 ? std::atoi(argv[1]) : 3;
    const unsigned seed = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u;
    Scene sep(seed), grp(seed), cold(seed);
    if (warm)
      for (Scene *s : {&sep, &grp}) { s->chain->SetWarmStart(true, 0.01); s->cairn->SetWarmStart(true, 0.01); }
    int differs_from_cold = 0;
    const int chain_joints = 10;   // Chain(10): nine links' joints and the anchor
    EnsembleGroup group({grp.chain.get(), grp.cairn.get()});
    double diff = 0.0;
    std::vector<int> chain_sep, chain_grp, cairn_sep, cairn_grp;
    compare(*sep.chain, *grp.chain, &diff);   // the two copies start from the same state
    compare(*sep.cairn, *grp.cairn, &diff);
    for (int f = 0; f < frames; ++f) {
      for (int k = 0; k < 5; ++k) sep.chain->Step(1e-3);
      sep.cairn->Step(5e-3);
      group.Step({1e-3, 5e-3});
      for (int k = 0; k < 4; ++k) group.Step({1e-3, 0.0});
      compare(*sep.chain, *grp.chain, &diff);
      compare(*sep.cairn, *grp.cairn, &diff);
      if (warm) {
        cold.cairn->Step(5e-3);
        double d = 0.0;
        compare(*sep.cairn, *cold.cairn, &d);
        differs_from_cold += d != 0.0 ? 1 : 0;
      }
      chain_sep.push_back((int)sep.chain->constraints().size() - chain_joints);
      chain_grp.push_back((int)grp.chain->constraints().size() - chain_joints);
      cairn_sep.push_back((int)sep.cairn->constraints().size());
      cairn_grp.push_back((int)grp.cairn->constraints().size());
    }
    std::printf("{\"frames\": %d, \"seed\": %u, \"max_abs_diff\": ", frames, seed);
    if (std::isinf(diff)) std::printf("Infinity, ");   // (what Python's json reads)
    else std::printf("%.17g, ", diff);
    print_list("chain_contacts_separate", chain_sep); std::printf(", ");
    print_list("chain_contacts_group", chain_grp); std::printf(", ");
    print_list("cairn_contacts_separate", cairn_sep); std::printf(", ");
    print_list("cairn_contacts_group", cairn_grp);
    if (warm) std::printf(", \"differs_from_cold\": %d", differs_from_cold);
    std::printf(", \"world_ensembles\": %d, \"worlds_created\": %d}\n", group.world_ensembles(), group.worlds_created());
  } catch (const std::exception &e) {
    std::fprintf(stderr, "frame_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
