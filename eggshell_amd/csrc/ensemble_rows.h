// ensemble_rows.h (no HIP) -- the row order of an ensemble, decided here and nowhere else: ensemble e's constraints in
// the order its own Ensemble would list them -- its joints, then its contacts, both in list order (ensembles.cc:234-239).
// That order fixes the Murty loop's first offender and the Schur partition of the dense step (world_dense.cpp) and the
// pivots of the direct relaxation's factorisation (world_stabilize.cpp), so both plans take it from ensemble_rows.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace egs {

// the ensemble of a body: body_off [E + 1] are the ensembles' first bodies (a plain world, E = 1, needs no table)
inline int ensemble_of(int E, const std::vector<int32_t> &body_off, int32_t body) {
  return E == 1 ? 0 : (int)(std::upper_bound(body_off.begin(), body_off.end(), body) - body_off.begin()) - 1;
}

struct EnsembleRows {
  std::vector<int32_t> start;   // [E + 1] into cons
  std::vector<int32_t> cons;    // [m] constraint indices, grouped by ensemble
  int count(int e) const { return start[(size_t)e + 1] - start[(size_t)e]; }
};

// body0 / body1 [m]: the world's constraint list (a constraint belongs to the ensemble of its first body that is not
// the ground)
inline EnsembleRows ensemble_rows(int E, const std::vector<int32_t> &body_off, int m, const int32_t *body0, const int32_t *body1) {
  EnsembleRows r;
  r.start.assign((size_t)E + 1, 0);
  std::vector<int32_t> ens((size_t)m, 0);
  for (int c = 0; c < m; ++c) {
    ens[(size_t)c] = ensemble_of(E, body_off, body0[c] >= 0 ? body0[c] : body1[c]);
    ++r.start[(size_t)ens[(size_t)c] + 1];
  }
  for (int e = 0; e < E; ++e) r.start[(size_t)e + 1] += r.start[(size_t)e];
  // a stable bucket sort: the world lists joints (grouped by ensemble) before contacts (grouped by ensemble)
  r.cons.assign((size_t)m, 0);
  std::vector<int32_t> next(r.start.begin(), r.start.end() - 1);
  for (int c = 0; c < m; ++c) r.cons[(size_t)next[(size_t)ens[(size_t)c]]++] = c;
  return r;
}

}  // namespace egs
