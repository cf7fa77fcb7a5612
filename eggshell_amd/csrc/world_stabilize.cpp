// world_stabilize.cpp -- Ensemble::InitStabilize / PostStabilize (ensembles.cc:602-646) for every ensemble of a world
// on the device, by two routes: egs_world_stabilize (the relaxation solve on the sparse sweeps, stabilize.h) and
// egs_world_stabilize_direct (a rank-revealing direct solve per ensemble, stabilize_direct.h), their info entries,
// and the one-shot egs_relax_blocks_direct.
#include <cmath>

#include "stabilize.h"
#include "world.h"

using namespace egs;

namespace {

// What both routes do with their arguments: the checks -- bodies set, mode, max_steps, the direct route's rank_tol in
// its place (NULL: the sweep route has none), fp64 -- and the reference's constants of the two passes.
struct StabilizePlan {
  bool post = false, detect = false;
  int cap = 0;              // relaxation steps at most
  double h = 0.0;           // the relaxation's time step
  double threshold = 0.0;   // an ensemble is settled at err_sq <= threshold
  double scale = 0.0;       // of the relaxation velocity
};
egs_status world_stabilize_plan(egs_world *w, int32_t mode, int32_t max_steps, int32_t detect_contacts, const double *rank_tol,
                                StabilizePlan &out) {
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  if (mode != EGS_STABILIZE_INIT && mode != EGS_STABILIZE_POST)
    return fail(w->ctx, EGS_ERR_INVALID, "mode must be EGS_STABILIZE_INIT or EGS_STABILIZE_POST");
  if (max_steps < 0) return fail(w->ctx, EGS_ERR_INVALID, "max_steps must be >= 0");
  if (rank_tol && (std::isnan(*rank_tol) || *rank_tol >= 1.0))
    return fail(w->ctx, EGS_ERR_INVALID, "rank_tol must be below 1 (<= 0: 1e-10)");
  if (w->precision != EGS_F64) return fail(w->ctx, EGS_ERR_UNSUPPORTED, "stabilisation is fp64 (the reference's is)");
  constexpr double kAllowNumericalError = 1e-9, kSimTimeStep = 0.001;   // constants.h:5-6
  out.post = mode == EGS_STABILIZE_POST;
  out.detect = !out.post && detect_contacts != 0;                        // PostStabilize never detects
  out.cap = max_steps > 0 ? max_steps : out.post ? 500 : 100;            // ensembles.cc:606, PostStabilize(500)
  out.h = out.post ? kSimTimeStep * 100 : kSimTimeStep * 500;            // ensembles.cc:614, 638
  out.threshold = kAllowNumericalError;
  out.scale = -1.0 * 0.2;                                                // CalculateVelocityRelaxation(0.2)
  return EGS_OK;
}

// the ensembles a stabilise call left unsettled
int world_unsettled(const std::vector<double> &err_sq, double threshold) {
  int u = 0;
  for (double e2 : err_sq) u += !(e2 <= threshold) ? 1 : 0;   // NaN counts as unsettled
  return u;
}

// The relaxation system of egs_world_stabilize (the solve of CalculateVelocityRelaxation, ensembles.cc:659-666, as the
// adapter's stabilize.cpp sets it up): the world problem's constraint topology with M^-1 = I, every row an equality
// and rhs = err.  Made on the first stabilise call, re-topologised only when the world has re-planned since; its plan
// follows from the identity masses (isotropic: the ISO / LINSYM forms of choose_sweep may apply).
void world_relax_system(egs_world *w) {
  SweepRelax &x = w->rx;
  if (x.prob && x.built_for == w->replans) return;
  hipStream_t s = w->ctx->stream;
  const int m = w->prob->m;
  const int32_t *b0 = w->topo_b0.data(), *b1 = w->topo_b1.data();
  if (!x.prob) {
    egs_problem *created = nullptr;
    if (egs_problem_create(w->ctx, w->n, m, b0, b1, EGS_F64, &created) != EGS_OK)
      throw HipError(std::string("world: relaxation system: ") + egs_last_error(w->ctx));
    x.prob = created;
    std::vector<double> eye((size_t)(w->n > 0 ? w->n : 1) * 36, 0.0);
    for (int b = 0; b < w->n; ++b)
      for (int k = 0; k < 6; ++k) eye[(size_t)b * 36 + 7 * k] = 1.0;
    upload(x.prob->Minv_d, eye.data(), (size_t)w->n * 36, s);
    x.prob->minv_r_valid = false;   // the first solve converts the blocks and finds them isotropic
    x.prob->have_state = true;
  } else {
    problem_set_topology(x.prob, m, b0, b1, /*fresh=*/false);
  }
  egs_problem *rx = x.prob;
  const size_t rows = (size_t)(m > 0 ? m : 1) * 3;
  HIPCHK(hipMemsetAsync(rx->is_eq.p, 1, rows, s));
  x.eq_scratch.alloc(rows);
  rx->joint_pairs = w->prob->joint_pairs;
  rx->have_constraints = true;
  x.built_for = w->replans;
}

// J and err of the world's constraint list at the current body state, the blocks straight into the relaxation
// system and err as its rhs (the assembly's rhs, lo, hi and row types are not used by the relaxation).
void world_relax_assemble(egs_world *w) {
  egs_problem *p = w->prob, *rx = w->rx.prob;
  AssembleArgs a = assemble_args(p, 1.0, 0.2);
  a.J0 = rx->J0.p; a.J1 = rx->J1.p;
  a.lo = rx->lo.p; a.hi = rx->hi.p;   // read by no equality row
  a.rhs = rx->wres.p;                  // scratch: the solve writes w there
  a.err = real<double>(rx->rhs);
  a.is_eq = w->rx.eq_scratch.p;
  // no motor: the relaxation reads J and err only.  The limits stay: an active stop's err[2] = sin(theta - limit) is a
  // row of (J J^T) y = err, an inactive one's is 0 as a free hinge's
  // Likewise a slider's travel stop: err[2] = x - limit while it is active, 0 as a free hinge's axis row otherwise
  HingeTables tables = hinge_tables(p);
  tables.motor = nullptr;
  launch_assemble<double>(a, p->angular, tables, w->ctx->stream);
  HIPCHK(hipGetLastError());
  rx->have_blocks = true;
  rx->lin_neg = !rx->joint_pairs;
}

// Every ensemble's constraint list in the order its own Ensemble holds it (ensemble_rows.h), the size class of each
// (stabilize_direct.h) and the workspace of the global class: the tables of egs_world_stabilize_direct.
// Host work only, redone after a re-plan.  EGS_ERR_UNSUPPORTED, with nothing staged, if an ensemble is above the limit.
egs_status world_direct_plan(egs_world *w) {
  DirectRelax &d = w->dr;
  auto verdict = [&]() {
    return d.max_rows > kDirectMaxRows
        ? fail(w->ctx, EGS_ERR_UNSUPPORTED, "an ensemble has " + std::to_string(d.max_rows) + " rows: the direct relaxation takes at most " +
                                             std::to_string(kDirectMaxRows))
        : EGS_OK;
  };
  if (d.built_for == w->replans) return verdict();
  const egs_problem *p = w->prob;
  const int E = w->ens.n_ens;
  EnsembleRows er = ensemble_rows(E, w->ens.body_off, p->m, p->h_body0.data(), p->h_body1.data());
  d.rows.assign((size_t)E, 0);
  d.max_rows = 0;
  std::vector<int32_t> cls[kDirectClasses], lists;
  std::vector<int64_t> off((size_t)E, 0);
  int64_t total = 0;
  for (int e = 0; e < E; ++e) {
    const int rows = 3 * er.count(e);
    d.rows[(size_t)e] = rows;
    d.max_rows = std::max(d.max_rows, rows);
    cls[direct_class(rows)].push_back(e);   // an ensemble without constraints too: its err_sq = 0 ends it
    off[(size_t)e] = total;
    total += (int64_t)direct_ws_size((size_t)rows);
  }
  d.built_for = w->replans;
  if (d.max_rows > kDirectMaxRows) return verdict();
  for (int c = 0; c < kDirectClasses; ++c) {
    d.count[c] = (int)cls[c].size();
    lists.insert(lists.end(), cls[c].begin(), cls[c].end());
  }
  if (er.cons.empty()) er.cons.push_back(0);   // no constraint at all: one word, read by no kernel
  stage(w->ctx, d.cons, er.cons);
  stage(w->ctx, d.cstart, er.start);
  stage(w->ctx, d.lists, lists);
  stage(w->ctx, d.wsoff, off);
  d.ws.alloc((size_t)(total > 0 ? total : 1));
  return EGS_OK;
}

}  // namespace

extern "C" {

egs_status egs_world_stabilize(egs_world *w, int32_t mode, int32_t max_steps, int32_t detect_contacts,
                               const egs_solve_params *params, int32_t *n_unsettled) {
  if (!w) return EGS_ERR_INVALID;
  if (n_unsettled) *n_unsettled = 0;
  StabilizePlan sp;
  if (egs_status st = world_stabilize_plan(w, mode, max_steps, detect_contacts, nullptr, sp)) return st;
  // stabilize.cpp's relaxation solve: SOR, omega 1.5, cfm 0, tol 1e-11, at most 20000 sweeps, checked every 10
  egs_solve_params prm;
  egs_default_params(&prm);
  prm.method = EGS_SOR; prm.cfm = 0.0; prm.tol = 1e-11; prm.max_iters = 20000; prm.check_every = 10;
  if (params) prm = *params;
  if (egs_status st = validate_params(w->ctx, &prm)) return st;
  const int E = w->ens.n_ens;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    SweepRelax &x = w->rx;
    w->lambda_stale = true;
    world_drop_history(w);
    w->st.steps.clear(); w->st.err_sq.clear();
    x.ints.alloc(2 * (size_t)E + 5);
    x.err_sq.alloc((size_t)E);
    x.h.alloc(8);
    int32_t *h_rx = x.h.p;
    int32_t *d_active = x.ints.p, *d_steps = d_active + E, *d_count = d_steps + E, *d_jo = d_count + 1, *d_co = d_jo + 2;
    if (E > 1) {
      x.batch.segs = w->ens.batch.segs;
      x.batch.ensure(E);
    }
    PhaseTimer lap{w, w->t_stab, /*sync=*/true};
    for (int pass = 0;; ++pass) {
      if (sp.detect) world_update_contacts(w, nullptr);                  // ensembles.cc:603, 616 (pruning included)
      lap(0);
      world_relax_system(w);
      lap(1);
      egs_problem *p = w->prob, *rx = x.prob;
      if (p->m > 0) world_relax_assemble(w);
      StabErrArgs ea;
      if (E > 1) {
        ea.jo = w->ens.d_joff.p; ea.co = w->ens.d_coff.p;
      } else {   // the plain world's one ensemble: its joints, then its contacts
        h_rx[2] = 0; h_rx[3] = (int32_t)w->jb0.size(); h_rx[4] = 0; h_rx[5] = w->m_contacts;
        HIPCHK(hipMemcpyAsync(d_jo, h_rx + 2, 4 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        ea.jo = d_jo; ea.co = d_co;
      }
      ea.mj = (int32_t)w->jb0.size();
      ea.err = real<double>(rx->rhs);
      ea.active = d_active; ea.steps = d_steps; ea.err_sq = x.err_sq.p; ea.n_active = d_count;
      ea.first = pass == 0 ? 1 : 0; ea.max_steps = sp.cap; ea.threshold = sp.threshold;
      HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int32_t), s));
      launch_stab_err(ea, E, s);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(h_rx, d_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      lap(2);
      if (w->trace) w->t_stab[5] += 1;
      if (h_rx[0] == 0) break;
      // (J J^T) y = err and the list-order J^T y (ensembles.cc:659-666).  A finished ensemble is not tested and none of
      // its states is selected; the sweeps still cover it (ensembles share no body), its rows are never read.
      egs_status st = E > 1 ? do_solve_batch(rx, &prm, x.batch, d_active) : do_solve(rx, &prm, nullptr);
      if (st != EGS_OK) return st;
      lap(3);
      accumulators_from_lambda(rx);
      // a lambda out of a timed-out ordering wait moves no body (egs_world_step's rule)
      HIPCHK(hipMemcpyAsync(h_rx + 1, rx->error_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (h_rx[1] != 0) return report_stall(rx);
      StabRelaxArgs ra;
      ra.n = w->n; ra.post = sp.post ? 1 : 0;
      ra.ens = E > 1 ? w->ens.d_ens.p : nullptr; ra.active = d_active;
      ra.acc = real<double>(rx->acc);
      ra.scale = sp.scale; ra.h = sp.h;
      ra.pos = p->pos.p; ra.R = p->R.p; ra.v = p->v.p; ra.w = p->w.p;
      launch_stab_relax(ra, s);
      HIPCHK(hipGetLastError());
      lap(4);
    }
    w->st.steps.resize((size_t)E); w->st.err_sq.resize((size_t)E);
    HIPCHK(hipMemcpyAsync(w->st.steps.data(), d_steps, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(w->st.err_sq.data(), x.err_sq.p, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_unsettled) *n_unsettled = world_unsettled(w->st.err_sq, sp.threshold);
    return EGS_OK;
  });
}

egs_status egs_world_stabilize_info(egs_world *w, int32_t n_ensembles, int32_t *steps, double *err_sq) {
  if (!w) return EGS_ERR_INVALID;
  if (egs_status st = world_check_ensembles(w, n_ensembles)) return st;
  if (w->st.steps.size() != (size_t)n_ensembles) return fail(w->ctx, EGS_ERR_INVALID, "no egs_world_stabilize / egs_world_stabilize_direct yet");
  if (steps) std::copy(w->st.steps.begin(), w->st.steps.end(), steps);
  if (err_sq) std::copy(w->st.err_sq.begin(), w->st.err_sq.end(), err_sq);
  return EGS_OK;
}

egs_status egs_world_stabilize_direct(egs_world *w, int32_t mode, int32_t max_steps, int32_t detect_contacts, double rank_tol,
                                      int32_t *n_unsettled) {
  if (!w) return EGS_ERR_INVALID;
  if (n_unsettled) *n_unsettled = 0;
  StabilizePlan sp;
  if (egs_status st = world_stabilize_plan(w, mode, max_steps, detect_contacts, &rank_tol, sp)) return st;
  const int E = w->ens.n_ens;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    DirectRelax &d = w->dr;
    if (!sp.detect)   // the list the call works on is known now: refuse before anything changes
      if (egs_status st = world_direct_plan(w)) return st;
    w->lambda_stale = true;
    world_drop_history(w);
    w->st.steps.clear(); w->st.err_sq.clear(); w->st.rank.clear(); w->st.rows.clear();
    d.ints.alloc(3 * (size_t)E + 1);
    d.err_sq.alloc((size_t)E);
    d.h.alloc(16);
    StabDirectArgs a;
    a.active = d.ints.p; a.steps = a.active + E; a.rank = a.steps + E; a.n_active = a.rank + E;
    a.err_sq = d.err_sq.p;
    a.loop = sp.detect ? 0 : 1; a.post = sp.post ? 1 : 0;
    a.max_steps = sp.cap;
    a.threshold = sp.threshold;
    a.rank_tol = rank_tol > 0 ? rank_tol : 1e-10;
    a.scale = sp.scale;
    a.h = sp.h;
    for (int pass = 0;; ++pass) {
      if (sp.detect) {                                                    // ensembles.cc:603, 616 (pruning included)
        world_update_contacts(w, nullptr);
        if (egs_status st = world_direct_plan(w)) return st;              // over the limit: this pass moves no body
      }
      egs_problem *p = w->prob;
      a.as = assemble_args(p, 1.0, 0.2);
      a.limit = hinge_tables(p).limit;
      a.slider = p->sliders;
      a.travel = hinge_tables(p).travel;
      a.pos = p->pos.p; a.R = p->R.p; a.v = p->v.p; a.w = p->w.p;
      a.cons = d.cons.p; a.cstart = d.cstart.p;
      a.bo = E > 1 ? w->ens.d_boff.p : nullptr;
      a.ws_off = d.wsoff.p; a.ws = d.ws.p;
      a.first = pass == 0 ? 1 : 0;
      HIPCHK(hipMemsetAsync(a.n_active, 0, sizeof(int32_t), s));
      int at = 0;
      for (int c = 0; c < kDirectClasses; ++c) {
        launch_stab_direct(a, d.lists.p + at, d.count[c], c, s);
        at += d.count[c];
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(d.h.p, a.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (!sp.detect || d.h.p[0] == 0) break;
    }
    w->st.steps.resize((size_t)E); w->st.err_sq.resize((size_t)E); w->st.rank.resize((size_t)E);
    HIPCHK(hipMemcpyAsync(w->st.steps.data(), a.steps, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(w->st.rank.data(), a.rank, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(w->st.err_sq.data(), a.err_sq, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    w->st.rows = d.rows;
    if (n_unsettled) *n_unsettled = world_unsettled(w->st.err_sq, sp.threshold);
    return EGS_OK;
  });
}

egs_status egs_world_stabilize_rank(egs_world *w, int32_t n_ensembles, int32_t *rows, int32_t *rank) {
  if (!w) return EGS_ERR_INVALID;
  if (egs_status st = world_check_ensembles(w, n_ensembles)) return st;
  if (w->st.rank.size() != (size_t)n_ensembles) return fail(w->ctx, EGS_ERR_INVALID, "no egs_world_stabilize_direct yet");
  if (rows) std::copy(w->st.rows.begin(), w->st.rows.end(), rows);
  if (rank) std::copy(w->st.rank.begin(), w->st.rank.end(), rank);
  return EGS_OK;
}

egs_status egs_relax_blocks_direct(egs_context *ctx, int32_t n_bodies, int32_t m, const int32_t *body0, const int32_t *body1,
                                   const double *J0, const double *J1, const double *err, double rank_tol, double *y,
                                   int32_t *rank) {
  if (!ctx) return EGS_ERR_INVALID;
  if (!rank || (m > 0 && (!J0 || !J1 || !err || !y))) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (std::isnan(rank_tol) || rank_tol >= 1.0) return fail(ctx, EGS_ERR_INVALID, "rank_tol must be below 1 (<= 0: 1e-10)");
  if (egs_status st = check_topology(ctx, n_bodies, m, body0, body1)) return st;
  if (3 * (int64_t)m > kDirectMaxRows) return fail(ctx, EGS_ERR_UNSUPPORTED, "the direct relaxation takes at most 1024 rows");
  *rank = 0;
  if (m == 0) return EGS_OK;
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t mm = (size_t)m;
    DevBuf<int32_t> db, dr;
    DevBuf<double> dJ, dv, dws;
    db.alloc(2 * mm); dr.alloc(1); dJ.alloc(36 * mm); dv.alloc(6 * mm);
    dws.alloc(std::max<size_t>(direct_ws_size(3 * mm), 1));
    HIPCHK(hipMemcpyAsync(db.p, body0, mm * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(db.p + mm, body1, mm * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dJ.p, J0, 18 * mm * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dJ.p + 18 * mm, J1, 18 * mm * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dv.p, err, 3 * mm * sizeof(double), hipMemcpyHostToDevice, s));
    RelaxDirectArgs a;
    a.m = m; a.body0 = db.p; a.body1 = db.p + mm; a.J0 = dJ.p; a.J1 = dJ.p + 18 * mm; a.err = dv.p;
    a.rank_tol = rank_tol > 0 ? rank_tol : 1e-10;
    a.ws = dws.p; a.y = dv.p + 3 * mm; a.rank = dr.p;
    launch_relax_direct(a, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(y, a.y, 3 * mm * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(rank, dr.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return EGS_OK;
  });
}

}  // extern "C"
