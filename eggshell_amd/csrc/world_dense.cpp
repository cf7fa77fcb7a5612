// world_dense.cpp -- the dense steps of a world, egs_world_step_dense and egs_world_step_dense_each: one fused mixed LCP
// per ensemble (dense_world.h), the multi-launch path for the ensembles above the fused cap, the dense friction pyramid
// (egs_world_set_dense_friction) and the info entries of the last dense step.
#include <limits>

#include "dense_lcp.h"
#include "world.h"

using namespace egs;

namespace {

// The dense row space of every ensemble (egs_world_step_dense): ensemble e's constraints in the order its own
// Ensemble would list them (ensemble_rows.h), which decides the Murty loop's first offender and the Schur partition;
// workspace offsets; the fused kernel's size classes.  Host tables only: building them is not a re-plan.
void world_dense_plan(egs_world *w) {
  const egs_problem *p = w->prob;
  DenseStep &d = w->dense;
  const int E = w->ens.n_ens;
  d.rows = ensemble_rows(E, w->ens.body_off, p->m, p->h_body0.data(), p->h_body1.data());
  d.off.assign((size_t)E, 0);
  d.max_m = 0;
  for (auto &l : d.cls) l.clear();
  d.big.clear();
  int64_t off = 0;
  for (int e = 0; e < E; ++e) {
    const int me = d.rows.count(e), N = 3 * me;
    d.off[(size_t)e] = off;
    off += (int64_t)dense_ws_size((size_t)N);
    d.max_m = std::max(d.max_m, me);
    if (N == 0) continue;   // v_dot = M^-1 f (ensembles.cc:504-505): nothing to solve
    if (N <= kDenseClassRows[0]) d.cls[0].push_back(e);
    else if (N <= kDenseClassRows[1]) d.cls[1].push_back(e);
    else if (N <= kFusedDenseMax) d.cls[2].push_back(e);
    else d.big.push_back(e);
  }
  std::vector<int32_t> lists;
  for (const auto &l : d.cls) lists.insert(lists.end(), l.begin(), l.end());
  if (lists.empty()) lists.push_back(0);
  stage(w->ctx, d.cons, d.rows.cons);   // (a dense step plans only a list with constraints: not empty)
  stage(w->ctx, d.cstart, d.rows.start);
  stage(w->ctx, d.wsoff, d.off);
  stage(w->ctx, d.lists, lists);
  d.ws.alloc((size_t)(off > 0 ? off : 1));
  d.status.alloc((size_t)E);
  d.fstatus.alloc((size_t)E);
  d.big_rows_valid = false;
  d.built_for = w->replans;
}

// egs_world_step_dense's ensembles above the fused cap: the multi-launch path on each ensemble's workspace slice, one
// after another (row types and bounds read back once per re-plan).  x: the world problem's lambda.  The first
// failure's message goes to big_msg.  dt_each [E] (host, may be NULL): an ensemble with dt 0 sits out, it is not solved.
// pyramid: friction is on and egs_world_set_dense_friction allows it -- the fixed-point iteration from the host
// (mixed_friction_host) on the ensemble's matrix and right-hand side read back, beta from the read-back x.
void world_dense_big(egs_world *w, double cfm_coeff, int32_t use_bounds, double *x, std::string &big_msg, const double *dt_each,
                     bool pyramid) {
  hipStream_t s = w->ctx->stream;
  DenseStep &d = w->dense;
  if (!d.big_rows_valid) {
    size_t rows = 0;
    for (int e : d.big) rows += (size_t)d.rows_of(e);
    std::vector<double> c4(rows * 3);
    size_t r0 = 0;
    for (int e : d.big) {
      const size_t N = (size_t)d.rows_of(e);
      const double *vb = d.ws.p + d.off[(size_t)e] + dense_ws_vec(N);
      HIPCHK(hipMemcpyAsync(c4.data() + 3 * r0, vb + N, 3 * N * sizeof(double), hipMemcpyDeviceToHost, s));   // lo, hi, C
      r0 += N;
    }
    HIPCHK(hipStreamSynchronize(s));
    d.big_C.resize(rows); d.big_lo.resize(rows); d.big_hi.resize(rows);
    r0 = 0;
    for (int e : d.big) {
      const size_t N = (size_t)d.rows_of(e);
      for (size_t k = 0; k < N; ++k) {
        d.big_lo[r0 + k] = c4[3 * r0 + k];
        d.big_hi[r0 + k] = c4[3 * r0 + N + k];
        d.big_C[r0 + k] = c4[3 * r0 + 2 * N + k] != 0.0 ? 1 : 0;
      }
      r0 += N;
    }
    d.big_rows_valid = true;
  }
  size_t r0 = 0;
  for (int e : d.big) {
    const int N = d.rows_of(e);
    if (dt_each && dt_each[e] == 0.0) { r0 += (size_t)N; continue; }
    double *A = d.ws.p + d.off[(size_t)e];
    double *vb = A + dense_ws_vec((size_t)N), *xs = vb + 4 * (size_t)N;
    DenseEnsStatus &st = d.info[(size_t)e];
    bool spd = true;
    st.condition = dense_condition_estimate(w->ctx->dense, N, A, &spd);    // ensembles.cc:513-521
    st.cfm = st.condition < 1e7 ? 0.0 : cfm_coeff;
    if (st.cfm != 0.0) launch_dense_world_add_diag(A, N, st.cfm, s);
    int piv = 0;
    std::string msg;
    bool good;
    if (pyramid) {
      const size_t n = (size_t)N;
      std::vector<double> hA(n * n), hb(n), hmu(n), hx(n), hw(n);
      std::vector<int32_t> nrow(n, -1);
      HIPCHK(hipMemcpyAsync(hA.data(), A, n * n * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(hb.data(), vb, n * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (size_t i = 1; i < n; ++i)                       // the factorisations read the lower triangle: one matrix
        for (size_t j = 0; j < i; ++j) hA[j * n + i] = hA[i * n + j];
      const int mj = (int)w->jb0.size();
      for (size_t k = 0; k < n; ++k) {
        const int c = d.rows.cons[(size_t)d.rows.start[(size_t)e] + k / 3];
        hmu[k] = c < mj ? -1.0 : w->friction.h[(size_t)e];
        if (k % 3 < 2 && hmu[k] >= 0.0) nrow[k] = (int32_t)(k - k % 3 + 2);
      }
      DenseFrictionStatus &fs = d.finfo[(size_t)e];
      int out = 0;
      good = mixed_friction_host(w->ctx->dense, N, hA.data(), hb.data(), d.big_C.data() + r0, d.big_lo.data() + r0,
                                 d.big_hi.data() + r0, nrow.data(), hmu.data(), 0, d.fric_outer, d.fric_tol, hx.data(),
                                 hw.data(), nullptr, &piv, &out, &fs.change, &msg);
      fs.outer = out;
      fs.converged = (good && fs.change <= d.fric_tol) ? 1 : 0;
      if (good) {
        HIPCHK(hipMemcpyAsync(xs, hx.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                   // hx is this scope's
      }
    } else {
      good = dense_mixed_constraints_device(w->ctx->dense, N, A, vb, d.big_C.data() + r0, d.big_lo.data() + r0,
                                            d.big_hi.data() + r0, use_bounds != 0, false, 0, 0.0, nullptr, nullptr, xs, &piv, &msg);
    }
    st.ok = good ? 1 : 0;
    st.pivots = piv;
    if (good) launch_dense_world_scatter(d.cons.p + d.rows.start[(size_t)e], N, xs, x, s);
    else if (big_msg.empty()) big_msg = msg;
    r0 += (size_t)N;
  }
  HIPCHK(hipGetLastError());
}

// the friction and use_bounds arguments of the dense entries, after their step guard
egs_status world_dense_guard(egs_world *w, int32_t use_bounds) {
  if (w->friction.any && w->dense.fric_outer == 0)
    return fail(w->ctx, EGS_ERR_UNSUPPORTED, "the dense solvers have no friction pyramid (turn friction off first)");
  if (use_bounds != 0 && use_bounds != 1) return fail(w->ctx, EGS_ERR_INVALID, "use_bounds must be 0 or 1");
  if (w->friction.any && use_bounds != 1) return fail(w->ctx, EGS_ERR_INVALID, "the dense friction pyramid needs use_bounds = 1");
  // as egs_problem_step_dense: a hinge's axis row is a box row, and one pinned at lo = hi = 0 is not Murty's to solve
  bool hinges = false, pinned = false;
  int pinned_slider = -1;
  for (size_t i = 0; i < w->jkind.size(); ++i) {
    if (w->jkind[i] == EGS_JOINT_SLIDER_AXIS) {   // a slider's rail row likewise
      hinges = true;
      if (pinned_slider < 0 && (w->jmotor.empty() || !(w->jmotor[2 * i + 1] > 0))) pinned_slider = (int)i;
      continue;
    }
    if (w->jkind[i] != EGS_JOINT_HINGE_AXIS) continue;
    hinges = true;
    pinned = pinned || w->jmotor.empty() || !(w->jmotor[2 * i + 1] > 0);
  }
  if (hinges && use_bounds != 1)
    return fail(w->ctx, EGS_ERR_UNSUPPORTED, "the dense step takes a hinge axis row as a box row: a hinge needs use_bounds = 1");
  if (!w->jlimit.empty()) {   // (kept only while a hinge has a stop) pinned or one-sided is decided on the device: the host cannot tell
    int first = -1;
    limits_fault(w->jkind.size(), w->jkind.data(), w->jlimit.data(), &first);
    return fail(w->ctx, EGS_ERR_UNSUPPORTED, "the dense step has no hinge limits: hinge joint " + std::to_string(first) +
                                                 " has a stop (take the table away, or use the sweeps)");
  }
  if (!w->jtravel.empty()) {   // (kept only while a slider has a finite stop) likewise
    int first = -1;
    travel_fault(w->jkind.size(), w->jkind.data(), w->jtravel.data(), &first);
    return fail(w->ctx, EGS_ERR_UNSUPPORTED, "the dense step has no travel stops: slider joint " + std::to_string(first) +
                                                 " has a stop (take the table away, or use the sweeps)");
  }
  if (pinned_slider >= 0)
    return fail(w->ctx, EGS_ERR_UNSUPPORTED, "the dense step cannot pin a free slider's rail row at lo = hi = 0: slider joint " +
                                                 std::to_string(pinned_slider) + " (give it a motor with a force > 0, or use the sweeps)");
  if (pinned)
    return fail(w->ctx, EGS_ERR_UNSUPPORTED, "the dense step cannot pin a free hinge's axis row at lo = hi = 0 (give the hinge a motor with tau > 0, or use the sweeps)");
  return EGS_OK;
}

// egs_world_step_dense (dt_each == NULL) and egs_world_step_dense_each (dt_each / erp_each [E], host, validated) after
// their guards
egs_status world_step_direct(egs_world *w, double dt, double erp, const double *dt_each, const double *erp_each,
                             double cfm_coeff, int32_t use_bounds, int32_t detect_contacts, int32_t *n_failed) {
  DenseStep &d = w->dense;
  d.was_last = false;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    EnsembleRates rates;
    const EnsembleRates *each = world_step_begin(w, dt_each, erp_each, detect_contacts, nullptr, rates);
    egs_problem *p = w->prob;
    BatchSolveState &batch = w->ens.batch;
    const int E = w->ens.n_ens;
    if (!d.h_status) d.h_status = static_cast<DenseEnsStatus *>(d.pinned.take((size_t)E * sizeof(DenseEnsStatus)));
    d.info.assign((size_t)E, DenseEnsStatus{1.0, 0.0, 1, 0});   // contact-free ensembles: solved, no pivots
    d.finfo.assign((size_t)E, DenseFrictionStatus{0.0, 1, 1});  // (and without the pyramid: one solve)
    const bool pyramid = w->friction.any && d.fric_outer > 0;
    if (pyramid && !d.h_fstatus)
      d.h_fstatus = static_cast<DenseFrictionStatus *>(d.pinned.take((size_t)E * sizeof(DenseFrictionStatus)));
    std::string big_msg;
    bool sits_out = false;
    for (int e = 0; dt_each && e < E; ++e) sits_out |= dt_each[e] == 0.0;
    w->ws.last = false;
    if (pyramid) world_fill_friction(w);   // (the sweep steps fill whenever friction is on: the dense step solves no other)
    if (w->restitution.any || p->restitution) world_fill_restitution(w);
    if (p->m > 0) {
      world_assemble(w, dt, erp, each);                              // J, err, bounds, rhs (ensembles.cc:565-570)
      // the dense step takes no start; an ensemble sitting out keeps its history through the rows matched here
      if (w->ws.on && sits_out) world_warm_match(w, each->dt);
      if (d.built_for != w->replans) world_dense_plan(w);
      DenseWorldArgs a;
      a.cons = d.cons.p; a.cstart = d.cstart.p; a.ws_off = d.wsoff.p;
      a.body0 = p->body0.p; a.body1 = p->body1.p;
      a.J0 = real<double>(p->J0); a.J1 = real<double>(p->J1);
      a.Minv = p->Minv_d.p;
      a.rhs = real<double>(p->rhs);
      a.lo = real<double>(p->lo); a.hi = real<double>(p->hi);
      a.is_eq = p->is_eq.p;
      a.ws = d.ws.p; a.x = real<double>(p->x); a.status = d.status.p;
      a.cfm_coeff = cfm_coeff; a.use_bounds = use_bounds;
      launch_dense_world_system(a, E, d.max_m, s);                   // A_e = J M^-1 J^T (ensembles.cc:510)
      // ensembles sitting out (dt 0) are not solved: this step's fused lists go without them and their lambda rows are 0
      const int32_t *lists = d.lists.p;
      int count[3] = {(int)d.cls[0].size(), (int)d.cls[1].size(), (int)d.cls[2].size()};
      if (sits_out) {
        world_each_block(w);
        int32_t *h_lists = reinterpret_cast<int32_t *>(w->each.h_block.p + 2 * (size_t)E);
        int k = 0;
        for (int c = 0; c < 3; ++c) {
          count[c] = 0;
          for (int e : d.cls[c])
            if (dt_each[e] != 0.0) { h_lists[k++] = e; ++count[c]; }
        }
        d.lists_step.alloc((size_t)E);
        if (k > 0) HIPCHK(hipMemcpyAsync(d.lists_step.p, h_lists, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(w->each.ev, s));
        lists = d.lists_step.p;
        HIPCHK(hipMemsetAsync(a.x, 0, (size_t)p->m * 3 * sizeof(double), s));
      }
      DenseWorldFriction fa{};
      if (pyramid) {
        fa.mu = real<double>(p->mu); fa.status = d.fstatus.p;
        fa.tol = d.fric_tol; fa.max_outer = d.fric_outer;
      }
      int at = 0;
      for (int c = 0; c < 3; ++c) {                                  // the rest of ComputeVDot, one workgroup each
        if (pyramid) launch_dense_world_friction(a, fa, lists + at, count[c], c, s);
        else launch_dense_world_fused(a, lists + at, count[c], c, s);
        at += count[c];
      }
      HIPCHK(hipGetLastError());
      if (!d.big.empty()) world_dense_big(w, cfm_coeff, use_bounds, a.x, big_msg, dt_each, pyramid);   // above the fused cap
      // one read-back of the fused ensembles' figures
      if (at > 0) {
        HIPCHK(hipMemcpyAsync(d.h_status, d.status.p, (size_t)E * sizeof(DenseEnsStatus), hipMemcpyDeviceToHost, s));
        if (pyramid)
          HIPCHK(hipMemcpyAsync(d.h_fstatus, d.fstatus.p, (size_t)E * sizeof(DenseFrictionStatus), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (const auto &l : d.cls)
          for (int e : l)
            if (!(dt_each && dt_each[e] == 0.0)) {
              d.info[(size_t)e] = d.h_status[e];
              if (pyramid) d.finfo[(size_t)e] = d.h_fstatus[e];
            }
      }
    }
    int nf = 0, first = -1, max_piv = 0;
    for (int e = 0; e < E; ++e) {
      const DenseEnsStatus &st = d.info[(size_t)e];
      if (!st.ok && first < 0) first = e;
      nf += st.ok ? 0 : 1;
      max_piv = std::max(max_piv, (int)st.pivots);
      if (E > 1) { batch.h_ints.p[e] = st.pivots; batch.h_res.p[e] = std::numeric_limits<double>::quiet_NaN(); }
    }
    p->last_iterations = max_piv;
    d.was_last = true;
    if (n_failed) *n_failed = nf;
    if (nf > 0) {   // the reference Panics (ensembles.cc:531-534): no body is advanced
      std::string msg = "ensemble " + std::to_string(first) + ": MixedConstraintsSolver did not reach a solution";
      if (!big_msg.empty()) msg += " (" + big_msg + ")";
      if (nf > 1) msg += "; " + std::to_string(nf) + " of " + std::to_string(E) + " ensembles failed";
      return fail(w->ctx, EGS_ERR_LCP_FAILED, msg);
    }
    w->lambda_stale = false;   // every ensemble solved: x holds this step's lambda for the current list
    if (w->ws.on) world_warm_snapshot(w, sits_out ? each->dt : nullptr);   // the history is the dense lambda
    if (p->m > 0) accumulators_from_lambda(p);                    // a = M^-1 J^T lambda
    else zero_accumulators(p);
    world_integrate(w, dt, each);
    return EGS_OK;
  });
}

}  // namespace

extern "C" {

egs_status egs_world_step_dense(egs_world *w, double dt, double erp, double cfm_coeff, int32_t use_bounds,
                                int32_t detect_contacts, int32_t *n_failed) {
  if (!w) return EGS_ERR_INVALID;
  if (n_failed) *n_failed = 0;
  if (egs_status st = world_step_guard(w, dt, "the dense path is fp64 (the reference's is)")) return st;
  if (egs_status st = world_dense_guard(w, use_bounds)) return st;
  return world_step_direct(w, dt, erp, nullptr, nullptr, cfm_coeff, use_bounds, detect_contacts, n_failed);
}

egs_status egs_world_step_dense_each(egs_world *w, int32_t n_ensembles, const double *dt, const double *erp,
                                     double cfm_coeff, int32_t use_bounds, int32_t detect_contacts, int32_t *n_failed) {
  if (!w) return EGS_ERR_INVALID;
  if (n_failed) *n_failed = 0;
  if (egs_status st = world_each_guard(w, n_ensembles, dt, erp, "the dense path is fp64 (the reference's is)")) return st;
  if (egs_status st = world_dense_guard(w, use_bounds)) return st;
  return world_step_direct(w, 0.0, 0.0, dt, erp, cfm_coeff, use_bounds, detect_contacts, n_failed);
}

egs_status egs_world_dense_info(egs_world *w, int32_t n_ensembles, double *condition, double *cfm, int32_t *pivots,
                                int32_t *ok) {
  if (!w) return EGS_ERR_INVALID;
  if (egs_status st = world_check_ensembles(w, n_ensembles)) return st;
  if (w->dense.info.size() != (size_t)n_ensembles) return fail(w->ctx, EGS_ERR_INVALID, "no egs_world_step_dense yet");
  for (int e = 0; e < n_ensembles; ++e) {
    const DenseEnsStatus &st = w->dense.info[(size_t)e];
    if (condition) condition[e] = st.condition;
    if (cfm) cfm[e] = st.cfm;
    if (pivots) pivots[e] = st.pivots;
    if (ok) ok[e] = st.ok;
  }
  return EGS_OK;
}

egs_status egs_world_set_dense_friction(egs_world *w, int32_t max_outer, double tol) {
  if (!w) return EGS_ERR_INVALID;
  if (max_outer < 0) return fail(w->ctx, EGS_ERR_INVALID, "max_outer must be >= 0 (0: the dense steps refuse friction)");
  if (!(tol >= 0)) return fail(w->ctx, EGS_ERR_INVALID, "tol must be >= 0");
  w->dense.fric_outer = max_outer;
  w->dense.fric_tol = tol;
  return EGS_OK;
}

egs_status egs_world_dense_friction_info(egs_world *w, int32_t n_ensembles, int32_t *outer, int32_t *converged, double *change) {
  if (!w) return EGS_ERR_INVALID;
  if (egs_status st = world_check_ensembles(w, n_ensembles)) return st;
  if (w->dense.finfo.size() != (size_t)n_ensembles) return fail(w->ctx, EGS_ERR_INVALID, "no egs_world_step_dense yet");
  for (int e = 0; e < n_ensembles; ++e) {
    const DenseFrictionStatus &fs = w->dense.finfo[(size_t)e];
    if (outer) outer[e] = fs.outer;
    if (converged) converged[e] = fs.converged;
    if (change) change[e] = fs.change;
  }
  return EGS_OK;
}

}  // extern "C"
