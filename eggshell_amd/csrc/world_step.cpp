// world_step.cpp -- the sweep steps of a world, egs_world_step and egs_world_step_each (a time step and an erp per
// ensemble), with the warm start (egs_world_set_warm_start: match, solve from x0, snapshot; warm_start.h), and what the
// dense steps (world_dense.cpp) share with them: the guards, the front and the tail of a step, the coefficient fills.
#include <cmath>

#include "warm_start.h"
#include "world.h"

using namespace egs;

namespace {

// The problem's per-constraint coefficients for the current list from a per-ensemble table: joints -1, every contact
// its ensemble's coefficient (a batched world's body -> ensemble table; a plain world has one ensemble).
template <typename REAL>
void world_fill(egs_world *w, const CoeffTable &t, REAL *out) {
  egs_problem *p = w->prob;
  launch_fill_friction<REAL>(p->m, (int)w->jb0.size(), p->body0.p, p->body1.p, w->ens.n_ens > 1 ? w->ens.d_ens.p : nullptr, t.d.p,
                             out, w->ctx->stream);
  HIPCHK(hipGetLastError());
}

// dt [E] and erp [E] to the device through the page-locked block, no stream synchronisation; the tables of the step
EnsembleRates world_send_rates(egs_world *w, const double *dt, const double *erp) {
  hipStream_t s = w->ctx->stream;
  EachRates &r = w->each;
  DevBuf<int32_t> &d_ens = w->ens.d_ens;
  const size_t E = (size_t)w->ens.n_ens, bytes = E * sizeof(double);
  if (!d_ens.p) {   // a plain world: every body in ensemble 0
    d_ens.alloc((size_t)(w->n > 0 ? w->n : 1));
    HIPCHK(hipMemsetAsync(d_ens.p, 0, d_ens.count * sizeof(int32_t), s));
  }
  const bool same = r.sent.size() == 2 * E && std::memcmp(r.sent.data(), dt, bytes) == 0 &&
                    std::memcmp(r.sent.data() + E, erp, bytes) == 0;
  if (!same) {
    world_each_block(w);
    std::memcpy(r.h_block.p, dt, bytes);
    std::memcpy(r.h_block.p + E, erp, bytes);
    r.d_rates.alloc(2 * E);
    HIPCHK(hipMemcpyAsync(r.d_rates.p, r.h_block.p, 2 * bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(r.ev, s));
    r.sent.assign(r.h_block.p, r.h_block.p + 2 * E);
  }
  return EnsembleRates{d_ens.p, r.d_rates.p, r.d_rates.p + E};
}

// egs_world_step (dt_each == NULL) and egs_world_step_each (dt_each / erp_each [E], host, validated) after their guards
egs_status world_step_sweeps(egs_world *w, double dt, double erp, const double *dt_each, const double *erp_each,
                             const egs_solve_params *params, int32_t detect_contacts, egs_solve_stats *stats) {
  w->dense.was_last = false;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    PhaseTimer lap{w, w->t_phase, /*sync=*/false};
    EnsembleRates rates;
    const EnsembleRates *each = world_step_begin(w, dt_each, erp_each, detect_contacts, &lap, rates);
    egs_problem *p = w->prob;
    BatchSolveState &batch = w->ens.batch;
    const int E = w->ens.n_ens;
    const bool batched = E > 1, warm = w->ws.on;
    w->ws.last = false;
    if (w->friction.any || p->friction) world_fill_friction(w);
    if (w->restitution.any || p->restitution) world_fill_restitution(w);
    if (p->m > 0) {
      world_assemble(w, dt, erp, each);
      // x0 from the history; an ensemble without one gets its rhs rows, the default start.  The problem takes the
      // start for this solve only, also when the solve throws.
      struct GivenStart {
        egs_problem *p;
        explicit GivenStart(egs_problem *q) : p(q) { if (p) p->start_mode = EGS_START_GIVEN; }
        ~GivenStart() { if (p) p->start_mode = EGS_START_RHS; }
      };
      if (warm) world_warm_match(w, each ? each->dt : nullptr);
      egs_status st;
      {
        const GivenStart given(warm ? p : nullptr);
        st = batched ? do_solve_batch(p, params, batch) : do_solve(p, params, stats);
      }
      if (st != EGS_OK) return st;
      // the body state must not be advanced with a lambda that came out of a timed-out ordering
      // wait: look at the flag before integrating (one 4-byte read-back per step)
      HIPCHK(hipStreamSynchronize(s));
      if (stall_seen(p)) return report_stall(p);
      w->lambda_stale = false;   // x holds this step's lambda for the current list
      if (warm) { world_warm_snapshot(w, each ? each->dt : nullptr); w->ws.last = true; }
      if (batched && stats) {   // the slowest ensemble's sweep count and the largest residual
        std::memset(stats, 0, sizeof *stats);
        fill_stats(p, stats);
        for (int e = 0; e < E; ++e) {
          stats->iterations = std::max(stats->iterations, batch.h_ints.p[e]);
          const double r = batch.h_res.p[e];
          if (!std::isnan(stats->residual) && (std::isnan(r) || r > stats->residual)) stats->residual = r;   // NaN wins
        }
      }
    } else {  // no constraints: v_dot = M^-1 f (ensembles.cc:504-505)
      if (egs_status st = validate_params(w->ctx, params)) return st;
      w->lambda_stale = false;
      if (warm) world_warm_snapshot(w, each ? each->dt : nullptr);   // an empty list is a history too
      zero_accumulators(p);
      if (stats) { std::memset(stats, 0, sizeof *stats); fill_stats(p, stats); }
      if (batched) {
        std::fill(batch.h_ints.p, batch.h_ints.p + E, 0);
        std::fill(batch.h_res.p, batch.h_res.p + E, 0.0);
      }
    }
    world_integrate(w, dt, each);
    if (w->trace) { HIPCHK(hipStreamSynchronize(s)); lap(3); w->t_phase[4] += 1; }
    return EGS_OK;
  });
}

}  // namespace

namespace egs {

egs_status world_step_guard(egs_world *w, double dt, const char *fp64_what) {
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  if (!(dt > 0)) return fail(w->ctx, EGS_ERR_INVALID, "dt must be > 0");
  if (fp64_what && w->precision != EGS_F64) return fail(w->ctx, EGS_ERR_UNSUPPORTED, fp64_what);
  return EGS_OK;
}

egs_status world_each_guard(egs_world *w, int32_t n_ensembles, const double *dt, const double *erp, const char *fp64_what) {
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  if (!dt || !erp) return fail(w->ctx, EGS_ERR_INVALID, "NULL dt / erp table");
  if (egs_status st = world_check_ensembles(w, n_ensembles)) return st;
  for (int e = 0; e < n_ensembles; ++e)
    if (!(dt[e] >= 0)) return fail(w->ctx, EGS_ERR_INVALID, "dt[" + std::to_string(e) + "] must be >= 0 (0: the ensemble sits out)");
  if (fp64_what && w->precision != EGS_F64) return fail(w->ctx, EGS_ERR_UNSUPPORTED, fp64_what);
  return EGS_OK;
}

void world_each_block(egs_world *w) {
  EachRates &r = w->each;
  const size_t E = (size_t)w->ens.n_ens;
  r.h_block.alloc(2 * E + (E + 1) / 2);   // once: E is the world's
  if (!r.ev) HIPCHK(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(r.ev));   // long past by the next step: no wait in practice
}

const EnsembleRates *world_step_begin(egs_world *w, const double *dt_each, const double *erp_each, int32_t detect_contacts,
                                      PhaseTimer *lap, EnsembleRates &rates) {
  refresh_live_mass(w->prob);
  if (dt_each) rates = world_send_rates(w, dt_each, erp_each);
  if (detect_contacts) world_update_contacts(w, lap);
  return dt_each ? &rates : nullptr;
}

// The problem's friction coefficients for the list about to be solved, in the solve's precision
void world_fill_friction(egs_world *w) {
  egs_problem *p = w->prob;
  p->friction = w->friction.any && p->m > 0;
  if (!p->friction) return;
  p->mu.alloc((size_t)p->m * p->real_size());
  with_real(p, [&](auto r) { world_fill(w, w->friction, real<decltype(r)>(p->mu)); });
}

// The problem's restitution coefficients for the list about to be assembled, in fp64 (the assembly's precision)
void world_fill_restitution(egs_world *w) {
  egs_problem *p = w->prob;
  p->restitution = w->restitution.any && p->m > 0;
  if (!p->restitution) return;
  p->rest.alloc((size_t)p->m);
  p->rest_vth = w->rest_vth;
  world_fill(w, w->restitution, p->rest.p);
}

void world_assemble(egs_world *w, double dt, double erp, const EnsembleRates *each) {
  if (each) do_assemble_each(w->prob, *each);
  else do_assemble(w->prob, dt, erp);
}

void world_integrate(egs_world *w, double dt, const EnsembleRates *each) {
  egs_problem *p = w->prob;
  const BodyState state{p->pos.p, p->R.p, p->v.p, p->w.p};
  if (each) {
    do_velocity_each(p, *each);
    launch_advance_each(p->n, state, p->v6.p, each->body_ens, each->dt, w->ctx->stream);
  } else {
    do_velocity(p, dt);
    launch_advance(p->n, state, state, p->v6.p, dt, w->ctx->stream);
  }
  HIPCHK(hipGetLastError());
}

// ---- warm start (egs_world_set_warm_start) ---------------------------------------------------------------------------
// no ensemble has a history any more
void world_drop_history(egs_world *w) {
  WarmStart &ws = w->ws;
  if (!ws.on || !ws.valid.p) return;
  HIPCHK(hipMemsetAsync(ws.valid.p, 0, (size_t)w->ens.n_ens, w->ctx->stream));
  ws.mj = ws.mc = 0;
}

// x0 of the assembled list from the history (REAL [3m]), sources into ws.source, and the solve's start into the
// problem's start buffer: x0, but the rhs rows of an ensemble that sits the step out (dt_each, device, may be NULL)
void world_warm_match(egs_world *w, const double *dt_each) {
  egs_problem *p = w->prob;
  WarmStart &ws = w->ws;
  const EnsembleLayout &L = w->ens;
  hipStream_t s = w->ctx->stream;
  const int mj = (int)w->jb0.size(), mc = p->m - mj;
  const bool joints_kept = ws.mj == mj;   // (set_joints drops the history: a safeguard)
  if (!joints_kept) world_drop_history(w);
  p->start.alloc((size_t)p->m * 3 * p->real_size());
  ws.x0.alloc((size_t)p->m * 3 * p->real_size());
  ws.source.alloc((size_t)p->m);
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    MatchArgs<REAL> a;
    a.n_ens = L.n_ens; a.mj = mj; a.m_old = ws.mc; a.m_new = mc;
    if (L.n_ens > 1) { a.joint_off = L.d_joff.p; a.old_off = ws.coff.p; a.new_off = L.d_coff.p; }
    a.valid = ws.valid.p;
    a.old_b0 = ws.b0.p; a.old_b1 = ws.b1.p; a.old_pos = ws.pos.p; a.old_stride = 3;
    a.old_lambda = real<REAL>(ws.lambda);
    a.new_b0 = p->body0.p + mj; a.new_b1 = p->body1.p + mj;
    a.new_pos = p->data.p + (size_t)mj * 7; a.new_stride = 7;
    a.new_rhs = real<REAL>(p->rhs);
    a.r2 = ws.radius * ws.radius;
    a.x0 = real<REAL>(ws.x0); a.source = ws.source.p;
    a.dt = dt_each; a.start = real<REAL>(p->start);
    launch_match_contacts<REAL>(a, s);
  });
  HIPCHK(hipGetLastError());
}

// the list just solved becomes the history (x: its lambda); dt_each (device, may be NULL): who sat out
void world_warm_snapshot(egs_world *w, const double *dt_each) {
  egs_problem *p = w->prob;
  WarmStart &ws = w->ws;
  const EnsembleLayout &L = w->ens;
  hipStream_t s = w->ctx->stream;
  const int mj = (int)w->jb0.size(), mc = p->m - mj;
  const size_t rs = p->real_size(), mm = (size_t)(p->m > 0 ? p->m : 1), cc = (size_t)(mc > 0 ? mc : 1);
  HIPCHK(hipStreamSynchronize(s));   // a growing buffer is freed: the match kernel has read it by now
  ws.b0.alloc(cc); ws.b1.alloc(cc); ws.pos.alloc(cc * 3); ws.lambda.alloc(mm * 3 * rs);
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    SnapshotArgs<REAL> a;
    a.n_ens = L.n_ens; a.mj = mj; a.mc = mc;
    if (L.n_ens > 1) { a.joint_off = L.d_joff.p; a.contact_off = L.d_coff.p; }
    a.dt = dt_each;
    a.b0 = p->body0.p + mj; a.b1 = p->body1.p + mj; a.pos = p->data.p + (size_t)mj * 7; a.stride = 7;
    a.x0 = real<REAL>(ws.x0); a.x = real<REAL>(p->x);
    a.h_b0 = ws.b0.p; a.h_b1 = ws.b1.p; a.h_pos = ws.pos.p; a.h_lambda = real<REAL>(ws.lambda);
    a.valid = ws.valid.p;
    launch_warm_snapshot<REAL>(a, s);
  });
  HIPCHK(hipGetLastError());
  if (L.n_ens > 1)
    HIPCHK(hipMemcpyAsync(ws.coff.p, L.d_coff.p, ((size_t)L.n_ens + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  ws.mj = mj; ws.mc = mc;
}

}  // namespace egs

extern "C" {

egs_status egs_world_step(egs_world *w, double dt, double erp, const egs_solve_params *params,
                          int32_t detect_contacts, egs_solve_stats *stats) {
  if (!w) return EGS_ERR_INVALID;
  if (egs_status st = world_step_guard(w, dt, nullptr)) return st;
  return world_step_sweeps(w, dt, erp, nullptr, nullptr, params, detect_contacts, stats);
}

egs_status egs_world_step_each(egs_world *w, int32_t n_ensembles, const double *dt, const double *erp,
                               const egs_solve_params *params, int32_t detect_contacts, egs_solve_stats *stats) {
  if (!w) return EGS_ERR_INVALID;
  if (egs_status st = world_each_guard(w, n_ensembles, dt, erp, nullptr)) return st;
  return world_step_sweeps(w, 0.0, 0.0, dt, erp, params, detect_contacts, stats);
}

egs_status egs_world_set_warm_start(egs_world *w, int32_t enable, double match_radius) {
  if (!w) return EGS_ERR_INVALID;
  if (enable && !(match_radius >= 0)) return fail(w->ctx, EGS_ERR_INVALID, "match_radius must be >= 0");
  return guarded(w->ctx, [&]() -> egs_status {
    WarmStart &ws = w->ws;
    const size_t E = (size_t)w->ens.n_ens;
    ws.on = enable != 0;
    ws.radius = enable ? match_radius : 0.0;
    ws.last = false;
    if (ws.on) {   // switched on (or on again): no history
      ws.valid.alloc(E);
      ws.coff.alloc(E + 1);
      HIPCHK(hipMemsetAsync(ws.coff.p, 0, (E + 1) * sizeof(int32_t), w->ctx->stream));
      world_drop_history(w);
    }
    return EGS_OK;
  });
}

egs_status egs_world_get_start(egs_world *w, int32_t max_rows, int32_t *rows_out, double *x0, int32_t *source) {
  if (!w || !w->prob || !rows_out) return EGS_ERR_INVALID;
  *rows_out = 3 * w->prob->m;
  if (!w->ws.last) return fail(w->ctx, EGS_ERR_INVALID, "the last step was not a warm-started sweep step");
  if (3 * w->prob->m > max_rows) return fail(w->ctx, EGS_ERR_INVALID, "max_rows too small");
  if (!x0) return fail(w->ctx, EGS_ERR_INVALID, "x0 is NULL");
  return guarded(w->ctx, [&]() -> egs_status {
    egs_problem *p = w->prob;
    hipStream_t s = w->ctx->stream;
    const size_t rows = (size_t)p->m * 3;
    std::vector<float> tmp(p->precision == EGS_F32 ? rows : 0);
    HIPCHK(hipMemcpyAsync(tmp.empty() ? (void *)x0 : (void *)tmp.data(), w->ws.x0.p, rows * p->real_size(), hipMemcpyDeviceToHost, s));
    if (source) HIPCHK(hipMemcpyAsync(source, w->ws.source.p, (size_t)p->m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < tmp.size(); ++i) x0[i] = (double)tmp[i];
    return EGS_OK;
  });
}

}  // extern "C"
