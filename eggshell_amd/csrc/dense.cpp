// dense.cpp -- the dense and LCP entries of the C ABI: the dense system of a problem and a step solved on it
// (egs_problem_dense_*, egs_problem_step_dense), and the stateless solvers on host matrices (egs_dense_*,
// egs_mixed_constraints_*, egs_box_lcp_*) over dense_lcp.h.
#include "dense_lcp.h"
#include "dense_world.h"
#include "problem.h"

#include <cmath>
#include <limits>

using namespace egs;

namespace {

// The dense system of Ensemble::ComputeVDot (ensembles.cc:510, 513-521) from the blocks the problem holds.
egs_status build_dense_system(egs_problem *p, double cfm) {
  egs_context *ctx = p->ctx;
  if (p->precision != EGS_F64) return fail(ctx, EGS_ERR_UNSUPPORTED, "the dense path is fp64 (the reference's is)");
  if (!p->have_blocks) return fail(ctx, EGS_ERR_INVALID, "no system uploaded (set_blocks or assemble first)");
  if ((size_t)p->m * 3 > 46340) return fail(ctx, EGS_ERR_INVALID, "dense system too large (more than 2^31 entries)");
  const size_t N = (size_t)p->m * 3;
  ensure_system(p);
  p->dense_A.alloc(N * N > 0 ? N * N : 1);
  launch_dense_system(p->m, p->body0.p, p->body1.p, real<double>(p->J0), real<double>(p->J1), p->Minv_d.p, cfm,
                      p->dense_A.p, ctx->stream);
  HIPCHK(hipGetLastError());
  p->dense_cfm = cfm;
  return EGS_OK;
}

// the outcome of a direct solver, as every LCP entry reports it
egs_status lcp_result(egs_context *ctx, bool good, int piv, const std::string &msg, const char *what, int32_t *ok, int32_t *pivots) {
  if (ok) *ok = good ? 1 : 0;
  if (pivots) *pivots = piv;
  if (!good) return fail(ctx, EGS_ERR_LCP_FAILED, msg.empty() ? what : msg);
  return EGS_OK;
}

egs_status box_lcp_incremental_entry(egs_context *ctx, int algorithm, int32_t n, double *A, const double *b, const double *lo,
                                     const double *hi, int32_t max_steps, double *x, double *w, int32_t *perm, int32_t *ok,
                                     int32_t *pivots) {
  if (!ctx) return EGS_ERR_INVALID;
  if (ok) *ok = 0;
  if (n < 1 || n > kIncrementalMaxRows) return fail(ctx, EGS_ERR_INVALID, "incremental box LCP: 1 <= n <= 1024");
  if (!A || !b || !lo || !hi || !x || !w) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    int piv = 0;
    std::string msg;
    const bool good = box_lcp_incremental(ctx->stream, algorithm, n, A, b, lo, hi, x, w, perm, max_steps, 0.0, &piv, &msg);
    return lcp_result(ctx, good, piv, msg, "the box LCP solver did not reach a solution", ok, pivots);
  });
}

// ---- the front end the batch entries share ----
// page-locked staging from the context's arena, the launches bracketed for egs_kernel_time
LaunchHooks context_hooks(egs_context *ctx) {
  LaunchHooks hooks;
  hooks.take = [](void *self, size_t bytes) { return static_cast<egs_context *>(self)->pinned.take(bytes); };
  hooks.mark = [](void *self, bool begin) { record_kernel_event(static_cast<egs_context *>(self), begin); };
  hooks.self = ctx;
  return hooks;
}

void fresh_staging(egs_context *ctx) {
  HIPCHK(hipStreamSynchronize(ctx->stream));     // nothing may still be reading the staging memory
  ctx->pinned.reset();
}

// the rule of the single entry's symmetry check (dense_mixed_impl, dense_lcp.hip)
bool symmetric_enough(const double *A, int n) {
  double amax = 0.0, asym = 0.0;
  for (int i = 1; i < n; ++i)
    for (int j = 0; j < i; ++j) {
      const double v = A[(size_t)i * n + j];
      amax = std::fmax(amax, std::fabs(v));
      asym = std::fmax(asym, std::fabs(v - A[(size_t)j * n + i]));
    }
  return !(asym > 1e-10 * std::max(amax, 1e-300));
}

// Problems packed one after another: problem k's matrix at a_off[k] doubles, its vectors at v_off[k] rows; those with
// rows go to `fused` or `single`.
struct RaggedBatch {
  std::vector<int64_t> a_off, v_off;
  std::vector<int32_t> fused, single;
  int64_t at = 0, vt = 0;
  // refuse(k, too_large) is the entry's own check of problem k, made once its offsets are known: the message to fail
  // with, or an empty one; too_large: n[k]^2 is beyond int32.  Returns the first message, in problem order.
  template <class Fuse, class Refuse>
  std::string split(int count, const int32_t *n, Fuse fuse, Refuse refuse) {
    a_off.resize(count); v_off.resize(count);
    for (int k = 0; k < count; ++k) {
      const int nk = n[k];
      a_off[k] = at; v_off[k] = vt;
      std::string msg = refuse(k, (int64_t)nk * nk > INT32_MAX);
      if (!msg.empty()) return msg;
      if (nk > 0) (fuse(nk) ? fused : single).push_back(k);
      at += (int64_t)nk * nk; vt += nk;
    }
    return {};
  }
};

// the size rule of the two mixed batch entries, in `what`'s name
std::string mixed_size_refusal(const char *what, int nk, int k, bool too_large) {
  if (nk < 0) return std::string(what) + ": n < 0, problem " + std::to_string(k);
  if (too_large) return std::string(what) + ": n too large, problem " + std::to_string(k);
  return {};
}

}  // namespace

extern "C" {

egs_status egs_problem_dense_system(egs_problem *p, double cfm, double *A) {
  if (!p) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    if (egs_status st = build_dense_system(p, cfm)) return st;
    const size_t N = (size_t)p->m * 3;
    if (A && N) {
      HIPCHK(hipMemcpyAsync(A, p->dense_A.p, N * N * sizeof(double), hipMemcpyDeviceToHost, p->ctx->stream));
      HIPCHK(hipStreamSynchronize(p->ctx->stream));
    }
    return EGS_OK;
  });
}

egs_status egs_problem_dense_condition(egs_problem *p, double cfm, double *estimate) {
  if (!p || !estimate) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    if (egs_status st = build_dense_system(p, cfm)) return st;
    bool spd = true;
    *estimate = dense_condition_estimate(p->ctx->dense, 3 * p->m, p->dense_A.p, &spd);
    return EGS_OK;   // not positive definite: +inf, i.e. "ill-conditioned" to the caller (ensembles.cc:514)
  });
}

egs_status egs_dense_iterate(egs_context *ctx, int32_t N, const double *A, const double *b, const uint8_t *C, const double *lo,
                             const double *hi, const egs_solve_params *params, double *x, egs_solve_stats *stats) {
  if (!ctx) return EGS_ERR_INVALID;
  if (egs_status st = validate_params(ctx, params)) return st;
  if (N < 0 || (N > 0 && (!A || !b || !x))) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (N > 0 && (C || lo || hi) && !(C && lo && hi)) return fail(ctx, EGS_ERR_INVALID, "C, lo and hi come together (or all NULL: every row an equality)");
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<uint8_t> all_eq;
    std::vector<double> zeros;
    if (!C) { all_eq.assign((size_t)std::max(N, 1), 1); zeros.assign((size_t)std::max(N, 1), 0.0); }   // sparse_iterations.cc:229-233
    int it = 0;
    double res = 0.0;
    dense_iterate(ctx->stream, N, A, b, C ? C : all_eq.data(), lo ? lo : zeros.data(), hi ? hi : zeros.data(), params->method,
                  params->omega, params->max_iters, params->tol, x, &it, &res);
    if (stats) {
      std::memset(stats, 0, sizeof *stats);
      stats->iterations = it;
      stats->residual = res;
      stats->status = EGS_OK;
    }
    return EGS_OK;
  });
}

egs_status egs_dense_iterate_batch(egs_context *ctx, int32_t count, const int32_t *n, const double *A, const double *b, const uint8_t *C,
                                   const double *lo, const double *hi, const egs_solve_params *params, double *x, int32_t *iterations,
                                   double *residual, double *residual_history) {
  if (!ctx) return EGS_ERR_INVALID;
  if (egs_status st = validate_params(ctx, params)) return st;
  if (count < 0) return fail(ctx, EGS_ERR_INVALID, "dense iteration batch: count < 0");
  if (count == 0) return EGS_OK;
  if (!n) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  int64_t rows = 0;
  for (int k = 0; k < count; ++k) {
    if (n[k] < 0 || n[k] > 1024) return fail(ctx, EGS_ERR_INVALID, "dense iteration batch: 0 <= n <= 1024, problem " + std::to_string(k));
    rows += n[k];
  }
  if (rows > 0 && (!A || !b || !x)) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (rows > 0 && (C || lo || hi) && !(C && lo && hi)) return fail(ctx, EGS_ERR_INVALID, "C, lo and hi come together (or all NULL: every row an equality)");
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    fresh_staging(ctx);
    dense_iterate_batch(ctx->stream, context_hooks(ctx), count, n, A, b, C, lo, hi, params->method, params->omega, params->max_iters, params->tol, x,
                        iterations, residual, residual_history);
    return EGS_OK;
  });
}

egs_status egs_dense_condition(egs_context *ctx, int32_t N, const double *A, double *estimate, double *pivot_bound) {
  if (!ctx) return EGS_ERR_INVALID;
  if (N < 0 || !estimate || (N > 0 && !A)) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf<double> dA;
    dA.alloc((size_t)N * N);
    if (N) HIPCHK(hipMemcpyAsync(dA.p, A, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    bool spd = true;
    double pb = 1.0;
    *estimate = dense_condition_estimate(ctx->dense, N, dA.p, &spd, &pb);
    if (pivot_bound) *pivot_bound = spd ? pb : *estimate;
    return EGS_OK;
  });
}

egs_status egs_problem_step_dense(egs_problem *p, double dt, double erp, double cfm, int32_t use_bounds, int32_t *ok,
                                  int32_t *pivots) {
  if (!p) return EGS_ERR_INVALID;
  if (!p->have_state || !p->have_constraints) return fail(p->ctx, EGS_ERR_INVALID, "set_state and set_constraints first");
  if (!(dt > 0)) return fail(p->ctx, EGS_ERR_INVALID, "dt must be > 0");
  if (p->friction && p->dense_fric_outer == 0)
    return fail(p->ctx, EGS_ERR_UNSUPPORTED, "the dense solvers have no friction pyramid (turn friction off first)");
  if (p->friction && use_bounds != 1) return fail(p->ctx, EGS_ERR_INVALID, "the dense friction pyramid needs use_bounds = 1");
  // a hinge's axis row pinned at lo = hi = 0 does not meet Murty's preconditions (lcp.cc:161-164), and without the
  // bounds a motored one would be solved as a lambda >= 0 row
  if (p->hinges && (use_bounds & 1) == 0)
    return fail(p->ctx, EGS_ERR_UNSUPPORTED, "the dense step takes a hinge axis row as a box row: a hinge needs use_bounds bit 0");
  // whether a limited hinge's axis row is pinned or one-sided is decided on the device (limit_row): the host cannot tell
  if (p->limits)
    return fail(p->ctx, EGS_ERR_UNSUPPORTED, "the dense step has no hinge limits: hinge constraint " + std::to_string(p->limited_hinge) +
                                                 " has a stop (take the table away, or use the sweeps)");
  if (p->travels)
    return fail(p->ctx, EGS_ERR_UNSUPPORTED, "the dense step has no travel stops: slider constraint " + std::to_string(p->stopped_slider) +
                                                 " has a stop (take the table away, or use the sweeps)");
  if (p->pinned_slider >= 0)
    return fail(p->ctx, EGS_ERR_UNSUPPORTED, "the dense step cannot pin a free slider's rail row at lo = hi = 0: slider constraint " +
                                                 std::to_string(p->pinned_slider) + " (give it a motor with a force > 0, or use the sweeps)");
  if (p->hinges_pinned)
    return fail(p->ctx, EGS_ERR_UNSUPPORTED, "the dense step cannot pin a free hinge's axis row at lo = hi = 0 (give the hinge a motor with tau > 0, or use the sweeps)");
  if (ok) *ok = 0;
  return guarded(p->ctx, [&]() -> egs_status {
    egs_context *ctx = p->ctx;
    hipStream_t s = ctx->stream;
    if (stall_seen(p)) return report_stall(p);
    refresh_live_mass(p);
    do_assemble(p, dt, erp);                                  // J, err, bounds, rhs (ensembles.cc:565-570)
    if (p->m == 0) {                                           // v_dot = M^-1 f (ensembles.cc:504-505)
      zero_accumulators(p);
      do_velocity(p, dt);
      if (ok) *ok = 1;
      return EGS_OK;
    }
    if (egs_status st = build_dense_system(p, cfm)) return st;   // ensembles.cc:510, 513-521
    const size_t rows = (size_t)p->m * 3;
    if (!p->h_rows_valid || p->h_rows_eq.size() != rows) {
      p->h_rows_eq.resize(rows); p->h_rows_lo.resize(rows); p->h_rows_hi.resize(rows);
      HIPCHK(hipMemcpyAsync(p->h_rows_eq.data(), p->is_eq.p, rows, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(p->h_rows_lo.data(), p->lo.p, rows * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(p->h_rows_hi.data(), p->hi.p, rows * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      p->h_rows_valid = true;
    }
    const std::vector<uint8_t> &C = p->h_rows_eq;
    const std::vector<double> &lo = p->h_rows_lo, &hi = p->h_rows_hi;
    int piv = 0;
    std::string msg;
    bool good;
    p->dense_fric_valid = false;
    if (p->friction) {
      // the pyramid: the fixed-point iteration from the host on the matrix and right-hand side read back; rows 0 and 1
      // of a constraint with mu >= 0 are pyramid rows of its row 2 (egs_problem_set_friction's meaning)
      std::vector<double> hA(rows * rows), hb(rows), hmu((size_t)p->m), mu_row(rows), hx(rows), hw(rows);
      std::vector<int32_t> nrow(rows, -1);
      HIPCHK(hipMemcpyAsync(hA.data(), p->dense_A.p, rows * rows * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(hb.data(), real<double>(p->rhs), rows * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(hmu.data(), real<double>(p->mu), (size_t)p->m * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (size_t i = 1; i < rows; ++i)                     // the factorisations read the lower triangle: one matrix
        for (size_t j = 0; j < i; ++j) hA[j * rows + i] = hA[i * rows + j];
      for (size_t k = 0; k < rows; ++k) {
        mu_row[k] = hmu[k / 3];
        if (k % 3 < 2 && mu_row[k] >= 0.0) {
          nrow[k] = (int32_t)(k - k % 3 + 2);
          if (C[k - k % 3 + 2]) return fail(ctx, EGS_ERR_INVALID, "dense friction: the normal row of a pyramid constraint is an equality row");
        }
      }
      int out = 0;
      double change = 0.0;
      good = mixed_friction_host(ctx->dense, (int)rows, hA.data(), hb.data(), C.data(), lo.data(), hi.data(), nrow.data(), mu_row.data(), 0,
                                 p->dense_fric_outer, p->dense_fric_tol, hx.data(), hw.data(), nullptr, &piv, &out, &change, &msg);
      p->dense_fric_valid = true;
      p->dense_fric_solves = out;
      p->dense_fric_change = change;
      p->dense_fric_converged = (good && change <= p->dense_fric_tol) ? 1 : 0;
      if (good) {
        HIPCHK(hipMemcpyAsync(real<double>(p->x), hx.data(), rows * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                    // hx is this scope's
      }
    } else {
      // Lcp::MixedConstraintsSolver (ensembles.cc:531) on the device matrix; lambda lands in the problem's x
      good = dense_mixed_constraints_device(ctx->dense, (int)rows, p->dense_A.p, real<double>(p->rhs), C.data(), lo.data(), hi.data(),
                                            (use_bounds & 1) != 0, (use_bounds & 2) != 0, 0, 0.0, nullptr, nullptr, real<double>(p->x),
                                            &piv, &msg);
    }
    if (pivots) *pivots = piv;
    if (!good) return fail(ctx, EGS_ERR_LCP_FAILED, msg.empty() ? "MixedConstraintsSolver did not reach a solution" : msg);
    if (ok) *ok = 1;
    p->last_iterations = piv;
    p->have_lambda = true;
    accumulators_from_lambda(p);                              // a = M^-1 J^T lambda
    do_velocity(p, dt);                                       // ensembles.cc:535, 572
    return EGS_OK;
  });
}

egs_status egs_problem_set_dense_friction(egs_problem *p, int32_t max_outer, double tol) {
  if (!p) return EGS_ERR_INVALID;
  if (max_outer < 0) return fail(p->ctx, EGS_ERR_INVALID, "max_outer must be >= 0 (0: egs_problem_step_dense refuses friction)");
  if (!(tol >= 0)) return fail(p->ctx, EGS_ERR_INVALID, "tol must be >= 0");
  p->dense_fric_outer = max_outer;
  p->dense_fric_tol = tol;
  return EGS_OK;
}

egs_status egs_problem_dense_friction_info(egs_problem *p, int32_t *outer, int32_t *converged, double *change) {
  if (!p) return EGS_ERR_INVALID;
  if (!p->dense_fric_valid) return fail(p->ctx, EGS_ERR_INVALID, "no egs_problem_step_dense with the friction pyramid yet");
  if (outer) *outer = p->dense_fric_solves;
  if (converged) *converged = p->dense_fric_converged;
  if (change) *change = p->dense_fric_change;
  return EGS_OK;
}

egs_status egs_mixed_constraints_solve(egs_context *ctx, int32_t N, const double *A, const double *b,
                                       const uint8_t *C, const double *lo, const double *hi, int32_t use_bounds,
                                       double *x, double *w, int32_t *ok, int32_t *pivots) {
  return egs_mixed_constraints_solve_limits(ctx, N, A, b, C, lo, hi, use_bounds, 0, 0.0, x, w, ok, pivots);
}

egs_status egs_mixed_constraints_solve_limits(egs_context *ctx, int32_t N, const double *A, const double *b,
                                              const uint8_t *C, const double *lo, const double *hi, int32_t use_bounds,
                                              int32_t max_pivots, double max_seconds, double *x, double *w, int32_t *ok,
                                              int32_t *pivots) {
  if (!ctx) return EGS_ERR_INVALID;
  if (N < 0 || (N > 0 && (!A || !b || !C || !lo || !hi || !x || !w))) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (ok) *ok = 0;
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    int piv = 0;
    std::string msg;
    const bool good = dense_mixed_constraints(ctx->dense, N, A, b, C, lo, hi, (use_bounds & 1) != 0,
                                              (use_bounds & 2) != 0, x, w, &piv, &msg, max_pivots, max_seconds);
    return lcp_result(ctx, good, piv, msg, "MixedConstraintsSolver did not reach a solution", ok, pivots);
  });
}

egs_status egs_mixed_constraints_solve_batch(egs_context *ctx, int32_t count, const int32_t *n, const double *A, const double *b,
                                             const uint8_t *C, const double *lo, const double *hi, int32_t use_bounds, int32_t max_pivots,
                                             double *x, double *w, int32_t *ok, int32_t *pivots) {
  if (!ctx) return EGS_ERR_INVALID;
  // everything is checked before anything is launched or written
  if (count < 0) return fail(ctx, EGS_ERR_INVALID, "mixed constraints batch: count < 0");
  if (use_bounds < 0 || use_bounds > 3) return fail(ctx, EGS_ERR_INVALID, "mixed constraints batch: use_bounds is a mask of bits 0 and 1");
  if (max_pivots < 0) return fail(ctx, EGS_ERR_INVALID, "mixed constraints batch: max_pivots < 0");
  if (count == 0) return EGS_OK;
  if (!n || !ok) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  const bool block_pivoting = (use_bounds & 2) != 0;
  RaggedBatch batch;
  const std::string refused = batch.split(count, n, [&](int nk) { return nk <= kFusedDenseMax && !block_pivoting; },
                                          [&](int k, bool too_large) { return mixed_size_refusal("mixed constraints batch", n[k], k, too_large); });
  if (!refused.empty()) return fail(ctx, EGS_ERR_INVALID, refused);
  const std::vector<int64_t> &a_off = batch.a_off, &v_off = batch.v_off;
  const std::vector<int32_t> &fused = batch.fused, &single = batch.single;
  if (batch.vt > 0 && (!A || !b || !C || !lo || !hi || !x || !w)) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  for (int k = 0; k < count; ++k)
    if (!symmetric_enough(A + a_off[k], n[k]))
      return fail(ctx, EGS_ERR_INVALID, "A must be symmetric (J M^-1 J^T + cfm I is): problem " + std::to_string(k));
  for (int k = 0; k < count; ++k) {
    ok[k] = n[k] == 0 ? 1 : 0;
    if (pivots) pivots[k] = 0;
  }
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    if (!fused.empty()) {
      fresh_staging(ctx);
      mixed_constraints_fused(ctx->dense, context_hooks(ctx), (int)fused.size(), fused.data(), n, a_off.data(), v_off.data(), A, b, C, lo,
                              hi, (use_bounds & 1) != 0, max_pivots, x, w, ok, pivots);
    }
    // beyond the fused size, or with block pivoting: the single-problem path, one problem after another
    for (const int k : single) {
      int piv = 0;
      const bool good = dense_mixed_constraints(ctx->dense, n[k], A + a_off[k], b + v_off[k], C + v_off[k], lo + v_off[k], hi + v_off[k],
                                                (use_bounds & 1) != 0, block_pivoting, x + v_off[k], w + v_off[k], &piv, nullptr, max_pivots,
                                                0.0);
      ok[k] = good ? 1 : 0;
      if (pivots) pivots[k] = piv;
    }
    return EGS_OK;     // per-problem outcome in ok[]
  });
}

egs_status egs_mixed_friction_solve_batch(egs_context *ctx, int32_t count, const int32_t *n, const double *A, const double *b,
                                          const uint8_t *C, const double *lo, const double *hi, const int32_t *normal_row,
                                          const double *mu, int32_t max_pivots, int32_t max_outer, double tol, double *x, double *w,
                                          double *beta, int32_t *ok, int32_t *pivots, int32_t *outer, double *change) {
  if (!ctx) return EGS_ERR_INVALID;
  // everything is checked before anything is launched or written
  if (count < 0) return fail(ctx, EGS_ERR_INVALID, "mixed friction batch: count < 0");
  if (max_pivots < 0) return fail(ctx, EGS_ERR_INVALID, "mixed friction batch: max_pivots < 0");
  if (max_outer < 0) return fail(ctx, EGS_ERR_INVALID, "mixed friction batch: max_outer < 0");
  if (!(tol >= 0)) return fail(ctx, EGS_ERR_INVALID, "mixed friction batch: tol must be >= 0");
  if (count == 0) return EGS_OK;
  if (!n || !ok || !outer || !change) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  RaggedBatch batch;
  const std::string refused = batch.split(count, n, [](int nk) { return nk <= kFusedDenseMax; },
                                          [&](int k, bool too_large) { return mixed_size_refusal("mixed friction batch", n[k], k, too_large); });
  if (!refused.empty()) return fail(ctx, EGS_ERR_INVALID, refused);
  const std::vector<int64_t> &a_off = batch.a_off, &v_off = batch.v_off;
  const std::vector<int32_t> &fused = batch.fused, &single = batch.single;
  if (batch.vt > 0 && (!A || !b || !C || !lo || !hi || !normal_row || !mu || !x || !w)) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  for (int k = 0; k < count; ++k) {
    const int nk = n[k];
    const int32_t *nr = normal_row + v_off[k];
    const uint8_t *Ck = C + v_off[k];
    for (int i = 0; i < nk; ++i) {
      const int f = nr[i];
      if (f == -1) continue;
      if (f < -1 || f >= nk)
        return fail(ctx, EGS_ERR_INVALID, "mixed friction batch: normal_row out of range, problem " + std::to_string(k));
      if (Ck[f] || nr[f] != -1)
        return fail(ctx, EGS_ERR_INVALID, "mixed friction batch: a normal row must be a plain inequality row, problem " + std::to_string(k));
      if (!(mu[v_off[k] + i] >= 0))
        return fail(ctx, EGS_ERR_INVALID, "mixed friction batch: mu must be >= 0 on a pyramid row, problem " + std::to_string(k));
    }
    if (!symmetric_enough(A + a_off[k], nk))
      return fail(ctx, EGS_ERR_INVALID, "A must be symmetric (J M^-1 J^T + cfm I is): problem " + std::to_string(k));
  }
  if (max_outer == 0) max_outer = 32;
  for (int k = 0; k < count; ++k) {
    ok[k] = n[k] == 0 ? 1 : 0;
    if (pivots) pivots[k] = 0;
    outer[k] = n[k] == 0 ? 1 : 0;
    change[k] = 0.0;
  }
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    if (!fused.empty()) {
      fresh_staging(ctx);
      const MixedFrictionBatch fr{normal_row, mu, max_outer, tol, beta, outer, change};
      mixed_constraints_fused(ctx->dense, context_hooks(ctx), (int)fused.size(), fused.data(), n, a_off.data(), v_off.data(), A, b, C, lo, hi,
                              true, max_pivots, x, w, ok, pivots, &fr);
    }
    // beyond the fused size: the same iteration from the host, one problem after another
    for (const int k : single) {
      int piv = 0, out = 0;
      const int64_t v = v_off[k];
      const bool good = mixed_friction_host(ctx->dense, n[k], A + a_off[k], b + v, C + v, lo + v, hi + v, normal_row + v, mu + v,
                                            max_pivots, max_outer, tol, x + v, w + v, beta ? beta + v : nullptr, &piv, &out, &change[k],
                                            nullptr);
      ok[k] = good ? 1 : 0;
      if (pivots) pivots[k] = piv;
      outer[k] = out;
    }
    return EGS_OK;     // per-problem outcome in ok[]
  });
}

egs_status egs_box_lcp_dantzig(egs_context *ctx, int32_t n, double *A, const double *b, const double *lo, const double *hi,
                               int32_t max_steps, double *x, double *w, int32_t *perm, int32_t *ok, int32_t *pivots) {
  return box_lcp_incremental_entry(ctx, 1, n, A, b, lo, hi, max_steps, x, w, perm, ok, pivots);
}
egs_status egs_box_lcp_murty(egs_context *ctx, int32_t n, double *A, const double *b, const double *lo, const double *hi,
                             int32_t max_iterations, double *x, double *w, int32_t *perm, int32_t *ok, int32_t *iterations) {
  return box_lcp_incremental_entry(ctx, 0, n, A, b, lo, hi, max_iterations, x, w, perm, ok, iterations);
}

egs_status egs_box_lcp_batch(egs_context *ctx, int32_t algorithm, int32_t count, const int32_t *n, double *A, const double *b,
                             const double *lo, const double *hi, int32_t max_steps, double max_seconds, double *x, double *w,
                             int32_t *perm, int32_t *ok, int32_t *pivots) {
  if (!ctx) return EGS_ERR_INVALID;
  if (count < 0 || (count > 0 && (!n || !A || !b || !lo || !hi || !x || !w || !ok))) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (algorithm != 0 && algorithm != 1) return fail(ctx, EGS_ERR_INVALID, "algorithm: 0 (Murty) or 1 (Cottle-Dantzig)");
  for (int k = 0; k < count; ++k) {
    ok[k] = 0;
    if (n[k] < 1 || n[k] > kIncrementalMaxRows) return fail(ctx, EGS_ERR_INVALID, "incremental box LCP: 1 <= n <= 1024");
  }
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    box_lcp_incremental_batch(ctx->stream, algorithm, count, n, A, b, lo, hi, max_steps, max_seconds, x, w, perm, ok, pivots, nullptr);
    return EGS_OK;     // per-problem outcome in ok[]
  });
}

egs_status egs_box_lcp_schur(egs_context *ctx, int32_t n, double *A, const double *b, const double *lo, const double *hi,
                             int32_t algorithm, int32_t nub, int32_t reference_quirks, int32_t max_iterations, double max_seconds,
                             double *x, double *w, int32_t *perm, int32_t *ok, int32_t *nub_out, int32_t *pivots) {
  if (!ctx) return EGS_ERR_INVALID;
  if (ok) *ok = 0;
  if (n < 1 || nub > n) return fail(ctx, EGS_ERR_INVALID, "SolveLCP_BoxSchur: n >= 1, nub <= n");
  if (!A || !b || !lo || !hi || !x || !w) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (algorithm != 0 && algorithm != 1) return fail(ctx, EGS_ERR_INVALID, "algorithm: 0 (Murty) or 1 (Cottle-Dantzig)");
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    int piv = 0, nub_found = 0;
    std::string msg;
    const bool good = box_lcp_schur(ctx->dense, n, A, b, lo, hi, algorithm, nub, reference_quirks != 0, max_iterations, max_seconds,
                                    x, w, perm, &nub_found, &piv, &msg);
    if (nub_out) *nub_out = nub_found;
    return lcp_result(ctx, good, piv, msg, "SolveLCP_BoxSchur did not reach a solution", ok, pivots);
  });
}

egs_status egs_box_lcp_schur_batch(egs_context *ctx, int32_t algorithm, int32_t count, const int32_t *n, double *A, const double *b,
                                   const double *lo, const double *hi, const int32_t *nub, int32_t reference_quirks,
                                   int32_t max_iterations, double max_seconds, double *x, double *w, int32_t *perm, int32_t *ok,
                                   int32_t *nub_out, int32_t *pivots) {
  if (!ctx) return EGS_ERR_INVALID;
  if (count < 0 || (count > 0 && (!n || !A || !b || !lo || !hi || !x || !w || !ok))) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (algorithm != 0 && algorithm != 1) return fail(ctx, EGS_ERR_INVALID, "algorithm: 0 (Murty) or 1 (Cottle-Dantzig)");
  if (count == 0) return EGS_OK;
  // everything is checked before anything is written
  const double big = std::numeric_limits<double>::max();
  const bool q6 = reference_quirks != 0;
  RaggedBatch batch;
  const std::string refused = batch.split(
      count, n, [](int nk) { return nk <= kDantzigMaxRows; },
      [&](int k, bool too_large) -> std::string {
        const int nk = n[k];
        if (nk < 1 || (nub && nub[k] > nk)) return "SolveLCP_BoxSchur: n >= 1, nub <= n";
        if (too_large) return "SolveLCP_BoxSchur: n too large";
        const double *lk = lo + batch.v_off[k], *hk = hi + batch.v_off[k];
        const int hook = nub ? nub[k] : -1;
        for (int i = 0; i < nk; ++i) {
          // the rows the partition leaves behind the unbounded ones (toolkit/lcp.cc:660-669) go to the inner solver
          const bool bounded = hook >= 0 ? i >= hook : (q6 ? (lk[i] > -big || hk[i] < -big) : (lk[i] > -big || hk[i] < big));
          if (!bounded) continue;
          // lo <= 0 <= hi (toolkit/lcp.h:134); Dantzig also needs lo < hi (toolkit/lcp.cc:448-450)
          if (!(lk[i] <= 0.0) || !(hk[i] >= 0.0) || (algorithm == 1 && !(lk[i] < hk[i])))
            return "SolveLCP_BoxSchur: the bounded rows need lo <= 0 <= hi (and lo < hi for Cottle-Dantzig)";
        }
        return {};
      });
  if (!refused.empty()) return fail(ctx, EGS_ERR_INVALID, refused);
  const std::vector<int64_t> &a_off = batch.a_off, &v_off = batch.v_off;
  const std::vector<int32_t> &fused = batch.fused, &single = batch.single;
  for (int k = 0; k < count; ++k) ok[k] = 0;
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    if (!fused.empty()) {
      fresh_staging(ctx);
      box_lcp_schur_fused(ctx->stream, context_hooks(ctx), algorithm, (int)fused.size(), fused.data(), n, a_off.data(), v_off.data(), A, b, lo, hi,
                          nub, q6, max_iterations, max_seconds, x, w, perm, ok, nub_out, pivots);
    }
    // beyond the fused size: the single-problem path, one problem after another
    for (const int k : single) {
      int piv = 0, nub_found = 0;
      std::string msg;
      const bool good = box_lcp_schur(ctx->dense, n[k], A + a_off[k], b + v_off[k], lo + v_off[k], hi + v_off[k], algorithm,
                                      nub ? nub[k] : -1, q6, max_iterations, max_seconds, x + v_off[k], w + v_off[k],
                                      perm ? perm + v_off[k] : nullptr, &nub_found, &piv, &msg);
      ok[k] = good ? 1 : 0;
      if (nub_out) nub_out[k] = nub_found;
      if (pivots) pivots[k] = piv;
    }
    return EGS_OK;     // per-problem outcome in ok[]
  });
}

}  // extern "C"
