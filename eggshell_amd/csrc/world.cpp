// world.cpp -- struct egs_world and the egs_world_* entries of the C ABI, with the stateless egs_update_contacts[_joints]:
// Ensemble::Step (ensembles.cc:390-427) resident on the device, for one ensemble or a batch of them, on the sparse
// sweeps (egs_world_step), the dense path (egs_world_step_dense), either with a time step and an erp per ensemble
// (egs_world_step_each, egs_world_step_dense_each), and the stabilisation passes (egs_world_stabilize,
// egs_world_stabilize_direct), the warm start of the sweep steps (egs_world_set_warm_start: match, solve from x0,
// snapshot; warm_start.h), and the one-shot egs_relax_blocks_direct.
// The world works on its egs_problem through problem.h.
#include <chrono>
#include <cmath>
#include <limits>

#include "collide.h"
#include "dense_lcp.h"
#include "dense_world.h"
#include "problem.h"
#include "stabilize.h"
#include "stabilize_direct.h"
#include "warm_start.h"

using namespace egs;

// ---------------------------------------------------------------------------
// Body state lives in the current egs_problem's buffers; each step runs
// UpdateContacts (Collider) -> [re-plan only if the constraint topology
// changed] -> assemble -> solve -> velocity -> StepPositions_ODE, and only the
// contact topology (8 bytes per contact) crosses PCIe, to feed the host plan.
struct egs_world {
  egs_context *ctx = nullptr;
  int n = 0, precision = EGS_F64;
  egs_problem *prob = nullptr;
  DevBuf<double> dside;
  // egs_world_set_shapes: egs_shape per body on the device, handed to every Collider::run (shapes = false: NULL, the
  // all-box launches); host copies of the shapes and the side lengths, for the check that a sphere's sides are (d, d, d)
  bool shapes = false;
  DevBuf<int32_t> dshape;
  std::vector<int32_t> h_shape;
  std::vector<double> h_side;
  Collider col;
  std::vector<int32_t> jb0, jb1;       // permanent constraints (joints), listed first (ensembles.cc:234-239)
  std::vector<double> jdata;
  DevBuf<int32_t> djb0, djb1;          // the same on the device, for joint-vs-contact pruning
  DevBuf<double> djdata;
  std::vector<int32_t> topo_b0, topo_b1;
  PinnedArena topo_pinned;             // page-locked landing area for the contact topology
  int32_t *h_b0 = nullptr, *h_b1 = nullptr;
  size_t h_cap = 0;
  int m_contacts = 0;
  int replans = 0;
  bool have_bodies = false;
  // batched world (egs_world_create_batch, n_ens > 1): bodies, joints and contacts are grouped by ensemble
  int n_ens = 1;
  std::vector<int32_t> body_off, joint_off;   // [n_ens + 1]
  DevBuf<int32_t> d_ens, d_boff, d_joff;       // body -> ensemble [n], body and joint offsets [n_ens + 1]
  DevBuf<int32_t> d_coff;                      // contact offsets [n_ens + 1], written by the collider
  BatchSolveState batch;
  // egs_world_step_each / _dense_each: dt [E] | erp [E] on the device and the values last sent (an equal pair is not
  // sent again); the page-locked block they go through -- dt, erp, then the E list words of a dense step with
  // ensembles sitting out -- and the event behind the last copy out of it; that step's fused lists.  A plain world
  // gets its body -> ensemble table (all 0) on its first such step.
  DevBuf<double> d_rates;
  std::vector<double> rates_sent;
  PinnedBuf<double> h_each;
  hipEvent_t each_ev = nullptr;
  DevBuf<int32_t> dn_lists_step;
  // egs_world_step_dense: each ensemble's dense row space (its joints, then its contacts, as its own Ensemble lists
  // them), built on the first dense step after a re-plan; the figures of the last dense step
  int dense_plan_replans = -1;           // w->replans the tables below were built for
  std::vector<int32_t> dn_start;         // [E + 1] into dn_cons (host copy)
  std::vector<int64_t> dn_off;           // [E] workspace offsets (host copy)
  std::vector<int32_t> dn_class[3], dn_big;   // ensembles per fused size class; above the fused cap
  int dn_max_m = 0;
  DevBuf<int32_t> dn_cons, dn_cstart, dn_lists;
  DevBuf<int64_t> dn_wsoff;
  DevBuf<double> dn_ws;
  DevBuf<DenseEnsStatus> dn_status;
  std::vector<uint8_t> dn_big_C;         // C / lo / hi of the ensembles above the cap, read back once per re-plan
  std::vector<double> dn_big_lo, dn_big_hi;
  bool dn_big_rows_valid = false;
  PinnedArena dn_pinned;
  DenseEnsStatus *h_dn_status = nullptr;
  std::vector<DenseEnsStatus> dn_info;   // [E] of the last dense step
  bool last_dense = false;               // the last step was egs_world_step_dense (batch_info reports its pivots)
  // egs_world_stabilize, all made on its first call: the relaxation system (the world's topology with M^-1 = I, every
  // row an equality, rhs = err; re-topologised when the world re-plans), its batched stopping state, and per ensemble
  // active [E], steps [E], err_sq [E]; a plain world's row offsets jo / co [2] each
  egs_problem *rx = nullptr;
  int rx_replans = -1;                   // w->replans rx's topology was set for
  BatchSolveState rx_batch;
  DevBuf<int32_t> rx_ints;               // active [E] | steps [E] | n_active | jo [2] | co [2]
  DevBuf<double> rx_err_sq;              // [E]
  DevBuf<uint8_t> rx_eq_scratch;         // the assembly's row types, not used (every relaxation row is an equality)
  PinnedBuf<int32_t> h_rx;               // page-locked, 8 words: n_active, stall flag, jo [2], co [2]
  // EGS_WORLD_TRACE=1: host wall time per phase of egs_world_stabilize's passes, printed by egs_world_destroy
  double t_stab[6] = {0, 0, 0, 0, 0, 0};   // detection + world re-plan, relaxation re-topology, assembly + test + count
                                           // read-back, solve, J^T y + stall check + relaxation step; passes
  std::vector<int32_t> st_steps;         // [E] of the last egs_world_stabilize (empty: none yet)
  std::vector<double> st_err_sq;
  // egs_world_stabilize_direct, all made on its first call: every ensemble's constraint list in its own order and
  // the size-class lists (stabilize_direct.h; host tables rebuilt after a re-plan), the global class's workspace, and
  // per ensemble active [E], steps [E], rank [E], then n_active
  int dr_replans = -1;                   // w->replans the tables below were built for
  int dr_max_rows = 0;
  std::vector<int32_t> dr_rows;          // [E] rows of each ensemble
  int dr_count[kDirectClasses] = {0, 0, 0};
  DevBuf<int32_t> dr_cons, dr_cstart, dr_lists, dr_ints;
  DevBuf<int64_t> dr_wsoff;
  DevBuf<double> dr_ws, dr_err_sq;
  PinnedBuf<int32_t> h_dr;               // page-locked: n_active
  std::vector<int32_t> st_rank, st_rows; // [E] of the last egs_world_stabilize_direct (empty: none yet)
  // egs_world_set_warm_start: a step's solve starts from the previous step's lambda (warm_start.h).  The history is
  // the list the last successful step solved -- its contacts' bodies and positions, every constraint's rows (joints
  // first) in the world's precision, the contact offsets (batched) -- and valid [E]: has ensemble e a history?
  // Dropped (valid = 0) wherever lambda_stale would be set, by set_bodies and by set_joints.  The step's x0 is the
  // world's ws_x0, what the solve starts from the problem's start buffer; ws_source [m] says where each constraint's rows came from.
  bool warm = false, last_warm = false;
  double warm_radius = 0.0;
  int ws_mj = 0, ws_mc = 0;              // the history's joints and contacts
  DevBuf<int32_t> ws_b0, ws_b1, ws_coff, ws_source;
  DevBuf<double> ws_pos;
  DevBuf<unsigned char> ws_lambda, ws_x0;
  DevBuf<uint8_t> ws_valid;
  // egs_world_set_friction: the Coulomb pyramid, one coefficient per ensemble (< 0: the reference's box).  friction:
  // some coefficient is >= 0; then every step fills the problem's per-constraint coefficients from the current list
  // (world_fill_friction) before its solve.
  bool friction = false;
  DevBuf<double> d_fric;                 // [E]
  std::vector<double> h_fric;            // [E], the host's copy (the dense step's ensembles above the fused cap)
  // egs_world_set_restitution: one coefficient per ensemble (< 0: none) and the threshold speed.  restitution: some
  // coefficient is >= 0; then every step fills the problem's per-constraint table from the current list
  // (world_fill_restitution) before its assembly.
  bool restitution = false;
  DevBuf<double> d_rest;                 // [E]
  double rest_vth = 0.0;
  // egs_world_set_dense_friction: max_outer > 0 makes the dense steps solve the pyramid (the fixed-point iteration of
  // mixed_solve_device.h) while friction is on; 0: they refuse.  The outcomes of the last dense step, per ensemble.
  int dense_fric_outer = 0;
  double dense_fric_tol = 0.0;
  DevBuf<DenseFrictionStatus> dn_fstatus;
  DenseFrictionStatus *h_dn_fstatus = nullptr;
  std::vector<DenseFrictionStatus> dn_finfo;   // [E] of the last dense step
  std::vector<int32_t> dn_cons_host;     // dn_cons on the host
  bool lambda_stale = false;             // a stabilise call changed bodies / contacts since the last step's solve
  // EGS_WORLD_TRACE=1: host wall time per phase of egs_world_step, printed by egs_world_destroy
  bool trace = false;
  double t_phase[5] = {0, 0, 0, 0, 0};   // collide, topology D2H + compare, re-plan, solve + integrate (enqueue), steps
};

namespace {

void world_make_problem(egs_world *w, const int32_t *b0, const int32_t *b1, int m) {
  hipStream_t s = w->ctx->stream;
  if (!w->prob) {
    egs_problem *created = nullptr;
    egs_status st = egs_problem_create(w->ctx, w->n, m, b0, b1, w->precision, &created);
    if (st != EGS_OK) throw HipError(std::string("world: egs_problem_create: ") + egs_last_error(w->ctx));
    w->prob = created;
  } else {  // same bodies, new constraint list: the body state stays where it is
    if (check_topology(w->ctx, w->n, m, b0, b1) != EGS_OK)
      throw std::invalid_argument(egs_last_error(w->ctx));
    problem_set_topology(w->prob, m, b0, b1, /*fresh=*/false);
  }
  egs_problem *np = w->prob;
  // constraint kinds: joints first, then contacts; joint descriptors are static
  std::vector<int32_t> kind((size_t)(m > 0 ? m : 1), EGS_CONTACT_BOX);
  const int mj = (int)w->jb0.size();
  for (int i = 0; i < mj; ++i) kind[i] = EGS_JOINT_BALL;
  if (m > 0) {
    kind.resize((size_t)m);
    stage(w->ctx, np->kind, kind);   // through the pinned arena (reset only after a synchronise): no wait here
    note_kinds(np, kind.data());
    if (mj > 0) upload(np->data, w->jdata.data(), (size_t)mj * 7, s);
  }
  np->have_constraints = true;
  np->h_rows_valid = false;
  w->topo_b0.assign(b0, b0 + m); w->topo_b1.assign(b1, b1 + m);
  ++w->replans;
}

// UpdateContacts + pruning on the device (ensembles.cc:393-394), the topology read-back, and a re-plan only when the
// constraint topology changed: the front of egs_world_step and egs_world_step_dense.
template <typename LAP>
void world_update_contacts(egs_world *w, LAP &&lap) {
  hipStream_t s = w->ctx->stream;
  const int mj = (int)w->jb0.size();
  const int mc = w->col.run(s, w->n, w->prob->pos.p, w->prob->R.p, w->dside.p, mj, w->djb0.p, w->djb1.p, w->djdata.p,
                            w->shapes ? w->dshape.p : nullptr);
  lap(0);
  const size_t mt = (size_t)mj + (size_t)mc;
  if (mt > w->h_cap) {   // grow-only; the stream is idle here (col.run synchronised)
    w->topo_pinned.reset();
    w->h_cap = mt + mt / 4 + 64;
    w->h_b0 = static_cast<int32_t *>(w->topo_pinned.take(2 * w->h_cap * sizeof(int32_t)));
    w->h_b1 = w->h_b0 + w->h_cap;
  }
  std::copy(w->jb0.begin(), w->jb0.end(), w->h_b0);
  std::copy(w->jb1.begin(), w->jb1.end(), w->h_b1);
  if (mc > 0) {   // the GPU writes the 8 bytes per contact straight into page-locked host memory
    w->col.export_topology(s, mc, w->h_b0 + mj, w->h_b1 + mj);
    HIPCHK(hipStreamSynchronize(s));
  }
  const bool changed = mt != w->topo_b0.size() || (mt > 0 && (
                       std::memcmp(w->h_b0, w->topo_b0.data(), mt * sizeof(int32_t)) != 0 ||
                       std::memcmp(w->h_b1, w->topo_b1.data(), mt * sizeof(int32_t)) != 0));
  lap(1);
  if (changed) world_make_problem(w, w->h_b0, w->h_b1, (int)mt);  // host plan only on topology change
  lap(2);
  if (mc > 0)
    HIPCHK(hipMemcpyAsync(w->prob->data.p + (size_t)mj * 7, w->col.data(), (size_t)mc * 7 * sizeof(double),
                          hipMemcpyDeviceToDevice, s));
  w->m_contacts = mc;
}

// The dense row space of every ensemble (egs_world_step_dense): ensemble e's constraints in the order its own
// Ensemble would list them -- its joints, then its contacts (ensembles.cc:234-239) -- which decides the Murty loop's
// first offender and the Schur partition; workspace offsets; the fused kernel's size classes.  Host tables only:
// building them is not a re-plan.
void world_dense_plan(egs_world *w) {
  const egs_problem *p = w->prob;
  const int E = w->n_ens, m = p->m;
  std::vector<int32_t> ens((size_t)(m > 0 ? m : 1), 0), count((size_t)E, 0);
  for (int c = 0; c < m; ++c) {
    const int32_t b = p->h_body0[(size_t)c] >= 0 ? p->h_body0[(size_t)c] : p->h_body1[(size_t)c];
    const int e = E == 1 ? 0 : (int)(std::upper_bound(w->body_off.begin(), w->body_off.end(), b) - w->body_off.begin()) - 1;
    ens[(size_t)c] = e;
    ++count[(size_t)e];
  }
  w->dn_start.assign((size_t)E + 1, 0);
  w->dn_off.assign((size_t)E, 0);
  w->dn_max_m = 0;
  for (auto &l : w->dn_class) l.clear();
  w->dn_big.clear();
  int64_t off = 0;
  for (int e = 0; e < E; ++e) {
    const int me = count[(size_t)e], N = 3 * me;
    w->dn_start[(size_t)e + 1] = w->dn_start[(size_t)e] + me;
    w->dn_off[(size_t)e] = off;
    off += (int64_t)dense_ws_size((size_t)N);
    w->dn_max_m = std::max(w->dn_max_m, me);
    if (N == 0) continue;   // v_dot = M^-1 f (ensembles.cc:504-505): nothing to solve
    if (N <= kDenseClassRows[0]) w->dn_class[0].push_back(e);
    else if (N <= kDenseClassRows[1]) w->dn_class[1].push_back(e);
    else if (N <= kFusedDenseMax) w->dn_class[2].push_back(e);
    else w->dn_big.push_back(e);
  }
  // a stable bucket sort: the world lists joints (grouped by ensemble) before contacts (grouped by ensemble)
  std::vector<int32_t> cons((size_t)(m > 0 ? m : 1), 0), next(w->dn_start.begin(), w->dn_start.end() - 1);
  for (int c = 0; c < m; ++c) cons[(size_t)next[(size_t)ens[(size_t)c]]++] = c;
  std::vector<int32_t> lists;
  for (const auto &l : w->dn_class) lists.insert(lists.end(), l.begin(), l.end());
  if (lists.empty()) lists.push_back(0);
  stage(w->ctx, w->dn_cons, cons);
  w->dn_cons_host = cons;
  stage(w->ctx, w->dn_cstart, w->dn_start);
  stage(w->ctx, w->dn_wsoff, w->dn_off);
  stage(w->ctx, w->dn_lists, lists);
  w->dn_ws.alloc((size_t)(off > 0 ? off : 1));
  w->dn_status.alloc((size_t)E);
  w->dn_fstatus.alloc((size_t)E);
  w->dn_big_rows_valid = false;
  w->dense_plan_replans = w->replans;
}

// The relaxation system of egs_world_stabilize (the solve of CalculateVelocityRelaxation, ensembles.cc:659-666, as the
// adapter's stabilize.cpp sets it up): the world problem's constraint topology with M^-1 = I, every row an equality
// and rhs = err.  Made on the first stabilise call, re-topologised only when the world has re-planned since; its plan
// follows from the identity masses (isotropic: the ISO / LINSYM forms of choose_sweep may apply).
void world_relax_system(egs_world *w) {
  if (w->rx && w->rx_replans == w->replans) return;
  hipStream_t s = w->ctx->stream;
  const int m = w->prob->m;
  const int32_t *b0 = w->topo_b0.data(), *b1 = w->topo_b1.data();
  if (!w->rx) {
    egs_problem *created = nullptr;
    if (egs_problem_create(w->ctx, w->n, m, b0, b1, EGS_F64, &created) != EGS_OK)
      throw HipError(std::string("world: relaxation system: ") + egs_last_error(w->ctx));
    w->rx = created;
    std::vector<double> eye((size_t)(w->n > 0 ? w->n : 1) * 36, 0.0);
    for (int b = 0; b < w->n; ++b)
      for (int k = 0; k < 6; ++k) eye[(size_t)b * 36 + 7 * k] = 1.0;
    upload(w->rx->Minv_d, eye.data(), (size_t)w->n * 36, s);
    w->rx->minv_r_valid = false;   // the first solve converts the blocks and finds them isotropic
    w->rx->have_state = true;
  } else {
    problem_set_topology(w->rx, m, b0, b1, /*fresh=*/false);
  }
  egs_problem *rx = w->rx;
  const size_t rows = (size_t)(m > 0 ? m : 1) * 3;
  HIPCHK(hipMemsetAsync(rx->is_eq.p, 1, rows, s));
  w->rx_eq_scratch.alloc(rows);
  rx->joint_pairs = w->prob->joint_pairs;
  rx->have_constraints = true;
  w->rx_replans = w->replans;
}

// J and err of the world's constraint list at the current body state, the blocks straight into the relaxation
// system and err as its rhs (the assembly's rhs, lo, hi and row types are not used by the relaxation).
void world_relax_assemble(egs_world *w) {
  egs_problem *p = w->prob, *rx = w->rx;
  AssembleArgs a = assemble_args(p, 1.0, 0.2);
  a.J0 = rx->J0.p; a.J1 = rx->J1.p;
  a.lo = rx->lo.p; a.hi = rx->hi.p;   // read by no equality row
  a.rhs = rx->wres.p;                  // scratch: the solve writes w there
  a.err = real<double>(rx->rhs);
  a.is_eq = w->rx_eq_scratch.p;
  launch_assemble<double>(a, w->ctx->stream);
  HIPCHK(hipGetLastError());
  rx->have_blocks = true;
  rx->lin_neg = !rx->joint_pairs;
}

// Every ensemble's constraint list in the order its own Ensemble holds it (its joints, then its contacts), the size
// class of each (stabilize_direct.h) and the workspace of the global class: the tables of egs_world_stabilize_direct.
// Host work only, redone after a re-plan.  EGS_ERR_UNSUPPORTED, with nothing staged, if an ensemble is above the limit.
egs_status world_direct_plan(egs_world *w) {
  auto verdict = [&]() {
    return w->dr_max_rows > kDirectMaxRows
        ? fail(w->ctx, EGS_ERR_UNSUPPORTED, "an ensemble has " + std::to_string(w->dr_max_rows) + " rows: the direct relaxation takes at most " +
                                             std::to_string(kDirectMaxRows))
        : EGS_OK;
  };
  if (w->dr_replans == w->replans) return verdict();
  const egs_problem *p = w->prob;
  const int E = w->n_ens, m = p->m;
  std::vector<int32_t> ens((size_t)(m > 0 ? m : 1), 0), start((size_t)E + 1, 0);
  for (int c = 0; c < m; ++c) {
    const int32_t b = p->h_body0[(size_t)c] >= 0 ? p->h_body0[(size_t)c] : p->h_body1[(size_t)c];
    const int e = E == 1 ? 0 : (int)(std::upper_bound(w->body_off.begin(), w->body_off.end(), b) - w->body_off.begin()) - 1;
    ens[(size_t)c] = e;
    ++start[(size_t)e + 1];
  }
  w->dr_rows.assign((size_t)E, 0);
  w->dr_max_rows = 0;
  std::vector<int32_t> cls[kDirectClasses];
  std::vector<int64_t> off((size_t)E, 0);
  int64_t total = 0;
  for (int e = 0; e < E; ++e) {
    const int rows = 3 * start[(size_t)e + 1];
    start[(size_t)e + 1] += start[(size_t)e];
    w->dr_rows[(size_t)e] = rows;
    w->dr_max_rows = std::max(w->dr_max_rows, rows);
    cls[direct_class(rows)].push_back(e);   // an ensemble without constraints too: its err_sq = 0 ends it
    off[(size_t)e] = total;
    total += (int64_t)direct_ws_size((size_t)rows);
  }
  w->dr_replans = w->replans;
  if (w->dr_max_rows > kDirectMaxRows) return verdict();
  // a stable bucket sort: the world lists joints (grouped by ensemble) before contacts (grouped by ensemble)
  std::vector<int32_t> cons((size_t)(m > 0 ? m : 1), 0), next(start.begin(), start.end() - 1), lists;
  for (int c = 0; c < m; ++c) cons[(size_t)next[(size_t)ens[(size_t)c]]++] = c;
  for (int c = 0; c < kDirectClasses; ++c) {
    w->dr_count[c] = (int)cls[c].size();
    lists.insert(lists.end(), cls[c].begin(), cls[c].end());
  }
  stage(w->ctx, w->dr_cons, cons);
  stage(w->ctx, w->dr_cstart, start);
  stage(w->ctx, w->dr_lists, lists);
  stage(w->ctx, w->dr_wsoff, off);
  w->dr_ws.alloc((size_t)(total > 0 ? total : 1));
  return EGS_OK;
}

// "bodies set, dt > 0, fp64" of the stepping entries, in that order; fp64_what = NULL: either precision will do
egs_status world_step_guard(egs_world *w, double dt, const char *fp64_what) {
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  if (!(dt > 0)) return fail(w->ctx, EGS_ERR_INVALID, "dt must be > 0");
  if (fp64_what && w->precision != EGS_F64) return fail(w->ctx, EGS_ERR_UNSUPPORTED, fp64_what);
  return EGS_OK;
}

// the arguments of the _each entries, in the scalar guard's order: bodies set, the tables and every dt[e] >= 0, fp64
egs_status world_each_guard(egs_world *w, int32_t n_ensembles, const double *dt, const double *erp, const char *fp64_what) {
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  if (!dt || !erp) return fail(w->ctx, EGS_ERR_INVALID, "NULL dt / erp table");
  if (n_ensembles != w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's");
  for (int e = 0; e < n_ensembles; ++e)
    if (!(dt[e] >= 0)) return fail(w->ctx, EGS_ERR_INVALID, "dt[" + std::to_string(e) + "] must be >= 0 (0: the ensemble sits out)");
  if (fp64_what && w->precision != EGS_F64) return fail(w->ctx, EGS_ERR_UNSUPPORTED, fp64_what);
  return EGS_OK;
}

// the host may write the page-locked block of the _each entries again: the last copy out of it has been made
void world_each_block(egs_world *w) {
  const size_t E = (size_t)w->n_ens;
  w->h_each.alloc(2 * E + (E + 1) / 2);   // once: E is the world's
  if (!w->each_ev) HIPCHK(hipEventCreateWithFlags(&w->each_ev, hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(w->each_ev));   // long past by the next step: no wait in practice
}

// dt [E] and erp [E] to the device through the page-locked block, no stream synchronisation; the tables of the step
EnsembleRates world_send_rates(egs_world *w, const double *dt, const double *erp) {
  hipStream_t s = w->ctx->stream;
  const size_t E = (size_t)w->n_ens, bytes = E * sizeof(double);
  if (!w->d_ens.p) {   // a plain world: every body in ensemble 0
    w->d_ens.alloc((size_t)(w->n > 0 ? w->n : 1));
    HIPCHK(hipMemsetAsync(w->d_ens.p, 0, w->d_ens.count * sizeof(int32_t), s));
  }
  const bool same = w->rates_sent.size() == 2 * E && std::memcmp(w->rates_sent.data(), dt, bytes) == 0 &&
                    std::memcmp(w->rates_sent.data() + E, erp, bytes) == 0;
  if (!same) {
    world_each_block(w);
    std::memcpy(w->h_each.p, dt, bytes);
    std::memcpy(w->h_each.p + E, erp, bytes);
    w->d_rates.alloc(2 * E);
    HIPCHK(hipMemcpyAsync(w->d_rates.p, w->h_each.p, 2 * bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(w->each_ev, s));
    w->rates_sent.assign(w->h_each.p, w->h_each.p + 2 * E);
  }
  return EnsembleRates{w->d_ens.p, w->d_rates.p, w->d_rates.p + E};
}

// the assembly of a step: J, err, bounds, rhs (ensembles.cc:565-570), on one dt / erp or on every ensemble's own
void world_assemble(egs_world *w, double dt, double erp, const EnsembleRates *each) {
  if (each) do_assemble_each(w->prob, *each);
  else do_assemble(w->prob, dt, erp);
}

// the tail of a step: velocities from the accumulators (ensembles.cc:535, 572), then StepPositions_ODE
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
  if (!w->warm || !w->ws_valid.p) return;
  HIPCHK(hipMemsetAsync(w->ws_valid.p, 0, (size_t)w->n_ens, w->ctx->stream));
  w->ws_mj = w->ws_mc = 0;
}

// x0 of the assembled list from the history (REAL [3m]), sources into ws_source, and the solve's start into the
// problem's start buffer: x0, but the rhs rows of an ensemble that sits the step out (dt_each, device, may be NULL)
void world_warm_match(egs_world *w, const double *dt_each) {
  egs_problem *p = w->prob;
  hipStream_t s = w->ctx->stream;
  const int mj = (int)w->jb0.size(), mc = p->m - mj;
  const bool joints_kept = w->ws_mj == mj;   // (set_joints drops the history: a safeguard)
  if (!joints_kept) world_drop_history(w);
  p->start.alloc((size_t)p->m * 3 * p->real_size());
  w->ws_x0.alloc((size_t)p->m * 3 * p->real_size());
  w->ws_source.alloc((size_t)p->m);
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    MatchArgs<REAL> a;
    a.n_ens = w->n_ens; a.mj = mj; a.m_old = w->ws_mc; a.m_new = mc;
    if (w->n_ens > 1) { a.joint_off = w->d_joff.p; a.old_off = w->ws_coff.p; a.new_off = w->d_coff.p; }
    a.valid = w->ws_valid.p;
    a.old_b0 = w->ws_b0.p; a.old_b1 = w->ws_b1.p; a.old_pos = w->ws_pos.p; a.old_stride = 3;
    a.old_lambda = real<REAL>(w->ws_lambda);
    a.new_b0 = p->body0.p + mj; a.new_b1 = p->body1.p + mj;
    a.new_pos = p->data.p + (size_t)mj * 7; a.new_stride = 7;
    a.new_rhs = real<REAL>(p->rhs);
    a.r2 = w->warm_radius * w->warm_radius;
    a.x0 = real<REAL>(w->ws_x0); a.source = w->ws_source.p;
    a.dt = dt_each; a.start = real<REAL>(p->start);
    launch_match_contacts<REAL>(a, s);
  });
  HIPCHK(hipGetLastError());
}

// the list just solved becomes the history (x: its lambda); dt_each (device, may be NULL): who sat out
void world_warm_snapshot(egs_world *w, const double *dt_each) {
  egs_problem *p = w->prob;
  hipStream_t s = w->ctx->stream;
  const int mj = (int)w->jb0.size(), mc = p->m - mj;
  const size_t rs = p->real_size(), mm = (size_t)(p->m > 0 ? p->m : 1), cc = (size_t)(mc > 0 ? mc : 1);
  HIPCHK(hipStreamSynchronize(s));   // a growing buffer is freed: the match kernel has read it by now
  w->ws_b0.alloc(cc); w->ws_b1.alloc(cc); w->ws_pos.alloc(cc * 3); w->ws_lambda.alloc(mm * 3 * rs);
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    SnapshotArgs<REAL> a;
    a.n_ens = w->n_ens; a.mj = mj; a.mc = mc;
    if (w->n_ens > 1) { a.joint_off = w->d_joff.p; a.contact_off = w->d_coff.p; }
    a.dt = dt_each;
    a.b0 = p->body0.p + mj; a.b1 = p->body1.p + mj; a.pos = p->data.p + (size_t)mj * 7; a.stride = 7;
    a.x0 = real<REAL>(w->ws_x0); a.x = real<REAL>(p->x);
    a.h_b0 = w->ws_b0.p; a.h_b1 = w->ws_b1.p; a.h_pos = w->ws_pos.p; a.h_lambda = real<REAL>(w->ws_lambda);
    a.valid = w->ws_valid.p;
    launch_warm_snapshot<REAL>(a, s);
  });
  HIPCHK(hipGetLastError());
  if (w->n_ens > 1)
    HIPCHK(hipMemcpyAsync(w->ws_coff.p, w->d_coff.p, ((size_t)w->n_ens + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  w->ws_mj = mj; w->ws_mc = mc;
}

// EGS_WORLD_TRACE=1: host wall time per phase of an entry, lap(k) adds the time since the last lap to acc[k].
// sync: wait for the stream first (the stabilise passes; a step must not)
struct PhaseTimer {
  using clk = std::chrono::steady_clock;
  egs_world *w;
  double *acc;
  bool sync;
  clk::time_point t0 = clk::now();
  void operator()(int k) {
    if (!w->trace) return;
    if (sync) HIPCHK(hipStreamSynchronize(w->ctx->stream));
    const auto t1 = clk::now();
    acc[k] += std::chrono::duration<double, std::micro>(t1 - t0).count();
    t0 = t1;
  }
};

// egs_world_step_dense's ensembles above the fused cap: the multi-launch path on each ensemble's workspace slice, one
// after another (row types and bounds read back once per re-plan).  x: the world problem's lambda.  The first
// failure's message goes to big_msg.  dt_each [E] (host, may be NULL): an ensemble with dt 0 sits out, it is not solved.
// pyramid: friction is on and egs_world_set_dense_friction allows it -- the fixed-point iteration from the host
// (mixed_friction_host) on the ensemble's matrix and right-hand side read back, beta from the read-back x.
void world_dense_big(egs_world *w, double cfm_coeff, int32_t use_bounds, double *x, std::string &big_msg, const double *dt_each,
                     bool pyramid) {
  hipStream_t s = w->ctx->stream;
  auto rows_of = [&](int e) { return 3 * (w->dn_start[(size_t)e + 1] - w->dn_start[(size_t)e]); };
  if (!w->dn_big_rows_valid) {
    size_t rows = 0;
    for (int e : w->dn_big) rows += (size_t)rows_of(e);
    std::vector<double> c4(rows * 3);
    size_t r0 = 0;
    for (int e : w->dn_big) {
      const size_t N = (size_t)rows_of(e);
      const double *vb = w->dn_ws.p + w->dn_off[(size_t)e] + dense_ws_vec(N);
      HIPCHK(hipMemcpyAsync(c4.data() + 3 * r0, vb + N, 3 * N * sizeof(double), hipMemcpyDeviceToHost, s));   // lo, hi, C
      r0 += N;
    }
    HIPCHK(hipStreamSynchronize(s));
    w->dn_big_C.resize(rows); w->dn_big_lo.resize(rows); w->dn_big_hi.resize(rows);
    r0 = 0;
    for (int e : w->dn_big) {
      const size_t N = (size_t)rows_of(e);
      for (size_t k = 0; k < N; ++k) {
        w->dn_big_lo[r0 + k] = c4[3 * r0 + k];
        w->dn_big_hi[r0 + k] = c4[3 * r0 + N + k];
        w->dn_big_C[r0 + k] = c4[3 * r0 + 2 * N + k] != 0.0 ? 1 : 0;
      }
      r0 += N;
    }
    w->dn_big_rows_valid = true;
  }
  size_t r0 = 0;
  for (int e : w->dn_big) {
    const int N = rows_of(e);
    if (dt_each && dt_each[e] == 0.0) { r0 += (size_t)N; continue; }
    double *A = w->dn_ws.p + w->dn_off[(size_t)e];
    double *vb = A + dense_ws_vec((size_t)N), *xs = vb + 4 * (size_t)N;
    DenseEnsStatus &st = w->dn_info[(size_t)e];
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
        const int c = w->dn_cons_host[(size_t)w->dn_start[(size_t)e] + k / 3];
        hmu[k] = c < mj ? -1.0 : w->h_fric[(size_t)e];
        if (k % 3 < 2 && hmu[k] >= 0.0) nrow[k] = (int32_t)(k - k % 3 + 2);
      }
      DenseFrictionStatus &fs = w->dn_finfo[(size_t)e];
      int out = 0;
      good = mixed_friction_host(w->ctx->dense, N, hA.data(), hb.data(), w->dn_big_C.data() + r0, w->dn_big_lo.data() + r0,
                                 w->dn_big_hi.data() + r0, nrow.data(), hmu.data(), 0, w->dense_fric_outer, w->dense_fric_tol, hx.data(),
                                 hw.data(), nullptr, &piv, &out, &fs.change, &msg);
      fs.outer = out;
      fs.converged = (good && fs.change <= w->dense_fric_tol) ? 1 : 0;
      if (good) {
        HIPCHK(hipMemcpyAsync(xs, hx.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                   // hx is this scope's
      }
    } else {
      good = dense_mixed_constraints_device(w->ctx->dense, N, A, vb, w->dn_big_C.data() + r0, w->dn_big_lo.data() + r0,
                                            w->dn_big_hi.data() + r0, use_bounds != 0, false, 0, 0.0, nullptr, nullptr, xs, &piv, &msg);
    }
    st.ok = good ? 1 : 0;
    st.pivots = piv;
    if (good) launch_dense_world_scatter(w->dn_cons.p + w->dn_start[(size_t)e], N, xs, x, s);
    else if (big_msg.empty()) big_msg = msg;
    r0 += (size_t)N;
  }
  HIPCHK(hipGetLastError());
}

// The problem's friction coefficients for the list about to be solved: joints -1, every contact its ensemble's
// coefficient (a batched world's body -> ensemble table; a plain world has one ensemble).
void world_fill_friction(egs_world *w) {
  egs_problem *p = w->prob;
  p->friction = w->friction && p->m > 0;
  if (!p->friction) return;
  p->mu.alloc((size_t)p->m * p->real_size());
  const int mj = (int)w->jb0.size();
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    launch_fill_friction<REAL>(p->m, mj, p->body0.p, p->body1.p, w->n_ens > 1 ? w->d_ens.p : nullptr, w->d_fric.p,
                               real<REAL>(p->mu), w->ctx->stream);
  });
  HIPCHK(hipGetLastError());
}

// The problem's restitution coefficients for the list about to be assembled, as world_fill_friction fills mu: joints
// -1, every contact its ensemble's coefficient, in fp64 (the assembly's precision).
void world_fill_restitution(egs_world *w) {
  egs_problem *p = w->prob;
  p->restitution = w->restitution && p->m > 0;
  if (!p->restitution) return;
  p->rest.alloc((size_t)p->m);
  p->rest_vth = w->rest_vth;
  launch_fill_friction<double>(p->m, (int)w->jb0.size(), p->body0.p, p->body1.p, w->n_ens > 1 ? w->d_ens.p : nullptr,
                               w->d_rest.p, p->rest.p, w->ctx->stream);
  HIPCHK(hipGetLastError());
}

// egs_world_step (dt_each == NULL) and egs_world_step_each (dt_each / erp_each [E], host, validated) after their guards
egs_status world_step_sweeps(egs_world *w, double dt, double erp, const double *dt_each, const double *erp_each,
                             const egs_solve_params *params, int32_t detect_contacts, egs_solve_stats *stats) {
  w->last_dense = false;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    PhaseTimer lap{w, w->t_phase, /*sync=*/false};
    refresh_live_mass(w->prob);   // live inertia: M^-1, f_ext and Wf of the state this step starts from (a free body reads Wf too)
    EnsembleRates rates;
    if (dt_each) rates = world_send_rates(w, dt_each, erp_each);
    const EnsembleRates *each = dt_each ? &rates : nullptr;
    if (detect_contacts) world_update_contacts(w, lap);
    egs_problem *p = w->prob;
    const bool batched = w->n_ens > 1;
    w->last_warm = false;
    if (w->friction || p->friction) world_fill_friction(w);
    if (w->restitution || p->restitution) world_fill_restitution(w);
    if (p->m > 0) {
      world_assemble(w, dt, erp, each);
      // x0 from the history; an ensemble without one gets its rhs rows, the default start.  The problem takes the
      // start for this solve only, also when the solve throws.
      struct GivenStart {
        egs_problem *p;
        explicit GivenStart(egs_problem *q) : p(q) { if (p) p->start_mode = EGS_START_GIVEN; }
        ~GivenStart() { if (p) p->start_mode = EGS_START_RHS; }
      };
      if (w->warm) world_warm_match(w, each ? each->dt : nullptr);
      egs_status st;
      {
        const GivenStart given(w->warm ? p : nullptr);
        st = batched ? do_solve_batch(p, params, w->batch) : do_solve(p, params, stats);
      }
      if (st != EGS_OK) return st;
      // the body state must not be advanced with a lambda that came out of a timed-out ordering
      // wait: look at the flag before integrating (one 4-byte read-back per step)
      HIPCHK(hipStreamSynchronize(s));
      if (stall_seen(p)) return report_stall(p);
      w->lambda_stale = false;   // x holds this step's lambda for the current list
      if (w->warm) { world_warm_snapshot(w, each ? each->dt : nullptr); w->last_warm = true; }
      if (batched && stats) {   // the slowest ensemble's sweep count and the largest residual
        std::memset(stats, 0, sizeof *stats);
        fill_stats(p, stats);
        for (int e = 0; e < w->n_ens; ++e) {
          stats->iterations = std::max(stats->iterations, w->batch.h_ints.p[e]);
          const double r = w->batch.h_res.p[e];
          if (!std::isnan(stats->residual) && (std::isnan(r) || r > stats->residual)) stats->residual = r;   // NaN wins
        }
      }
    } else {  // no constraints: v_dot = M^-1 f (ensembles.cc:504-505)
      if (egs_status st = validate_params(w->ctx, params)) return st;
      w->lambda_stale = false;
      if (w->warm) world_warm_snapshot(w, each ? each->dt : nullptr);   // an empty list is a history too
      zero_accumulators(p);
      if (stats) { std::memset(stats, 0, sizeof *stats); fill_stats(p, stats); }
      if (batched) {
        std::fill(w->batch.h_ints.p, w->batch.h_ints.p + w->n_ens, 0);
        std::fill(w->batch.h_res.p, w->batch.h_res.p + w->n_ens, 0.0);
      }
    }
    world_integrate(w, dt, each);
    if (w->trace) { HIPCHK(hipStreamSynchronize(s)); lap(3); w->t_phase[4] += 1; }
    return EGS_OK;
  });
}

// egs_world_step_dense (dt_each == NULL) and egs_world_step_dense_each (dt_each / erp_each [E], host, validated) after
// their guards
egs_status world_step_direct(egs_world *w, double dt, double erp, const double *dt_each, const double *erp_each,
                             double cfm_coeff, int32_t use_bounds, int32_t detect_contacts, int32_t *n_failed) {
  w->last_dense = false;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    refresh_live_mass(w->prob);   // as world_step_sweeps
    EnsembleRates rates;
    if (dt_each) rates = world_send_rates(w, dt_each, erp_each);
    const EnsembleRates *each = dt_each ? &rates : nullptr;
    if (detect_contacts) world_update_contacts(w, [](int) {});
    egs_problem *p = w->prob;
    const int E = w->n_ens;
    if (!w->h_dn_status) w->h_dn_status = static_cast<DenseEnsStatus *>(w->dn_pinned.take((size_t)E * sizeof(DenseEnsStatus)));
    w->dn_info.assign((size_t)E, DenseEnsStatus{1.0, 0.0, 1, 0});   // contact-free ensembles: solved, no pivots
    w->dn_finfo.assign((size_t)E, DenseFrictionStatus{0.0, 1, 1});  // (and without the pyramid: one solve)
    const bool pyramid = w->friction && w->dense_fric_outer > 0;
    if (pyramid && !w->h_dn_fstatus)
      w->h_dn_fstatus = static_cast<DenseFrictionStatus *>(w->dn_pinned.take((size_t)E * sizeof(DenseFrictionStatus)));
    std::string big_msg;
    bool sits_out = false;
    for (int e = 0; dt_each && e < E; ++e) sits_out |= dt_each[e] == 0.0;
    w->last_warm = false;
    if (pyramid) world_fill_friction(w);
    if (w->restitution || p->restitution) world_fill_restitution(w);
    if (p->m > 0) {
      world_assemble(w, dt, erp, each);                              // J, err, bounds, rhs (ensembles.cc:565-570)
      // the dense step takes no start; an ensemble sitting out keeps its history through the rows matched here
      if (w->warm && sits_out) world_warm_match(w, each->dt);
      if (w->dense_plan_replans != w->replans) world_dense_plan(w);
      DenseWorldArgs a;
      a.cons = w->dn_cons.p; a.cstart = w->dn_cstart.p; a.ws_off = w->dn_wsoff.p;
      a.body0 = p->body0.p; a.body1 = p->body1.p;
      a.J0 = real<double>(p->J0); a.J1 = real<double>(p->J1);
      a.Minv = p->Minv_d.p;
      a.rhs = real<double>(p->rhs);
      a.lo = real<double>(p->lo); a.hi = real<double>(p->hi);
      a.is_eq = p->is_eq.p;
      a.ws = w->dn_ws.p; a.x = real<double>(p->x); a.status = w->dn_status.p;
      a.cfm_coeff = cfm_coeff; a.use_bounds = use_bounds;
      launch_dense_world_system(a, E, w->dn_max_m, s);               // A_e = J M^-1 J^T (ensembles.cc:510)
      // ensembles sitting out (dt 0) are not solved: this step's fused lists go without them and their lambda rows are 0
      const int32_t *lists = w->dn_lists.p;
      int count[3] = {(int)w->dn_class[0].size(), (int)w->dn_class[1].size(), (int)w->dn_class[2].size()};
      if (sits_out) {
        world_each_block(w);
        int32_t *h_lists = reinterpret_cast<int32_t *>(w->h_each.p + 2 * (size_t)E);
        int k = 0;
        for (int c = 0; c < 3; ++c) {
          count[c] = 0;
          for (int e : w->dn_class[c])
            if (dt_each[e] != 0.0) { h_lists[k++] = e; ++count[c]; }
        }
        w->dn_lists_step.alloc((size_t)E);
        if (k > 0) HIPCHK(hipMemcpyAsync(w->dn_lists_step.p, h_lists, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(w->each_ev, s));
        lists = w->dn_lists_step.p;
        HIPCHK(hipMemsetAsync(a.x, 0, (size_t)p->m * 3 * sizeof(double), s));
      }
      DenseWorldFriction fa{};
      if (pyramid) {
        fa.mu = real<double>(p->mu); fa.status = w->dn_fstatus.p;
        fa.tol = w->dense_fric_tol; fa.max_outer = w->dense_fric_outer;
      }
      int at = 0;
      for (int c = 0; c < 3; ++c) {                                  // the rest of ComputeVDot, one workgroup each
        if (pyramid) launch_dense_world_friction(a, fa, lists + at, count[c], c, s);
        else launch_dense_world_fused(a, lists + at, count[c], c, s);
        at += count[c];
      }
      HIPCHK(hipGetLastError());
      if (!w->dn_big.empty()) world_dense_big(w, cfm_coeff, use_bounds, a.x, big_msg, dt_each, pyramid);   // above the fused cap
      // one read-back of the fused ensembles' figures
      if (at > 0) {
        HIPCHK(hipMemcpyAsync(w->h_dn_status, w->dn_status.p, (size_t)E * sizeof(DenseEnsStatus), hipMemcpyDeviceToHost, s));
        if (pyramid)
          HIPCHK(hipMemcpyAsync(w->h_dn_fstatus, w->dn_fstatus.p, (size_t)E * sizeof(DenseFrictionStatus), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (const auto &l : w->dn_class)
          for (int e : l)
            if (!(dt_each && dt_each[e] == 0.0)) {
              w->dn_info[(size_t)e] = w->h_dn_status[e];
              if (pyramid) w->dn_finfo[(size_t)e] = w->h_dn_fstatus[e];
            }
      }
    }
    int nf = 0, first = -1, max_piv = 0;
    for (int e = 0; e < E; ++e) {
      const DenseEnsStatus &st = w->dn_info[(size_t)e];
      if (!st.ok && first < 0) first = e;
      nf += st.ok ? 0 : 1;
      max_piv = std::max(max_piv, (int)st.pivots);
      if (E > 1) { w->batch.h_ints.p[e] = st.pivots; w->batch.h_res.p[e] = std::numeric_limits<double>::quiet_NaN(); }
    }
    p->last_iterations = max_piv;
    w->last_dense = true;
    if (n_failed) *n_failed = nf;
    if (nf > 0) {   // the reference Panics (ensembles.cc:531-534): no body is advanced
      std::string msg = "ensemble " + std::to_string(first) + ": MixedConstraintsSolver did not reach a solution";
      if (!big_msg.empty()) msg += " (" + big_msg + ")";
      if (nf > 1) msg += "; " + std::to_string(nf) + " of " + std::to_string(E) + " ensembles failed";
      return fail(w->ctx, EGS_ERR_LCP_FAILED, msg);
    }
    w->lambda_stale = false;   // every ensemble solved: x holds this step's lambda for the current list
    if (w->warm) world_warm_snapshot(w, sits_out ? each->dt : nullptr);   // the history is the dense lambda
    if (p->m > 0) accumulators_from_lambda(p);                    // a = M^-1 J^T lambda
    else zero_accumulators(p);
    world_integrate(w, dt, each);
    return EGS_OK;
  });
}

// What is wrong with a shape array (nothing: an empty string): a value that is no egs_shape, or -- where the side lengths are
// known (side != NULL) -- a sphere whose side row is not three equal positive numbers.
std::string shapes_fault(int n, const int32_t *shape, const double *side) {
  for (int b = 0; b < n; ++b) {
    if (shape[b] != EGS_SHAPE_BOX && shape[b] != EGS_SHAPE_SPHERE)
      return "body " + std::to_string(b) + ": unknown shape " + std::to_string(shape[b]);
    if (shape[b] != EGS_SHAPE_SPHERE || !side) continue;
    const double *d = side + 3 * (size_t)b;
    if (!(d[0] > 0) || d[1] != d[0] || d[2] != d[0])
      return "body " + std::to_string(b) + ": a sphere's side_lengths must be (d, d, d) with d > 0";
  }
  return std::string();
}

egs_status update_contacts_entry(egs_context *ctx, int32_t n, const double *pos, const double *R, const double *side,
                                 int32_t m_joints, const int32_t *jb0, const int32_t *jb1, const double *jdata,
                                 const int32_t *shape, int32_t max_contacts, int32_t *m_out, int32_t *body0,
                                 int32_t *body1, double *data) {
  if (!ctx) return EGS_ERR_INVALID;
  if (n < 0 || m_joints < 0 || !m_out || (n > 0 && (!pos || !R || !side)) || (m_joints > 0 && (!jb0 || !jb1 || !jdata)) ||
      (max_contacts > 0 && (!body0 || !body1 || !data)))
    return fail(ctx, EGS_ERR_INVALID, "NULL array");
  for (int q = 0; q < m_joints; ++q)
    if (jb0[q] < -1 || jb0[q] >= n || jb1[q] < -1 || jb1[q] >= n) return fail(ctx, EGS_ERR_INVALID, "joint body index out of range");
  if (shape) {
    const std::string fault = shapes_fault(n, shape, side);
    if (!fault.empty()) return fail(ctx, EGS_ERR_INVALID, fault);
  }
  *m_out = 0;
  // only body-body joints can prune (the pair scan never visits the ground, quirk Q4)
  std::vector<int32_t> b0, b1; std::vector<double> jd;
  for (int q = 0; q < m_joints; ++q)
    if (jb0[q] >= 0 && jb1[q] >= 0) { b0.push_back(jb0[q]); b1.push_back(jb1[q]); jd.insert(jd.end(), jdata + 7 * (size_t)q, jdata + 7 * (size_t)q + 7); }
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    *m_out = update_contacts(ctx->stream, n, pos, R, side, max_contacts, body0, body1, data, nullptr, nullptr,
                             (int)b0.size(), b0.data(), b1.data(), jd.data(), shape);
    return EGS_OK;
  });
}

}  // namespace

extern "C" {

egs_status egs_update_contacts_joints(egs_context *ctx, int32_t n, const double *pos, const double *R,
                                      const double *side, int32_t m_joints, const int32_t *jb0, const int32_t *jb1,
                                      const double *jdata, int32_t max_contacts, int32_t *m_out, int32_t *body0,
                                      int32_t *body1, double *data) {
  return update_contacts_entry(ctx, n, pos, R, side, m_joints, jb0, jb1, jdata, nullptr, max_contacts, m_out, body0, body1, data);
}

egs_status egs_update_contacts_shapes(egs_context *ctx, int32_t n, const double *pos, const double *R,
                                      const double *side, int32_t m_joints, const int32_t *jb0, const int32_t *jb1,
                                      const double *jdata, const int32_t *shape, int32_t max_contacts, int32_t *m_out,
                                      int32_t *body0, int32_t *body1, double *data) {
  return update_contacts_entry(ctx, n, pos, R, side, m_joints, jb0, jb1, jdata, shape, max_contacts, m_out, body0, body1, data);
}

egs_status egs_update_contacts(egs_context *ctx, int32_t n, const double *pos, const double *R, const double *side,
                               int32_t max_contacts, int32_t *m_out, int32_t *body0, int32_t *body1, double *data) {
  return egs_update_contacts_joints(ctx, n, pos, R, side, 0, nullptr, nullptr, nullptr, max_contacts, m_out, body0, body1, data);
}

egs_status egs_world_create(egs_context *ctx, int32_t n_bodies, int32_t precision, egs_world **out) {
  if (!ctx || !out || n_bodies < 0) return EGS_ERR_INVALID;
  *out = nullptr;
  if (precision != EGS_F64 && precision != EGS_F32) return fail(ctx, EGS_ERR_INVALID, "unknown precision");
  egs_world *w = new (std::nothrow) egs_world;
  if (!w) return fail(ctx, EGS_ERR_HIP, "host allocation failed");
  w->ctx = ctx; w->n = n_bodies; w->precision = precision;
  { const char *te = std::getenv("EGS_WORLD_TRACE"); w->trace = te && std::atoi(te) != 0; }
  egs_status st = guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    w->dside.alloc((size_t)(n_bodies > 0 ? n_bodies : 1) * 3);
    return EGS_OK;
  });
  if (st != EGS_OK) { delete w; return st; }
  *out = w;
  return EGS_OK;
}

void egs_world_destroy(egs_world *w) {
  if (!w) return;
  if (w->trace && w->t_phase[4] > 0) {
    const double k = 1.0 / w->t_phase[4];
    std::fprintf(stderr, "egs_world trace (%d steps, %d re-plans), us/step: collide %.1f  topology %.1f  re-plan %.1f  solve+integrate %.1f\n",
                 (int)w->t_phase[4], w->replans, w->t_phase[0] * k, w->t_phase[1] * k, w->t_phase[2] * k, w->t_phase[3] * k);
  }
  if (w->trace && w->t_stab[5] > 0) {
    const double k = 1.0 / w->t_stab[5];
    std::fprintf(stderr, "egs_world stabilize trace (%d passes), us/pass: detect+re-plan %.1f  relaxation re-topology %.1f  "
                 "assemble+test %.1f  solve %.1f  J^T y+relax %.1f\n", (int)w->t_stab[5], w->t_stab[0] * k, w->t_stab[1] * k,
                 w->t_stab[2] * k, w->t_stab[3] * k, w->t_stab[4] * k);
  }
  if (w->prob) egs_problem_destroy(w->prob);
  if (w->rx) egs_problem_destroy(w->rx);
  if (w->each_ev) (void)hipEventDestroy(w->each_ev);
  delete w;
}

egs_status egs_world_set_bodies(egs_world *w, const double *pos, const double *R, const double *v, const double *wv,
                                const double *Minv, const double *f_ext, const double *side_lengths) {
  if (!w) return EGS_ERR_INVALID;
  // the first call needs everything; afterwards NULL = keep (M^-1, f_ext and the side lengths
  // are frozen at Init in the reference, Q5)
  if (w->n > 0 && !w->have_bodies && (!pos || !R || !v || !wv || !Minv || !f_ext || !side_lengths))
    return fail(w->ctx, EGS_ERR_INVALID, "NULL array on the first egs_world_set_bodies");
  if (w->shapes && side_lengths) {   // new side lengths under the shapes in force: nothing changes if they do not fit
    const std::string fault = shapes_fault(w->n, w->h_shape.data(), side_lengths);
    if (!fault.empty()) return fail(w->ctx, EGS_ERR_INVALID, fault);
  }
  return guarded(w->ctx, [&]() -> egs_status {
    if (!w->prob) world_make_problem(w, w->jb0.data(), w->jb1.data(), (int)w->jb0.size());
    egs_status st = egs_problem_set_state(w->prob, pos, R, v, wv, Minv, f_ext);
    if (st != EGS_OK) return st;
    world_drop_history(w);
    if (side_lengths) {
      upload(w->dside, side_lengths, (size_t)w->n * 3, w->ctx->stream);
      w->h_side.assign(side_lengths, side_lengths + (size_t)w->n * 3);
    }
    w->have_bodies = true;
    return EGS_OK;
  });
}

egs_status egs_world_set_live_inertia(egs_world *w, const double *inertia_body, const double *torque) {
  if (!w) return EGS_ERR_INVALID;
  egs_status made = guarded(w->ctx, [&]() -> egs_status {   // valid before egs_world_set_bodies, as set_bodies itself is
    if (!w->prob) world_make_problem(w, w->jb0.data(), w->jb1.data(), (int)w->jb0.size());
    return EGS_OK;
  });
  if (made != EGS_OK) return made;
  return set_live_inertia(w->prob, inertia_body, torque);
}

egs_status egs_world_get_mass(egs_world *w, double *Minv, double *f_ext) {
  if (!w) return EGS_ERR_INVALID;
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  return egs_problem_get_mass(w->prob, Minv, f_ext);
}

egs_status egs_world_set_shapes(egs_world *w, const int32_t *shape) {
  if (!w) return EGS_ERR_INVALID;
  if (shape) {   // against the side lengths if egs_world_set_bodies has given them, else there when it does
    const std::string fault = shapes_fault(w->n, shape, w->h_side.empty() ? nullptr : w->h_side.data());
    if (!fault.empty()) return fail(w->ctx, EGS_ERR_INVALID, fault);
  }
  return guarded(w->ctx, [&]() -> egs_status {
    if (shape && w->n > 0) {
      w->dshape.alloc((size_t)w->n);
      upload(w->dshape, shape, (size_t)w->n, w->ctx->stream);
      w->h_shape.assign(shape, shape + w->n);
    }
    w->shapes = shape && w->n > 0;
    if (!w->shapes) w->h_shape.clear();
    world_drop_history(w);
    return EGS_OK;
  });
}

egs_status egs_world_create_batch(egs_context *ctx, int32_t n_ensembles, const int32_t *n_bodies, int32_t precision,
                                  egs_world **out, int32_t *body_offset) {
  if (!ctx || !out) return EGS_ERR_INVALID;
  *out = nullptr;
  if (n_ensembles < 1 || !n_bodies) return fail(ctx, EGS_ERR_INVALID, "bad ensemble count / NULL size table");
  std::vector<int32_t> off((size_t)n_ensembles + 1, 0);
  long nb = 0;
  for (int e = 0; e < n_ensembles; ++e) {
    if (n_bodies[e] < 0) return fail(ctx, EGS_ERR_INVALID, "negative ensemble size");
    nb += n_bodies[e];
    if (nb > INT32_MAX) return fail(ctx, EGS_ERR_INVALID, "batch too large for 32-bit indices");
    off[(size_t)e + 1] = (int32_t)nb;
  }
  if (body_offset) std::copy(off.begin(), off.end(), body_offset);
  egs_status st = egs_world_create(ctx, (int32_t)nb, precision, out);
  if (st != EGS_OK || n_ensembles == 1) return st;   // one ensemble: the plain world, nothing else
  egs_world *w = *out;
  st = guarded(ctx, [&]() -> egs_status {
    const size_t E = (size_t)n_ensembles;
    w->n_ens = n_ensembles;
    w->body_off = off;
    w->joint_off.assign(E + 1, 0);
    std::vector<int32_t> ens((size_t)(nb > 0 ? nb : 1), 0);
    for (size_t e = 0; e < E; ++e)
      for (int32_t b = off[e]; b < off[e + 1]; ++b) ens[(size_t)b] = (int32_t)e;
    w->d_ens.alloc(ens.size()); upload(w->d_ens, ens.data(), ens.size(), ctx->stream);
    w->d_boff.alloc(E + 1); upload(w->d_boff, off.data(), E + 1, ctx->stream);
    w->d_joff.alloc(E + 1); upload(w->d_joff, w->joint_off.data(), E + 1, ctx->stream);
    w->d_coff.alloc(E + 1); upload(w->d_coff, w->joint_off.data(), E + 1, ctx->stream);   // no contacts yet
    w->batch.segs = EnsembleSegs{n_ensembles, 0, w->d_joff.p, w->d_coff.p, w->d_boff.p};
    w->batch.ensure(n_ensembles);
    std::fill(w->batch.h_ints.p, w->batch.h_ints.p + E + 2, 0);
    std::fill(w->batch.h_res.p, w->batch.h_res.p + E, 0.0);
    w->col.set_ensembles(n_ensembles, w->d_ens.p, w->d_boff.p, w->d_coff.p);
    return EGS_OK;
  });
  if (st != EGS_OK) { egs_world_destroy(w); *out = nullptr; }
  return st;
}

egs_status egs_world_set_joints(egs_world *w, int32_t m_joints, const int32_t *body0, const int32_t *body1,
                                const double *data) {
  if (!w || m_joints < 0 || (m_joints > 0 && (!body0 || !body1 || !data))) return EGS_ERR_INVALID;
  std::vector<int32_t> joint_off;
  if (w->n_ens > 1) {   // every joint inside one ensemble, the joints grouped by ensemble (order within kept)
    joint_off.assign((size_t)w->n_ens + 1, 0);
    auto ens_of = [&](int32_t b) {
      return (int)(std::upper_bound(w->body_off.begin(), w->body_off.end(), b) - w->body_off.begin()) - 1;
    };
    int last = 0;
    for (int i = 0; i < m_joints; ++i) {
      const int32_t a = body0[i], b = body1[i];
      if (a < -1 || a >= w->n || b < -1 || b >= w->n || (a < 0 && b < 0))
        return fail(w->ctx, EGS_ERR_INVALID, "joint body index out of range");
      const int ea = a >= 0 ? ens_of(a) : -1, eb = b >= 0 ? ens_of(b) : -1;
      if (ea >= 0 && eb >= 0 && ea != eb) return fail(w->ctx, EGS_ERR_INVALID, "joint between two ensembles");
      const int e = ea >= 0 ? ea : eb;
      if (e < last) return fail(w->ctx, EGS_ERR_INVALID, "joints not grouped by ensemble");
      last = e;
      ++joint_off[(size_t)e + 1];
    }
    for (int e = 0; e < w->n_ens; ++e) joint_off[(size_t)e + 1] += joint_off[(size_t)e];
  }
  w->jb0.assign(body0, body0 + m_joints);
  w->jb1.assign(body1, body1 + m_joints);
  w->jdata.assign(data, data + (size_t)m_joints * 7);
  return guarded(w->ctx, [&]() -> egs_status {
    w->djb0.alloc((size_t)m_joints); w->djb1.alloc((size_t)m_joints); w->djdata.alloc((size_t)m_joints * 7);
    if (m_joints > 0) {
      upload(w->djb0, body0, (size_t)m_joints, w->ctx->stream);
      upload(w->djb1, body1, (size_t)m_joints, w->ctx->stream);
      upload(w->djdata, data, (size_t)m_joints * 7, w->ctx->stream);
    }
    world_make_problem(w, w->jb0.data(), w->jb1.data(), m_joints);   // contacts are re-detected by the next step
    w->m_contacts = 0;
    world_drop_history(w);
    if (w->n_ens > 1) {
      const size_t E1 = (size_t)w->n_ens + 1;
      w->joint_off = joint_off;
      upload(w->d_joff, joint_off.data(), E1, w->ctx->stream);
      HIPCHK(hipMemsetAsync(w->d_coff.p, 0, E1 * sizeof(int32_t), w->ctx->stream));
      w->batch.segs.mj = m_joints;
    }
    return EGS_OK;
  });
}

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

egs_status egs_world_step_dense(egs_world *w, double dt, double erp, double cfm_coeff, int32_t use_bounds,
                                int32_t detect_contacts, int32_t *n_failed) {
  if (!w) return EGS_ERR_INVALID;
  if (n_failed) *n_failed = 0;
  if (egs_status st = world_step_guard(w, dt, "the dense path is fp64 (the reference's is)")) return st;
  if (w->friction && w->dense_fric_outer == 0)
    return fail(w->ctx, EGS_ERR_UNSUPPORTED, "the dense solvers have no friction pyramid (turn friction off first)");
  if (use_bounds != 0 && use_bounds != 1) return fail(w->ctx, EGS_ERR_INVALID, "use_bounds must be 0 or 1");
  if (w->friction && use_bounds != 1) return fail(w->ctx, EGS_ERR_INVALID, "the dense friction pyramid needs use_bounds = 1");
  return world_step_direct(w, dt, erp, nullptr, nullptr, cfm_coeff, use_bounds, detect_contacts, n_failed);
}

egs_status egs_world_step_dense_each(egs_world *w, int32_t n_ensembles, const double *dt, const double *erp,
                                     double cfm_coeff, int32_t use_bounds, int32_t detect_contacts, int32_t *n_failed) {
  if (!w) return EGS_ERR_INVALID;
  if (n_failed) *n_failed = 0;
  if (egs_status st = world_each_guard(w, n_ensembles, dt, erp, "the dense path is fp64 (the reference's is)")) return st;
  if (w->friction && w->dense_fric_outer == 0)
    return fail(w->ctx, EGS_ERR_UNSUPPORTED, "the dense solvers have no friction pyramid (turn friction off first)");
  if (use_bounds != 0 && use_bounds != 1) return fail(w->ctx, EGS_ERR_INVALID, "use_bounds must be 0 or 1");
  if (w->friction && use_bounds != 1) return fail(w->ctx, EGS_ERR_INVALID, "the dense friction pyramid needs use_bounds = 1");
  return world_step_direct(w, 0.0, 0.0, dt, erp, cfm_coeff, use_bounds, detect_contacts, n_failed);
}

egs_status egs_world_dense_info(egs_world *w, int32_t n_ensembles, double *condition, double *cfm, int32_t *pivots,
                                int32_t *ok) {
  if (!w) return EGS_ERR_INVALID;
  if (n_ensembles != w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's");
  if (w->dn_info.size() != (size_t)w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "no egs_world_step_dense yet");
  for (int e = 0; e < w->n_ens; ++e) {
    const DenseEnsStatus &st = w->dn_info[(size_t)e];
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
  w->dense_fric_outer = max_outer;
  w->dense_fric_tol = tol;
  return EGS_OK;
}

egs_status egs_world_dense_friction_info(egs_world *w, int32_t n_ensembles, int32_t *outer, int32_t *converged, double *change) {
  if (!w) return EGS_ERR_INVALID;
  if (n_ensembles != w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's");
  if (w->dn_finfo.size() != (size_t)w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "no egs_world_step_dense yet");
  for (int e = 0; e < w->n_ens; ++e) {
    const DenseFrictionStatus &fs = w->dn_finfo[(size_t)e];
    if (outer) outer[e] = fs.outer;
    if (converged) converged[e] = fs.converged;
    if (change) change[e] = fs.change;
  }
  return EGS_OK;
}

egs_status egs_world_get_bodies(egs_world *w, double *pos, double *R, double *v, double *wv) {
  if (!w || !w->prob) return EGS_ERR_INVALID;
  return egs_problem_get_state(w->prob, pos, R, v, wv);
}

egs_status egs_world_get_contacts(egs_world *w, int32_t max_contacts, int32_t *m_out, int32_t *body0, int32_t *body1,
                                  double *data) {
  if (!w || !m_out) return EGS_ERR_INVALID;
  *m_out = w->m_contacts;
  if (w->m_contacts > max_contacts) return fail(w->ctx, EGS_ERR_INVALID, "max_contacts too small");
  return guarded(w->ctx, [&]() -> egs_status {
    const size_t mc = (size_t)w->m_contacts;
    hipStream_t s = w->ctx->stream;
    if (mc && body0) HIPCHK(hipMemcpyAsync(body0, w->col.body0(), mc * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (mc && body1) HIPCHK(hipMemcpyAsync(body1, w->col.body1(), mc * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (mc && data) HIPCHK(hipMemcpyAsync(data, w->col.data(), mc * 7 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return EGS_OK;
  });
}

egs_status egs_world_get_lambda(egs_world *w, int32_t max_rows, int32_t *rows_out, double *lambda) {
  if (!w || !w->prob || !rows_out) return EGS_ERR_INVALID;
  *rows_out = 3 * w->prob->m;
  if (w->lambda_stale)
    return fail(w->ctx, EGS_ERR_INVALID, "no step lambda for the constraint list egs_world_stabilize left: step first");
  if (3 * w->prob->m > max_rows) return fail(w->ctx, EGS_ERR_INVALID, "max_rows too small");
  if (w->prob->m == 0) return EGS_OK;
  return egs_problem_get_lambda(w->prob, lambda);
}

egs_status egs_world_set_warm_start(egs_world *w, int32_t enable, double match_radius) {
  if (!w) return EGS_ERR_INVALID;
  if (enable && !(match_radius >= 0)) return fail(w->ctx, EGS_ERR_INVALID, "match_radius must be >= 0");
  return guarded(w->ctx, [&]() -> egs_status {
    w->warm = enable != 0;
    w->warm_radius = enable ? match_radius : 0.0;
    w->last_warm = false;
    if (w->warm) {   // switched on (or on again): no history
      w->ws_valid.alloc((size_t)w->n_ens);
      w->ws_coff.alloc((size_t)w->n_ens + 1);
      HIPCHK(hipMemsetAsync(w->ws_coff.p, 0, ((size_t)w->n_ens + 1) * sizeof(int32_t), w->ctx->stream));
      world_drop_history(w);
    }
    return EGS_OK;
  });
}

egs_status egs_world_set_friction(egs_world *w, int32_t n_ensembles, const double *mu) {
  if (!w) return EGS_ERR_INVALID;
  if (!mu) return fail(w->ctx, EGS_ERR_INVALID, "NULL friction table");
  if (n_ensembles != w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's");
  bool any = false;
  for (int e = 0; e < n_ensembles; ++e) {
    if (mu[e] != mu[e]) return fail(w->ctx, EGS_ERR_INVALID, "NaN friction coefficient");
    any |= mu[e] >= 0;
  }
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    HIPCHK(hipStreamSynchronize(s));   // a step in flight may still read the old table
    w->d_fric.alloc((size_t)n_ensembles);
    w->h_fric.assign(mu, mu + n_ensembles);
    HIPCHK(hipMemcpyAsync(w->d_fric.p, mu, (size_t)n_ensembles * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // mu is the caller's
    w->friction = any;
    if (!any && w->prob) w->prob->friction = false;
    return EGS_OK;
  });
}

egs_status egs_world_set_restitution(egs_world *w, int32_t n_ensembles, const double *rest, double vth) {
  if (!w) return EGS_ERR_INVALID;
  if (!rest) return fail(w->ctx, EGS_ERR_INVALID, "NULL restitution table");
  if (n_ensembles != w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's");
  if (!(vth >= 0) || std::isinf(vth)) return fail(w->ctx, EGS_ERR_INVALID, "the restitution threshold must be finite and >= 0");
  bool any = false;
  for (int e = 0; e < n_ensembles; ++e) {
    if (rest[e] != rest[e] || std::isinf(rest[e])) return fail(w->ctx, EGS_ERR_INVALID, "NaN or infinite restitution coefficient");
    any |= rest[e] >= 0;
  }
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    HIPCHK(hipStreamSynchronize(s));   // a step in flight may still read the old table
    w->d_rest.alloc((size_t)n_ensembles);
    HIPCHK(hipMemcpyAsync(w->d_rest.p, rest, (size_t)n_ensembles * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // rest is the caller's
    w->restitution = any;
    w->rest_vth = vth;
    if (!any && w->prob) w->prob->restitution = false;
    return EGS_OK;
  });
}

egs_status egs_world_get_start(egs_world *w, int32_t max_rows, int32_t *rows_out, double *x0, int32_t *source) {
  if (!w || !w->prob || !rows_out) return EGS_ERR_INVALID;
  *rows_out = 3 * w->prob->m;
  if (!w->last_warm) return fail(w->ctx, EGS_ERR_INVALID, "the last step was not a warm-started sweep step");
  if (3 * w->prob->m > max_rows) return fail(w->ctx, EGS_ERR_INVALID, "max_rows too small");
  if (!x0) return fail(w->ctx, EGS_ERR_INVALID, "x0 is NULL");
  return guarded(w->ctx, [&]() -> egs_status {
    egs_problem *p = w->prob;
    hipStream_t s = w->ctx->stream;
    const size_t rows = (size_t)p->m * 3;
    std::vector<float> tmp(p->precision == EGS_F32 ? rows : 0);
    HIPCHK(hipMemcpyAsync(tmp.empty() ? (void *)x0 : (void *)tmp.data(), w->ws_x0.p, rows * p->real_size(), hipMemcpyDeviceToHost, s));
    if (source) HIPCHK(hipMemcpyAsync(source, w->ws_source.p, (size_t)p->m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < tmp.size(); ++i) x0[i] = (double)tmp[i];
    return EGS_OK;
  });
}

egs_status egs_world_batch_info(egs_world *w, int32_t n_ensembles, int32_t *joint_offset, int32_t *contact_offset,
                                int32_t *iterations, double *residual) {
  if (!w) return EGS_ERR_INVALID;
  if (n_ensembles != w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's");
  const size_t E = (size_t)w->n_ens;
  if (w->n_ens > 1) {
    if (joint_offset) std::copy(w->joint_off.begin(), w->joint_off.end(), joint_offset);
    return guarded(w->ctx, [&]() -> egs_status {
      if (contact_offset) {
        HIPCHK(hipMemcpyAsync(contact_offset, w->d_coff.p, (E + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, w->ctx->stream));
        HIPCHK(hipStreamSynchronize(w->ctx->stream));
      }
      if (iterations) std::copy(w->batch.h_ints.p, w->batch.h_ints.p + E, iterations);
      if (residual) std::copy(w->batch.h_res.p, w->batch.h_res.p + E, residual);
      return EGS_OK;
    });
  }
  // one ensemble: the plain world's own figures
  if (joint_offset) { joint_offset[0] = 0; joint_offset[1] = (int32_t)w->jb0.size(); }
  if (contact_offset) { contact_offset[0] = 0; contact_offset[1] = w->m_contacts; }
  if (!iterations && !residual) return EGS_OK;
  egs_solve_stats st{};
  if (w->prob && !w->last_dense) {
    if (egs_status r = egs_problem_get_stats(w->prob, &st)) return r;
  }
  if (iterations) iterations[0] = w->last_dense ? w->dn_info[0].pivots : st.iterations;
  if (residual) residual[0] = w->last_dense ? std::numeric_limits<double>::quiet_NaN() : st.residual;
  return EGS_OK;
}

egs_status egs_world_info(egs_world *w, int32_t *n_constraints, int32_t *n_contacts, int32_t *replans) {
  if (!w) return EGS_ERR_INVALID;
  if (n_constraints) *n_constraints = w->prob ? w->prob->m : 0;
  if (n_contacts) *n_contacts = w->m_contacts;
  if (replans) *replans = w->replans;
  return EGS_OK;
}


egs_status egs_world_stabilize(egs_world *w, int32_t mode, int32_t max_steps, int32_t detect_contacts,
                               const egs_solve_params *params, int32_t *n_unsettled) {
  if (!w) return EGS_ERR_INVALID;
  if (n_unsettled) *n_unsettled = 0;
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  if (mode != EGS_STABILIZE_INIT && mode != EGS_STABILIZE_POST)
    return fail(w->ctx, EGS_ERR_INVALID, "mode must be EGS_STABILIZE_INIT or EGS_STABILIZE_POST");
  if (max_steps < 0) return fail(w->ctx, EGS_ERR_INVALID, "max_steps must be >= 0");
  if (w->precision != EGS_F64) return fail(w->ctx, EGS_ERR_UNSUPPORTED, "stabilisation is fp64 (the reference's is)");
  // stabilize.cpp's relaxation solve: SOR, omega 1.5, cfm 0, tol 1e-11, at most 20000 sweeps, checked every 10
  egs_solve_params prm;
  egs_default_params(&prm);
  prm.method = EGS_SOR; prm.cfm = 0.0; prm.tol = 1e-11; prm.max_iters = 20000; prm.check_every = 10;
  if (params) prm = *params;
  if (egs_status st = validate_params(w->ctx, &prm)) return st;
  constexpr double kAllowNumericalError = 1e-9, kSimTimeStep = 0.001;   // constants.h:5-6
  const bool post = mode == EGS_STABILIZE_POST;
  const int cap = max_steps > 0 ? max_steps : post ? 500 : 100;         // ensembles.cc:606, PostStabilize(500)
  const double h = post ? kSimTimeStep * 100 : kSimTimeStep * 500;      // ensembles.cc:614, 638
  const bool detect = !post && detect_contacts != 0;                     // PostStabilize never detects
  const int E = w->n_ens;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    w->lambda_stale = true;
    world_drop_history(w);
    w->st_steps.clear(); w->st_err_sq.clear();
    w->rx_ints.alloc(2 * (size_t)E + 5);
    w->rx_err_sq.alloc((size_t)E);
    w->h_rx.alloc(8);
    int32_t *h_rx = w->h_rx.p;
    int32_t *d_active = w->rx_ints.p, *d_steps = d_active + E, *d_count = d_steps + E, *d_jo = d_count + 1, *d_co = d_jo + 2;
    if (E > 1) {
      w->rx_batch.segs = w->batch.segs;
      w->rx_batch.ensure(E);
    }
    PhaseTimer lap{w, w->t_stab, /*sync=*/true};
    for (int pass = 0;; ++pass) {
      if (detect) world_update_contacts(w, [](int) {});                  // ensembles.cc:603, 616 (pruning included)
      lap(0);
      world_relax_system(w);
      lap(1);
      egs_problem *p = w->prob, *rx = w->rx;
      if (p->m > 0) world_relax_assemble(w);
      StabErrArgs ea;
      if (E > 1) {
        ea.jo = w->d_joff.p; ea.co = w->d_coff.p;
      } else {   // the plain world's one ensemble: its joints, then its contacts
        h_rx[2] = 0; h_rx[3] = (int32_t)w->jb0.size(); h_rx[4] = 0; h_rx[5] = w->m_contacts;
        HIPCHK(hipMemcpyAsync(d_jo, h_rx + 2, 4 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        ea.jo = d_jo; ea.co = d_co;
      }
      ea.mj = (int32_t)w->jb0.size();
      ea.err = real<double>(rx->rhs);
      ea.active = d_active; ea.steps = d_steps; ea.err_sq = w->rx_err_sq.p; ea.n_active = d_count;
      ea.first = pass == 0 ? 1 : 0; ea.max_steps = cap; ea.threshold = kAllowNumericalError;
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
      egs_status st = E > 1 ? do_solve_batch(rx, &prm, w->rx_batch, d_active) : do_solve(rx, &prm, nullptr);
      if (st != EGS_OK) return st;
      lap(3);
      accumulators_from_lambda(rx);
      // a lambda out of a timed-out ordering wait moves no body (egs_world_step's rule)
      HIPCHK(hipMemcpyAsync(h_rx + 1, rx->error_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (h_rx[1] != 0) return report_stall(rx);
      StabRelaxArgs ra;
      ra.n = w->n; ra.post = post ? 1 : 0;
      ra.ens = E > 1 ? w->d_ens.p : nullptr; ra.active = d_active;
      ra.acc = real<double>(rx->acc);
      ra.scale = -1.0 * 0.2; ra.h = h;                                   // CalculateVelocityRelaxation(0.2)
      ra.pos = p->pos.p; ra.R = p->R.p; ra.v = p->v.p; ra.w = p->w.p;
      launch_stab_relax(ra, s);
      HIPCHK(hipGetLastError());
      lap(4);
    }
    w->st_steps.resize((size_t)E); w->st_err_sq.resize((size_t)E);
    HIPCHK(hipMemcpyAsync(w->st_steps.data(), d_steps, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(w->st_err_sq.data(), w->rx_err_sq.p, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_unsettled) {
      int u = 0;
      for (double e2 : w->st_err_sq) u += !(e2 <= kAllowNumericalError) ? 1 : 0;   // NaN counts as unsettled
      *n_unsettled = u;
    }
    return EGS_OK;
  });
}

egs_status egs_world_stabilize_info(egs_world *w, int32_t n_ensembles, int32_t *steps, double *err_sq) {
  if (!w) return EGS_ERR_INVALID;
  if (n_ensembles != w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's");
  if (w->st_steps.size() != (size_t)w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "no egs_world_stabilize / egs_world_stabilize_direct yet");
  if (steps) std::copy(w->st_steps.begin(), w->st_steps.end(), steps);
  if (err_sq) std::copy(w->st_err_sq.begin(), w->st_err_sq.end(), err_sq);
  return EGS_OK;
}

egs_status egs_world_stabilize_direct(egs_world *w, int32_t mode, int32_t max_steps, int32_t detect_contacts, double rank_tol,
                                      int32_t *n_unsettled) {
  if (!w) return EGS_ERR_INVALID;
  if (n_unsettled) *n_unsettled = 0;
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  if (mode != EGS_STABILIZE_INIT && mode != EGS_STABILIZE_POST)
    return fail(w->ctx, EGS_ERR_INVALID, "mode must be EGS_STABILIZE_INIT or EGS_STABILIZE_POST");
  if (max_steps < 0) return fail(w->ctx, EGS_ERR_INVALID, "max_steps must be >= 0");
  if (std::isnan(rank_tol) || rank_tol >= 1.0) return fail(w->ctx, EGS_ERR_INVALID, "rank_tol must be below 1 (<= 0: 1e-10)");
  if (w->precision != EGS_F64) return fail(w->ctx, EGS_ERR_UNSUPPORTED, "stabilisation is fp64 (the reference's is)");
  constexpr double kAllowNumericalError = 1e-9, kSimTimeStep = 0.001;   // constants.h:5-6
  const bool post = mode == EGS_STABILIZE_POST;
  const bool detect = !post && detect_contacts != 0;                     // PostStabilize never detects
  const int E = w->n_ens;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    if (!detect)   // the list the call works on is known now: refuse before anything changes
      if (egs_status st = world_direct_plan(w)) return st;
    w->lambda_stale = true;
    world_drop_history(w);
    w->st_steps.clear(); w->st_err_sq.clear(); w->st_rank.clear(); w->st_rows.clear();
    w->dr_ints.alloc(3 * (size_t)E + 1);
    w->dr_err_sq.alloc((size_t)E);
    w->h_dr.alloc(16);
    StabDirectArgs a;
    a.active = w->dr_ints.p; a.steps = a.active + E; a.rank = a.steps + E; a.n_active = a.rank + E;
    a.err_sq = w->dr_err_sq.p;
    a.loop = detect ? 0 : 1; a.post = post ? 1 : 0;
    a.max_steps = max_steps > 0 ? max_steps : post ? 500 : 100;           // ensembles.cc:606, PostStabilize(500)
    a.threshold = kAllowNumericalError;
    a.rank_tol = rank_tol > 0 ? rank_tol : 1e-10;
    a.scale = -1.0 * 0.2;                                                 // CalculateVelocityRelaxation(0.2)
    a.h = post ? kSimTimeStep * 100 : kSimTimeStep * 500;                 // ensembles.cc:614, 638
    for (int pass = 0;; ++pass) {
      if (detect) {                                                       // ensembles.cc:603, 616 (pruning included)
        world_update_contacts(w, [](int) {});
        if (egs_status st = world_direct_plan(w)) return st;              // over the limit: this pass moves no body
      }
      egs_problem *p = w->prob;
      a.as = assemble_args(p, 1.0, 0.2);
      a.pos = p->pos.p; a.R = p->R.p; a.v = p->v.p; a.w = p->w.p;
      a.cons = w->dr_cons.p; a.cstart = w->dr_cstart.p;
      a.bo = E > 1 ? w->d_boff.p : nullptr;
      a.ws_off = w->dr_wsoff.p; a.ws = w->dr_ws.p;
      a.first = pass == 0 ? 1 : 0;
      HIPCHK(hipMemsetAsync(a.n_active, 0, sizeof(int32_t), s));
      int at = 0;
      for (int c = 0; c < kDirectClasses; ++c) {
        launch_stab_direct(a, w->dr_lists.p + at, w->dr_count[c], c, s);
        at += w->dr_count[c];
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(w->h_dr.p, a.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (!detect || w->h_dr.p[0] == 0) break;
    }
    w->st_steps.resize((size_t)E); w->st_err_sq.resize((size_t)E); w->st_rank.resize((size_t)E);
    HIPCHK(hipMemcpyAsync(w->st_steps.data(), a.steps, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(w->st_rank.data(), a.rank, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(w->st_err_sq.data(), a.err_sq, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    w->st_rows = w->dr_rows;
    if (n_unsettled) {
      int u = 0;
      for (double e2 : w->st_err_sq) u += !(e2 <= kAllowNumericalError) ? 1 : 0;   // NaN counts as unsettled
      *n_unsettled = u;
    }
    return EGS_OK;
  });
}

egs_status egs_world_stabilize_rank(egs_world *w, int32_t n_ensembles, int32_t *rows, int32_t *rank) {
  if (!w) return EGS_ERR_INVALID;
  if (n_ensembles != w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's");
  if (w->st_rank.size() != (size_t)w->n_ens) return fail(w->ctx, EGS_ERR_INVALID, "no egs_world_stabilize_direct yet");
  if (rows) std::copy(w->st_rows.begin(), w->st_rows.end(), rows);
  if (rank) std::copy(w->st_rank.begin(), w->st_rank.end(), rank);
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
