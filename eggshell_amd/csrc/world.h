// world.h -- struct egs_world, one member struct per feature, and the handful of functions that cross the world units
// (world.cpp, world_step.cpp, world_dense.cpp, world_stabilize.cpp, rays.cpp).  Included by those five only; the world works on
// its egs_problem through problem.h.
#pragma once

#include <chrono>

#include "collide.h"
#include "dense_world.h"
#include "ensemble_rows.h"
#include "problem.h"
#include "raycast.h"
#include "stabilize_direct.h"

namespace egs {

// batched world (egs_world_create_batch, n_ens > 1): bodies, joints and contacts are grouped by ensemble
struct EnsembleLayout {
  int n_ens = 1;
  std::vector<int32_t> body_off, joint_off;   // [n_ens + 1]
  DevBuf<int32_t> d_ens, d_boff, d_joff;       // body -> ensemble [n], body and joint offsets [n_ens + 1]
  DevBuf<int32_t> d_coff;                      // contact offsets [n_ens + 1], written by the collider
  BatchSolveState batch;
  int ensemble_of(int32_t body) const { return egs::ensemble_of(n_ens, body_off, body); }
};

// egs_world_step_each / _dense_each: dt [E] | erp [E] on the device and the values last sent (an equal pair is not
// sent again); the page-locked block they go through -- dt, erp, then the E list words of a dense step with
// ensembles sitting out -- and the event behind the last copy out of it.  A plain world gets its body -> ensemble
// table (all 0) on its first such step.
struct EachRates {
  DevBuf<double> d_rates;
  std::vector<double> sent;
  PinnedBuf<double> h_block;
  hipEvent_t ev = nullptr;
  ~EachRates() { if (ev) (void)hipEventDestroy(ev); }
};

// egs_world_step_dense: each ensemble's dense row space (its joints, then its contacts, as its own Ensemble lists
// them), built on the first dense step after a re-plan; the figures of the last dense step
struct DenseStep {
  int built_for = -1;                    // w->replans the tables below were built for
  EnsembleRows rows;                     // start [E + 1] into cons, cons (host copies)
  std::vector<int64_t> off;              // [E] workspace offsets (host copy)
  std::vector<int32_t> cls[3], big;      // ensembles per fused size class; above the fused cap
  int max_m = 0;
  DevBuf<int32_t> cons, cstart, lists;
  DevBuf<int32_t> lists_step;            // the fused lists of an _each step with ensembles sitting out
  DevBuf<int64_t> wsoff;
  DevBuf<double> ws;
  DevBuf<DenseEnsStatus> status;
  std::vector<uint8_t> big_C;            // C / lo / hi of the ensembles above the cap, read back once per re-plan
  std::vector<double> big_lo, big_hi;
  bool big_rows_valid = false;
  PinnedArena pinned;
  DenseEnsStatus *h_status = nullptr;
  std::vector<DenseEnsStatus> info;      // [E] of the last dense step
  bool was_last = false;                 // the last step was egs_world_step_dense (batch_info reports its pivots)
  // egs_world_set_dense_friction: max_outer > 0 makes the dense steps solve the pyramid (the fixed-point iteration of
  // mixed_solve_device.h) while friction is on; 0: they refuse.  The outcomes of the last dense step, per ensemble.
  int fric_outer = 0;
  double fric_tol = 0.0;
  DevBuf<DenseFrictionStatus> fstatus;
  DenseFrictionStatus *h_fstatus = nullptr;
  std::vector<DenseFrictionStatus> finfo;   // [E] of the last dense step
  int rows_of(int e) const { return 3 * rows.count(e); }
};

// egs_world_stabilize, all made on its first call: the relaxation system (the world's topology with M^-1 = I, every
// row an equality, rhs = err; re-topologised when the world re-plans), its batched stopping state, and per ensemble
// active [E], steps [E], err_sq [E]; a plain world's row offsets jo / co [2] each
struct SweepRelax {
  egs_problem *prob = nullptr;
  int built_for = -1;                    // w->replans prob's topology was set for
  BatchSolveState batch;
  DevBuf<int32_t> ints;                  // active [E] | steps [E] | n_active | jo [2] | co [2]
  DevBuf<double> err_sq;                 // [E]
  DevBuf<uint8_t> eq_scratch;            // the assembly's row types, not used (every relaxation row is an equality)
  PinnedBuf<int32_t> h;                  // page-locked, 8 words: n_active, stall flag, jo [2], co [2]
  ~SweepRelax() { if (prob) egs_problem_destroy(prob); }
};

// egs_world_stabilize_direct, all made on its first call: every ensemble's constraint list in its own order and
// the size-class lists (stabilize_direct.h; host tables rebuilt after a re-plan), the global class's workspace, and
// per ensemble active [E], steps [E], rank [E], then n_active
struct DirectRelax {
  int built_for = -1;                    // w->replans the tables below were built for
  int max_rows = 0;
  std::vector<int32_t> rows;             // [E] rows of each ensemble
  int count[kDirectClasses] = {0, 0, 0};
  DevBuf<int32_t> cons, cstart, lists, ints;
  DevBuf<int64_t> wsoff;
  DevBuf<double> ws, err_sq;
  PinnedBuf<int32_t> h;                  // page-locked: n_active
};

// what the last stabilise call left for the info entries
struct StabilizeResults {
  std::vector<int32_t> steps;            // [E] of the last egs_world_stabilize / _direct (empty: none yet)
  std::vector<double> err_sq;
  std::vector<int32_t> rank, rows;       // [E] of the last egs_world_stabilize_direct (empty: none yet)
};

// egs_world_set_warm_start: a step's solve starts from the previous step's lambda (warm_start.h).  The history is
// the list the last successful step solved -- its contacts' bodies and positions, every constraint's rows (joints
// first) in the world's precision, the contact offsets (batched) -- and valid [E]: has ensemble e a history?
// Dropped (valid = 0) wherever lambda_stale would be set, by set_bodies and by set_joints.  The step's x0 is the
// world's x0, what the solve starts from the problem's start buffer; source [m] says where each constraint's rows came from.
struct WarmStart {
  bool on = false, last = false;         // last: the last step was a warm-started sweep step
  double radius = 0.0;
  int mj = 0, mc = 0;                    // the history's joints and contacts
  DevBuf<int32_t> b0, b1, coff, source;
  DevBuf<double> pos;
  DevBuf<unsigned char> lambda, x0;
  DevBuf<uint8_t> valid;
};

// egs_world_set_friction / egs_world_set_restitution: one coefficient per ensemble (< 0: the reference's box / no
// bounce).  any: some coefficient is >= 0; then every step fills the problem's per-constraint table from the current
// list (world_fill_friction before its solve, world_fill_restitution before its assembly).
struct CoeffTable {
  bool any = false;
  DevBuf<double> d;                      // [E]
  std::vector<double> h;                 // [E], the host's copy (friction: read for the dense step's ensembles above the fused cap)
};

// egs_world_set_rays: the ray table on the device (n = 0: none), kept until the next egs_world_set_rays -- nothing a
// step, a re-plan, a stabilise call or egs_world_set_bodies writes is in here, and nothing in here is read by them.
// egs_world_cast_rays writes out = t [n] | normal [n][3] | hit [n] (int32) and reads it back in one copy through h.
struct RayTable {
  int n = 0;
  bool attached = false, grouped = false;   // some ray rides on a body; the rays name ensembles (batched world)
  DevBuf<int32_t> ens, body;
  DevBuf<double> geom;                   // origin [n][3] | dir [n][3] | tmax [n]
  DevBuf<unsigned char> out;
  PinnedBuf<unsigned char> h;
};

}  // namespace egs

// ---------------------------------------------------------------------------
// Body state lives in the current egs_problem's buffers; each step runs
// UpdateContacts (Collider) -> [re-plan only if the constraint topology
// changed] -> assemble -> solve -> velocity -> StepPositions_ODE, and only the
// contact topology (8 bytes per contact) crosses PCIe, to feed the host plan.
struct egs_world {
  egs_context *ctx = nullptr;
  int n = 0, precision = EGS_F64;
  egs_problem *prob = nullptr;
  egs::DevBuf<double> dside;
  // egs_world_set_shapes: egs_shape per body on the device, handed to every Collider::run (shapes = false: NULL, the
  // all-box launches); host copies of the shapes and the side lengths, for the check that a sphere's sides are (d, d, d)
  // capsules: h_shape holds an EGS_SHAPE_CAPSULE, so the collider launches its capsule instantiations
  bool shapes = false, capsules = false;
  egs::DevBuf<int32_t> dshape;
  std::vector<int32_t> h_shape;
  std::vector<double> h_side;
  egs::Collider col;
  std::vector<int32_t> jb0, jb1;       // permanent constraints (joints), listed first (ensembles.cc:234-239)
  std::vector<double> jdata;
  std::vector<int32_t> jkind;          // their kinds (egs_world_set_joints_kinds; all EGS_JOINT_BALL from egs_world_set_joints)
  std::vector<double> jmotor;          // egs_world_set_joint_motors: [joints][2] = (speed, tau); empty: off
  std::vector<double> jtravel;         // egs_world_set_slider_limits: [joints][2] = (xlo, xhi); empty: off (kept only while a slider has a finite stop)
  std::vector<double> jlimit;          // egs_world_set_joint_limits: [joints][8] = (q, sin lo, cos lo, sin hi, cos hi); empty: off
  int mj_ball = 0;                     // how many of them are ball joints
  egs::DevBuf<int32_t> djb0, djb1;     // the ball joints among them on the device, for joint-vs-contact pruning (an
  egs::DevBuf<double> djdata;          // angular block has no position): mj_ball entries, in list order
  std::vector<int32_t> topo_b0, topo_b1;
  egs::PinnedArena topo_pinned;        // page-locked landing area for the contact topology
  int32_t *h_b0 = nullptr, *h_b1 = nullptr;
  size_t h_cap = 0;
  int m_contacts = 0;
  int replans = 0;                     // the stamp the feature structs' built_for compare with
  bool have_bodies = false;
  bool lambda_stale = false;           // a stabilise call changed bodies / contacts since the last step's solve
  // EGS_WORLD_TRACE=1: host wall time per phase of egs_world_step and of egs_world_stabilize's passes, printed by
  // egs_world_destroy
  bool trace = false;
  double t_phase[5] = {0, 0, 0, 0, 0};   // collide, topology D2H + compare, re-plan, solve + integrate (enqueue), steps
  double t_stab[6] = {0, 0, 0, 0, 0, 0};   // detection + world re-plan, relaxation re-topology, assembly + test + count
                                           // read-back, solve, J^T y + stall check + relaxation step; passes
  egs::EnsembleLayout ens;
  egs::EachRates each;
  egs::DenseStep dense;
  egs::SweepRelax rx;
  egs::DirectRelax dr;
  egs::StabilizeResults st;
  egs::WarmStart ws;
  egs::CoeffTable friction, restitution;
  double rest_vth = 0.0;               // the restitution threshold speed
  egs::RayTable rays;
  ~egs_world() { if (prob) egs_problem_destroy(prob); }
};

namespace egs {

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

// the n_ensembles argument of the info and table entries
inline egs_status world_check_ensembles(egs_world *w, int32_t n_ensembles) {
  return n_ensembles != w->ens.n_ens ? fail(w->ctx, EGS_ERR_INVALID, "n_ensembles differs from the world's") : EGS_OK;
}

// ---- world.cpp -----------------------------------------------------------------------------------------------------
// What is wrong with a shape array (nothing: an empty string); side = NULL: the side lengths are not known yet
std::string shapes_fault(int n, const int32_t *shape, const double *side);
// UpdateContacts + pruning on the device (ensembles.cc:393-394), the topology read-back, and a re-plan only when the
// constraint topology changed: the front of every stepping entry and of the detecting stabilise passes.  lap (may be
// NULL) takes laps 0 .. 2: collide, topology, re-plan.
void world_update_contacts(egs_world *w, PhaseTimer *lap);

// ---- world_step.cpp ------------------------------------------------------------------------------------------------
// "bodies set, dt > 0, fp64" of the stepping entries, in that order; fp64_what = NULL: either precision will do
egs_status world_step_guard(egs_world *w, double dt, const char *fp64_what);
// the arguments of the _each entries, in the scalar guard's order: bodies set, the tables and every dt[e] >= 0, fp64
egs_status world_each_guard(egs_world *w, int32_t n_ensembles, const double *dt, const double *erp, const char *fp64_what);
// the host may write the page-locked block of the _each entries again: the last copy out of it has been made
void world_each_block(egs_world *w);
// The front of a step: live inertia (M^-1, f_ext and Wf of the state this step starts from; a free body reads Wf too),
// dt [E] and erp [E] to the device when the step has them (rates; returned, else NULL), the contact update.
const EnsembleRates *world_step_begin(egs_world *w, const double *dt_each, const double *erp_each, int32_t detect_contacts,
                                      PhaseTimer *lap, EnsembleRates &rates);
void world_fill_friction(egs_world *w);
void world_fill_restitution(egs_world *w);
// the assembly of a step: J, err, bounds, rhs (ensembles.cc:565-570), on one dt / erp or on every ensemble's own
void world_assemble(egs_world *w, double dt, double erp, const EnsembleRates *each);
// the tail of a step: velocities from the accumulators (ensembles.cc:535, 572), then StepPositions_ODE
void world_integrate(egs_world *w, double dt, const EnsembleRates *each);
// the warm start's history: dropped, matched against the assembled list, taken from the list just solved
void world_drop_history(egs_world *w);
void world_warm_match(egs_world *w, const double *dt_each);
void world_warm_snapshot(egs_world *w, const double *dt_each);

}  // namespace egs
