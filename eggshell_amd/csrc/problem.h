// problem.h -- the device-resident problem (struct egs_problem) and what the host units call on it: topology and
// plan (problem.cpp), assembly and velocity update (problem.cpp), the solve driver (solve.cpp).  The dense and world
// units use a problem through this header only.
#pragma once

#include "kernels.h"
#include "matvec_plan.h"
#include "plan.h"
#include "policy.h"
#include "runtime.h"

namespace egs {

// A plan's seven schedule tables on the device: lanes, the static timetable (plan.h), the tiles' body slots.
struct DevicePlan {
  DevBuf<LaneDesc> lanes;
  DevBuf<uint16_t> lane_level;
  DevBuf<int32_t> tile_period, tile_depth;
  DevBuf<int32_t> tile_nslots, tile_slot_off, slot_body;
  void stage(egs_context *ctx, const Plan &pl) {
    egs::stage(ctx, lanes, pl.lanes);
    egs::stage(ctx, lane_level, pl.lane_level);
    egs::stage(ctx, tile_period, pl.tile_period);
    egs::stage(ctx, tile_depth, pl.tile_depth);
    egs::stage(ctx, tile_nslots, pl.tile_nslots);
    egs::stage(ctx, tile_slot_off, pl.tile_slot_off);
    egs::stage(ctx, slot_body, pl.slot_body);
  }
};
// ... and the four of its oversize islands' body patches (ticket kernels: no timetable)
struct DevicePatches {
  DevBuf<LaneDesc> lanes;
  DevBuf<int32_t> tile_nslots, tile_slot_off, slot_body;
  void stage(egs_context *ctx, const Plan &pl) {
    egs::stage(ctx, lanes, pl.patch_lanes);
    egs::stage(ctx, tile_nslots, pl.patch_tile_nslots);
    egs::stage(ctx, tile_slot_off, pl.patch_tile_slot_off);
    egs::stage(ctx, slot_body, pl.patch_slot_body);
  }
};

}  // namespace egs

struct egs_problem {
  egs_context *ctx = nullptr;
  int n = 0, m = 0, precision = EGS_F64;
  egs::Plan plan;                     // 1 lane per constraint (built lazily when the quad schedule applies)
  bool tile_plan_ready = false;
  std::vector<int32_t> h_body0, h_body1;
  egs::DevicePlan tile;          // plan's tables
  // latency-optimised schedule (4 lanes per constraint, 64-constraint tiles);
  // used for GS/SOR when the problem is small and every island fits a tile
  egs::Plan planq;
  bool use_quad = false;
  uint32_t last_sched = 0;     // SweepSchedule::flags() of the last solve launch
  // ... of which egs_solve_stats.schedule leaves these out and egs_problem_get_schedule reports them: refinements of a
  // form that is already reported.  Callers compare that field exactly between a form's switch on and off.
  static constexpr uint32_t kSchedRefinements = EGS_SCHED_CHAIN;
  // ... and these are left out of egs_problem_get_schedule too, whose callers compare it with EGS_SCHED_CHAIN masked
  // against the statistics: egs_problem_get_schedule_full alone reports them
  static constexpr uint32_t kSchedFullOnly = EGS_SCHED_SHARE;
  // ... and these out of that one as well, whose callers compare it exactly on scenes that take the form:
  // egs_problem_get_schedule_forms alone reports them
  static constexpr uint32_t kSchedFormsOnly = EGS_SCHED_FACE | EGS_SCHED_FACE_SPLIT | EGS_SCHED_FACE_LEAN;
  bool lin_neg = false;        // J1_lin == -J0_lin on every two-body constraint, in value and bit for bit, signed zeros
                               // included (device assembly: contacts only, note_kinds; egs_problem_set_blocks: checked)
  bool joint_pairs = false;    // a ball joint joins two bodies: its assembled J1_lin holds +0 where J0_lin holds +0
  bool contacts_only = false;  // no constraint is a joint (note_kinds): every row has a contact's bounds, (-1, -1, 0) .. (1, 1, +inf)
  int linsym_bodies = -1;      // LINSYM's body preconditions (launch_linsym_bodies) on the device, -1: not decided yet
  // SHARE's precondition on the chained tile plan (plan.h: plan_shares_normals; launch_share_normals on the device):
  // 1 / 0, kShareUndecided: data came from the host and nobody has looked yet (the first choose_sweep that offers the
  // CHAIN form does: decide_share_normals, 4 bytes back), kShareDeviceData: data was, or will be, written on the device
  // (a world's collider) or is not there yet -- "no" without a look, which would cost a synchronisation per step.
  // Every writer of data sets one of the last two; a new tile plan turns a decided answer back to undecided.
  static constexpr int kShareUndecided = -1, kShareDeviceData = -2;
  int share_normals = kShareDeviceData;
  // FACE's precondition on a faced tile plan (plan.h: plan_faces_normals), the second answer of the same look: valid
  // while share_normals is 1, which it implies
  bool face_normals = false;
  // which kernel takes the oversize islands of a GS / SOR solve (choose_oversize_schedule; EGS_PATCH=0
  // forces the all-global kernel, EGS_QUAD_PATCH=0 the 1-lane patches) and how many workgroups the
  // all-global kernel's persistent grid may have: both from the runtime's occupancy of the kernels
  int oversize = 2;            // OversizeSchedule
  int global_max_blocks = 1;
  egs::DevicePlan quad;          // planq's tables
  egs::DevBuf<unsigned char> wsB0, wsB1, wsD, wsInv;
  egs::DevBuf<egs::GlobalDesc> gcons;
  egs::DevBuf<uint32_t> gtickets;
  egs::DevBuf<unsigned long long> trace;   // EGS_TRACE_UPDATES=1: [sweeps][m] completion times of the last patch launch
  int trace_sweeps = 0;
  egs::DevBuf<unsigned char> ggran;   // [n][6] x 16 B: data-tagged granules of the 4-lane body patches (quad_solve.hip)
  uint32_t gran_epoch = 0;
  // The FACE launch split in time (solve.cpp: face_work; step_face.hip).  The piece list is a function of
  // face_key = {tiles, resident slots, split tiles, s1, sweeps} alone: built and uploaded when that changes, never
  // inside a step otherwise.  face_sync: [0] the ticket counter, which only grows (face_ticket_base is what it stands
  // at before the next launch), [1 + tile] the launch epoch of the tile's last published first part.
  std::vector<egs::FacePiece> h_face_pieces;
  egs::DevBuf<egs::FacePiece> face_pieces;
  long face_key[5] = {-1, -1, -1, -1, -1};
  egs::DevBuf<uint32_t> face_sync;
  uint32_t face_ticket_base = 0, face_epoch = 0;
  // oversize islands as body patches (GS/SOR): LDS for private bodies, global for shared
  egs::DevicePatches patch;
  // topology + state (fp64)
  egs::DevBuf<int32_t> body0, body1, kind;
  egs::DevBuf<double> pos, R, v, w, Minv_d, f_ext, data, err, v6, res_partials;
  egs::DevBuf<double> Wf;            // M^-1 f_ext per body, rebuilt when either is re-uploaded
  bool wf_valid = false;
  // The deferred system.  A step whose launch assembled in its prologue without storing (step_solve.hip:
  // STORE_SYSTEM = false) leaves J0, J1, rhs, lo, hi, err and is_eq NOT materialised: sys_deferred is set and
  // {deferred_dt, deferred_erp} is what assemble_kernel needs to make them (ensure_system: the same bits).  Every
  // reader of those arrays calls ensure_system first, and so does every writer of an assembly input -- except
  // egs_problem_advance, the writer of the step loop: it writes the new state into the second set (prev_*) and swaps
  // the sets, so the state the step read stays intact in prev_* (deferred_prev) until the next step or advance.
  bool sys_deferred = false, deferred_prev = false;
  double deferred_dt = 0.0, deferred_erp = 0.0;
  egs::DevBuf<double> prev_pos, prev_R, prev_v, prev_w;
  // solver arrays, REAL = double or float (byte buffers)
  egs::DevBuf<unsigned char> Minv_r, J0, J1, lo, hi, rhs, x, acc, wres;
  egs::DevBuf<unsigned char> gB0, gB1, gD, gden, gdx;  // cross-workgroup workspace
  egs::DevBuf<uint8_t> is_eq;
  // [0]: device-side ordering wait timed out (EGS_ERR_STALL).  STICKY: the solve kernels OR into
  // it and only reporting it clears it, so a stall in any step of an asynchronous run is seen.
  // [1]: scratch word of the isotropy check.
  egs::DevBuf<int32_t> error_flag;
  // page-locked copy of [0] (64 bytes), refreshed by an async copy after every solve -- except one that was a FACE launch
  // alone, whose kernel stores to it through h_flag_dev where a wait overruns (step_face.hip)
  egs::PinnedBuf<int32_t> h_flag;
  int32_t *h_flag_dev = nullptr;    // its device address (hipHostGetDevicePointer, once per problem)
  // egs_problem_step's velocities.  The step offers them to its solve; a FACE launch that is the whole solve, on a plan
  // whose tiles hold every body (plan_covers_bodies: a body in no tile still moves by dt W f), writes them in its
  // epilogue and says so, and the step then skips velocity_kernel.
  enum { kVelocityNone = 0, kVelocityOffered = 1, kVelocityWritten = 2 };
  int step_velocity = kVelocityNone;
  bool plan_covers_bodies = false;  // of the tile plan: every body 0 .. n - 1 is a slot of some tile
  egs::PinnedBuf<double> h_hist;    // page-locked landing area of the stopping loop's per-sweep residual sums (+ the flag)
  // per-sweep history of a chunk of sweeps (tolerance-terminated solves, see kernels.h)
  egs::DevBuf<unsigned char> hist_x, hist_acc;
  egs::DevBuf<double> hist_out;
  int hist_sweeps = 0;        // 0: off for the next launch; k: record k sweeps
  bool residual_pending = false;   // wres/x hold a finished solve whose residual sums were not reduced yet
  bool have_blocks = false, have_state = false, have_constraints = false, minv_r_valid = false;
  // stand-alone mat-vec (matvec_plan.h): schedule built at the first product after a topology change
  egs::MatvecPlan mvplan;
  bool mv_ready = false;
  egs::DevBuf<egs::MvLane> mv_lanes;
  egs::DevBuf<egs::MvTile> mv_tiles;
  egs::DevBuf<egs::MvSlot> mv_slots;
  egs::DevBuf<uint16_t> mv_ents;
  egs::DevBuf<egs::MvBoundary> mv_boundary;
  egs::DevBuf<unsigned char> mv_T, mv_x, mv_y;
  egs::DevBuf<unsigned char> tmp_rows;   // [3m] REAL scratch
  egs::DevBuf<double> dense_A;        // J M^-1 J^T + cfm I of the dense path (egs_problem_dense_system), [3m][3m]
  double dense_cfm = -1.0;       // the cfm dense_A was built with (< 0: not built)
  // row types and bounds of the assembled system on the host (the dense path partitions by them): they depend on the
  // constraint kinds only (joints.cc:13-35, contact.cc:103-113), so they are read back once per set of kinds
  std::vector<uint8_t> h_rows_eq;
  std::vector<double> h_rows_lo, h_rows_hi;
  bool h_rows_valid = false;
  // Where a solve starts (egs_problem_set_start).  start holds x0 [3m] REAL: uploaded once (GIVEN) or copied from x
  // before a solve's first launch (PREVIOUS, while have_lambda).  start_active is set for the duration of a solve that
  // takes it (solve.cpp: StartScope): launch_solve_t hands it to every fresh launch as SolveArgs::x0.
  int start_mode = EGS_START_RHS;
  egs::DevBuf<unsigned char> start;
  bool have_lambda = false;    // x holds the lambda of a finished solve on the current constraint list
  bool start_active = false;
  // The Coulomb pyramid (egs_problem_set_friction, egs_world_set_friction): mu [m] REAL, one coefficient per constraint,
  // >= 0: rows 0 and 1 are bounded by +-mu x_n, < 0: the stored bounds.  friction: some coefficient is >= 0 -- the
  // solve launches and the residual take mu and run their friction forms (solve.cpp: choose_sweep); off, nothing reads
  // mu.  A new topology turns it off: the coefficients belong to the list they were given for.
  egs::DevBuf<unsigned char> mu;
  bool friction = false;
  // Restitution (egs_problem_set_restitution, egs_world_set_restitution): rest [m] fp64, one coefficient per constraint,
  // >= 0: a contact's normal row bounces above the approach speed rest_vth (assemble_device.h: restitution_target), < 0:
  // assembled as stored.  restitution: some coefficient is >= 0 -- then every assembly takes the table (assemble_args);
  // off, nothing reads it.  A new topology turns it off, as it does friction (the world refills both).
  egs::DevBuf<double> rest;
  bool restitution = false;
  double rest_vth = 0.0;
  // Hinge motors (egs_problem_set_motors, egs_world_set_joint_motors): motor [m][2] fp64 = (speed, tau) per constraint;
  // a HINGE_AXIS constraint with tau >= 0 gets +-tau on its axis row and speed / dt as its target (assemble_device.h:
  // motor_row).  motors: some hinge has tau >= 0 -- then every assemble_kernel launch takes the table (motor_table);
  // off, nothing reads it.  A new topology turns it off (the world refills it).  hinges / hinges_pinned: the kinds hold
  // a HINGE_AXIS / one whose axis row stays pinned at lo = hi = 0 under the table in force (the dense steps refuse it).
  egs::DevBuf<double> motor;
  bool motors = false;
  bool hinges = false, hinges_pinned = false;
  // Hinge limits (egs_problem_set_hinge_limits, egs_world_set_joint_limits): limit [m][8] fp64 = (q, sin lo, cos lo,
  // sin hi, cos hi) per constraint (assemble_device.h: limit_row).  limits: some hinge has a stop -- then every
  // assemble_kernel launch takes the table (hinge_tables) and the dense steps refuse, naming limited_hinge (the first
  // such constraint); off, nothing reads it.  A new topology or new constraints turn it off (the world refills it).
  egs::DevBuf<double> limit;
  bool limits = false;
  int limited_hinge = -1;
  bool angular = false;               // the kinds hold a LOCK or a HINGE_AXIS: the assembly launches their form (kernels.h)
  // Sliders (EGS_JOINT_SLIDER_AXIS).  sliders: the kinds hold one -- then every assemble_kernel launch runs the slider
  // form (hinge_tables) and no LINSYM schedule runs (note_kinds); pinned_slider: the first whose rail row stays pinned at
  // lo = hi = 0 under the motor table in force (-1: none; the dense steps refuse it by name).  Travel stops
  // (egs_problem_set_slider_limits, egs_world_set_slider_limits): travel [m][2] fp64 = (xlo, xhi) per constraint
  // (assemble_device.h: slider_stop_row).  travels: some slider has a finite stop -- then the slider form takes the
  // table and the dense steps refuse, naming stopped_slider (the first such); off, nothing reads it.  A new topology or
  // new constraints turn it off (the world refills it).
  bool sliders = false;
  int pinned_slider = -1;
  egs::DevBuf<double> travel;
  bool travels = false;
  int stopped_slider = -1;
  std::vector<int32_t> h_kind;         // the kinds of the list (note_kinds)
  // egs_problem_set_dense_friction: max_outer > 0 makes egs_problem_step_dense solve the pyramid while friction is on
  // (0: it refuses); the outcome of the last such step (egs_problem_dense_friction_info).
  int dense_fric_outer = 0;
  double dense_fric_tol = 0.0;
  bool dense_fric_valid = false;
  int dense_fric_solves = 0, dense_fric_converged = 0;
  double dense_fric_change = 0.0;
  // Live inertia (egs_problem_set_live_inertia): inertia_body [n][9], the applied torque [n][3]
  // (live_has_torque) and the mask [n] of the bodies whose inertia_body is not a multiple of the identity.  live_any:
  // the mask selects some body -- then refresh_live_mass launches live_mass_kernel at the start of every stepping entry
  // and minv_iso stays false (ensure_minv_real); without one the feature changes nothing at all.
  egs::DevBuf<double> live_inertia, live_torque;
  egs::DevBuf<uint8_t> live_mask;
  bool live_any = false, live_has_torque = false;
  bool minv_iso = false;       // every M^-1 block is diag(a,a,a,b,b,b): the tile kernel keeps no B (EGS_ISO=0 disables)
  int last_iterations = 0;
  size_t real_size() const { return precision == EGS_F32 ? sizeof(float) : sizeof(double); }
};

namespace egs {

// The precision of a problem's solver arrays as a type: f(float{}) or f(double{}).  The one place that turns
// egs_problem::precision into a template argument; a callable that differs by precision in more than the type
// (conversions, scale factors) does that inside.
template <typename F>
auto with_real(const egs_problem *p, F &&f) {
  if (p->precision == EGS_F32) return f(float{});
  return f(double{});
}
// a solver array (byte buffer) as the REAL array it holds
template <typename REAL>
REAL *real(const DevBuf<unsigned char> &b) { return reinterpret_cast<REAL *>(b.p); }

// ---- problem.cpp ---------------------------------------------------------------------------------------------------
egs_status check_topology(egs_context *ctx, int32_t n, int32_t m, const int32_t *body0, const int32_t *body1);
void problem_set_topology(egs_problem *p, int32_t m, const int32_t *body0, const int32_t *body1, bool fresh = true);
void ensure_tile_plan(egs_problem *p);
// share_normals of a problem whose tile plan is ready and chained, while it is kShareUndecided (synchronises once)
void decide_share_normals(egs_problem *p);
void ensure_minv_real(egs_problem *p);
// Live inertia: M^-1 (fp64 and working precision), f_ext and Wf of the masked bodies from the R and w the device holds
// now.  One launch, no synchronisation while the caller's M^-1 / f_ext uploads are converted already; a no-op unless
// live_any.  Every stepping entry calls it before anything reads those arrays.
void refresh_live_mass(egs_problem *p);
// the checks and the state change of egs_problem_set_live_inertia / egs_world_set_live_inertia
egs_status set_live_inertia(egs_problem *p, const double *inertia_body, const double *torque);
void note_kinds(egs_problem *p, const int32_t *kind);
// what egs_problem_set_constraints refuses in a list of kinds and descriptors (NULL: nothing)
const char *constraints_fault(int m, const int32_t *kind, const int32_t *body0, const double *data);
void note_assembled(egs_problem *p);
AssembleArgs assemble_args(egs_problem *p, double dt, double erp);
// the motor, limit and travel tables the assembly launches take beside it: p->motor / p->limit / p->travel while they
// are on, else NULL, and whether the list holds a slider
inline egs::HingeTables hinge_tables(const egs_problem *p) {
  return egs::HingeTables{p->motors ? p->motor.p : nullptr, p->limits ? p->limit.p : nullptr,
                          p->sliders && p->travels ? p->travel.p : nullptr, p->sliders};
}
// What is wrong with a travel table lim [m][2] for the kinds given (nothing: NULL): a NaN anywhere; on a SLIDER_AXIS
// row xlo = +inf, xhi = -inf or xlo > xhi.  *first: the first SLIDER_AXIS constraint with a finite stop (-1: none).
const char *travel_fault(size_t m, const int32_t *kind, const double *lim, int *first);
// What is wrong with a limit table lim [m][8] for the kinds given (nothing: NULL; rows of other kinds are not read),
// and in *first the first HINGE_AXIS constraint with a stop (-1: none).
const char *limits_fault(size_t m, const int32_t *kind, const double *lim, int *first);
// hinges / hinges_pinned / pinned_slider from the kinds and motor [m][2] (NULL: none): problem.h
void note_hinges(egs_problem *p, const double *motor);
void do_assemble(egs_problem *p, double dt, double erp);
// J0, J1, rhs, lo, hi, err and is_eq are materialised after this (a no-op unless the last step deferred them)
void ensure_system(egs_problem *p);
void do_velocity(egs_problem *p, double dt);
// do_assemble / do_velocity with every constraint / body on its ensemble's rates (kernels.h: EnsembleRates)
void do_assemble_each(egs_problem *p, const EnsembleRates &r);
void do_velocity_each(egs_problem *p, const EnsembleRates &r);
void zero_accumulators(egs_problem *p);
void post_flag_copy(egs_problem *p);
egs_status report_stall(egs_problem *p);
// Non-blocking look at the page-locked copy: true once the copy behind a stalled solve has
// landed.  Entry points that enqueue more work call it first; entry points that have just
// synchronised see every earlier solve.
inline bool stall_seen(const egs_problem *p) { return p->h_flag.p && *static_cast<volatile int32_t *>(p->h_flag.p) != 0; }

// ---- solve.cpp -----------------------------------------------------------------------------------------------------
egs_status validate_params(egs_context *ctx, const egs_solve_params *prm);
void fill_stats(egs_problem *p, egs_solve_stats *st);
void launch_residual(egs_problem *p);
double read_residual(egs_problem *p, int *err_flag);
egs_status do_solve(egs_problem *p, const egs_solve_params *prm, egs_solve_stats *stats, const AssembleArgs *assemble = nullptr);
bool step_fuses_assembly(egs_problem *p, const egs_solve_params *prm);
// the next solve starts from p->start instead of rhs: a GIVEN start, or PREVIOUS with a lambda to take
inline bool solve_takes_start(const egs_problem *p) {
  return p->start_mode == EGS_START_GIVEN || (p->start_mode == EGS_START_PREVIOUS && p->have_lambda);
}
void accumulators_from_lambda(egs_problem *p);

struct BatchSolveState {
  EnsembleSegs segs;               // device tables (owned by the world)
  DevBuf<int32_t> ints;            // running [E], iterations [E], n_running
  DevBuf<double> res;              // residual [E]
  DevBuf<double> err;              // [sweeps][E] of the last evaluation
  DevBuf<unsigned char> fin_x, fin_acc;
  PinnedBuf<int32_t> h_ints;       // page-locked: iterations [E], n_running, stall flag
  PinnedBuf<double> h_res;         // page-locked: residual [E]
  EnsembleStop stop() {
    const size_t E = (size_t)segs.n_ens;
    return EnsembleStop{ints.p, ints.p + E, res.p, ints.p + 2 * E};
  }
  void ensure(int E) {
    ints.alloc(2 * (size_t)E + 1);
    res.alloc((size_t)E);
    h_ints.alloc((size_t)E + 2);
    h_res.alloc((size_t)(E > 0 ? E : 1));
  }
};
egs_status do_solve_batch(egs_problem *p, const egs_solve_params *prm, BatchSolveState &B, const int32_t *active = nullptr);

}  // namespace egs
