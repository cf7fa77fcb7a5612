// kernels.h -- launch interface between the C-ABI layer and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "plan.h"

namespace egs {

struct AssembleCore {
  int32_t n, m;
  const double *pos, *R, *v, *w;                 // body state, fp64
  const double *Wf;                              // [n][6] M^-1 f_ext (launch_mass_times_force)
  const int32_t *kind, *body0, *body1;
  const double *data;                            // [m][7]
  double dt, erp;
  void *J0, *J1, *lo, *hi, *rhs;                 // REAL outputs
  double *err;                                   // [3m] fp64
  uint8_t *is_eq;
};
struct AssembleArgs : AssembleCore {
  // restitution (assemble_device.h: restitution_target): one coefficient per constraint [m], >= 0: a contact's normal
  // row bounces above the approach speed vth, < 0: as stored.  NULL = off.
  const double *rest = nullptr;
  double vth = 0.0;
};
// Per-ensemble rates of a step (egs_world_step_each), device tables: body -> ensemble [n], dt [n_ens], erp [n_ens].
// A constraint takes its first body's ensemble's pair instead of AssembleArgs' dt / erp, a body its ensemble's dt.
// dt[e] == 0: ensemble e sits the step out (rhs rows exactly 0, bodies left alone).  Kept out of AssembleArgs, which
// is part of SolveArgs: the kernel arguments of the solve launches stay what they are.
struct EnsembleRates {
  const int32_t *body_ens = nullptr;
  const double *dt = nullptr, *erp = nullptr;
};

// Flat system + tile plan, all device pointers.
template <typename REAL>
struct SolveArgs {
  const LaneDesc *lanes;
  const int32_t *tile_nslots;
  const int32_t *tile_slot_off;
  const int32_t *slot_body;
  const REAL *Minv;            // [n][36]
  const REAL *J0, *J1;         // [m][18]
  const uint8_t *is_eq;        // [3m]
  const REAL *lo, *hi, *rhs;   // [3m]
  REAL *x;                     // [3m]  in (resume) / out
  REAL *acc;                   // [n][6] in (resume) / out
  REAL *wres;                  // [3m]  out: A x - rhs
  // per-constraint derived blocks (quad kernel only), written by cons_prepare:
  REAL *wsB0, *wsB1;           // [m][18]  W J^T as 6x3 row-major
  REAL *wsD, *wsInv;           // [m][9], [m][3]
  const int32_t *body0, *body1; // [m] (cons_prepare only)
  int32_t m;
  int32_t *error_flag;
  REAL cfm, kscale;
  int32_t sweeps, resume, max_slots;
  uint32_t spin_limit;
  // static timetable of the same sweep (step_device.h, plan.h): per lane its level, per tile the
  // period P and the depth of the level DAG
  const uint16_t *lane_level = nullptr;
  const int32_t *tile_period = nullptr, *tile_depth = nullptr;
  int32_t n_tiles = 0;
  int32_t runs = 0;            // the timetable counts groups of four constraints (plan.h: Plan::runs)
  int32_t patch_runs = 0;      // body patches: the lanes come in chunks of four quads (Plan::patch_runs, quad_solve.hip)
  int iso = 0;              // 1: every M^-1 block is diag(a,a,a,b,b,b): B is formed on the fly (tile kernel)
  int linsym = 0;           // 1 (with iso, fp64, GROUP = 1): J1_lin = -J0_lin and wl0 = wl1 bit for bit on every
                            // two-body constraint: step_solve_kernel keeps one linear block (step_solve.hip: LINSYM)
  int steady = 0;           // 1: step_solve_kernel (GROUP = 1, no snapshots) runs the steady-state loop between the
                            // fill and the drain of its timetable (step_device.h)
  // step_solve_kernel's ASSEMBLE form (launch_step_solve_assemble): every lane assembles its constraint from this
  // body state in the prologue and also leaves the blocks where assemble_kernel would (J0 .. is_eq above point there).
  // An fp64 launch only: the fp32 argument block keeps the core alone and with it its size (16 bytes more cost the
  // fp32 Jacobi tile kernels two VGPRs and a wavefront of occupancy: DESIGN.md section 4j).
  std::conditional_t<sizeof(REAL) == 8, AssembleArgs, AssembleCore> assemble{};
  // Per-sweep history (tolerance-terminated solves): x after sweep s and each body's
  // accumulator once its last constraint of sweep s has run, s = 1..sweeps of this launch.
  // hist_residual then evaluates the reference's per-iteration stopping test for the
  // whole chunk from these snapshots: one launch and one read-back per chunk instead of
  // one per sweep.  NULL = off.
  REAL *hist_x = nullptr;      // [sweeps][m][3]
  REAL *hist_acc = nullptr;    // [sweeps][n_bodies][6]
  int32_t n_bodies = 0;
  // body patches on the 4-lane kernel: a shared body's accumulator crosses between patches as six data-tagged
  // 16-byte granules {value, launch epoch << 32 | ticket} (quad_solve.hip); NULL = the flag protocol (g_tick)
  void *gran = nullptr;        // [n_bodies][6] x 16 B
  uint32_t gran_epoch = 0;
  // diagnostics (EGS_TRACE_UPDATES=1): completion time (100 MHz wall clock) of every update of the 4-lane patch kernel
  unsigned long long *trace = nullptr;   // [sweeps][m]
  // the start of a fresh launch (!resume), [3m]; NULL: rhs, Q7.  Never aliases x.  step_solve_kernel's ASSEMBLE form
  // does not read it: a started step assembles with assemble_kernel (solve.cpp: choose_sweep)
  const REAL *x0 = nullptr;
  // Coulomb pyramid: one coefficient per constraint [m], >= 0: rows 0 and 1 are bounded by +-mu x_n (solve_device.h:
  // project_pyramid), < 0: the stored bounds.  NULL = friction off: the launch runs the instantiations without it.
  const REAL *mu = nullptr;
};

template <typename REAL>
struct GlobalArgs {
  const GlobalDesc *cons;      // [mg]
  int32_t mg, per_lane;        // constraints, constraints per lane
  int32_t n_bodies, pad0;
  const REAL *Minv, *J0, *J1;
  const uint8_t *is_eq;
  const REAL *lo, *hi, *rhs;
  REAL *x, *acc, *wres;
  REAL *B0, *B1, *D, *den, *dx; // workspace [mg][18|18|9|3|3]
  uint32_t *tickets;           // [n] zeroed before every launch
  int32_t *error_flag;
  REAL cfm, kscale;
  int32_t sweeps, resume, method;
  int32_t mode;                // 0 = full sweeps, 1 = ordered accumulate of dx only
  uint32_t spin_limit;
  // per-sweep snapshots for tolerance-terminated solves, as in SolveArgs (NULL = off)
  int32_t m = 0, pad1 = 0;     // all constraints of the problem (hist_x stride)
  REAL *hist_x = nullptr, *hist_acc = nullptr;
  const REAL *x0 = nullptr;    // the start of a fresh launch, as in SolveArgs (NULL: rhs, Q7)
  const REAL *mu = nullptr;    // the friction coefficients, as in SolveArgs (NULL: off)
};


// Wf[b] = M_b^-1 f_ext,b: both frozen at Init (Q5) unless live inertia is on, so assembly and the velocity update
// read these 48 B per body instead of the 288 B block and the force (same expression, same bits).
void launch_mass_times_force(int n, const double *Minv, const double *f_ext, double *Wf, hipStream_t s);
// Live inertia (egs_problem_set_live_inertia): for every body b with live_mask[b] != 0, from R [n][9], w [n][3] and
// inertia_body [n][9], the angular 3x3 of Minv[b] (fp64) and of Minv_r[b] (its (REAL) conversion), f_ext[b][3:6] =
// torque[b] + gyroscopic torque (torque NULL: the gyroscopic torque alone) and Wf[b], with the bits of
// orc_minv_blocks / orc_external_force / mass_times_force_kernel.  Other bodies are neither read nor written.
template <typename REAL>
void launch_live_mass(int n, const double *R, const double *w, const double *inertia_body, const double *torque,
                      const uint8_t *live_mask, double *Minv, REAL *Minv_r, double *f_ext, double *Wf, hipStream_t s);
template <typename REAL>
void launch_tile_solve(const SolveArgs<REAL> &a, int method, int n_tiles,
                       int block, hipStream_t s);
// the same GS / SOR sweep on the plan's static timetable: one workgroup barrier per time step, no tickets.  With
// a.iso on 256-constraint tiles: `group` tiles per workgroup (fp32: 1, 2 or 4; fp64: 1 or 3) and, fp64 with group 1,
// the LINSYM form if `linsym`; the per-sweep snapshots (a.hist_x) always take group 1 without LINSYM.  The caller
// decides both (solve.cpp: choose_sweep).
template <typename REAL>
void launch_step_solve(const SolveArgs<REAL> &a, int method, int n_tiles, int block, int group, bool linsym, hipStream_t s);
// the LINSYM form with the assembly in its prologue (a.assemble; a fresh solve, 256-constraint tiles, no snapshots;
// a.assemble.rest set: the restitution instantiations, the same sweep behind a prologue that bounces the normal rows):
// assemble_kernel and this launch in one, with the blocks, lambda, w and the accumulators of both, bit for bit.
// store_system = false: J0, J1, rhs, lo, hi, err and is_eq are not written (the caller defers them: problem.h)
void launch_step_solve_assemble(const SolveArgs<double> &a, int method, int n_tiles, bool store_system, hipStream_t s);
// the PAIR form of that launch, one update on a lane pair (step_pair.hip): the same arguments, the same bits on any plan,
// worth it on a pairable one
// chain (on a plan that is Plan::chained, a.steady on): the CHAIN form of its steady loop, the pair's accumulators in
// registers between its two updates; the same bits
// share (with chain, where the two contacts of every thread pair carry one normal: problem.h, share_normals): the SHARE
// form, one linear block and one pair of weights per lane for both constraints; the same bits.  share without chain
// is no form: std::logic_error
void launch_step_solve_pair(const SolveArgs<double> &a, int method, int n_tiles, bool store_system, bool chain, bool share,
                            hipStream_t s);
// the FACE form of the share launch (step_face.hip): GS, store-free, no restitution, on a plan that is Plan::faced whose
// groups of four carry one normal (problem.h: face_normals), a.steady on; 128 threads per tile; the same bits.
// tiles_per_cu: 3 or 4 resident tiles per CU (4: what the registers allow; 3: the launch asks for more LDS)
// w.pieces NULL: one workgroup per tile, blockIdx = tile.  Otherwise the persistent form (the launch split in time, or
// more tiles than resident slots): w.n_workgroups workgroups take the pieces of w.pieces (policy.h: face_piece_list) by
// ticket; a split tile's first part hands lambda and the accumulators to its second part through a.x / a.acc and
// flags[tile]; the same bits.
// w.v6 (NULL: off): the epilogue also writes the step's velocities of the bodies of its tile, velocity_kernel's
// expression on the accumulator it has just stored (a first part does not: its accumulators are not final).
struct FacePiece;
struct FaceWork {
  const FacePiece *pieces;   // [n_pieces]
  uint32_t *counter;         // the problem's ticket counter: never reset, ticket = the value drawn - ticket_base
  uint32_t *flags;           // [n_tiles] the epoch of the launch whose first part of the tile has been stored
  uint32_t ticket_base, epoch;
  int32_t n_pieces;
  int32_t n_workgroups;      // the grid: min(pieces, resident slots); every workgroup draws tickets until one is past the list
  double *v6;                // [n][6] the velocities egs_problem_step leaves (problem.h: v6), or NULL
  int32_t *host_stall;       // the device address of the problem's page-locked stall word: a wait that overran stores 1
};
// lean: the LEAN twins (linear held products alone, 168 VGPRs, six tiles per CU; tiles_per_cu may then be 6 too); the same bits.
// Where a lean tile's LDS request does not fit (policy.h: face_lds_bytes returns 0) the caller keeps the present form:
// asked for all the same, std::logic_error.
void launch_step_solve_face(const SolveArgs<double> &a, int n_tiles, int tiles_per_cu, bool lean, const FaceWork &w,
                            hipStream_t s);
// ... and the 4-lanes-per-constraint schedule on the same timetable (quad_solve.hip)
template <typename REAL>
void launch_step_quad(const SolveArgs<REAL> &a, int method, int n_tiles, int tile_size, hipStream_t s);
// max_blocks: how many workgroups of the persistent grid may be launched (all must be resident)
template <typename REAL>
void launch_global_solve(const GlobalArgs<REAL> &a, int max_blocks, hipStream_t s);
// workgroups per CU the hardware keeps resident for the cross-workgroup kernels' exact
// instantiations (hipOccupancyMaxActiveBlocksPerMultiprocessor, the smallest over method /
// history variants); 0 if the query fails
template <typename REAL> int occupancy_global_solve();
template <typename REAL> int occupancy_patch_solve(size_t lds_bytes);
template <typename REAL> int occupancy_quad_patch_solve(size_t lds_bytes);
template <typename REAL> int occupancy_step_quad(int tile_size, size_t lds_bytes);
// w = A x - rhs for the constraints of a GlobalDesc list (after the last sweep)
template <typename REAL>
void launch_global_wres(const GlobalArgs<REAL> &a, hipStream_t s);
// oversize islands cut into body patches (plan.h): LDS for private bodies,
// global sc1 hand-off for shared ones
template <typename REAL>
void launch_patch_solve(const SolveArgs<REAL> &a, int method, int n_tiles, uint32_t *tickets, hipStream_t s);
// latency-optimised variant: 4 lanes per constraint, 64 constraints per tile
template <typename REAL>
void launch_cons_prepare(const SolveArgs<REAL> &a, hipStream_t s);
template <typename REAL>
void launch_quad_solve(const SolveArgs<REAL> &a, int method, int n_tiles, int tile_size, hipStream_t s);
template <typename REAL>
void launch_quad_patch_solve(const SolveArgs<REAL> &a, int method, int n_tiles, uint32_t *tickets, hipStream_t s);
// motor [m][2] or NULL: the hinge motors (egs_problem_set_motors).  Like EnsembleRates it is kept out of AssembleArgs,
// which is part of SolveArgs<double>: the solve launches keep their kernel arguments, and the fused prologue of
// step_solve_kernel never sees a hinge (solve.cpp: choose_sweep).  angular: the list holds an EGS_JOINT_LOCK or an
// EGS_JOINT_HINGE_AXIS; false launches the form without them (and without the motors), the code of the lists before them.
// limit [m][8] or NULL: the hinge limits (egs_problem_set_hinge_limits), travelling the same way; with a table the
// angular form's instantiation with limit_row runs, without one the kernel the lists ran before the limits.
// slider: the list holds an EGS_JOINT_SLIDER_AXIS; then the slider form runs, with motor, limit and travel [m][2] (the
// sliders' travel stops, egs_problem_set_slider_limits) as run-time pointers, NULL = off.  Without a slider no launch
// reads travel, and every list runs the kernel it ran before the sliders.
struct HingeTables {
  const double *motor = nullptr, *limit = nullptr, *travel = nullptr;
  bool slider = false;
};
template <typename REAL>
void launch_assemble(const AssembleArgs &a, bool angular, const HingeTables &h, hipStream_t s);
// ... with every constraint on its ensemble's rates (a.dt and a.erp are not read)
template <typename REAL>
void launch_assemble_each(const AssembleArgs &a, const EnsembleRates &t, bool angular, const HingeTables &h, hipStream_t s);
// dst[r] = the bound lo[r] of a slider's pinned rail row (kind 5, row 2, lo == hi), src[r] of every other row; dst may
// be src.  What a tolerance-terminated solve of a list with a slider starts from (solve.cpp: StartScope): the stopping
// test leaves pinned rows out, so the start must hold them at their bound already.  The rows of every other kind keep
// their start, so an ensemble without a slider in a batch that holds one starts as its own world does.
template <typename REAL>
void launch_pin_start(int rows, const REAL *src, const int32_t *kind, const REAL *lo, const REAL *hi, REAL *dst, hipStream_t s);
// partial sums of squares by row category: out[4*blocks].  mu [rows / 3] (may be NULL: off): rows 0 and 1 of a
// constraint with mu >= 0 are sorted by the pyramid's bounds, as in the kernels below that
// take the coefficients from SolveArgs::mu.
template <typename REAL>
void launch_residual_partials(int rows, const REAL *wres, const REAL *x,
                              const REAL *lo, const REAL *hi,
                              const uint8_t *is_eq, const REAL *mu, double *out, int blocks,
                              hipStream_t s);
template <typename REAL>
void launch_velocity(int n, const double *v, const double *w, const double *Wf, const REAL *acc,
                     double dt, double *v6, hipStream_t s);
// body b takes dt_each[body_ens[b]]; a body whose ensemble sits the step out (dt 0) keeps its velocity: v6 = (v, w)
template <typename REAL>
void launch_velocity_each(int n, const double *v, const double *w, const double *Wf, const REAL *acc,
                          const int32_t *body_ens, const double *dt_each, double *v6, hipStream_t s);
// Residual partial sums (the 4 categories of sparse_iterations.cc:51-69, `blocks` partial
// sums each, same reduction order as launch_residual_partials) for every sweep of a recorded
// chunk: out [sweeps][blocks][4].  write_sweep >= 1 also stores that sweep's w into wres.
template <typename REAL>
void launch_hist_residual(const SolveArgs<REAL> &a, int sweeps, int blocks, double *out, int write_sweep, hipStream_t s);
// ---- batched worlds (egs_world_create_batch): the per-ensemble stopping rule ----
// Ensemble e owns the constraints [jo[e], jo[e+1]) (its joints) and [mj + co[e], mj + co[e+1]) (its
// contacts), i.e. its own 3 m_e rows in two ranges, and the bodies [bo[e], bo[e+1]).  Device arrays.
struct EnsembleSegs {
  int32_t n_ens = 0, mj = 0;
  const int32_t *jo = nullptr, *co = nullptr, *bo = nullptr;
};
// Per-ensemble state of a tolerance-terminated solve, device arrays [n_ens]: still running, sweeps taken,
// residual (the last one checked while running); n_running counts the ensembles left after a selection.
struct EnsembleStop {
  int32_t *running = nullptr, *iterations = nullptr;
  double *residual = nullptr;
  int32_t *n_running = nullptr;
};
// err [sweeps][n_ens]: the residual of sparse_iterations.cc:51-69 of every ensemble after every recorded
// sweep, bit for bit what a world holding only that ensemble computes -- its own 3 m_e rows blocked as
// residual_partials_kernel blocks them (kResidualBlocks x 256 threads), the partial sums combined in
// read_residual's order, the square roots on the device.  w from the snapshots (xs / as, strides
// 3m and 6n per sweep, the w of hist_residual_kernel) or, if ws != NULL, read from it (sweeps = 1).
// Ensembles with running[e] == 0 are skipped (running == NULL: none).
template <typename REAL>
void launch_seg_residual(const SolveArgs<REAL> &a, const EnsembleSegs &S, const int32_t *running, const REAL *xs,
                         const REAL *as, const REAL *ws, int sweeps, double *err, hipStream_t s);
// The reference's stopping test per running ensemble over err [sweeps][n_ens], entry k being the state after
// `first + k` sweeps: the first checked entry (all_checked, or a multiple of `every`, or max_iters) with
// !(err > tol) stops it; an ensemble still running at max_iters takes the last entry.  A stopping ensemble
// gets its sweep count and residual and its lambda rows / body accumulators copied from entry k of xs / as
// into fin_x / fin_acc.  init = 1: every ensemble counts as running (the test of x0).
template <typename REAL>
void launch_seg_select(const EnsembleSegs &S, const EnsembleStop &T, const double *err, int sweeps, int first,
                       int max_iters, int every, double tol, int all_checked, int init, const REAL *xs, size_t xstride,
                       const REAL *as, size_t astride, REAL *fin_x, REAL *fin_acc, hipStream_t s);
// fixed sweep count: iterations[e] = sweeps (0 for an ensemble without constraints), residual[e] = err[e]
void launch_seg_fixed(const EnsembleSegs &S, const EnsembleStop &T, const double *err, int sweeps, hipStream_t s);

// The per-constraint friction coefficients of a world's list (egs_world_set_friction): constraint i < mj is a joint and
// gets -1, a contact gets mu_ens[ensemble of its first body] (body_ens == NULL: a plain world, ensemble 0), rounded to
// REAL.  The restitution table of egs_world_set_restitution is filled by the same kernel, REAL = double.
template <typename REAL>
void launch_fill_friction(int m, int mj, const int32_t *body0, const int32_t *body1, const int32_t *body_ens,
                          const double *mu_ens, REAL *mu, hipStream_t s);

template <typename REAL>
void launch_convert_minv(int count, const double *src, REAL *dst, hipStream_t s);
// *flag (preset to 1) is cleared unless every 6x6 block is exactly diag(a, a, a, b, b, b)
template <typename REAL>
void launch_minv_iso(int n, const REAL *W, int *flag, hipStream_t s);
// clears *flag unless every constraint has a body on side 1 and, where it also has one on side 0, both bodies carry
// the same linear weight W[0] bit for bit (the body preconditions of step_solve_kernel's LINSYM form)
template <typename REAL>
void launch_linsym_bodies(int m, const int32_t *body0, const int32_t *body1, const REAL *W, int *flag, hipStream_t s);
// plan_shares_normals (plan.h) on the device, for a chained plan of 256-lane tiles: *flag &= the two constraints of
// every thread pair have the same three normal bit patterns in data [m][7] (bit 0 of a flag that starts at 3: any
// mismatch clears the whole flag), and plan_faces_normals with it: bit 1 stays set only if the first of every odd
// wavefront's pair also has the normal of the pair 64 lanes below it, so that with bit 0 the four members of a group
// carry one normal
void launch_share_normals(int n_tiles, const LaneDesc *lanes, const double *data, int *flag, hipStream_t s);

// A = J M^-1 J^T + cfm I, [3m][3m] row-major fp64 on the device (ensembles.cc:510, 513-521)
void launch_dense_system(int m, const int32_t *body0, const int32_t *body1, const double *J0, const double *J1,
                         const double *Minv, double cfm, double *A, hipStream_t s);

// the four state arrays are read from *_in and written to *_out (the same arrays, or four others: a body's lane reads
// all of its inputs before it writes)
struct BodyState {
  double *pos, *R, *v, *w;
};
void launch_advance(int n, const BodyState &in, const BodyState &out, const double *v6, double dt, hipStream_t s);
// in place, body b by dt_each[body_ens[b]]; a body whose ensemble sits the step out (dt 0) is neither read nor written
void launch_advance_each(int n, const BodyState &state, const double *v6, const int32_t *body_ens, const double *dt_each,
                         hipStream_t s);

constexpr int kResidualBlocks = 64;

}  // namespace egs
