/*
 * eggshell_amd.h -- C ABI of the MI355X (gfx950) constraint-solve library,
 * libeggshell_amd.so.  Plain pointers and sizes only; all arrays are host
 * memory, row-major, IEEE fp64 unless stated; the library owns device memory.
 *
 * It is a drop-in for ONE path of teenylasers/eggshell: the per-step
 * constraint solve.  Each entry point names the reference interface it
 * replaces (file:line relative to the reference tree).
 *
 * Conventions (as in the reference):
 *   - a body has 6 velocity coordinates [v_lin; omega] (ensembles.cc:429-436);
 *   - every constraint has exactly 3 rows (joints.cc:18-19, contact.cc:103);
 *   - body index -1 is the world (constraints.h:42-43);
 *   - rows are ordered as the ConstraintsList is (ensembles.cc:234-239);
 *   - is_eq[r] != 0 marks an equality row ("C" in the reference); inequality
 *     rows are clamped to [lo, hi], +-inf allowed
 *     (sparse_iterations_utils.cc:12-21).
 *
 * Error convention: every function returns an egs_status; nothing ever exits
 * the process (the reference Panics: toolkit/error.cc:92-100).  The message
 * for the last failure is egs_last_error().  Non-convergence of the iterative
 * solver is NOT an error, exactly as in the reference
 * (sparse_iterations.cc:208-225 returns the last iterate silently).
 */
#ifndef EGGSHELL_AMD_H
#define EGGSHELL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct egs_context egs_context; /* one per (process, GPU): device + stream */
typedef struct egs_problem egs_problem; /* one ensemble (or batch) resident on the GPU */

typedef enum {
  EGS_OK = 0,
  EGS_ERR_INVALID = 1,     /* bad argument (the reference would CHECK/Panic) */
  EGS_ERR_NO_DEVICE = 2,   /* no gfx950 device / HIP runtime unusable */
  EGS_ERR_HIP = 3,         /* a HIP call failed */
  EGS_ERR_STALL = 4,       /* device-side ordering wait timed out (bug guard).  The device flag is
                              sticky: a stall in an asynchronous call (step / solve without stats)
                              is returned by the next call on the problem that enqueues work once
                              the flag has landed, and at the latest by the next call that
                              synchronises (get_lambda / get_velocity / get_state / get_stats ...);
                              reporting clears it.  egs_world_step checks before it integrates. */
  EGS_ERR_UNSUPPORTED = 5, /* feature not built yet */
  EGS_ERR_LCP_FAILED = 6,  /* dense LCP did not reach a solution (lcp.cc:250) */
  EGS_ERR_INTERNAL = 7     /* a library invariant failed / host allocation failed */
} egs_status;

/* sparse_iterations.cc:21-26 */
typedef enum { EGS_JACOBI = 0, EGS_GAUSS_SEIDEL = 1, EGS_SOR = 2 } egs_method;
typedef enum { EGS_F64 = 0, EGS_F32 = 1 } egs_precision;
/* constraint descriptor kinds for device-side assembly */
typedef enum { EGS_JOINT_BALL = 0, EGS_CONTACT_BOX = 1, EGS_JOINT_LOCK = 2, EGS_JOINT_HINGE_AXIS = 3 } egs_constraint_kind;
/* ... and the slider block, a constraint kind like those four (the kind arrays are int32_t, not the enum type).  It is
 * 5: kind 4 is no kind and never will be, it stays EGS_ERR_INVALID for ever.  The value stands beside the enum, whose
 * four members are pinned as they are. */
enum { EGS_JOINT_SLIDER_AXIS = 5 };

/* Runtime form of the reference's compile-time constants:
 *   omega = 1.5 and max_iters = 500 (sparse_iterations.cc:15-19),
 *   tol = kAllowNumericalError = 1e-9 (constants.h:5),
 *   cfm = the `cfm` argument of sparse::*Iteration (sparse_iterations.h:26-34).
 * tol <= 0 runs exactly max_iters sweeps (the benchmark mode).
 * check_every = k evaluates the residual every k sweeps; k = 1 reproduces the
 * reference's stopping rule exactly. */
typedef struct {
  int32_t method;      /* egs_method */
  int32_t max_iters;
  int32_t check_every;
  int32_t reserved;
  double omega;
  double cfm;
  double tol;
} egs_solve_params;

typedef struct {
  int32_t iterations;  /* sweeps performed */
  int32_t status;      /* egs_status of the device run */
  double residual;     /* sparse_iterations.cc:51-69 metric of the returned x */
  int32_t n_islands;   /* connected components of the constraint graph */
  int32_t n_tiles;     /* workgroup-resident tiles */
  int32_t n_global;    /* constraints solved by the cross-workgroup path */
  int32_t reserved;    /* 1 = latency schedule (4 lanes per constraint) in use */
  int32_t schedule;    /* which kernels ran the last GS / SOR solve, egs_schedule_flags */
  int32_t tile_constraints; /* constraints per workgroup tile of that schedule */
} egs_solve_stats;

typedef enum {
  EGS_SCHED_QUAD = 1,          /* quad_solve_kernel: 4 lanes per constraint */
  EGS_SCHED_ISO = 2,           /* tile_solve_kernel, isotropic-body variant (no stored M^-1 J^T) */
  EGS_SCHED_QUAD_PATCHES = 4,  /* oversize islands: body patches on the 4-lane kernel */
  EGS_SCHED_LANE_PATCHES = 8,  /* oversize islands: body patches on the 1-lane kernel */
  EGS_SCHED_ALL_GLOBAL = 16,   /* oversize islands: the all-global kernel */
  EGS_SCHED_STATIC = 32,       /* step_solve_kernel / step_quad_kernel (with EGS_SCHED_QUAD): the plan's sweep on
                                  its static timetable (one workgroup barrier per time step) instead of tickets */
  EGS_SCHED_LEAN = 64,         /* reserved, never reported: a retired 128-VGPR form of the timetable sweep */
  EGS_SCHED_LINSYM = 128,      /* step_solve_kernel's LINSYM form: the fp64 isotropic timetable sweep with one linear
                                  block for both sides (J1_lin = -J0_lin and equal linear weights, bit for bit) */
  EGS_SCHED_FUSED_ASSEMBLY = 256,  /* egs_problem_step assembled the Jacobian in the LINSYM launch's prologue
                                      (no separate assembly kernel; the same blocks, bit for bit) */
  EGS_SCHED_DEFERRED_SYSTEM = 512, /* ... and that launch stored no system: J0, J1, rhs, lo, hi, err and is_eq are
                                      made on demand, by the first call that reads them (the same bits): one
                                      assembly launch, what the step saved.  Readers: get_blocks, matvec, a solve or
                                      a step that does not fuse, the dense entries, and the residual -- so a step
                                      asked for statistics, or get_stats after one, pays for it too */
  EGS_SCHED_START = 1024,          /* the solve started from a given x0 (egs_problem_set_start), not from rhs */
  EGS_SCHED_FRICTION = 2048,       /* the launch ran the kernels' friction forms (egs_problem_set_friction,
                                      egs_world_set_friction): tangential bounds +-mu x_n.  Clear with friction off */
  EGS_SCHED_PAIR = 4096,           /* the EGS_SCHED_FUSED_ASSEMBLY launch ran each update on a lane pair: two threads
                                      hold one side each of two constraints (plans whose half-wavefronts each hold one
                                      phase of the timetable, a pile of columns).  The same bits as one lane per
                                      constraint; EGS_STEP_PAIR=0 switches it off */
  EGS_SCHED_CHAIN = 8192,          /* ... whose steady loop (EGS_STEP_STEADY) keeps the pair's two bodies'
                                      accumulators in registers from the first of the pair's two updates to the second
                                      (plans whose pairs hold consecutive contacts of the same two bodies:
                                      egs_debug_plan_chained).  The same bits; EGS_STEP_CHAIN=0 switches it off.
                                      A refinement of EGS_SCHED_PAIR: egs_problem_get_schedule reports it,
                                      egs_solve_stats.schedule does not (its bits stay those of the pair launch) */
  EGS_SCHED_SHARE = 16384,         /* ... in which a thread keeps ONE linear Jacobian block and one pair of weights for
                                      its side of both constraints: the two contacts of every thread pair carry the
                                      same normal, bit for bit (egs_debug_plan_share), decided once per
                                      egs_problem_set_constraints.  The same bits; EGS_STEP_SHARE=0 switches it off.
                                      A refinement of EGS_SCHED_CHAIN: only egs_problem_get_schedule_full reports it
                                      (callers compare egs_problem_get_schedule with EGS_SCHED_CHAIN masked against
                                      egs_solve_stats.schedule).  A world, whose collider writes the contacts on the
                                      device, does not take the form */
  EGS_SCHED_FACE = 32768,          /* ... in which a thread pair holds the FOUR contact points of a box face and runs
                                      their four updates behind one barrier, the two bodies' accumulators in registers
                                      from the first to the last (plans that are faced: egs_debug_plan_faced; one
                                      normal per face: egs_debug_plan_face_normals; GS, the store-free launch, no
                                      restitution).  128 threads per 256-constraint tile.  The same bits;
                                      EGS_STEP_FACE=0 switches it off, EGS_STEP_FACE_TILES=3|4 sets the tiles per CU.
                                      In egs_problem_step the launch also writes the velocities where every body is
                                      in some tile, and no velocity kernel runs (EGS_STEP_FACE_VELOCITY=0: it does).
                                      With more tiles than resident slots, that many persistent workgroups take the
                                      tiles (EGS_STEP_FACE_PERSIST=0: a workgroup per tile; EGS_STEP_FACE_SLOTS=k
                                      stands for the slot count, for tests).
                                      A refinement of EGS_SCHED_SHARE: only egs_problem_get_schedule_forms reports it */
  EGS_SCHED_FACE_SPLIT = 65536,    /* ... whose launch is split in time: where the tiles fill the resident slots once
                                      or more and leave a remainder of at most half of them, that many tiles run as
                                      two workgroups, sweeps 1 .. s1 and s1 + 1 .. S, so that the last round keeps
                                      every slot busy (egs_debug_face_split).  The same bits; EGS_STEP_FACE_SPLIT=0
                                      switches it off, EGS_STEP_FACE_SPLIT_FORCE=h,s1 splits the last h tiles after
                                      s1 sweeps whatever the policy says.  Only egs_problem_get_schedule_forms
                                      reports it */
  EGS_SCHED_FACE_LEAN = 131072     /* ... on the LEAN kernels: fewer held products, 168 VGPRs, six tiles per CU instead
                                      of four, where that is predicted to shorten the launch (egs_debug_face_form).
                                      The same bits; EGS_STEP_FACE_LEAN=0 keeps the four-tile kernels everywhere, =1
                                      takes the lean ones wherever the form holds, EGS_STEP_FACE_TILES also accepts 6.
                                      Only egs_problem_get_schedule_forms reports it */
} egs_schedule_flags;

void egs_default_params(egs_solve_params *p); /* GS, 500, 1, omega 1.5, cfm 0, tol 1e-9 */

/* ---- context ------------------------------------------------------------ */
egs_status egs_context_create(int device_index, egs_context **out);
void egs_context_destroy(egs_context *ctx);
const char *egs_last_error(const egs_context *ctx);
egs_status egs_context_synchronize(egs_context *ctx);
/* The device's compute units, as the schedule policies count them (resident slots = CUs x tiles per CU). */
egs_status egs_context_cu_count(const egs_context *ctx, int32_t *cus);
/* hipEvent pair on the context's stream (the stream every kernel below is
 * launched on).  stop() synchronises and returns elapsed milliseconds. */
egs_status egs_timer_start(egs_context *ctx);
egs_status egs_timer_stop(egs_context *ctx, float *elapsed_ms);
/* Sum and count of the solve-kernel launch durations (hipEvents around each
 * launch) since the last reset; synchronises. */
egs_status egs_kernel_time(egs_context *ctx, double *sum_ms, int64_t *launches,
                           int reset);

/* ---- entry 1: replaces sparse::{Jacobi,GaussSeidel,SOR}Iteration
 *      (const ConstraintsList&, const MatrixXd& M_inverse, const VectorXd& rhs,
 *       double cfm)   sparse_iterations.h:26-34 / sparse_iterations.cc:148-286.
 * The C++ adapter flattens the ConstraintsList with m ComputeJ calls:
 *   Minv  [n][36]  the 6x6 diagonal blocks M_inverse.block<6,6>(6b,6b)
 *   body0/1 [m]    Constraint::i0_, i1_ (constraints.h:42-43)
 *   J0,J1 [m][18]  the 3x6 blocks ComputeJ returns (constraints.h:22-24)
 *   is_eq, lo, hi [3m], rhs [3m];  out x [3m].
 * x0 = rhs, stop at residual <= tol or max_iters sweeps.                     */
egs_status egs_solve_blocks(egs_context *ctx, int32_t n_bodies,
                            const double *Minv, int32_t m,
                            const int32_t *body0, const int32_t *body1,
                            const double *J0, const double *J1,
                            const uint8_t *is_eq, const double *lo,
                            const double *hi, const double *rhs,
                            const egs_solve_params *params, int32_t precision,
                            double *x, egs_solve_stats *stats);

/* ---- device-resident form of the same path (what bench.py times) -------- */
/* Analyses the constraint graph (islands -> workgroup tiles) and allocates
 * device storage.  The topology (body0/body1) is fixed for the problem's life;
 * values can be re-uploaded any number of times. */
egs_status egs_problem_create(egs_context *ctx, int32_t n_bodies, int32_t m,
                              const int32_t *body0, const int32_t *body1,
                              int32_t precision, egs_problem **out);
/* Batched form (BASELINE config 4: 1024 independent 64-body
 * ensembles): E ensembles in ONE problem.  body0/body1 hold the E constraint
 * lists back to back with ensemble-LOCAL body indices (-1 = world); the
 * returned offset tables ([E+1] each, may be NULL) say where ensemble e's
 * bodies and constraints live in the concatenated arrays every other
 * egs_problem_* call takes.  Ensembles never share a body, so each is its own
 * set of islands and results equal E separate solves bit for bit; one launch
 * sweeps them all. */
egs_status egs_problem_create_batch(egs_context *ctx, int32_t n_ensembles,
                                    const int32_t *n_bodies, const int32_t *n_constraints,
                                    const int32_t *body0, const int32_t *body1,
                                    int32_t precision, egs_problem **out,
                                    int32_t *body_offset, int32_t *constraint_offset);
void egs_problem_destroy(egs_problem *p);
/* upload the flat system of entry 1 (any pointer may be NULL = keep) */
egs_status egs_problem_set_blocks(egs_problem *p, const double *Minv,
                                  const double *J0, const double *J1,
                                  const uint8_t *is_eq, const double *lo,
                                  const double *hi, const double *rhs);
/* asynchronous on the context stream */
egs_status egs_problem_solve(egs_problem *p, const egs_solve_params *params,
                             egs_solve_stats *stats);
egs_status egs_problem_get_lambda(egs_problem *p, double *x /*[3m]*/);
/* a_b = Minv_b sum_i J_ib^T lambda_i, [n][6]: the solver's by-product,
 * so that v_dot = Minv f_ext + a (ensembles.cc:535) needs no extra pass. */
egs_status egs_problem_get_accumulators(egs_problem *p, double *a /*[n][6]*/);

/* w = A lambda - rhs of the last solve, [3m]: what GetResidualError
 * (sparse_iterations.cc:51-69) reduces; written by the solve kernels' epilogue. */
egs_status egs_problem_get_wres(egs_problem *p, double *w /*[3m]*/);

/* ---- where a solve starts.  The reference starts every solve from x0 = rhs (quirk Q7, sparse_iterations.cc:202);
 *      that is the default and nothing changes it unless this is called.  The mode is sticky until changed:
 *        EGS_START_RHS       x0 = rhs.
 *        EGS_START_GIVEN     x0 = the 3m rows passed with this call, uploaded once (converted to the problem's
 *                            precision) and used by every following solve.
 *        EGS_START_PREVIOUS  x0 = lambda of the last solve on this problem, copied on the device before each solve's
 *                            first launch; a problem that holds no lambda yet starts that solve from rhs.
 *      From x0 on the solve is the reference's: accumulators from x0 in list order, the sweeps, the stopping test
 *      (x0 itself is tested first: iterations = 0 if it passes), w = A x - rhs with the true rhs.  A solve that
 *      started from a given x0 reports EGS_SCHED_START.  egs_problem_step with a start in force assembles with the
 *      assembly kernel (EGS_SCHED_FUSED_ASSEMBLY stays clear).  The dense steps take no start.
 *      EGS_ERR_INVALID: an unknown mode, GIVEN with x0 = NULL, a NaN row.                                          */
#define EGS_START_RHS      0
#define EGS_START_GIVEN    1
#define EGS_START_PREVIOUS 2
egs_status egs_problem_set_start(egs_problem *p, int32_t mode, const double *x0 /*[3m], GIVEN only*/);

/* ---- Coulomb friction pyramid.  The reference bounds a contact's two tangential rows by the constant 1 (the friction
 *      box, contact.cc:103-113) and declares COULOMB_PYRAMID with empty bodies (contact.h:21-25); this is that model,
 *      off unless asked for.  mu holds one coefficient per constraint (the whole list of a batch problem), converted
 *      to the problem's precision.  mu[c] < 0: constraint c is solved as stored.  mu[c] >= 0: rows 0 and 1 of c are
 *      inequality rows with the bounds [-b, +b], whatever type and bounds are stored for them,
 *          b = x_n > 0 ? fl(mu[c] x_n) : 0,    x_n = the multiplier of row 2 (the normal row) held when the row is
 *      projected: the old iterate's (Jacobi), the previous sweep's (Gauss-Seidel, rows run 0, 1, 2; in the first sweep
 *      the start's, which may be negative), this sweep's (backward SOR, rows run 2, 1, 0).  Row 2 keeps its stored
 *      type and bounds.  w = A x - rhs is unchanged.  The residual, stopping rule and reported value alike, sorts such
 *      a row by the b of the iterate's own x_n: |x| < b adds w^2 to the strictly-inside sum; x = b > 0 with w > 0 to
 *      the at-hi sum; x = -b < 0 with w < 0 to the at-lo sum; |x| > b adds (|x| - b)^2 to the strictly-inside sum (a
 *      forward sweep clamps against the previous x_n); b = 0 = x adds nothing.
 *      mu = NULL, or no coefficient >= 0, turns friction off: every result and schedule flag is then what it is
 *      without this call.  On, the launches report EGS_SCHED_FRICTION, egs_problem_step does not fuse the assembly
 *      (EGS_SCHED_FUSED_ASSEMBLY stays clear) and egs_problem_step_dense returns EGS_ERR_UNSUPPORTED unless
 *      egs_problem_set_dense_friction has allowed it.  Starts, mat-vec and get_wres work alongside as they are.
 *      EGS_ERR_INVALID: a NaN coefficient (nothing changes).                                                       */
egs_status egs_problem_set_friction(egs_problem *p, const double *mu /*[m] or NULL*/);
/* The friction pyramid on the dense direct solver, opt-in.  max_outer > 0: while friction is on, egs_problem_step_dense
 * solves the pyramid by the fixed-point iteration of egs_mixed_friction_solve_batch (at most max_outer solves, stopping
 * change tol; the reference values are 32 and 1e-10) instead of refusing: rows 0 and 1 of a constraint with mu >= 0 are
 * pyramid rows whose normal row is its row 2.  The step runs the iteration from the host around the dense mixed solver
 * (every solve on the problem without its pinned rows, its Murty set from scratch), whatever the size.  use_bounds
 * must then be 1 (EGS_ERR_INVALID otherwise, also when a pyramid constraint's row 2 is an equality row).  Not converging
 * within max_outer is no failure: the step integrates the last iterate; egs_problem_dense_friction_info tells.
 * max_outer = 0 (the default) switches it off again: the step refuses as before.  The condition estimate, cfm,
 * EGS_ERR_LCP_FAILED and integration are unchanged.  EGS_ERR_INVALID: max_outer < 0, tol < 0 or NaN.                */
egs_status egs_problem_set_dense_friction(egs_problem *p, int32_t max_outer, double tol);
/* The last egs_problem_step_dense that solved the pyramid (any pointer may be NULL): solves made, converged
 * (change <= tol), the last change.  EGS_ERR_INVALID before the first such step.                                   */
egs_status egs_problem_dense_friction_info(egs_problem *p, int32_t *outer, int32_t *converged, double *change);

/* ---- Restitution: contacts that bounce.  The reference has none: a contact's normal row asks only for
 *      J v' >= erp depth / dt (ensembles.cc:569-570), so a dropped body stops dead.  This is Newton's law of restitution
 *      with that Baumgarte term as the floor, off unless asked for.  rest holds one coefficient per constraint, fp64
 *      whatever the problem's precision; vth >= 0 is one threshold speed.  Constraint c bounces only if its kind is
 *      EGS_CONTACT_BOX, a table is set and rest[c] >= 0; joints never bounce, rest[c] < 0 is assembled as stored.  For
 *      a bouncing contact the assembly forms row 2 of rhs in this order, in fp64 without contraction, and casts it:
 *          s0 = (v, w) of body0, s1 = (v, w) of body1                  (six zeros for a world side)
 *          vn = dot6p(J0 row 2, s0) + dot6p(J1 row 2, s1)              (the separating speed; approaching: vn < 0)
 *          t  = kk err[2]                                              (kk = -erp/dt/dt; the ensemble's pair in _each)
 *          if (vn < -vth) { b = (-(rest[c] vn)) / dt;  if (b > t) t = b; }
 *          rhs[2] = t - ju                                             (ju = J (v/dt + M^-1 f) as always)
 *      so that the normal row's complementarity becomes J v' >= max(erp depth / dt, -rest vn).  Rows 0 and 1, err, lo,
 *      hi, is_eq, J0 and J1 are untouched; a contact that does not trigger (vn >= -vth, or b <= t) gets the bits it
 *      gets without this call; an ensemble sitting a step out (dt[e] = 0) keeps rhs = 0 exactly.  Coefficients above 1
 *      are allowed.  It takes effect wherever the rhs is made -- egs_problem_assemble, egs_problem_step (the fused
 *      launch keeps the assembly in its prologue: EGS_SCHED_FUSED_ASSEMBLY, PAIR and CHAIN stay set, and a deferred
 *      system materialised later carries the table its step ran with), egs_problem_step_dense -- and composes with
 *      friction, dense friction, starts and live inertia, which read the restituted rhs where they read rhs.
 *      rest = NULL, or no coefficient >= 0, turns it off: every result and schedule flag is then what it is without
 *      this call.  A new topology turns it off (the coefficients belong to the list they were given for).
 *      EGS_ERR_INVALID: a NaN or infinite coefficient, vth < 0, NaN or infinite (nothing changes).                   */
egs_status egs_problem_set_restitution(egs_problem *p, const double *rest /*[m] or NULL = off*/, double vth);

/* ---- Angular joint blocks and the hinge motor.  The reference's joints.h has the ball joint alone.  Two angular 3x6
 *      blocks stand beside it, so that weld = BALL + LOCK and hinge = BALL + HINGE_AXIS on the same two bodies.  Both are
 *      joints in every sense: listed first in a world, never bouncing, friction coefficient -1, their own previous rows
 *      in a warm start.  Their linear Jacobian columns are exactly zero; err is (body0 quantity) - (body1 quantity) and
 *      d err/dt = J0 s0 + J1 s1 at err = 0, as for the ball joint.  body0 must be a body; body1 = -1 is the world.
 *      Assembled in fp64 without contraction in this order (mv3, mm3, d3, quat_to_R, align_to_z: assemble_device.h):
 *      EGS_JOINT_LOCK, data = (qw, qx, qy, qz, 0, 0, 0), the unit quaternion of Rref = R0(0)^T R1(0) (R0(0)^T, the
 *      target orientation transposed, for a world side):
 *          Rq = quat_to_R(q);  T = mm3(R0, Rq);  E = mm3(T, R1^T), R1^T formed by index     (a world side: E = T)
 *          err = (0.5*(E[7]-E[5]), 0.5*(E[2]-E[6]), 0.5*(E[3]-E[1]))       row-major: the axial vector, sin(theta) n
 *          J0 = [0 | I3], J1 = [0 | -1.0*I3] (zero for a world side); three equality rows, lo = hi = 0
 *      EGS_JOINT_HINGE_AXIS, data = (a0[3], a1[3], 0): the unit axis in body0's frame and in body1's (the world axis for
 *      a world side):
 *          s = mv3(R0, a0);  t = mv3(R1, a1) (a world side: a1);  Rn = align_to_z(s), rows (p, q, s^)
 *          c = t x s = (t1 s2 - t2 s1, t2 s0 - t0 s2, t0 s1 - t1 s0);  err = (d3(p, c), d3(q, c), 0)
 *          J0 = [0 | Rn], J1 = [0 | -1.0*Rn] (zero for a world side)
 *      Rows 0 and 1 are equality rows.  Row 2, the axis row, is an inequality row with lo = hi = 0: its multiplier is
 *      pinned at 0 and the hinge turns freely.  Both linearise sin(theta): they hold for errors below a right angle, and
 *      t = -s (the axes antiparallel) is a false equilibrium with err = 0.
 *      egs_problem_set_motors: motor [m][2] = (speed, tau) per constraint.  For a HINGE_AXIS constraint with tau >= 0
 *      (+inf allowed) the assembly sets lo[2] = -tau, hi[2] = +tau and rhs[2] = speed / dt - ju (the ensemble's dt in
 *      the _each forms; an ensemble sitting a step out keeps rhs = 0), so the solve asks for s^ . (w0' - w1') = speed
 *      within the torque limit.  tau < 0, and every other kind, is assembled as stored.  motor = NULL, or no hinge with
 *      tau >= 0, turns it off: every result and schedule flag is then what it is without this call.  A new topology or
 *      a new egs_problem_set_constraints turns it off.  EGS_ERR_INVALID: a NaN or infinite speed, a NaN tau (nothing
 *      changes).
 *      A list that holds one of these kinds never runs EGS_SCHED_LINSYM, FUSED_ASSEMBLY, PAIR or CHAIN; lists without
 *      them keep their schedules and their bits.  The dense steps (egs_problem_step_dense, egs_world_step_dense[_each])
 *      take LOCK rows as equality rows and a motored axis row with tau > 0 as a box row (use_bounds bit 0); an axis row
 *      pinned at lo = hi = 0 (no motor, or tau = 0) does not meet Murty's preconditions (lcp.cc:161-164), so they return
 *      EGS_ERR_UNSUPPORTED for it, and for any hinge when use_bounds bit 0 is clear.                                   */
egs_status egs_problem_set_motors(egs_problem *p, const double *motor /*[m][2] or NULL = off*/);

/* ---- Hinge angle limits: a per-constraint table on the EGS_JOINT_HINGE_AXIS block (no constraint kind of its own).
 *      lim [m][8] = (qw, qx, qy, qz, sin lo, cos lo, sin hi, cos hi), fp64 whatever the problem's precision.  q is the
 *      unit quaternion of Rref = R0(0)^T R1(0) (R0(0)^T for a world side), the EGS_JOINT_LOCK convention: it fixes
 *      theta = 0, and theta is body0's turn relative to body1 about s = R0 a0.  A (sin, cos) pair of (0, 0) means "no
 *      stop on that side"; a row with both pairs (0, 0), and any row of a constraint that is not HINGE_AXIS, is ignored.
 *      The table holds sines and cosines, so the device code uses no trigonometric function.  For a HINGE_AXIS
 *      constraint with a stop the assembly forms the block as above (s, t, Rn, c, err[0..1], J0, J1 keep their bits),
 *      then, in fp64 without contraction:
 *          Rq = quat_to_R(q);  T = mm3(R0, Rq);  E = mm3(T, R1^T), R1^T formed by index     (a world side: E = T)
 *          ax = (0.5*(E[7]-E[5]), 0.5*(E[2]-E[6]), 0.5*(E[3]-E[1]))
 *          sn = d3(s, ax)                                  sin(theta)
 *          cs = 0.5*(((E[0]+E[4])+E[8]) - 1.0)             cos(theta)
 *          upper set and sn*(1.0+chi) > shi*(1.0+cs):       err[2] = sn*chi - cs*shi;  lo[2] = -inf;  hi[2] = 0
 *          else lower set and sn*(1.0+clo) < slo*(1.0+cs):  err[2] = sn*clo - cs*slo;  lo[2] = 0;  hi[2] = +inf
 *          else: row 2 as without the table (err 0, lo = hi = 0)
 *      The comparison is tan(theta/2) against tan(limit/2), cross-multiplied: monotone in theta on (-pi, pi), no
 *      division.  err[2] = sin(theta - limit) in both cases, and rhs[2] is the ordinary kk err[2] - ju, so the solve asks
 *      for s^ . (w0' - w1') <= -erp sin(theta - hi) / dt with lambda <= 0 at the upper stop, the mirror image at the
 *      lower.  is_eq[2] stays 0.  Like the other angular errors this one linearises a sine, and the read-out wraps at
 *      +-pi: a hinge that overshoots a stop by more than pi - |limit| is seen on the other side.
 *      Motor and limit share the axis row: while a stop is active the row is the limit's and the motor leaves it alone for
 *      that step (the motor applies only when lo[2] == hi[2] after the block); inside the range the motor works as above.
 *      lim = NULL, or no hinge with a stop, turns limits off: every result and schedule flag is then what it is without
 *      this call.  A new topology or a new egs_problem_set_constraints turns them off.  The stabilise passes of a world
 *      take an active stop as one more row of (J J^T) y = err.  The dense steps return EGS_ERR_UNSUPPORTED while a hinge
 *      has a stop (whether its row is pinned is decided on the device).  EGS_ERR_INVALID (nothing changes): a non-finite
 *      entry; for a hinge with a stop a q that is not a unit quaternion within 1e-12, a pair that is neither (0, 0) nor on
 *      the unit circle within 1e-12, a stop at +-pi (1 + cos <= 0), lo above hi in the half-angle order.              */
egs_status egs_problem_set_hinge_limits(egs_problem *p, const double *lim /*[m][8] or NULL = off*/);

/* ---- Slider joints: EGS_JOINT_SLIDER_AXIS = 5 (4 stays invalid for ever).  A slider is LOCK + SLIDER_AXIS on the same
 *      two bodies, as a hinge is BALL + HINGE_AXIS; with the lock holding the relative orientation it is a general
 *      prismatic joint.  data = (a0[3], c[3], 0): a0 the unit rail direction in body0's frame; body0 must be a body.
 *      With body1 a body, c is a point of the rail in body0's frame and the rail's target point is body1's centre,
 *      P1 = pos[b1].  With body1 = -1 (the world), c is the world point the rail passes through, P1 = c, and the rail
 *      passes through body0's centre.  Assembled in fp64 without contraction and without a trigonometric function, in
 *      this order (mv3, align_to_z, crossmat, mm3, d3: assemble_device.h):
 *          s = mv3(R0, a0);  Rn = align_to_z(s), rows (p, q, s^)
 *          two bodies:  ro = mv3(R0, c);  D[k] = (p0[k] + ro[k]) - P1[k]
 *          world side:                    D[k] =  p0[k] - c[k]
 *          rel[k] = p0[k] - P1[k];  rw = mm3(Rn, crossmat(rel))             row r is (P1 - p0) x Rn_r
 *          J0 = [Rn | rw],  J1 = [-1.0*Rn | 0] (all zero for a world side)
 *          err = (d3(p, D), d3(q, D), 0)
 *      Rows 0 and 1 are equality rows.  Row 2, the rail row, is an inequality row with lo = hi = 0: its multiplier is
 *      pinned at 0 and the slider runs freely, as a free hinge's axis row.  d err/dt = J0 s0 + J1 s1 at err = 0 for rows 0
 *      and 1; for the travel x = d3(s^, D) it holds at every pose (s is rigid in body0 and body1 enters through its
 *      centre only).  The lever arm sits on body0 alone: J0^T lambda and J1^T lambda carry no net force and no net torque.
 *      Motor: egs_problem_set_motors applies to the rail row as to a hinge's axis row: (speed, f) with f >= 0 gives
 *      lo[2] = -f, hi[2] = +f, rhs[2] = speed / dt - ju, speed = dx/dt, body0's travel relative to body1 along s^.
 *      Travel stops: lim [m][2] = (xlo, xhi), fp64, -inf / +inf: no stop on that side; rows of other kinds are ignored.
 *      After the block is formed, its bits kept:
 *          xhi finite and x > xhi:       err[2] = x - xhi;  lo[2] = -inf;  hi[2] = 0
 *          else xlo finite and x < xlo:  err[2] = x - xlo;  lo[2] = 0;     hi[2] = +inf
 *          else: row 2 as without the table
 *      rhs[2] stays the ordinary kk err[2] - ju and is_eq[2] stays 0: the sign convention of the hinge stops, lambda <= 0
 *      at the upper stop.  While a stop is active the motor leaves the row alone for that step.  lim = NULL, or no slider
 *      with a finite stop, turns the stops off: every result and schedule flag is then what it is without this call.  A
 *      new topology or a new egs_problem_set_constraints turns them off.  EGS_ERR_INVALID (nothing changes): a NaN
 *      anywhere in the table; on a slider row xlo = +inf, xhi = -inf or xlo > xhi.  egs_problem_set_constraints refuses
 *      a slider with body0 < 0, a non-finite number among its seven, or an a0 that is no unit vector within 1e-12.
 *      A list that holds a slider runs none of EGS_SCHED_LINSYM, FUSED_ASSEMBLY, PAIR, CHAIN, SHARE, FACE (its J1 is not
 *      -J0); friction (coefficient -1), restitution and warm start treat it as any joint.  The stabilise passes of a
 *      world take an active stop as one more row of (J J^T) y = err and an inactive rail row as a free hinge's axis row.
 *      The dense steps take a motored rail row with f > 0 as a box row (use_bounds bit 0) and return
 *      EGS_ERR_UNSUPPORTED, naming the constraint, for a free slider (pinned row) and for any slider with a finite stop. */
egs_status egs_problem_set_slider_limits(egs_problem *p, const double *lim /*[m][2] or NULL = off*/);

/* ---- the matrix-free products: replace sparse::CalculateSparse{JMJtX,Lx,Ux,
 *      LxUx,Dx,UxDx,LxDx}(const ConstraintsList&, const MatrixXd& M_inverse,
 *      const VectorXd& x, double epsilon_diagonal, double scale_diagonal)
 *      sparse_iterations_utils.h / sparse_iterations_utils.cc:427-695.
 * With A = J M^-1 J^T (3m x 3m, never formed):
 *   EGS_MV_FULL   y = (A + eps I) x                          (:624-695; scale unused)
 *   EGS_MV_LOWER  y = strictLower(A) x  -- the strict lower triangle of a
 *                 constraint's own 3x3 block belongs to it   (:427-493, :484-486)
 *   EGS_MV_UPPER  y = strictUpper(A) x                       (:495-561, :522-524)
 *   EGS_MV_DIAG   y_r = ((A_rr + eps) * scale) x_r           (:571-603, :594)
 * and the sums the reference offers, added in its order: LOWER|UPPER (:563-569),
 * UPPER|DIAG (:606-613), LOWER|DIAG (:615-622).  The reference walks all O(m^2)
 * constraint pairs; here the cost is O(m).
 * Uses the blocks the problem holds (set_blocks or assemble).  x = NULL takes
 * the device-resident lambda of the last solve; y = NULL leaves the result on
 * the device (egs_problem_get_matvec) and makes the call asynchronous.        */
typedef enum { EGS_MV_LOWER = 1, EGS_MV_UPPER = 2, EGS_MV_DIAG = 4, EGS_MV_FULL = 8 } egs_matvec_part;
egs_status egs_problem_matvec(egs_problem *p, int32_t parts, double eps, double scale,
                              const double *x /*[3m] or NULL*/, double *y /*[3m] or NULL*/);
egs_status egs_problem_get_matvec(egs_problem *p, double *y /*[3m]*/);
/* one-shot form over flat host arrays, as egs_solve_blocks (the adapter's
 * sparse::CalculateSparse* functions call this) */
egs_status egs_matvec_blocks(egs_context *ctx, int32_t n_bodies, const double *Minv, int32_t m,
                             const int32_t *body0, const int32_t *body1, const double *J0,
                             const double *J1, int32_t parts, double eps, double scale,
                             int32_t precision, const double *x, double *y);

/* ---- entry 2: replaces the assembly half of Ensemble::StepVelocities_ODE
 *      (ensembles.cc:563-575): ComputeJ (ensembles.cc:38-87 ->
 *      joints.cc:13-35, contact.cc:38-117), ComputePositionConstraintError
 *      (ensembles.cc:156-171 -> joints.cc:3-11, contact.cc:14-22), the rhs
 *      (ensembles.cc:569-570) and, after the solve, the velocity update
 *      (ensembles.cc:535, 572).  Body state and constraint descriptors:
 *   pos [n][3], R [n][9] row-major, v [n][3], w [n][3] (global frame),
 *   Minv [n][36], f_ext [n][6]  (ensembles.cc:202-222; frozen at Init, Q5 --
 *                unless egs_problem_set_live_inertia turns live inertia on)
 *   kind [m] (egs_constraint_kind),
 *   data [m][7]: joint   = c0(3), c1(3) (c1 = world point if body1 = -1), 0
 *                contact = position(3), normal(3), depth (collision.h:12-27) */
egs_status egs_problem_set_state(egs_problem *p, const double *pos,
                                 const double *R, const double *v,
                                 const double *w, const double *Minv,
                                 const double *f_ext);
/* The compact form of Minv: per body 1/m and the 3x3 inverse of the
 * global-frame inertia, row-major -- all ConstructMassInertiaMatrixInverse
 * (ensembles.cc:202-212) ever stores; the 6x6 blocks are built from it. */
egs_status egs_problem_set_mass(egs_problem *p, const double *inv_mass,
                                const double *inv_inertia);
/* ---- live inertia: world-frame M^-1 and the gyroscopic torque follow the bodies.  Off by default: the reference
 * computes both in Ensemble::Init and never again (quirk Q5), and so does this library unless told otherwise here.
 *   inertia_body [n][9]  body-frame inertia, row-major; NULL turns live inertia off
 *   torque       [n][3]  an applied torque, world frame; NULL = none
 * With live inertia on, every stepping entry (egs_problem_assemble, egs_problem_step, egs_problem_step_dense, and
 * through the world egs_world_step[_each] and egs_world_step_dense[_each]) first recomputes on the device, from the R
 * and w the device holds AT THE START OF THAT STEP, what Ensemble::Init would compute at that state, for every body b
 * whose inertia_body[b] is not exactly a I_3 (all off-diagonals exactly 0, the three diagonals equal):
 *   I_g = (R I_b) R^T;   the angular 3x3 block of Minv[b] = I_g^-1 by cofactors;
 *   f_ext[b][3:6] = torque[b] + ((-[w]x) I_g) w,
 * in the operation order of ensembles.cc:202-222 (the bits of the CPU oracle's minv_blocks / external_force), and
 * with them the device's derived copies (the working-precision M^-1, M^-1 f_ext).  One more launch per step; no
 * synchronisation, read-back or upload.  The linear rows (1/m, f_ext[b][0:3]) are never touched: they stay the
 * caller's.  A body whose inertia_body IS a I_3 is skipped -- its Minv and f_ext rows stay what the caller uploaded
 * (rotation cannot change its world inertia, its gyroscopic torque vanishes) -- so a world of cubes or spheres with live
 * inertia on is bit for bit the world with it off, on the same schedule.  The refresh depends on the state only: a step
 * that fails, or an ensemble sitting a step out, leaves the arrays consistent with its unchanged bodies.
 * While it is on, a later egs_problem_set_state / egs_world_set_bodies that passes Minv / f_ext keeps their linear
 * rows; the angular parts of the bodies that are not skipped are overwritten at the next step.
 * EGS_ERR_INVALID, with nothing changed: a non-finite entry, an inertia_body[b] that is not exactly symmetric or not
 * positive definite (Sylvester's three leading minors).  Turning it off leaves the arrays what the last step made
 * them. */
egs_status egs_problem_set_live_inertia(egs_problem *p, const double *inertia_body /*[n][9] or NULL = off*/,
                                        const double *torque /*[n][3] or NULL*/);
/* Minv [n][36], f_ext [n][6] as the device holds them (fp64); either may be NULL.  With live inertia on they are first
 * brought to the state the device holds now (the refresh is idempotent: a step would compute the same). */
egs_status egs_problem_get_mass(egs_problem *p, double *Minv /*[n][36]*/, double *f_ext /*[n][6]*/);
egs_status egs_problem_set_constraints(egs_problem *p, const int32_t *kind,
                                       const double *data);
/* J, err, bounds, rhs = -(erp/dt^2) err - J (v/dt + Minv f_ext) on device */
egs_status egs_problem_assemble(egs_problem *p, double dt, double erp);
/* assemble + solve + v_new = v + dt (Minv f_ext + a): one whole hot-path pass */
egs_status egs_problem_step(egs_problem *p, double dt, double erp,
                            const egs_solve_params *params,
                            egs_solve_stats *stats);
egs_status egs_problem_get_blocks(egs_problem *p, double *J0, double *J1,
                                  uint8_t *is_eq, double *lo, double *hi,
                                  double *rhs, double *err);
egs_status egs_problem_get_velocity(egs_problem *p, double *v6 /*[n][6]*/);
/* Ensemble::StepPositions_ODE (ensembles.cc:577-591) on the device, after
 * egs_problem_step: p += dt (v + v_new)/2, R = WtoQ((w + w_new)/2, dt) R
 * (utils.cc:82-89), then v, w <- v_new, so the body state never leaves the
 * GPU between steps while the contact set is unchanged. */
egs_status egs_problem_advance(egs_problem *p, double dt);
egs_status egs_problem_get_state(egs_problem *p, double *pos, double *R, double *v, double *w);
/* fills stats->residual/iterations of the last solve (synchronises) */
egs_status egs_problem_get_stats(egs_problem *p, egs_solve_stats *stats);
/* The egs_schedule_flags of the last GS / SOR solve: the bits of egs_solve_stats.schedule and, with them, the
 * refinements that field leaves out (EGS_SCHED_CHAIN).  Host only: no synchronisation, no residual. */
egs_status egs_problem_get_schedule(egs_problem *p, int32_t *schedule);
/* ... and, with those, the refinements of a refinement (EGS_SCHED_SHARE).  Host only as well. */
egs_status egs_problem_get_schedule_full(egs_problem *p, int32_t *schedule);
/* ... and, with those, the form of the EGS_SCHED_SHARE launch that ran (EGS_SCHED_FACE): the two entries above and
 * egs_solve_stats.schedule keep the bits they have without it.  Host only as well. */
egs_status egs_problem_get_schedule_forms(egs_problem *p, int32_t *schedule);

/* ---- entry 3: replaces Lcp::MixedConstraintsSolver(A, b, C, x_lo, x_hi, x, w)
 *      lcp.h:21-23 / lcp.cc:276-336 (and Lcp::MurtyPrincipalPivot,
 *      lcp.cc:157-274).  A [N][N], b, C, lo, hi [N] -> x, w [N]; *ok as the
 *      reference's bool.  use_bounds is a bit mask:
 *        0      the reference: bounds ignored (quirk Q3), single-index pivots,
 *               cap min(1000, 2^n) pivots (lcp.cc:168)
 *        bit 0  honour x_lo/x_hi (the true box problem)
 *        bit 1  block principal pivoting instead of the single-index rule: same
 *               solution, tens of factorisations instead of hundreds, no cap --
 *               the reference's rule cannot finish N >~ 1200 mixed problems.    */
egs_status egs_mixed_constraints_solve(egs_context *ctx, int32_t N,
                                       const double *A, const double *b,
                                       const uint8_t *C, const double *lo,
                                       const double *hi, int32_t use_bounds,
                                       double *x, double *w, int32_t *ok,
                                       int32_t *pivots);

/* The same with the give-up limits of lcp::Settings (toolkit/lcp.h:161-167): max_pivots > 0
 * / max_seconds > 0 stop the pivoting loop there and the call reports *ok = 0
 * (EGS_ERR_LCP_FAILED), as SolveLCP returns false.  0 = the library's own cap.   */
egs_status egs_mixed_constraints_solve_limits(egs_context *ctx, int32_t N, const double *A, const double *b,
                                              const uint8_t *C, const double *lo, const double *hi,
                                              int32_t use_bounds, int32_t max_pivots, double max_seconds,
                                              double *x, double *w, int32_t *ok, int32_t *pivots);

/* Lcp::MixedConstraintsSolver (lcp.cc:276-336) on `count` independent problems in one call: what the reference's own
 * test of the function does one problem after another (100 random 50 x 50 mixed problems, lcp.cc:412-528), a study of
 * the condition / cfm rule, or an integrator that assembles its own J M^-1 J^T.  Packing as egs_box_lcp_batch /
 * egs_dense_iterate_batch: problem k has n[k] >= 0 rows, its full row-major symmetric matrix at A + sum_{j<k} n[j]^2,
 * its vectors (b, C, lo, hi, x, w) at sum_{j<k} n[j]; A is read only and never permuted.  use_bounds is the mask of
 * egs_mixed_constraints_solve; max_pivots as in egs_mixed_constraints_solve_limits (0 = the reference's cap
 * min(1000, 2^n_i)); there is no max_seconds, a fused kernel has no honest wall clock.
 * Problems of n[k] <= 112 rows with bit 1 clear are fused: one packed page-locked block, one device allocation, one
 * upload, at most one launch per size class (32 / 64 / 112 rows; a workgroup per problem runs the partition, the
 * Cholesky of A_ee, the Schur complement, the reference's Murty loop and the back-substitution on chip), one read-back,
 * one synchronisation; no workgroup waits on another.  Every other problem runs inside the same call, one after
 * another, on the path of egs_mixed_constraints_solve.  A problem's path depends on its own n alone.
 * Per problem, the single entry's semantics: w is exactly 0 on the equality rows, x holds A_ee^-1 (b_e - A_ei x_i)
 * there; ok[k] = the reference's bool, pivots[k] (pivots may be NULL) = the Murty steps (0 without inequality rows);
 * n[k] = 0 gives ok 1, pivots 0.  ok[k] = 0: A_ee or some A(S,S) is not positive definite, the cap was reached without
 * a sensible solution, or (bit 0) the inequality bounds break lcp.cc:161-164; x and w of that problem are then not
 * meaningful and its neighbours are untouched.
 * Returns EGS_OK whenever every problem was run (outcomes in ok[]; not the single entry's EGS_ERR_LCP_FAILED);
 * count = 0 is EGS_OK.  EGS_ERR_INVALID, with nothing launched and no output written: count < 0, some n[k] < 0,
 * use_bounds outside 0..3, max_pivots < 0, a NULL among the required pointers when sum n > 0, or a matrix the single
 * entry refuses as asymmetric (egs_last_error names the first such problem). */
egs_status egs_mixed_constraints_solve_batch(egs_context *ctx, int32_t count, const int32_t *n, const double *A,
                                             const double *b, const uint8_t *C, const double *lo, const double *hi,
                                             int32_t use_bounds, int32_t max_pivots, double *x, double *w, int32_t *ok,
                                             int32_t *pivots);

/* The Coulomb friction pyramid on the dense direct solver, for `count` independent problems on explicit matrices
 * (packing, fusing and size classes of egs_mixed_constraints_solve_batch; plain rows always honour their bounds, the
 * meaning of use_bounds bit 0).  Beside (A, b, C, lo, hi) a problem has, per row r, normal_row[r] (int32, an index
 * within its own problem, or -1: a plain row) and mu[r] >= 0.  A row with normal_row[r] = f >= 0 is a PYRAMID row: an
 * inequality row whatever C[r] says, bounded by [-beta_r, +beta_r] with beta_r following x_f; f must be a plain
 * inequality row.  The solve is the fixed-point iteration on beta:
 *   beta^0 = 0.  Solve k is the box LCP with the pyramid rows at [-beta^k, +beta^k]; a pyramid row with beta^k_r = 0
 *   is PINNED: x_r = 0 exactly, its w_r carries no condition, it never enters the active set.
 *   beta^{k+1}_r = x_f > 0 ? fl(mu_r x_f) : 0;  delta_k = max_r |beta^{k+1}_r - beta^k_r| / max(1, max_r beta^{k+1}_r).
 *   Stop at the first k with delta_k <= tol, or after max_outer solves (0 = 32).
 * x, w: the last solve's (w = 0 exactly on equality rows, A x - b on a pinned row); beta (may be NULL): the bounds x was
 * solved under, 0 on plain rows; outer[k]: solves made; change[k]: the last delta, so the run converged iff
 * change[k] <= tol; pivots[k] (may be NULL): Murty steps summed over the solves.  ok[k] = 0: an inner solve failed as
 * egs_mixed_constraints_solve_batch's does.  NOT converging within max_outer is no failure: ok[k] = 1 and the last
 * iterate is returned.  A problem without a pyramid row returns the bits of egs_mixed_constraints_solve_batch with
 * use_bounds = 1, and outer = 1.
 * Problems of n[k] <= 112 rows run fused, a workgroup each, the partition and the Schur complement once and every
 * solve starting its Murty set from the previous solve's final set.  Larger ones run inside the call, one after
 * another: the same iteration from the host around egs_mixed_constraints_solve's path, on the problem without its
 * pinned rows, every solve starting its set from scratch.
 * EGS_ERR_INVALID, with nothing launched and no output written: whatever egs_mixed_constraints_solve_batch refuses;
 * a normal_row outside -1 .. n[k] - 1, or one pointing at an equality row or at another pyramid row; a NaN or negative
 * mu on a pyramid row; max_outer < 0; tol < 0 or NaN. */
egs_status egs_mixed_friction_solve_batch(egs_context *ctx, int32_t count, const int32_t *n, const double *A, const double *b,
                                          const uint8_t *C, const double *lo, const double *hi, const int32_t *normal_row,
                                          const double *mu, int32_t max_pivots, int32_t max_outer, double tol, double *x,
                                          double *w, double *beta, int32_t *ok, int32_t *pivots, int32_t *outer, double *change);

/* Replaces sparse::JacobiIteration / GaussSeidelIteration / SORIteration on an EXPLICIT matrix:
 *   VectorXd sparse::XIteration(const MatrixXd& A, const VectorXd& b)                                    sparse_iterations.h:13-24
 *   VectorXd sparse::XIteration(const MatrixXd& A, const VectorXd& b, const ArrayXb& C, x_lo, x_hi)
 * i.e. BaseIteration(A, b, ...) of sparse_iterations.cc:72-144 with its dense solves
 * (sparse_iterations_utils.cc:25-40, 110-128, 245-262) and stopping test (:35-49, 128-141): x0 = b,
 * one sweep, one residual, stop at err <= tol or after max_iters sweeps.  A [N][N] row-major (general,
 * need not be symmetric; non-zero diagonal), N <= 1024; C / lo / hi all NULL = the 2-argument form
 * (every row an equality).  params: method, omega, max_iters, tol as for entry 1 (cfm unused: it is in A).
 * stats: iterations, residual.  The reference's spectral-radius gate (:113-121, Panic when
 * rho(M^-1 N) >= 1) is not evaluated: a diverging splitting runs to max_iters and reports its residual. */
egs_status egs_dense_iterate(egs_context *ctx, int32_t N, const double *A, const double *b, const uint8_t *C,
                             const double *lo, const double *hi, const egs_solve_params *params, double *x,
                             egs_solve_stats *stats);

/* The same on `count` independent systems in one device pipeline: the iterative twin of egs_box_lcp_batch, for the
 * sizes the reference's own study of the three iterations runs them on (3..50 rows, sparse_iterations.cc:355-513)
 * and a contact patch hands a projected iteration (8 contacts x 3 = 24 rows), where one call of egs_dense_iterate is
 * all launch and copy.  Packing as egs_box_lcp_batch: problem k has n[k] rows (0 <= n[k] <= 1024; 0 gives
 * iterations 0, residual 0, sparse_iterations.cc:79-81), its row-major matrix (general, non-zero diagonal) at
 * A + sum_{j<k} n[j]^2, its vectors (b, C, lo, hi, x) at sum_{j<k} n[j]; C / lo / hi all NULL = every row of every
 * problem an equality (the 2-argument form).  params: method, omega, max_iters, tol, shared by the batch, as for
 * egs_dense_iterate.  One upload, at most two launches (problems of up to 96 rows: a wavefront each with the matrix
 * in LDS; larger ones: the single call's workgroup each), one read-back, one synchronisation; no workgroup waits on
 * another.  iterations[k] / residual[k] (either may be NULL) and x are, bit for bit, what egs_dense_iterate reports
 * for problem k alone.  residual_history (may be NULL): [count][max_iters + 1], the convergence curve the reference
 * computes and only prints in a commented-out line (:134-137): entry 0 = the error of x0 = b (:124-126), entry s =
 * the error after sweep s (:131-133), NaN beyond iterations[k].  count = 0 is EGS_OK.  EGS_ERR_INVALID, with nothing
 * launched and no output written: count < 0, a size outside 0..1024, a method or omega egs_dense_iterate refuses,
 * max_iters < 0, a zero on some diagonal (egs_last_error names the first such problem). */
egs_status egs_dense_iterate_batch(egs_context *ctx, int32_t count, const int32_t *n, const double *A, const double *b,
                                   const uint8_t *C, const double *lo, const double *hi,
                                   const egs_solve_params *params, double *x, int32_t *iterations, double *residual,
                                   double *residual_history);

/* ---- the dense front half of Ensemble::ComputeVDot (ensembles.cc:498-538) on
 *      the device, for the sizes the reference's dense solver is meant for
 *      (Chain, Cairn): the problem's blocks (assemble or set_blocks) -> dense
 *      A = J M^-1 J^T + cfm I (ensembles.cc:510, 513-521), [3m][3m] row-major,
 *      kept on the device; A (host) may be NULL.  fp64 problems only.          */
egs_status egs_problem_dense_system(egs_problem *p, double cfm, double *A /*[3m][3m] or NULL*/);
/* Replaces CheckMatrixCondition / GetConditionNumber (ensembles.cc:514 -> utils.cc:256-287): the
 * reference takes sigma_max / sigma_min from a JacobiSVD (Eigen, absent here).  For the symmetric
 * positive definite A that is lambda_max / lambda_min: power iteration on A and inverse iteration
 * with A's Cholesky factor, on the device (up to 3m = 1024 rows; within a few per cent, never above
 * the true value; beyond 1024 rows the pivot bound (max L_ii / min L_ii)^2, a lower bound) -- +inf
 * when A is not positive definite.  The caller compares with kGoodConditionNumber = 1e7
 * (constants.h:12) and picks the cfm of the step, as ensembles.cc:513-521.                      */
egs_status egs_problem_dense_condition(egs_problem *p, double cfm, double *estimate);
/* The same for a caller's own symmetric positive definite matrix (A [N][N] row-major, host): replaces
 * GetConditionNumber(A) / CheckMatrixCondition(A) of utils.cc:256-287 as such.  *pivot_bound (may be
 * NULL) receives the cheap lower bound (max L_ii / min L_ii)^2 beside the estimate.               */
egs_status egs_dense_condition(egs_context *ctx, int32_t N, const double *A, double *estimate, double *pivot_bound);
/* One StepVelocities_ODE through the reference's LIVE dense path (ensembles.cc:563-575,
 * 498-538): assemble, dense system with the cfm the caller decided, then
 * Lcp::MixedConstraintsSolver on the device matrix (use_bounds as in entry 3), v update.
 * Nothing but 3m row types / bounds crosses PCIe; lambda, accumulators and v_new are
 * read with egs_problem_get_lambda / get_accumulators / get_velocity.             */
egs_status egs_problem_step_dense(egs_problem *p, double dt, double erp, double cfm,
                                  int32_t use_bounds, int32_t *ok, int32_t *pivots);

/* ---- contact generation ("next" row 1): replaces Ensemble::UpdateContacts
 *      (ensembles.cc:445-480 -> CollideBoxAndGround collision.cc:408-436,
 *      CollideBoxes collision.cc:166-388) and the contact-vs-contact pruning of
 *      CheckAndCorrectEnsembleState (ensembles.cc:308-328, 1e-6).
 * pos [n][3], R [n][9], side_lengths [n][3] -> the contact list in the
 * reference's order (ground contacts by body, then body pairs i < j):
 * body0/body1 [m] (-1 = ground), data [m][7] = position, normal, depth, ready
 * for egs_problem_set_constraints with kind = EGS_CONTACT_BOX.             */
egs_status egs_update_contacts(egs_context *ctx, int32_t n_bodies,
                               const double *pos, const double *R,
                               const double *side_lengths, int32_t max_contacts,
                               int32_t *m_out, int32_t *body0, int32_t *body1,
                               double *data);

/* The same with the joint-vs-contact check of CheckAndCorrectEnsembleState
 * (ensembles.cc:296-306): a contact within 1e-6 of a joint between the same two
 * bodies (Joint::GetConstraintPosition, joints.cc:57-75) is dropped.
 * jb0/jb1 [m_joints], jdata [m_joints][7] = c0, c1 as in set_constraints.     */
egs_status egs_update_contacts_joints(egs_context *ctx, int32_t n_bodies,
                                      const double *pos, const double *R,
                                      const double *side_lengths, int32_t m_joints,
                                      const int32_t *jb0, const int32_t *jb1,
                                      const double *jdata, int32_t max_contacts,
                                      int32_t *m_out, int32_t *body0,
                                      int32_t *body1, double *data);

/* ---- shapes: spheres beside boxes.
 * A sphere is a body whose side_lengths row is (d, d, d) with d > 0; r = d / 2 and its R is not read by the
 * collider.  The conventions are the box code's: body0 < body1 or body0 = -1 (ground), the normal points from body0
 * towards body1, depth >= 0, a pair exactly touching is a contact, a ground contact needs z < 0 strictly.
 *   sphere - ground: q = (c_x, c_y, c_z - r); contact iff q_z < 0: (q, (0, 0, 1), -q_z).
 *   sphere i - sphere j: d = c_j - c_i, L = |d|, s = L - (r_i + r_j); contact iff s <= 0; n = d / L ((0, 0, 1) when
 *     L == 0), depth = -s, position = c_i + n (r_i + L - r_j) / 2.
 *   sphere S - box B: p = R_B^T (c_S - c_B), h = side_B / 2, q_k = clamp(p_k, -h_k, h_k).  Centre outside (q != p):
 *     e = p - q, L = |e|, contact iff L - r <= 0, n_BS = R_B e / L, depth = r - L, box point R_B q + c_B.  Centre
 *     inside or on the surface: k = argmin_k (h_k - |p_k|) (lowest k on a tie), n_BS = sgn(p_k) (column k of R_B) with
 *     sgn(0) = +1, depth = (h_k - |p_k|) + r, box point = the centre moved onto that face.  Sphere point
 *     c_S - r n_BS; position = the midpoint of the two points; the normal is n_BS if the box is body0, else -n_BS.
 * A pair with a sphere has at most one contact; the joint-vs-contact pruning applies to it unchanged.  The list order
 * is unchanged and box-box pairs emit what they emit without shapes.  Inertia stays the caller's (Minv).
 *
 * A capsule (EGS_SHAPE_CAPSULE = 2) is a body whose side_lengths row is (d, d, l) with d > 0 and l > d strictly, both
 * finite (l == d is a sphere and is refused: use EGS_SHAPE_SPHERE).  r = d / 2, half axis e = (l - d) / 2 > 0, axis u =
 * column 2 of R (R[2], R[5], R[8]); "the ball at t" is the sphere of diameter d centred at c + t u, t in [-e, e];
 * end 0 is t = -e, end 1 is t = +e.  The conventions are the ones above, and every rule is one of the three sphere
 * rules applied to balls of the capsule:
 *   capsule - ground: the sphere - ground rule on the ball at end 0, then at end 1: at most 2 contacts, in that order.
 *   capsule - sphere: t = clamp((c_S - c) . u, -e, e); the sphere - sphere rule between the ball at t and the sphere,
 *     in the pair's (i, j) order: at most 1 contact.
 *   capsule i - capsule j: candidates in this order: end 0 of i against capsule j, end 1 of i against j, end 0 of j
 *     against capsule i, end 1 of j against i (each by the capsule - sphere rule, normal always i -> j), then the
 *     interior pair: the balls at the axes' common-perpendicular parameters (s, t), which exists only where s and t lie
 *     strictly inside both segments and the 2 x 2 determinant (u_i.u_i)(u_j.u_j) - (u_i.u_j)^2 is non-zero in the
 *     device's arithmetic.  Whenever the closest pair of the two segments involves an end it is one of the four end
 *     candidates, so parallel axes need no special case.  At most 5 contacts.
 *   capsule - box: dist(t) = the L of the sphere - box rule for a centre at c + t u (0 inside the box).  Candidates:
 *     end 0, end 1, then the interior point t*, each by the sphere - box rule.  t* is the lowest minimiser of dist on
 *     [-e, e] and counts only when strictly inside; if the axis enters the box (minimum 0) t* is the midpoint of the
 *     stretch of axis inside the box (the segment clipped against the three slabs).  dist^2 is a convex piecewise
 *     quadratic in t with at most 6 breakpoints (a box-frame coordinate of the axis crossing +-h_k); the minimiser is
 *     found exactly up to rounding from the ends, the breakpoints and each piece's stationary point.  At most 3.
 *   A candidate is emitted iff its sphere rule says contact.
 *   Flat rule (capsule - capsule and capsule - box): the interior candidate is dropped if an EMITTED end candidate's
 *   centre distance (for a box: its dist) is within 1e-9 of its own; 1e-9 is absolute, in metres, a constant of the
 *   kind of the collider's 1e-6.  So a log flat on a plate and two logs side by side get 2 contacts, a capsule bridging
 *   two boxes one per box; a crossed pair, a capsule see-sawing on a box edge and a capsule lying across a box narrower
 *   than itself get 1.  In that last case dist is constant along the stretch above the box up to rounding, and the
 *   contact's position ALONG that flat stretch is unspecified within the stretch.
 * The same-pair 1e-6 pruning and the joint-vs-contact pruning then run unchanged.  List order and the output of
 * box - box pairs and of spheres are unchanged.  A scene without a capsule launches the kernels it launched before.  */
typedef enum { EGS_SHAPE_BOX = 0, EGS_SHAPE_SPHERE = 1, EGS_SHAPE_CAPSULE = 2 } egs_shape;

/* egs_update_contacts_joints with shape [n_bodies] (egs_shape values) or NULL.  NULL, or all EGS_SHAPE_BOX, gives the
 * result of egs_update_contacts_joints bit for bit.  EGS_ERR_INVALID: an unknown shape value, a sphere whose
 * side_lengths row is not three equal positive numbers, a capsule whose row is not (d, d, l) with 0 < d < l, finite. */
egs_status egs_update_contacts_shapes(egs_context *ctx, int32_t n_bodies,
                                      const double *pos, const double *R,
                                      const double *side_lengths, int32_t m_joints,
                                      const int32_t *jb0, const int32_t *jb1,
                                      const double *jdata, const int32_t *shape,
                                      int32_t max_contacts, int32_t *m_out,
                                      int32_t *body0, int32_t *body1, double *data);

/* ---- carrying lambda across a contact list that changes: the start (x0 of egs_problem_set_start's
 *      EGS_START_GIVEN) of a solve on the new list from the lambda of the last solve on the old one.
 * Both lists hold n_ens >= 1 ensembles back to back (offsets [n_ens + 1], from 0 to m), each in the order
 * egs_update_contacts writes, i.e. ordered by (b0, b1) with the ground (-1) first; an old list that is not is
 * refused.  pos = the contacts' positions [m][3], lambda / rhs = their rows [m][3].  For new contact c of ensemble e:
 *   valid[e] == 0                       x0 = its rhs rows (the reference's start, Q7); source = -2
 *   otherwise, among e's old contacts of the same ordered pair (b0, b1), the one whose position is nearest
 *   (squared distance (dx^2 + dy^2) + dz^2 <= radius^2; a tie goes to the lowest old index):
 *                                       x0 = its lambda rows, bit for bit; source = its old index
 *   no such old contact                 x0 = 0; source = -1
 * Two new contacts may take the same old one.  Positions are compared in the world frame: the radius must exceed
 * what a contact point travels in one step.  One lane per new contact, a binary search for the pair's run in the
 * ensemble's old segment and a scan of that run.  EGS_ERR_INVALID: radius < 0 or NaN, bad offsets, NULL arrays.   */
egs_status egs_match_contacts(egs_context *ctx, int32_t n_ens,
    int32_t m_old, const int32_t *old_b0, const int32_t *old_b1, const double *old_pos, const double *old_lambda,
    const int32_t *old_off /*[n_ens+1]*/, const uint8_t *valid /*[n_ens]*/,
    int32_t m_new, const int32_t *new_b0, const int32_t *new_b1, const double *new_pos, const double *new_rhs,
    const int32_t *new_off, double radius, double *x0 /*[3 m_new]*/, int32_t *source /*[m_new]*/);

/* ---- the whole Ensemble::Step on the device ------------------------------
 * Ensemble::Step(dt, OPEN_DYNAMICS_ENGINE) (ensembles.cc:390-427) with the
 * sparse switch on: UpdateContacts + contact pruning, StepVelocities_ODE
 * (assembly, rhs, projected solve, velocity update) and StepPositions_ODE all
 * run on the GPU and the body state stays there between steps.  Only the
 * contact TOPOLOGY (body index pairs) is read back each step; the schedule is
 * re-planned on the host only when it changed.  Constraint list order as in
 * the reference: joints first, then contacts (ensembles.cc:234-239).         */
typedef struct egs_world egs_world;
egs_status egs_world_create(egs_context *ctx, int32_t n_bodies, int32_t precision, egs_world **out);
void egs_world_destroy(egs_world *w);
/* pos [n][3], R [n][9], v, w [n][3], Minv [n][36], f_ext [n][6] (frozen as
 * Ensemble::Init leaves them, quirk Q5, unless egs_world_set_live_inertia is
 * on: then their angular parts follow the bodies and only the linear rows
 * given here are kept), side_lengths [n][3] (body.h:91).
 * The first call needs every array; later calls may pass NULL for any of them
 * to keep what the device holds (typically Minv, f_ext, side_lengths). */
egs_status egs_world_set_bodies(egs_world *w, const double *pos, const double *R, const double *v,
                                const double *w_ang, const double *Minv, const double *f_ext,
                                const double *side_lengths);
/* shape [n_bodies] (egs_shape; global body indices in a batched world) for every entry that detects contacts:
 * egs_world_step[_each], egs_world_step_dense[_each], egs_world_stabilize[_direct] with detect_contacts = 1.  NULL
 * switches back to boxes.  Valid any time after the world is created; drops the warm-start history as
 * egs_world_set_bodies does.  EGS_ERR_INVALID, with nothing changed: an unknown value; a sphere whose side_lengths row
 * is not three equal positive numbers, a capsule whose row is not (d, d, l) with 0 < d < l -- checked when both are known, i.e. here if egs_world_set_bodies has given the
 * side lengths and in egs_world_set_bodies whenever it is given side_lengths while shapes are set.             */
egs_status egs_world_set_shapes(egs_world *w, const int32_t *shape);
/* ball joints: body0/body1 [m], data [m][7] = c0, c1 (world point if body1 = -1), 0 */
egs_status egs_world_set_joints(egs_world *w, int32_t m_joints, const int32_t *body0, const int32_t *body1,
                                const double *data);
/* ... of any joint kind (EGS_JOINT_BALL, EGS_JOINT_LOCK, EGS_JOINT_HINGE_AXIS, EGS_JOINT_SLIDER_AXIS; data as egs_problem_set_constraints
 * takes it, checked the same way).  kind = NULL, or all EGS_JOINT_BALL, is egs_world_set_joints bit for bit.  Only the
 * ball joints take part in the joint-versus-contact pruning of the collider: an angular block has no position.  The
 * batch rules are those of egs_world_set_joints.  Drops the motors of an earlier list.                          */
egs_status egs_world_set_joints_kinds(egs_world *w, int32_t m_joints, const int32_t *kind /*[m_joints] or NULL*/,
                                      const int32_t *body0, const int32_t *body1, const double *data);
/* egs_problem_set_motors for the world's joints: motor [m_joints][2] = (speed, tau), NULL = off.  Every step's
 * assembly carries it, re-planned lists included; the stabilise entries work on positions and ignore it.
 * EGS_ERR_INVALID as egs_problem_set_motors (nothing changes).                                                   */
egs_status egs_world_set_joint_motors(egs_world *w, const double *motor /*[m_joints][2] or NULL = off*/);
/* egs_problem_set_hinge_limits for the world's joints: lim [m_joints][8], NULL = off.  Every step's assembly carries
 * it, re-planned lists included, each ensemble of a batch its own rows; the stabilise entries take an active stop as a
 * row of their system; the dense steps return EGS_ERR_UNSUPPORTED while a hinge has a stop.  egs_world_set_joints[_kinds]
 * drops it.  EGS_ERR_INVALID as egs_problem_set_hinge_limits (nothing changes).                                  */
egs_status egs_world_set_joint_limits(egs_world *w, const double *lim /*[m_joints][8] or NULL = off*/);
/* egs_problem_set_slider_limits for the world's joints: lim [m_joints][2] = (xlo, xhi), NULL = off.  Every step's
 * assembly carries it, re-planned lists included; the stabilise entries take an active stop as a row of their system;
 * the dense steps return EGS_ERR_UNSUPPORTED while a slider has a finite stop.  egs_world_set_joints[_kinds] drops it.
 * EGS_ERR_INVALID as egs_problem_set_slider_limits (nothing changes).                                            */
egs_status egs_world_set_slider_limits(egs_world *w, const double *lim /*[m_joints][2] or NULL = off*/);
egs_status egs_world_step(egs_world *w, double dt, double erp, const egs_solve_params *params,
                          int32_t detect_contacts, egs_solve_stats *stats);
egs_status egs_world_get_bodies(egs_world *w, double *pos, double *R, double *v, double *w_ang);
egs_status egs_world_get_contacts(egs_world *w, int32_t max_contacts, int32_t *m_out, int32_t *body0,
                                  int32_t *body1, double *data);
egs_status egs_world_get_lambda(egs_world *w, int32_t max_rows, int32_t *rows_out, double *lambda);
/* The system the last step assembled, as egs_problem_get_blocks returns it, joints first: m = egs_world_info's
 * n_constraints, J0 / J1 [m][18], is_eq / lo / hi / rhs / err [3m]; any pointer may be NULL. */
egs_status egs_world_get_blocks(egs_world *w, double *J0, double *J1, uint8_t *is_eq, double *lo, double *hi,
                                double *rhs, double *err);
/* Live inertia for the world's bodies: egs_problem_set_live_inertia / egs_problem_get_mass (above) with global body
 * indices in a batched world.  The refresh is the first thing every egs_world_step[_each] and
 * egs_world_step_dense[_each] enqueues; the stabilise entries work with M = I and do not refresh -- the step after
 * them does, from the poses they left.  The state is per body, so each ensemble of a batched world holds the bits of
 * a world created for it alone.  Valid any time after the world is created; get_mass after egs_world_set_bodies. */
egs_status egs_world_set_live_inertia(egs_world *w, const double *inertia_body, const double *torque);
egs_status egs_world_get_mass(egs_world *w, double *Minv, double *f_ext);

/* ---- warm start: a step's solve starts from the previous step's lambda instead of rhs (quirk Q7).  Off by default;
 * off, nothing in a step changes.  On, egs_world_step and egs_world_step_each run
 *   collide, re-plan on change, assemble, MATCH into x0, solve from x0, stall check, SNAPSHOT, integrate:
 *   - a contact takes the lambda rows of the nearest contact of the same ordered body pair of the list the last step
 *     solved, within match_radius (the rule of egs_match_contacts; none: 0), a joint its own previous rows;
 *   - a step without history -- the first one, after egs_world_set_bodies, egs_world_set_joints or any
 *     egs_world_stabilize* -- is the default step bit for bit (x0 = rhs rows, source -2) except that its
 *     egs_solve_stats.schedule carries EGS_SCHED_START like every warm step's: the solve was handed a start, which
 *     happens to be rhs; a stalled solve leaves the
 *     history as it was; a step without constraints leaves an empty history (the next contacts start from 0);
 *   - batched worlds: history, validity and offsets per ensemble, each ensemble the bits of a world holding only it.
 *     An ensemble that sits a step out (dt[e] = 0) is solved from its rhs rows as ever (its lambda rows are 0) and
 *     keeps the history it held;
 *   - the dense steps take no start; after one the history is that step's lambda.
 * Positions are matched in the world frame: match_radius (>= 0, metres) must exceed what a contact point travels in
 * one step.
 * egs_world_get_start: x0 [3m] of the last warm sweep step and, if asked, per constraint the index (among the
 * previous list's contacts; a joint: its own index) its rows came from, -1 or -2 as egs_match_contacts reports;
 * EGS_ERR_INVALID if the last step was not one.                                                                  */
egs_status egs_world_set_warm_start(egs_world *w, int32_t enable, double match_radius);
/* The friction pyramid of egs_problem_set_friction for a world: one coefficient per ensemble (n_ensembles must be the
 * world's, 1 for a plain world).  Every contact of ensemble e takes mu[e], every joint -1; mu[e] < 0 keeps the
 * reference's friction box for that ensemble.  The per-constraint coefficients are filled on the device from the
 * current contact list at every step.  egs_world_step and egs_world_step_each solve with it; egs_world_step_dense and
 * egs_world_step_dense_each return EGS_ERR_UNSUPPORTED while any coefficient is >= 0, unless
 * egs_world_set_dense_friction has allowed it.  Warm start and stabilisation are untouched.  EGS_ERR_INVALID: mu NULL, a NaN, a wrong n_ensembles (nothing changes).                              */
egs_status egs_world_set_friction(egs_world *w, int32_t n_ensembles, const double *mu /*[E]*/);
/* Restitution (egs_problem_set_restitution) for a world: one coefficient per ensemble (n_ensembles must be the world's,
 * 1 for a plain world) and one threshold speed.  Every contact of ensemble e takes rest[e], every joint -1; rest[e] < 0:
 * that ensemble's contacts do not bounce and get the bits of a world without this call.  The per-constraint table is
 * filled on the device from the current contact list at every step (no read-back, no upload), so the contacts of a
 * re-planned list carry their ensemble's coefficient.  egs_world_step[_each] and egs_world_step_dense[_each] assemble
 * with it; warm start matches and snapshots after the restituted solve; the stabilise entries work on positions and
 * ignore it.  EGS_ERR_INVALID: rest NULL, a NaN or infinite coefficient, vth < 0, NaN or infinite, a wrong n_ensembles
 * (nothing changes).                                                                                              */
egs_status egs_world_set_restitution(egs_world *w, int32_t n_ensembles, const double *rest /*[E]*/, double vth);
egs_status egs_world_get_start(egs_world *w, int32_t max_rows, int32_t *rows_out, double *x0, int32_t *source /*[m] or NULL*/);
egs_status egs_world_info(egs_world *w, int32_t *n_constraints, int32_t *n_contacts, int32_t *replans);

/* ---- many ensembles in one world ------------------------------------------
 * The reference steps every Ensemble of a frame in turn (model.cc:37-70:
 * SimulationStep() calls Step() on each).  A batched world holds E
 * independent ensembles and steps them all in one device pipeline; after
 * every step each ensemble holds exactly the bits a world created for it
 * alone would hold: bodies, contact list (order included), lambda, sweep
 * count and residual.
 *   - n_bodies [E] (>= 0 each, E >= 1); body_offset [E+1] (may be NULL)
 *     receives where ensemble e's bodies start in the concatenated arrays
 *     that egs_world_set_bodies / get_bodies take.
 *   - egs_world_set_joints keeps global body indices; a joint may not join
 *     two ensembles (the world, -1, is allowed) and the joints must be
 *     grouped by non-decreasing ensemble: EGS_ERR_INVALID otherwise.
 *   - Contacts never join two ensembles; the contact list (get_contacts) is,
 *     ensemble by ensemble, its ground contacts then its body pairs i < j.
 *   - With tol > 0 each ensemble stops on its own residual, as its own
 *     Step() would; egs_solve_stats from egs_world_step then reports the
 *     largest sweep count and the largest residual over the ensembles.
 * E = 1 is egs_world_create(ctx, n_bodies[0], ...) itself.                   */
egs_status egs_world_create_batch(egs_context *ctx, int32_t n_ensembles, const int32_t *n_bodies,
                                  int32_t precision, egs_world **out, int32_t *body_offset);
/* Per-ensemble figures of a world (n_ensembles must be the world's; a plain
 * world is one ensemble).  joint_offset / contact_offset [E+1]: ensemble e's
 * joints are constraints [joint_offset[e], joint_offset[e+1]) and its contacts
 * [contact_offset[e], contact_offset[e+1]) of get_contacts, i.e. constraint
 * mj + k of get_lambda's rows (joints first).  iterations / residual [E]: the
 * last step's solve of each ensemble (model.cc:37-70, one Step() each).
 * Any pointer may be NULL.                                                   */
egs_status egs_world_batch_info(egs_world *w, int32_t n_ensembles, int32_t *joint_offset,
                                int32_t *contact_offset, int32_t *iterations, double *residual);

/* Ensemble::Step(dt, OPEN_DYNAMICS_ENGINE) on the reference's live path (kSparseImplementation = false,
 * ensembles.cc:390-427, 498-538, 563-591), for every ensemble of a world (plain or batched).  Per ensemble,
 * on its own constraint list in the reference's order (its joints, then its contacts):
 * A = J M^-1 J^T; cond(A) < 1e7 ? A : A + cfm_coeff*I; Lcp::MixedConstraintsSolver(A, rhs, C, lo, hi);
 * velocity update; midpoint positions.  use_bounds: 0 = the reference (quirk Q3), 1 = true box problem.
 * fp64 worlds only (EGS_ERR_UNSUPPORTED otherwise).  If any ensemble's solve fails (the reference Panics,
 * ensembles.cc:531-534), the call returns EGS_ERR_LCP_FAILED, egs_last_error names the first failing
 * ensemble and NO body of the world is advanced.  *n_failed (may be NULL) = how many failed.
 *   - Contact detection, pruning and re-planning are those of egs_world_step; the two steps may alternate on
 *     one world (they share the bodies, the contact list, get_lambda and batch_info's offsets), and switching
 *     between them does not re-plan.  After a dense step batch_info reports iterations[e] = principal pivots
 *     and residual[e] = NaN.
 *   - An ensemble of at most 112 rows (3 per constraint) is solved by one fused kernel, a workgroup per
 *     ensemble, the whole ComputeVDot in LDS (size classes of <= 32, <= 64 and <= 112 rows; the class depends
 *     on the ensemble's own size only, so its bits do not depend on the rest of the batch).  Larger ensembles
 *     are solved one after another inside the same call by the multi-launch path of egs_problem_step_dense
 *     (the condition estimate of egs_problem_dense_condition, then the dense mixed solver).
 *   - An ensemble without constraints gets v_dot = M^-1 f (ensembles.cc:504-505), ok = 1, pivots = 0.   */
egs_status egs_world_step_dense(egs_world *w, double dt, double erp, double cfm_coeff, int32_t use_bounds,
                                int32_t detect_contacts, int32_t *n_failed);
/* Per-ensemble figures of the last egs_world_step_dense ([E] each, any may be NULL): the condition estimate
 * (+inf when A is not positive definite), the cfm actually added (0 or cfm_coeff), the principal pivots,
 * and ok (1 = solved).  n_ensembles must be the world's; EGS_ERR_INVALID before the first dense step.    */
egs_status egs_world_dense_info(egs_world *w, int32_t n_ensembles, double *condition, double *cfm,
                                int32_t *pivots, int32_t *ok);
/* The friction pyramid on the dense steps, opt-in (egs_problem_set_dense_friction for a world).  max_outer > 0: while
 * egs_world_set_friction is on, egs_world_step_dense and egs_world_step_dense_each solve every ensemble's pyramid --
 * every contact's rows 0 and 1 bounded by +-mu[e] x of its row 2, joints and ensembles with mu[e] < 0 as stored --
 * by the fixed-point iteration of egs_mixed_friction_solve_batch.  Ensembles of at most 112 rows run it inside the fused
 * kernel (its pyramid form: mu read per gathered constraint from the table the step fills; partition and Schur
 * complement once; each solve starts its Murty set from the previous solve's); larger ones from the host around the
 * multi-launch path (each solve from scratch).  use_bounds must be 1 while friction is on (EGS_ERR_INVALID otherwise).
 * A world whose friction is off steps exactly as without this call.  Each ensemble of a batched world gets the bits of
 * its own one-ensemble world.  Not converging within max_outer is no failure.  max_outer = 0 (the default): the dense
 * steps refuse friction as before.  EGS_ERR_INVALID: max_outer < 0, tol < 0 or NaN.                                */
egs_status egs_world_set_dense_friction(egs_world *w, int32_t max_outer, double tol);
/* Per-ensemble outcomes of the pyramid in the last dense step ([E] each, any may be NULL): solves made, converged
 * (change <= tol), the last change; an ensemble without constraints, sitting out, or stepped with friction off reports
 * 1, 1, 0.  n_ensembles must be the world's; EGS_ERR_INVALID before the first dense step.                          */
egs_status egs_world_dense_friction_info(egs_world *w, int32_t n_ensembles, int32_t *outer, int32_t *converged,
                                         double *change);

/* ---- a time step and an erp per ensemble -----------------------------------------------------------------------
 * The reference's frame steps its ensembles at different rates (model.cc:80, 108: the cairn with kSimTimeStep*5,
 * the chain with kSimTimeStep).  egs_world_step_each is egs_world_step with ensemble e stepped by dt[e] with
 * erp[e]; egs_world_step_dense_each is egs_world_step_dense likewise.  n_ensembles must be the world's (a plain
 * world is one ensemble).  dt[e] > 0: the ensemble takes its Ensemble::Step(dt[e]).  dt[e] == 0: the ensemble sits
 * this step out.  dt[e] < 0 or NaN, dt or erp NULL, wrong n_ensembles: EGS_ERR_INVALID and nothing moved.  All
 * dt[e] == 0 is valid (nothing moves).  After the call every ensemble holds, bit for bit, what a world holding only
 * it holds after the same call with that ensemble's dt and erp.
 *   - An ensemble with dt[e] > 0: assembly, rhs (ensembles.cc:569-570), velocity update (:535, :572) and
 *     StepPositions_ODE (:577-591) use dt[e] and erp[e] in the expressions, and in the order, of the scalar entries:
 *     -erp / dt / dt, vel / dt + Wf, v + dt * (...), rotate by |w| dt.
 *   - An ensemble with dt[e] == 0: its bodies (pos, R, v, w) are not touched, bit for bit (they are skipped, not
 *     multiplied by zero).  Contact detection still runs over the whole world; it is a function of the poses alone,
 *     so this ensemble's list comes out as it was.  Its rhs rows are exactly 0 (not computed through 1/dt), hence
 *     its rows of egs_world_get_lambda are 0.  egs_world_batch_info reports residual 0 for it and, with tol > 0,
 *     iterations 0; with a fixed sweep count it reports max_iters, as for every ensemble.  On the dense path it is
 *     not solved: ok = 1, pivots = 0, condition 1, cfm 0 (batch_info's residual is NaN there, as for every
 *     ensemble after a dense step).  A failure of another ensemble on the dense path still advances no body.
 *   - All dt[e] equal and all erp[e] equal: the world is left bit-identical to what the scalar entry with that dt
 *     and erp leaves, egs_world_batch_info and egs_solve_stats included.
 *   - Everything else -- the stopping rule per ensemble, re-planning only on a topology change, get_lambda after a
 *     stabilise call, stall handling, fp32 worlds on the sweeps and fp64 only on the dense path -- is as in the
 *     scalar entries.  The _each forms may alternate freely with the scalar forms, with egs_world_stabilize* and
 *     with each other on one world; none of that re-plans.  The 2 E rates reach the device without a stream
 *     synchronisation, and only when they differ from the last call's.                                            */
egs_status egs_world_step_each(egs_world *w, int32_t n_ensembles, const double *dt, const double *erp,
                               const egs_solve_params *params, int32_t detect_contacts, egs_solve_stats *stats);
egs_status egs_world_step_dense_each(egs_world *w, int32_t n_ensembles, const double *dt, const double *erp,
                                     double cfm_coeff, int32_t use_bounds, int32_t detect_contacts, int32_t *n_failed);

/* Ensemble::InitStabilize (mode EGS_STABILIZE_INIT, ensembles.cc:602-622) or Ensemble::PostStabilize(max_steps)
 * (EGS_STABILIZE_POST, ensembles.cc:624-646) for every ensemble of a world (plain or batched).  Per ensemble, on its
 * own constraint list in the reference's order (its joints, then its contacts): err_sq = sum err_i^2; while
 * err_sq > 1e-9 (constants.h:5) and steps < max_steps: solve (J J^T) y = err, v_r = -0.2 J^T y (J^T y summed per body
 * in list order), p += h v_r[0:3], R = WtoR(v_r[3:6], h) R (StepPositions_ExplicitEuler, ensembles.cc:553-561),
 * then err_sq again.  INIT: h = 0.5, velocities untouched.  POST: h = 0.1, then v += v_r[0:3], w += v_r[3:6].
 * max_steps = 0: the reference's 100 (INIT) / 500 (POST); hitting it is not an error.  fp64 worlds only
 * (EGS_ERR_UNSUPPORTED otherwise).  *n_unsettled (may be NULL) = ensembles that ended with err_sq > 1e-9 (or NaN).
 *   - INIT with detect_contacts = 1 detects and prunes contacts as egs_world_step does, once before the first test
 *     and after every position step (InitStabilize's UpdateContacts); POST never detects.
 *   - The solve is the adapter's (stabilize.cpp): the matrix-free sweep with M^-1 = I, every row an equality; params
 *     NULL = SOR, omega 1.5, cfm 0, tol 1e-11, at most 20000 sweeps, checked every 10.  Each ensemble stops on its
 *     own test; a stopped ensemble is frozen (bodies, contacts, steps, err_sq) while the others go on, so each
 *     ensemble of a batch ends with the bits a world holding it alone ends with.  An ensemble without constraints
 *     takes 0 steps (err_sq = 0).
 *   - A stall of the relaxation solve returns EGS_ERR_STALL; that pass moves no body.
 *   - Afterwards get_contacts / batch_info describe the final contact list and egs_world_get_lambda returns
 *     EGS_ERR_INVALID until the next egs_world_step / egs_world_step_dense (there is no step lambda for that list).
 *   - EGS_ERR_INVALID, nothing moved: before egs_world_set_bodies, an unknown mode, max_steps < 0.
 *   - The first call allocates the relaxation system; egs_world_step allocates and launches nothing for it.   */
#define EGS_STABILIZE_INIT 0   /* Ensemble::InitStabilize, ensembles.cc:602-622 */
#define EGS_STABILIZE_POST 1   /* Ensemble::PostStabilize(max_steps), ensembles.cc:624-646 */
egs_status egs_world_stabilize(egs_world *w, int32_t mode, int32_t max_steps, int32_t detect_contacts,
                               const egs_solve_params *params, int32_t *n_unsettled);
/* Per-ensemble figures of the last egs_world_stabilize ([E] each, any may be NULL): relaxation steps taken and the
 * final err_sq.  n_ensembles must be the world's; EGS_ERR_INVALID before the first stabilise call.              */
egs_status egs_world_stabilize_info(egs_world *w, int32_t n_ensembles, int32_t *steps, double *err_sq);

/* egs_world_stabilize with the relaxation solve done directly: the same loops, the same mode, max_steps (0 = 100 /
 * 500), freezing of stopped ensembles, *n_unsettled, and the same state of get_contacts / get_lambda afterwards;
 * egs_world_stabilize_info reports steps / err_sq of whichever of the two ran last.  One workgroup per ensemble does a
 * whole pass on chip: assembly, err_sq, the lower triangle of A = J J^T, its factorisation, the solve, the list-order
 * J^T y and the position step.  With a fixed constraint list (POST, or INIT with detect_contacts = 0) ALL passes run
 * inside one launch, with one read-back per call; INIT with detection takes one launch per pass between the world's
 * collide / prune / re-plan-on-change steps.
 *   - The factorisation is the LDL^T with symmetric diagonal pivoting that ldlt() (ensembles.cc:662) is (largest
 *     |diagonal|, lowest index on ties), but it STOPS at the first pivot <= rank_tol * |first pivot| and takes y = 0
 *     on the rows left; rank_tol <= 0 means 1e-10.  Redundant contact points make J J^T singular (a 2x2x2 box stack:
 *     96 rows, rank 48): dividing by its rounding-noise pivots gives |y| ~ 3e14 and a correction wrong by 5x its own
 *     size, while err is consistent, so every solution has the same J^T y and the truncated one equals the least
 *     squares correction to 3e-16.  Where J J^T is positive definite nothing is truncated and the result is ldlt()'s.
 *     Where err is NOT consistent (the contacts of tilted boxes over-determine the bodies: a 5-box cairn has 84 rows
 *     of rank 30) the rows left carry a residual rho, and the leading block is solved for
 *     L1^-1 b1 + (W^T W)^-1 L2^T rho instead of L1^-1 b1 (W = [L1; L2], the truncated unit lower factor): a small
 *     positive definite solve that makes J^T y the least-squares correction J^T (J J^T)^+ err, which the sweep
 *     route converges to.  With consistent err rho = 0 and nothing changes.
 *   - Ensembles of up to 126 rows (42 constraints) live in LDS (<= 48 rows: one wavefront; above: four); larger ones,
 *     up to 1024 rows, keep the matrices and the Jacobian in a per-ensemble device workspace.  The class depends on the
 *     ensemble's own rows only, so each ensemble of a batch ends with the bits a world holding it alone ends with.
 *   - EGS_ERR_UNSUPPORTED: an fp32 world; an ensemble above 1024 rows (if detection pushes one over the limit in
 *     mid-call, that pass moves no body and egs_world_stabilize_info has nothing to report).  EGS_ERR_INVALID:
 *     before egs_world_set_bodies, an unknown mode, max_steps < 0, rank_tol NaN or >= 1.  Nothing is moved then.
 *   - The first call allocates its tables; egs_world_stabilize, egs_world_step and egs_world_step_dense allocate and
 *     launch nothing for it.                                                                                      */
egs_status egs_world_stabilize_direct(egs_world *w, int32_t mode, int32_t max_steps, int32_t detect_contacts,
                                      double rank_tol, int32_t *n_unsettled);
/* Per-ensemble figures of the last egs_world_stabilize_direct ([E] each, any may be NULL): the rows of the ensemble's
 * system (3 per constraint, on the final list) and the rank of the last pass it solved (0: none).  n_ensembles must
 * be the world's; EGS_ERR_INVALID before the first direct call.                                                   */
egs_status egs_world_stabilize_rank(egs_world *w, int32_t n_ensembles, int32_t *rows, int32_t *rank);
/* One-shot: (J J^T) y = err for one constraint list by the same device code, one workgroup.  J0 / J1 [m][18]
 * row-major blocks (zero for a world side, body index -1), err and y [3m]; y = 0 on the rows the truncation left,
 * *rank = pivots taken; rank_tol as above.  3m <= 1024 (EGS_ERR_UNSUPPORTED above).                              */
egs_status egs_relax_blocks_direct(egs_context *ctx, int32_t n_bodies, int32_t m, const int32_t *body0,
                                   const int32_t *body1, const double *J0, const double *J1, const double *err,
                                   double rank_tol, double *y, int32_t *rank);

/* Replaces lcp::SolveLCP_BoxDantzig (toolkit/lcp.cc:444-619; reached from lcp::SolveLCP with
 * Settings.algorithm = COTTLE_DANTZIG, box_lcp = true, schur_complement = false, toolkit/lcp.cc:776-779):
 * Cottle-Dantzig principal pivoting on A x = b + w with lo <= x <= hi, the Cholesky factor of the active
 * set kept up to date row by row (AddCholeskyRow / SwapCholeskyRows, toolkit/lcp.cc:91-157; O(n^2) per
 * pivot).  A [n][n] row-major: only the lower triangle is read, and it is PERMUTED IN PLACE exactly as the
 * reference leaves it (toolkit/lcp.h:170-171); perm[k] = original index of the final row k (may be NULL).
 * Requires lo <= 0 <= hi and lo < hi (toolkit/lcp.cc:448-450: EGS_ERR_INVALID otherwise) and
 * 1 <= n <= 1024 (n <= 96: one wavefront, both matrices in LDS; above: four wavefronts, A permuted in place
 * in device memory).  max_steps > 0 gives up after that many pivot steps, 0 = the library's cap of
 * 20 n + 1000 (*ok = 0, EGS_ERR_LCP_FAILED) -- the device loop always has an exit, where the reference's
 * has none (toolkit/lcp.cc:493) -- as does a non-positive pivot (A not positive definite).                  */
egs_status egs_box_lcp_dantzig(egs_context *ctx, int32_t n, double *A, const double *b, const double *lo,
                               const double *hi, int32_t max_steps, double *x, double *w, int32_t *perm,
                               int32_t *ok, int32_t *pivots);

/* Replaces lcp::SolveLCP_BoxMurty (toolkit/lcp.cc:380-442; with lo = 0, hi = +inf / DBL_MAX it is
 * SolveLCP_Murty, :333-378) on its LinearReducer (:213-328): principal pivoting that moves the first
 * violated index (in the caller's order) in or out of the index set and keeps the set's Cholesky factor
 * up to date row by row.  Same arguments, limits (n <= 1024, lo <= 0 <= hi) and in-place permutation of A's
 * lower triangle as egs_box_lcp_dantzig; max_iterations > 0 = Settings::max_iterations (the call then
 * reports *ok = 0, EGS_ERR_LCP_FAILED, as the reference returns false, toolkit/lcp.cc:438-441).       */
egs_status egs_box_lcp_murty(egs_context *ctx, int32_t n, double *A, const double *b, const double *lo,
                             const double *hi, int32_t max_iterations, double *x, double *w, int32_t *perm,
                             int32_t *ok, int32_t *iterations);

/* The same two solvers (algorithm 0 = SolveLCP_BoxMurty, 1 = SolveLCP_BoxDantzig) on `count` independent
 * problems in ONE launch, a workgroup per problem -- what a batch of ensembles hands lcp::SolveLCP
 * (toolkit/lcp.h:172-174), which the reference calls once per problem.  Problem k has n[k] rows; its matrix
 * sits at A + sum_{j<k} n[j]^2 (row-major, lower triangle read and permuted in place), its vectors (b, lo, hi,
 * x, w, perm) at sum_{j<k} n[j].  ok[k] / pivots[k]: the problem's own outcome and step count -- the same as
 * its single call.  max_steps / max_seconds: Settings::max_iterations / max_time per problem (0 = the
 * library's cap / none).  Returns EGS_OK when every problem was run (see ok[]); EGS_ERR_INVALID for a bad
 * size or bounds that break lo <= 0 <= hi (lo < hi for Dantzig).  perm, pivots may be NULL.               */
egs_status egs_box_lcp_batch(egs_context *ctx, int32_t algorithm, int32_t count, const int32_t *n, double *A,
                             const double *b, const double *lo, const double *hi, int32_t max_steps,
                             double max_seconds, double *x, double *w, int32_t *perm, int32_t *ok,
                             int32_t *pivots);

/* Replaces lcp::SolveLCP_BoxSchur (toolkit/lcp.cc:627-747), what lcp::SolveLCP (toolkit/lcp.h:172-174,
 * toolkit/lcp.cc:752-785) runs under its default Settings (schur_complement = true, box_lcp = true):
 * the two-pointer partition that brings the unbounded rows (lo = -infinity, hi = +infinity; "infinity" =
 * DBL_MAX or the real one) to the front, Z = L L' on them, the Schur complement R = C - B Z^-1 B' and its
 * right-hand side (:714-727), the box LCP on R by SolveLCP_BoxMurty (algorithm 0) or SolveLCP_BoxDantzig
 * (1), and y = Z^-1 (c - B' z).  A: row-major n x n, ONLY THE LOWER TRIANGLE IS READ OR WRITTEN
 * (toolkit/lcp.h:73); it is permuted in place as the reference leaves it: by the partition and, when no row
 * is unbounded, by the inner solver's pivoting (:695-700).  perm[k] = original index of row k after the
 * partition (may be NULL).  nub >= 0 is the reference's test hook (:623-626: that many leading indexes are
 * taken as unbounded unseen), -1 scans the bounds; *nub_out = test_nub_from_SolveLCP_BoxSchur.
 * reference_quirks != 0 keeps the literal tests `hi < -DBL_MAX` of :664, 669 (the lower
 * bound alone decides); 0 tests hi against +DBL_MAX.  max_iterations / max_seconds as above.  Bounded parts
 * beyond 1024 rows are solved by block principal pivoting (same solution).                                  */
egs_status egs_box_lcp_schur(egs_context *ctx, int32_t n, double *A, const double *b, const double *lo,
                             const double *hi, int32_t algorithm, int32_t nub, int32_t reference_quirks,
                             int32_t max_iterations, double max_seconds, double *x, double *w, int32_t *perm,
                             int32_t *ok, int32_t *nub_out, int32_t *pivots);

/* egs_box_lcp_schur on `count` independent problems -- what a batch of ensembles hands lcp::SolveLCP under its
 * DEFAULT Settings.  Packing as egs_box_lcp_batch: problem k has n[k] rows, its matrix at A + sum_{j<k} n[j]^2,
 * its vectors (b, lo, hi, x, w, perm) at sum_{j<k} n[j].  Per problem the semantics are exactly those of
 * egs_box_lcp_schur: only the lower triangle is read or written, perm is the partition's permutation, pivots[k] the
 * inner solver's steps, nub_out[k] = test_nub_from_SolveLCP_BoxSchur; nub[k] >= 0 is the test hook, nub = NULL (or
 * nub[k] < 0) scans the bounds.  reference_quirks, max_iterations and max_seconds hold for every problem of the call.
 * Problems of n <= 96 rows are FUSED: one upload, ONE launch with a workgroup per problem (partition, Z = L L',
 * the Schur complement, the inner box LCP and the back-substitution all in LDS, in the operation order of the plain
 * column-oriented algorithm), one read-back, through page-locked staging of the context.  Problems with more rows
 * are not fused: they run inside the same call, one after another, on the egs_box_lcp_schur path.
 * Returns EGS_OK when every problem was run -- outcomes in ok[k] (0: the inner solver gave up or Z is not
 * positive definite; x and w of such a problem are not meaningful).  EGS_ERR_INVALID, nothing written: a size < 1,
 * nub[k] > n[k], or a bounded row that breaks lo <= 0 <= hi (lo < hi for Dantzig).  count = 0 is EGS_OK.
 * perm, nub_out, pivots may be NULL.                                                                          */
egs_status egs_box_lcp_schur_batch(egs_context *ctx, int32_t algorithm, int32_t count, const int32_t *n, double *A,
                                   const double *b, const double *lo, const double *hi, const int32_t *nub,
                                   int32_t reference_quirks, int32_t max_iterations, double max_seconds, double *x,
                                   double *w, int32_t *perm, int32_t *ok, int32_t *nub_out, int32_t *pivots);

/* ---- diagnostics (host only, needs no GPU) -------------------------------
 * The schedule the solver derives from the constraint graph: islands, the
 * workgroup tile each constraint lands in (-1 = cross-workgroup path) and the
 * per-body tickets (rank/count of the constraint among its body's, list
 * order) that make the parallel sweep reproduce the reference's list order
 * (sparse_iterations_utils.cc:159-243, 292-373).  Arrays [m], may be NULL.   */
/* Diagnostics: with EGS_TRACE_UPDATES=1 in the environment the 4-lane patch kernel stamps every update with the
 * device's 100 MHz wall clock; this copies the stamps of the problem's last such launch, [sweeps][m] (0 = not
 * written), for tools/trace_patches.py, which walks the critical chain of the sweep pipeline.                  */
egs_status egs_problem_debug_trace(egs_problem *p, uint64_t *out, int64_t count, int32_t *sweeps);
/* The body patches an oversize island is cut into (plan.cpp::build_patches): per constraint its patch (-1: none),
 * its lane in the patch, and per side bit 0 = the list-order predecessor on that body sits in another patch, bit 1 =
 * the successor does (the hand-offs that cross global memory).  Arrays [m], may be NULL.                      */
egs_status egs_debug_plan_patches(int32_t n_bodies, int32_t m, const int32_t *body0, const int32_t *body1,
                                  int32_t *n_patches, int32_t *cons_patch, int32_t *cons_lane, int32_t *remote0,
                                  int32_t *remote1);
egs_status egs_debug_plan(int32_t n_bodies, int32_t m, const int32_t *body0,
                          const int32_t *body1, int32_t tile_size,
                          int32_t *n_islands, int32_t *n_tiles,
                          int32_t *n_global, int32_t *cons_tile,
                          int32_t *pos0, int32_t *cnt0, int32_t *pos1,
                          int32_t *cnt1);

/* The LDS slot numbers of the same schedule: per constraint the slot of each side
 * (0 = the world), and per constraint's tile the number of slots it allocates.
 * Slot numbers decide LDS banks; a body keeps one slot in its
 * tile.  Arrays [m], may be NULL; constraints on the cross-workgroup path get -1.  */
egs_status egs_debug_plan_slots(int32_t n_bodies, int32_t m, const int32_t *body0,
                                const int32_t *body1, int32_t tile_size,
                                int32_t *lane, int32_t *slot0, int32_t *slot1,
                                int32_t *tile_nslots);

/* The static timetable of the same schedule (step_device.h): constraint c
 * runs its update of sweep s at time step level[c] + period * s of its tile, level = depth in the
 * list-order dependency DAG of one sweep (sparse_iterations_utils.cc:159-243: a constraint reads
 * what the previous constraint of each of its bodies wrote), period = the largest level span of a
 * body in the tile, depth = levels in the tile.  Arrays [m] (period / depth: the values of the
 * constraint's tile), may be NULL; -1 on the cross-workgroup path.
 * tile_size = 0: the 4-lanes-per-constraint plan with its automatic tile size.
 * *runs = 1 (4-lane plan only): every aligned group of four consecutive constraints joins the same two bodies (the four
 * contact points of a box face) and is ONE node of the timetable: level / period / depth then count
 * groups, and the group's four updates run back to back inside its time step, in list order
 * (reversed in a backward sweep), handing the accumulators from lane to lane.                     */
egs_status egs_debug_plan_timetable(int32_t n_bodies, int32_t m, const int32_t *body0,
                                    const int32_t *body1, int32_t tile_size,
                                    int32_t *level, int32_t *period, int32_t *depth, int32_t *runs);

/* Host only: *pairable = 1 if, in the 256-lane tile plan of the graph, every half-wavefront of lanes (32 consecutive
 * lanes, aligned) is idle or holds constraints of one phase (level mod period) of its tile's timetable: what the fused
 * step launch asks of a plan before it runs an update on a lane pair (EGS_SCHED_PAIR).                              */
egs_status egs_debug_plan_pairable(int32_t n_bodies, int32_t m, const int32_t *body0, const int32_t *body1,
                                   int32_t *pairable);

/* Host only: *chained = 1 if that plan is pairable, every tile's period is even, and the two constraints of every
 * thread pair of the lane-pair form -- A = lane 64 w + l and B = lane 64 w + 32 + l of a tile, l < 32 -- are consecutive
 * updates of the same two bodies: no B without an A, level[A] even, and where both exist the same two LDS slots and
 * level[B] = level[A] + 1.  What the step launch asks before it keeps a pair's accumulators in registers from the
 * first of the two updates to the second (EGS_SCHED_CHAIN).                                                        */
egs_status egs_debug_plan_chained(int32_t n_bodies, int32_t m, const int32_t *body0, const int32_t *body1,
                                  int32_t *chained);

/* Host only: *share = 1 if that plan is chained and, with data the constraint descriptors [m][7] of
 * egs_problem_set_constraints, the two constraints of every thread pair that holds an A and a B have the same contact
 * normal as bit patterns: data[7 A + 3 .. 5] and data[7 B + 3 .. 5] compared as integers (-0.0 is not +0.0).  A pair
 * with an A alone asks nothing.  What the step launch asks before a thread keeps one linear block for both
 * (EGS_SCHED_SHARE).                                                                                               */
egs_status egs_debug_plan_share(int32_t n_bodies, int32_t m, const int32_t *body0, const int32_t *body1,
                                const double *data, int32_t *share);

/* Host only: *faced = 1 if that plan is chained and the four constraints of every thread pair of the face form -- plan
 * lanes 128 W + 32 k + l of a tile, k = 0 .. 3, l < 32, W = 0, 1 -- are consecutive updates of the same two bodies: every
 * tile's period is a multiple of 4, member k exists only if member k - 1 does, level[member 0] is a multiple of 4,
 * every member has member 0's two LDS slots and level[member 0] + k, and per tile, per block of four time steps
 * ((level / 4) mod (period / 4)) and per LDS slot other than the world's, all constraints that use the slot belong to
 * one such group.  What the step launch asks before it runs a face's four updates behind one barrier (EGS_SCHED_FACE). */
egs_status egs_debug_plan_faced(int32_t n_bodies, int32_t m, const int32_t *body0, const int32_t *body1,
                                int32_t *faced);

/* Host only: *face = 1 if that plan is faced and every member of every such group has member 0's contact normal as bit
 * patterns (data as in egs_debug_plan_share).  A group with one member asks nothing.                               */
egs_status egs_debug_plan_face_normals(int32_t n_bodies, int32_t m, const int32_t *body0, const int32_t *body1,
                                       const double *data, int32_t *face);

/* Host only: the split of the FACE launch in time (EGS_SCHED_FACE_SPLIT) for n_tiles tiles on `slots` resident slots
 * (CUs x tiles per CU) whose timetable has the given depth and period, at `sweeps` sweeps -- the policy the library
 * itself applies.  force_tiles < 0: the policy decides; otherwise the last force_tiles tiles (clamped to n_tiles) are
 * split after force_s1 sweeps (outside 1 .. sweeps - 1: no split).  *split_tiles and *s1: the answer, 0 and 0 for no
 * split.  pieces (NULL, or room for 4 x (n_tiles + n_tiles) values): the launch's work list in ticket order, per
 * piece {tile, resume, sweeps of the piece, kind: 0 whole, 1 first part, 2 second part}; *n_pieces its length.     */
egs_status egs_debug_face_split(int32_t n_tiles, int32_t slots, int32_t depth, int32_t period, int32_t sweeps,
                                int32_t force_tiles, int32_t force_s1, int32_t *split_tiles, int32_t *s1,
                                int32_t *pieces, int32_t *n_pieces);

/* Host only: the form of the FACE launch (EGS_SCHED_FACE_LEAN) for n_tiles tiles on a GPU of `cus` CUs whose timetable
 * has the given depth and period, at `sweeps` sweeps -- the policy the library itself applies: the present kernels on
 * 4 x cus resident slots against the lean ones on 6 x cus, each with the split and persistence rules applied to its own
 * slot count.  *lean: 1 where the lean form is predicted shorter; us[0], us[1] (NULL, or room for two): the predicted
 * launch times of the present and the lean form in microseconds; split[0..1], split[2..3] (NULL, or room for four):
 * each form's split tiles and s1.  max_slots > 0: *lds_bytes (NULL: not asked) is the LDS a lean tile with that many
 * body slots asks for at six tiles per CU, 0 where it does not fit (the launch then keeps the present kernels).   */
egs_status egs_debug_face_form(int32_t n_tiles, int32_t cus, int32_t depth, int32_t period, int32_t sweeps,
                               int32_t max_slots, int32_t *lean, double *us, int32_t *split, int64_t *lds_bytes);

/* Which kernel takes islands larger than a workgroup in a GS / SOR solve (host only, the
 * chooser the library itself uses): 0 = body patches on the 4-lanes-per-constraint kernel,
 * 1 = body patches on the 1-lane kernel, 2 = the all-global kernel.  Patches wait on each
 * other, so their count must not exceed (workgroups per CU of the kernel, as
 * hipOccupancyMaxActiveBlocksPerMultiprocessor reports for the exact instantiation) x CUs.  */
int32_t egs_debug_choose_oversize_schedule(int32_t n_patch_tiles, int32_t quad_per_cu,
                                           int32_t patch_per_cu, int32_t cu_count,
                                           int32_t patches_enabled, int32_t quad_patches_enabled);

/* The schedule of the matrix-free products (host only): constraints are
 * partitioned into workgroup tiles; a body touched from more than one tile is
 * "shared" and its constraints form the boundary list that a pre-pass publishes.
 * cons_tile / cons_lane [m], may be NULL.  tile_size = 128 or 256.               */
egs_status egs_debug_matvec_plan(int32_t n_bodies, int32_t m, const int32_t *body0,
                                 const int32_t *body1, int32_t tile_size, int32_t *n_tiles,
                                 int32_t *n_islands, int32_t *n_shared_bodies,
                                 int32_t *n_boundary, int32_t *cons_tile, int32_t *cons_lane);

/* ---- ray casts: a question put to the solids the collider knows -- the ground and the three shapes of egs_shape.
 * Ray.  Origin o[3] and direction d[3] are finite and d != 0.  d is not normalised by the library: t is in units of d,
 *   so a unit d gives metres.  tmax >= 0, +inf allowed.  The ray is the set o + t d, 0 <= t <= tmax.
 * Result per ray.  body (int32): -2 no hit, -1 the ground, otherwise the global body index.  t (fp64): tmax on a miss.
 *   normal[3]: the unit outward normal of the surface at the hit; (0, 0, 0) on a miss and where the origin is inside the
 *   solid (then t = 0).
 * Solids.  The collider's conventions; R is taken as orthonormal and is not renormalised.  All of it runs in fp64 on
 *   the fp64 pos / R / side / shape arrays the collider reads, whatever the world's solve precision, without fused
 *   multiply-adds, a . b = (a0 b0 + a1 b1) + a2 b2.
 *   Entering root of |w + t d|^2 = r^2 (used for every ball and, in the perpendicular components, for the capsule's
 *     side): the perpendicular-offset form, which does not cancel for a far origin.  s = (w . d) / (d . d),
 *     m = w - s d, disc = r^2 - m . m; no root unless disc >= 0; t = -s - sqrt(disc / (d . d)); it counts iff t >= 0.
 *   Ground: the half space z < 0.  Origin inside iff o_z < 0 strictly.  Otherwise a hit iff d_z < 0, at
 *     t = o_z / (-d_z), normal (0, 0, 1).  A level ray (d_z == 0) never hits, at any height.
 *   Sphere: side row (d, d, d), r = d / 2, R not read.  w = o - c.  Inside iff w . w < r^2.  Otherwise the entering
 *     root; normal = (w + t d) normalised.
 *   Box: the slab test in the box frame, p = R^T (o - c), q = R^T d, h = side / 2.  An axis with q_k == 0 exactly
 *     rejects iff |p_k| > h_k; otherwise its roots are (-h_k - p_k) / q_k and (h_k - p_k) / q_k.  t_in = the largest
 *     near root, t_out = the smallest far root.  A hit iff t_in <= t_out and t_out > 0.  t_in < 0: the origin is inside.
 *     Otherwise t = t_in, normal = -sgn(q_k) (column k of R) for the axis k that gave t_in (lowest k on a tie).
 *   Capsule: side row (d, d, l), u = column 2 of R, r = d / 2, e = (l - d) / 2: the union of the cylinder
 *     {|s| <= e, rho <= r} and the balls at c -+ e u.  w = o - c.  Inside iff |w - s u|^2 < r^2 with
 *     s = min(max(w . u, -e), e), the collider's clamp.  Otherwise the smallest of three candidates' t, compared with
 *     strict < in this order: the side, the ball at end 0 (c - e u), the ball at end 1.  Side: w' = w - (w . u) u,
 *     d' = d - (d . u) u, the entering root of |w' + t d'|^2 = r^2 with d' . d' in the place of d . d; it does not
 *     exist when d' . d' == 0 exactly, and counts only when t >= 0 and (w . u) + t (d . u) lies in [-e, e]; normal =
 *     (w' + t d') normalised.  A ball: the sphere's entering root and normal about its centre.
 * Choosing among solids.  The smallest computed t with t <= tmax; a tie goes to the ground first, then to the lowest
 *   body index; a solid that holds the origin counts with t = 0, so an origin inside several reports the first of them
 *   in that order.  The answer therefore does not depend on the order in which bodies are visited.
 * On a surface, along a face, through an edge -- each falls the way the comparisons above say, in fp64:
 *   origin on the ground plane (o_z == 0): not inside; looking down it hits at t = 0, level or up it misses.
 *   origin on a sphere (w . w == r^2 in fp64): not inside; it hits only if the rounded root is >= 0, so a ray leaving
 *     outwards misses and one heading inwards hits at t = 0 or misses by the last bit -- a root of -1 ulp is a miss.
 *   origin on a box face: t_in == 0 is a hit at t = 0 with that face's normal, whether the ray heads in or runs along
 *     the face inside the other two slabs (q_k == 0 and |p_k| == h_k is not rejected); leaving outwards t_out == 0 misses.
 *   a ray through a box edge or corner: two or three near roots tie, the lowest axis gives the normal; if rounding
 *     makes t_in > t_out the ray misses.
 *   a grazing ray (disc == 0) hits; the seam of a capsule: side and ball give the same point, the side wins a tie;
 *   a ray exactly along a capsule's axis has no side candidate and hits an end ball at its pole.
 *   t == tmax is a hit.  A hit at t = -0.0 (a root (0) / (negative)) is reported as computed.
 * A bounding-sphere rejection may run before the exact tests and never changes a result (its bound is inflated beyond
 *   the rounding of the tests); by default it runs where an ensemble holds more than 128 bodies on average, and
 *   EGS_RAY_CULL=0 / 1 in the environment forces it off / on.
 * Frames.  A ray may be attached to a body b of its own ensemble (ray_body[i] = b, -1 = world frame): o, d are then in
 *   b's frame, the device forms o_w = c_b + R_b o (each component c + ((R0 o0 + R1 o1) + R2 o2)) and d_w = R_b d from
 *   the state it holds at that moment, and body b is not tested: a sensor follows its carrier with no read-back and
 *   never sees its own hull.
 * Ensembles.  In a batched world every ray names its ensemble; it sees that ensemble's bodies and the ground, nothing else.
 *
 * egs_cast_rays: host arrays, one ensemble, as egs_update_contacts_shapes takes them (shape NULL = boxes; shapes and
 *   sides checked by the same rules).  ray_body [n_rays] or NULL = world frame; normal [n_rays][3] or NULL.
 *   n_rays = 0 is EGS_OK.
 * egs_world_set_rays: stores the table on the device; n_rays = 0 drops it.  ray_ens [n_rays], non-decreasing, is
 *   required in a batched world and may be NULL in a plain one; ray_body holds global body indices.  The table
 *   survives egs_world_set_bodies, steps, re-plans and the stabilise entries.
 * egs_world_cast_rays: one launch on the world's stream against the state the device holds now, one read-back, one
 *   synchronise; *n_out (may be NULL) = the table's size.  Valid after egs_world_set_bodies.  Casting reads the world
 *   and writes nothing the steps read.
 * EGS_ERR_INVALID, with nothing changed and no output written: a required array NULL; a non-finite o or d, a zero d; a
 *   negative or NaN tmax; a ray_ens out of range or not non-decreasing; a ray_body out of range or outside the ray's
 *   ensemble; max_rays smaller than the table; a cast with no table.                                               */
egs_status egs_cast_rays(egs_context *ctx, int32_t n_bodies, const double *pos, const double *R,
                         const double *side_lengths, const int32_t *shape /*or NULL = boxes*/,
                         int32_t n_rays, const int32_t *ray_body /*[n_rays] or NULL = world frame*/,
                         const double *origin, const double *dir, const double *tmax,
                         int32_t *hit_body, double *t, double *normal /*[n_rays][3] or NULL*/);
egs_status egs_world_set_rays(egs_world *w, int32_t n_rays, const int32_t *ray_ens /*NULL: plain world*/,
                              const int32_t *ray_body, const double *origin, const double *dir, const double *tmax);
egs_status egs_world_cast_rays(egs_world *w, int32_t max_rays, int32_t *n_out,
                               int32_t *hit_body, double *t, double *normal);

#ifdef __cplusplus
}
#endif
#endif
