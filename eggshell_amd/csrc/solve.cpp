// solve.cpp -- the solve driver behind egs_problem_solve / _step and the world: which kernels one launch runs
// (SweepSchedule / choose_sweep, applying policy.h), the launch itself, the residual metric, the fixed-count and
// tolerance-terminated loops of the reference (do_solve) and their per-ensemble form for batched worlds
// (do_solve_batch).  No extern "C" entry lives here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>

#include "policy.h"
#include "problem.h"
#include "stabilize.h"

namespace egs {
namespace {

// Which kernels one solve launch runs.  Every policy switch of the sweep is read here, once per launch (tests change
// them between calls in one process), and nowhere else; launch_solve_t dispatches on the answer.
struct SweepSchedule {
  bool quad = false;        // 4 lanes per constraint (planq) instead of 1 (plan)
  bool timetable = false;   // the plan's static timetable (step_device.h, quad_solve.hip) instead of tickets
  int iso = 0;              // SolveArgs::iso: the isotropic-body variant of the 1-lane tile kernels
  int group = 1;            // tiles per workgroup of step_solve_kernel
  bool linsym = false;      // step_solve_kernel's LINSYM form
  bool assemble = false;    // ... with the assembly in its prologue (egs_problem_step)
  bool defer = false;       // ... which stores no system: the problem defers it (problem.h: ensure_system)
  bool pair = false;        // ... in its PAIR form: one update on a lane pair (step_pair.hip)
  bool chain = false;       // ... whose steady loop keeps a pair's accumulators in registers between its two updates (CHAIN)
  bool share = false;       // ... and a thread one linear block and one pair of weights for both constraints (SHARE)
  bool face = false;        // ... on a thread pair per box face: four updates behind one barrier, 128 threads per tile (FACE)
  bool face_lean = false;   // ... in its LEAN form: fewer held products, 168 VGPRs, six tiles per CU (policy.h: face_form_policy)
  int face_tiles = kFaceTilesPerCu;   // ... at this many resident tiles per CU (policy.h; EGS_STEP_FACE_TILES)
  FaceSplit split;          // ... with the last split.tiles tiles cut after sweep split.s1 (policy.h: face_split_policy)
  long face_slots = 0;      // ... the workgroups of that launch the GPU holds at once (EGS_STEP_FACE_SLOTS)
  bool face_persistent = false;   // ... on that many persistent workgroups that take pieces: split, or more tiles than slots
  bool started = false;     // the solve starts from a given x0 (problem.h: start_active), not from rhs
  bool friction = false;    // the kernels' friction forms: SolveArgs::mu is the problem's (problem.h: friction)
  int steady = 0;           // SolveArgs::steady: step_solve_kernel's steady-state loop (it applies at group 1, no snapshots)
  int oversize = -1;        // OversizeSchedule of the launch's oversize islands, -1: it has none
  // the bits of the kernels that ran (egs_schedule_flags); fill_stats adds those of the problem's plans
  uint32_t flags() const {
    return (iso ? EGS_SCHED_ISO : 0) | (timetable ? EGS_SCHED_STATIC : 0) | (linsym ? EGS_SCHED_LINSYM : 0) |
           (assemble ? EGS_SCHED_FUSED_ASSEMBLY : 0) | (defer ? EGS_SCHED_DEFERRED_SYSTEM : 0) |
           (started ? EGS_SCHED_START : 0) | (friction ? EGS_SCHED_FRICTION : 0) | (pair ? EGS_SCHED_PAIR : 0) |
           (chain ? EGS_SCHED_CHAIN : 0) | (share ? EGS_SCHED_SHARE : 0) |
           (face ? EGS_SCHED_FACE : 0) | (split.tiles > 0 ? EGS_SCHED_FACE_SPLIT : 0) |
           (face_lean ? EGS_SCHED_FACE_LEAN : 0);
  }
};

// hist: the launch records per-sweep snapshots; resume: it continues the previous launch; offer_assembly: the caller
// has not assembled the system and hands the assembly to the launch if its kernel can take it.
SweepSchedule choose_sweep(egs_problem *p, int method, int sweeps, bool hist, bool resume, bool offer_assembly) {
  SweepSchedule s;
  s.started = p->start_active;
  s.friction = p->friction;
  s.quad = p->use_quad && method != EGS_JACOBI;
  if (!s.quad) ensure_tile_plan(p);
  const Plan &pl = s.quad ? p->planq : p->plan;
  const char *se = std::getenv("EGS_STEP");   // 0 / 1: tickets / the timetable wherever the plan has levels
  s.timetable = method != EGS_JACOBI && pl.levels_ok && pl.n_tiles > 0 && (se ? std::atoi(se) != 0 : timetable_pays(pl, sweeps));
  if (s.quad) return s;
  // the timetable kernel's steady-state loop, on wherever the kernel has it; EGS_STEP_STEADY=0 keeps the general loop
  const char *ye = std::getenv("EGS_STEP_STEADY");
  s.steady = s.timetable && !(ye && std::atoi(ye) == 0);
  if (!pl.global.empty()) s.oversize = method == EGS_JACOBI ? kAllGlobal : p->oversize;
  if (pl.n_tiles > 0 && p->minv_iso && pl.block == 256) {
    const char *ie = std::getenv("EGS_ISO");   // 2: the variant wherever the bodies allow it (experiments)
    // the ticket kernel's isotropic variant has no registers to spare for the snapshots; the timetable kernel has an
    // instantiation of its own for them
    s.iso = (!hist || s.timetable) && ((ie && std::atoi(ie) == 2) || iso_schedule_pays(p->m, p->ctx->cu_count, p->precision));
  }
  if (!s.timetable || !s.iso || hist) return s;
  // The CU holds three fp64 (168 VGPRs) resp. four fp32 (128) isotropic tiles.  Walking them on one clock pays for
  // the four fp32 tiles (C4: 0.281 ms against 0.368); with three fp64 tiles the 12-wavefront barrier costs more than
  // the collisions it avoids (C3 x 24: 1.06 ms against 0.95), so fp64 keeps GROUP = 1.  EGS_STEP_GROUP=k forces k.
  const bool f32 = p->precision == EGS_F32;
  const char *ge = std::getenv("EGS_STEP_GROUP");
  const int g = ge && std::atoi(ge) >= 1 ? std::atoi(ge) : f32 ? 4 : 1;
  s.group = f32 ? (g >= 4 ? 4 : g >= 2 ? 2 : 1) : (g >= 3 ? 3 : 1);
  // one linear block for both sides (step_solve.hip: LINSYM); EGS_ISO_LINSYM=0 disables the form
  const char *le = std::getenv("EGS_ISO_LINSYM");
  s.linsym = !f32 && s.group == 1 && p->lin_neg && p->linsym_bodies == 1 && !(le && std::atoi(le) == 0);
  // ... with the assembly in its prologue: a fresh launch in which every constraint is a lane of some tile.
  // EGS_FUSED_ASSEMBLY=0 keeps assemble_kernel.  The ASSEMBLE form starts from rhs: a started solve is not offered it.
  // Its sweep projects with a contact's bounds as literals and reads no lo, hi or is_eq (step_solve.hip), so the
  // list must hold no joint at all.  LINSYM already implies it (lin_neg: no two-body joint; linsym_bodies: a body on
  // side 1, where a one-body joint has none), but the kernel depends on it, so it is required here by name.
  // A friction step is not offered it either: that form sits at 168 VGPRs with nothing spare for the coefficient
  // (DESIGN.md section 4g), so the step runs assemble_kernel and the LINSYM friction sweep.
  const char *fe = std::getenv("EGS_FUSED_ASSEMBLY");
  s.assemble = offer_assembly && s.linsym && p->contacts_only && !s.friction && !resume && !solve_takes_start(p) && pl.global.empty() && !(fe && std::atoi(fe) == 0);
  // ... which stores no system (problem.h: ensure_system).  EGS_STEP_DEFER_SYSTEM=0 keeps the eager stores.
  const char *de = std::getenv("EGS_STEP_DEFER_SYSTEM");
  s.defer = s.assemble && !(de && std::atoi(de) == 0);
  // ... on a lane pair per update, where the plan's half-wavefronts each hold one phase (plan.h: pairable).
  // EGS_STEP_PAIR=0 keeps one lane per constraint.
  const char *pe = std::getenv("EGS_STEP_PAIR");
  s.pair = s.assemble && pl.pairable && !(pe && std::atoi(pe) == 0);
  // ... with the accumulators of a pair in registers from the first of its two updates to the second, where the pair
  // holds consecutive updates of the same two bodies (plan.h: chained).  The form is the PAIR kernel's steady loop, so
  // it goes with that loop.  EGS_STEP_CHAIN=0 keeps the LDS round trip.
  const char *ce = std::getenv("EGS_STEP_CHAIN");
  s.chain = s.pair && pl.chained && s.steady && !(ce && std::atoi(ce) == 0);
  // ... and one linear block and one pair of weights per thread for both constraints of the pair, where the two have
  // the same contact normal bit for bit (problem.h: share_normals, decided here once per constraint upload or plan,
  // never for descriptors written on the device).  EGS_STEP_SHARE=0 keeps both copies.
  const char *he = std::getenv("EGS_STEP_SHARE");
  if (s.chain && p->share_normals == egs_problem::kShareUndecided) decide_share_normals(p);
  s.share = s.chain && p->share_normals == 1 && !(he && std::atoi(he) == 0);
  // ... and the four contact points of a face on one thread pair, where the plan lays them 32 lanes apart with nothing
  // else on their bodies inside a block of four steps (plan.h: faced) and all four carry one normal (problem.h:
  // face_normals).  The form has the forward sweep of the store-free launch without restitution; backward SOR, the
  // storing launch and the restitution twin keep SHARE.  EGS_STEP_FACE=0 keeps SHARE everywhere;
  // EGS_STEP_FACE_TILES=3|4 sets the resident tiles per CU.
  const char *ae = std::getenv("EGS_STEP_FACE"), *te = std::getenv("EGS_STEP_FACE_TILES");
  s.face = s.share && pl.faced && p->face_normals && method == EGS_GAUSS_SEIDEL && s.defer && !p->restitution &&
           !(ae && std::atoi(ae) == 0);
  // ... in its LEAN form (six tiles per CU) where the policy predicts the shorter launch for it and a tile's LDS request
  // fits six to a CU.  EGS_STEP_FACE_LEAN=0 keeps the present kernels everywhere, =1 takes the lean ones wherever FACE
  // holds and the request fits; EGS_STEP_FACE_TILES=6 asks for the lean form too.  Where the tiles per CU or the slot
  // count are given, the policy (which compares the two forms at their own slot counts) is not asked.
  const char *ne = std::getenv("EGS_STEP_FACE_LEAN"), *ke = std::getenv("EGS_STEP_FACE_SLOTS");
  const int tiles_env = te ? std::atoi(te) : 0, lean_env = ne ? std::atoi(ne) : -1;
  if (s.face && lean_env != 0 && face_lds_bytes(pl.max_slots, true, kFaceLeanTilesPerCu) != 0) {
    if (lean_env == 1 || tiles_env == kFaceLeanTilesPerCu) s.face_lean = true;
    else if (lean_env < 0 && !te && !ke)
      s.face_lean = face_form_policy(pl.n_tiles, p->ctx->cu_count, pl.max_depth, pl.max_period, sweeps).lean;
  }
  if (s.face_lean) s.face_tiles = kFaceLeanTilesPerCu;
  if (tiles_env == 3 || tiles_env == 4) s.face_tiles = tiles_env;
  // ... split in time where the last round would leave half the resident slots empty or more (policy.h).
  // EGS_STEP_FACE_SPLIT=0 keeps one workgroup per tile; EGS_STEP_FACE_SPLIT_FORCE=h,s1 splits the last h tiles after s1
  // sweeps whatever the policy says (tests, experiments).  EGS_STEP_FACE_SLOTS=k stands for the resident slots, in the
  // policy and as the grid of the persistent launch (tests: no small scene has more tiles than the GPU has slots).
  const char *xe = std::getenv("EGS_STEP_FACE_SPLIT"), *xf = std::getenv("EGS_STEP_FACE_SPLIT_FORCE");
  s.face_slots = ke && std::atol(ke) > 0 ? std::atol(ke) : (long)p->ctx->cu_count * s.face_tiles;
  if (s.face && !(xe && std::atoi(xe) == 0)) {
    long h = 0, s1 = 0;
    if (xf && std::sscanf(xf, "%ld,%ld", &h, &s1) == 2) s.split = face_split_forced(pl.n_tiles, h, s1, sweeps);
    else if (!xf) s.split = face_split_policy(pl.n_tiles, s.face_slots, pl.max_depth, pl.max_period, sweeps);
    // ... and persistent workgroups on the whole-tile list wherever the tiles take more than one round: with a
    // workgroup per tile the hardware refills freed slots late.  EGS_STEP_FACE_PERSIST=0 keeps
    // the persistent form for split launches alone.
    const char *re = std::getenv("EGS_STEP_FACE_PERSIST");
    s.face_persistent = s.split.tiles > 0 || (face_persist_pays(pl.n_tiles, s.face_slots) && !(re && std::atoi(re) == 0));
  }
  return s;
}

// The problem's system, solution and accumulators as the solve and residual kernels read them (kernels.h; SolveArgs and
// GlobalArgs name them alike); hist: the per-sweep snapshots too.  The friction coefficients go with them exactly while
// friction is on, which is what selects the kernels' friction forms (choose_sweep reports it).
template <typename ARGS, typename REAL>
void system_args(ARGS &a, const egs_problem *p, REAL cfm, bool hist) {
  a.m = p->m; a.n_bodies = p->n;
  a.Minv = real<REAL>(p->Minv_r);
  a.J0 = real<REAL>(p->J0); a.J1 = real<REAL>(p->J1);
  a.is_eq = p->is_eq.p;
  a.lo = real<REAL>(p->lo); a.hi = real<REAL>(p->hi);
  a.rhs = real<REAL>(p->rhs);
  a.x = real<REAL>(p->x); a.acc = real<REAL>(p->acc);
  a.wres = real<REAL>(p->wres);
  a.error_flag = p->error_flag.p;
  a.mu = p->friction ? real<REAL>(p->mu) : nullptr;
  a.cfm = cfm; a.spin_limit = spin_limit();
  if (hist) { a.hist_x = real<REAL>(p->hist_x); a.hist_acc = real<REAL>(p->hist_acc); }
}

// The plan's fields are the launch's.
template <typename REAL>
SolveArgs<REAL> solve_args(const egs_problem *p, REAL cfm, bool hist) {
  SolveArgs<REAL> a{};
  a.body0 = p->body0.p; a.body1 = p->body1.p;
  system_args(a, p, cfm, hist);
  return a;
}

// ... and as the all-global kernels read them, on the tile plan's oversize islands
template <typename REAL>
GlobalArgs<REAL> global_args(const egs_problem *p, REAL cfm, bool hist) {
  GlobalArgs<REAL> g{};
  g.cons = p->gcons.p; g.mg = (int)p->plan.global.size(); g.per_lane = 1;
  system_args(g, p, cfm, hist);
  g.B0 = real<REAL>(p->gB0); g.B1 = real<REAL>(p->gB1);
  g.D = real<REAL>(p->gD); g.den = real<REAL>(p->gden);
  g.dx = real<REAL>(p->gdx);
  g.tickets = p->gtickets.p;
  return g;
}

// The work of a persistent FACE launch: the piece list (built and uploaded when its key changes: never inside a step
// otherwise), the ticket counter and the tiles' flags.  Neither is reset between launches: the counter only grows and
// the kernel subtracts what it stood at, the flags carry the launch's epoch (on a wrap they are cleared, as the
// granules' tags are).
FaceWork face_work(egs_problem *p, int n_tiles, long slots, FaceSplit f, int sweeps) {
  hipStream_t st = p->ctx->stream;
  const long key[5] = {n_tiles, slots, f.tiles, f.s1, sweeps};
  if (!std::equal(key, key + 5, p->face_key)) {
    face_piece_list(n_tiles, slots, f, sweeps, p->h_face_pieces);
    p->face_pieces.alloc(p->h_face_pieces.size());
    HIPCHK(hipMemcpyAsync(p->face_pieces.p, p->h_face_pieces.data(), p->h_face_pieces.size() * sizeof(FacePiece),
                          hipMemcpyHostToDevice, st));
    std::copy(key, key + 5, p->face_key);
  }
  const size_t words = 1 + (size_t)n_tiles;
  if (p->face_sync.cap < words) {
    p->face_sync.alloc(words);
    HIPCHK(hipMemsetAsync(p->face_sync.p, 0, p->face_sync.cap * sizeof(uint32_t), st));
    p->face_ticket_base = 0;
    p->face_epoch = 0;
  }
  if (++p->face_epoch == 0) {   // the epoch wrapped: old flags could match again
    HIPCHK(hipMemsetAsync(p->face_sync.p + 1, 0, (p->face_sync.cap - 1) * sizeof(uint32_t), st));
    p->face_epoch = 1;
  }
  FaceWork w{};
  w.pieces = p->face_pieces.p;
  w.counter = p->face_sync.p;
  w.flags = p->face_sync.p + 1;
  w.ticket_base = p->face_ticket_base;
  w.epoch = p->face_epoch;
  w.n_pieces = (int32_t)p->h_face_pieces.size();
  w.n_workgroups = (int32_t)std::min<long>(w.n_pieces, slots);
  // every piece is drawn once, and every workgroup draws one ticket past the list before it ends (modulo 2^32, as the
  // counter itself)
  p->face_ticket_base += (uint32_t)w.n_pieces + (uint32_t)w.n_workgroups;
  return w;
}

// The timetable sweep of the one-lane plan: exactly one of the four launchers of the step units (kernels.h), as the
// schedule says.  An assembling launch (sc.assemble: fp64, `assemble` given) also leaves the problem's record of the
// system it assembled.
template <typename REAL>
void launch_timetable(egs_problem *p, const SweepSchedule &sc, SolveArgs<REAL> &a, int method, int sweeps,
                      const AssembleArgs *assemble) {
  const int n_tiles = p->plan.n_tiles;
  hipStream_t st = p->ctx->stream;
  if (!sc.assemble) {
    launch_step_solve<REAL>(a, method, n_tiles, p->plan.block, sc.group, sc.linsym, st);
    return;
  }
  if constexpr (sizeof(REAL) == 8) {
    a.assemble = *assemble;
    if (sc.face) {
      FaceWork w = sc.face_persistent ? face_work(p, n_tiles, sc.face_slots, sc.split, sweeps) : FaceWork{};
      w.host_stall = p->h_flag_dev;
      // the step's velocities from the epilogue, where egs_problem_step offers them and every body is in some tile (one
      // in none still moves by dt W f: velocity_kernel's).  EGS_STEP_FACE_VELOCITY=0 keeps velocity_kernel.
      const char *ve = std::getenv("EGS_STEP_FACE_VELOCITY");
      if (p->step_velocity == egs_problem::kVelocityOffered && p->plan_covers_bodies && !(ve && std::atoi(ve) == 0)) {
        w.v6 = p->v6.p;
        p->step_velocity = egs_problem::kVelocityWritten;
      }
      launch_step_solve_face(a, n_tiles, sc.face_tiles, sc.face_lean, w, st);
    } else if (sc.pair) launch_step_solve_pair(a, method, n_tiles, !sc.defer, sc.chain, sc.share, st);
    else launch_step_solve_assemble(a, method, n_tiles, !sc.defer, st);
    // the system this launch assembled: stored, or the problem's to make on demand from the state it read
    p->sys_deferred = sc.defer;
    p->deferred_prev = false;
    p->deferred_dt = assemble->dt; p->deferred_erp = assemble->erp;
  }
}

template <typename REAL>
void launch_solve_t(egs_problem *p, int method, REAL cfm, REAL kscale, int sweeps, int resume, const AssembleArgs *assemble) {
  egs_context *ctx = p->ctx;
  const bool hist = p->hist_sweeps > 0;
  const SweepSchedule sc = choose_sweep(p, method, sweeps, hist, resume, assemble != nullptr);
  if (assemble && !sc.assemble)   // egs_problem_step asked choose_sweep for this launch before it skipped assemble_kernel
    throw std::logic_error("fused assembly offered to a launch that does not take it");
  p->last_sched = sc.flags();
  // the start of a fresh launch: the problem's x0, or NULL: rhs (Q7)
  const REAL *x0 = (p->start_active && !resume) ? real<REAL>(p->start) : nullptr;
  record_kernel_event(ctx, true);
  // oversize islands accumulate in global memory (all bodies on the all-global kernel, shared
  // bodies of patches): from zero, unless this launch continues the previous one
  if (sc.oversize >= 0 && !resume)
    HIPCHK(hipMemsetAsync(p->acc.p, 0, (size_t)(p->n > 0 ? p->n : 1) * 6 * sizeof(REAL), ctx->stream));
  if (sc.quad || p->plan.n_tiles > 0) {
    const Plan &pl = sc.quad ? p->planq : p->plan;
    const DevicePlan &dp = sc.quad ? p->quad : p->tile;
    SolveArgs<REAL> a = solve_args(p, cfm, hist);
    a.lanes = dp.lanes.p;
    a.tile_nslots = dp.tile_nslots.p; a.tile_slot_off = dp.tile_slot_off.p; a.slot_body = dp.slot_body.p;
    a.wsB0 = real<REAL>(p->wsB0); a.wsB1 = real<REAL>(p->wsB1);
    a.wsD = real<REAL>(p->wsD); a.wsInv = real<REAL>(p->wsInv);
    a.kscale = kscale;
    a.sweeps = sweeps;
    a.resume = resume;
    a.x0 = x0;
    a.max_slots = pl.max_slots;
    a.iso = sc.iso;
    a.linsym = sc.linsym;
    a.steady = sc.steady;
    if (sc.quad) launch_cons_prepare<REAL>(a, ctx->stream);
    if (sc.timetable) {
      a.lane_level = dp.lane_level.p; a.tile_period = dp.tile_period.p; a.tile_depth = dp.tile_depth.p;
      a.runs = pl.runs ? 1 : 0;
    }
    if (sc.quad) {
      if (sc.timetable) launch_step_quad<REAL>(a, method, pl.n_tiles, pl.block, ctx->stream);
      else launch_quad_solve<REAL>(a, method, pl.n_tiles, pl.block, ctx->stream);
    } else if (sc.timetable) {
      launch_timetable(p, sc, a, method, sweeps, assemble);
    } else {
      launch_tile_solve<REAL>(a, method, pl.n_tiles, pl.block, ctx->stream);
    }
  }
  const bool patch = sc.oversize == kQuadPatches || sc.oversize == kLanePatches;
  if (patch && p->plan.block != 256)   // patch lanes are laid out for 256-thread workgroups
    throw std::logic_error("patch schedule built with a tile size other than 256");
  if (patch) {
    SolveArgs<REAL> a = solve_args(p, cfm, hist);
    a.lanes = p->patch.lanes.p; a.tile_nslots = p->patch.tile_nslots.p; a.tile_slot_off = p->patch.tile_slot_off.p;
    a.slot_body = p->patch.slot_body.p;
    a.kscale = kscale; a.sweeps = sweeps; a.resume = resume;
    a.x0 = x0;
    a.max_slots = p->plan.patch_max_slots;
    HIPCHK(hipMemsetAsync(p->gtickets.p, 0, sizeof(uint32_t) * (size_t)(p->n > 0 ? p->n : 1), ctx->stream));
    if (sc.oversize == kQuadPatches) {
      {   // hand-offs between patches as data-tagged granules (EGS_GRANULES=0: payload + flag, the round-2 protocol)
        const char *ge = std::getenv("EGS_GRANULES");
        if (!(ge && std::atoi(ge) == 0)) {
          const size_t bytes = (size_t)(p->n > 0 ? p->n : 1) * 6 * 16;
          if (p->ggran.cap < bytes) {
            p->ggran.alloc(bytes);
            HIPCHK(hipMemsetAsync(p->ggran.p, 0, bytes, ctx->stream));
            p->gran_epoch = 0;
          }
          if (++p->gran_epoch == 0) {     // the epoch wrapped: old tags could match again
            HIPCHK(hipMemsetAsync(p->ggran.p, 0, bytes, ctx->stream));
            p->gran_epoch = 1;
          }
          a.gran = p->ggran.p;
          a.gran_epoch = p->gran_epoch;
        }
      }
      if (std::getenv("EGS_TRACE_UPDATES") && sweeps > 0) {
        p->trace.alloc((size_t)sweeps * p->m);
        HIPCHK(hipMemsetAsync(p->trace.p, 0, (size_t)sweeps * p->m * sizeof(unsigned long long), ctx->stream));
        p->trace_sweeps = sweeps;
        a.trace = p->trace.p;
      }
      // 4 lanes per constraint, 1024-thread patches: the LDS hop is about half as long
      a.wsB0 = real<REAL>(p->wsB0); a.wsB1 = real<REAL>(p->wsB1);
      a.wsD = real<REAL>(p->wsD); a.wsInv = real<REAL>(p->wsInv);
      launch_cons_prepare<REAL>(a, ctx->stream);
      a.patch_runs = p->plan.patch_runs ? 1 : 0;
      launch_quad_patch_solve<REAL>(a, method, p->plan.n_patch_tiles, p->gtickets.p, ctx->stream);
    } else {
      launch_patch_solve<REAL>(a, method, p->plan.n_patch_tiles, p->gtickets.p, ctx->stream);
    }
    launch_global_wres<REAL>(global_args(p, cfm, false), ctx->stream);
  } else if (sc.oversize == kAllGlobal) {
    GlobalArgs<REAL> g = global_args(p, cfm, hist && method != EGS_JACOBI);
    g.kscale = kscale;
    g.sweeps = sweeps;
    g.resume = resume;
    g.x0 = x0;
    g.method = method;
    launch_global_solve<REAL>(g, p->global_max_blocks, ctx->stream);
  }
  record_kernel_event(ctx, false);
  HIPCHK(hipGetLastError());
}

void launch_solve(egs_problem *p, const egs_solve_params &prm, int sweeps, int resume, const AssembleArgs *assemble = nullptr) {
  ensure_minv_real(p);
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    const REAL ks = prm.method == EGS_SOR ? REAL(1) / (REAL)prm.omega : REAL(1);   // the scale in the solve's precision
    launch_solve_t<REAL>(p, prm.method, (REAL)prm.cfm, ks, sweeps, resume, assemble);
  });
}

// The reference's residual metric from one block of 4 x kResidualBlocks partial sums (residual_partials_kernel,
// hist_residual_kernel): block index outer, category inner.
double residual_metric(const double *part) {
  double sum[4] = {0, 0, 0, 0};
  for (int b = 0; b < kResidualBlocks; ++b)
    for (int k = 0; k < 4; ++k) sum[k] += part[4 * b + k];
  return std::sqrt(sum[0]) + (std::sqrt(sum[1]) + std::sqrt(sum[2]) + std::sqrt(sum[3]));
}

// ---- the stopping loop's schedule (tol > 0), shared by do_solve and do_solve_batch ----------------
// With recorded chunks the residual of x0 is not waited for: its partial sums ride on the first chunk's
// read-back and the chunk is launched at once (EGS_DEFER_RESIDUAL=0: read on its own).
bool defer_first_residual(const egs_solve_params *prm) {
  const char *e = std::getenv("EGS_DEFER_RESIDUAL");
  return prm->max_iters > 1 && !(e && std::atoi(e) == 0);
}
// Fast form, same result: sweeps run in chunks while the kernels record x and the per-body accumulators
// after every sweep ... on every schedule, oversize islands on the patch kernels or the all-global kernel
// included.  Only Jacobi on oversize islands, which is a launch per sweep anyway, takes the plain loop.
bool use_history(egs_problem *p, const egs_solve_params *prm) {
  const bool quad = p->use_quad && prm->method != EGS_JACOBI;
  if (!quad) ensure_tile_plan(p);
  return (quad || p->plan.global.empty() || prm->method != EGS_JACOBI) && prm->max_iters > 1;
}
// Up to 256 recorded sweeps per launch within 2 GiB of snapshots (24 C3 piles: 14 MB per sweep).  The first
// launch records at most 64 and every further one twice as many as the one before: a solve that converges
// early wastes little, a long one pays the timetable's fill and the read-back once per 256 sweeps.
struct ChunkSchedule {
  int K = 1, cur = 1;
  ChunkSchedule(const egs_problem *p, const egs_solve_params *prm) {
    const size_t rs = p->real_size(), m = (size_t)p->m, n = (size_t)(p->n > 0 ? p->n : 1);
    const size_t per_sweep = (3 * m + 6 * n) * rs;
    K = (int)std::min<size_t>(256, std::max<size_t>(1, (size_t(2048) << 20) / per_sweep));
    K = std::min(K, prm->max_iters);
    cur = std::min(K, 64);
  }
  int next(int left) {
    const int chunk = std::min(cur, left);
    cur = std::min(2 * cur, K);
    return chunk;
  }
};
// snapshot buffers for K sweeps; bodies without constraints never get a snapshot written: theirs stays zero
void prepare_history(egs_problem *p, int K) {
  const size_t rs = p->real_size(), m = (size_t)p->m, n = (size_t)(p->n > 0 ? p->n : 1);
  p->hist_x.alloc((size_t)K * 3 * m * rs);
  p->hist_acc.alloc((size_t)K * 6 * n * rs);
  HIPCHK(hipMemsetAsync(p->hist_acc.p, 0, (size_t)K * 6 * n * rs, p->ctx->stream));
}
// the snapshots are scratch of ONE call: a problem object that once ran a tolerance-terminated solve on a large
// system must not keep up to 2 GiB of HBM (and the page-locked mirror) for the rest of its life.  Small ones stay
// (a converging Chain re-solves every step); the stream-ordered free waits for the kernels above.
void release_large_history(egs_problem *p) {
  static const size_t keep_mb = [] { const char *e = std::getenv("EGS_HIST_KEEP_MB"); return e ? (size_t)std::atol(e) : (size_t)256; }();
  if (p->hist_x.bytes() + p->hist_acc.bytes() > (keep_mb << 20)) {
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    p->hist_x.release(); p->hist_acc.release(); p->hist_out.release();
  }
}

// One solve's start (egs_problem_set_start): decided before the first launch, in force until the solve returns.
// PREVIOUS takes its copy of x here, so x0 never aliases x; a problem without a lambda for its constraint list starts
// from rhs.  Launches outside a solve (accumulators_from_lambda) never see a start.
// pin: a tolerance-terminated solve of a list that holds a slider.  Its stopping test is first made on the start, and it
// leaves pinned rows (lo == hi, no equality row) out; a free slider's rail row is such a row, and where the start
// satisfies every other row (a world-side slider on a vertical rail: only the rail row has a right-hand side) the solve
// would return lambda_rail = rhs != 0 without a sweep.  So that solve always takes a start, rhs if it has no other, with
// every pinned rail row at its bound (launch_pin_start), the value the first sweep would give it.  The system is stored by
// then (tol > 0 never fuses the assembly).  Lists without a slider start as they always have.
struct StartScope {
  egs_problem *p;
  explicit StartScope(egs_problem *q, bool pin = false) : p(q) {
    bool take = p->m > 0 && solve_takes_start(p);
    const size_t bytes = (size_t)p->m * 3 * p->real_size();
    if (take && p->start_mode == EGS_START_PREVIOUS) {
      p->start.alloc(bytes);
      HIPCHK(hipMemcpyAsync(p->start.p, p->x.p, bytes, hipMemcpyDeviceToDevice, p->ctx->stream));
    }
    if (pin && p->m > 0) {
      if (!take) p->start.alloc(bytes);
      with_real(p, [&](auto r) {
        using REAL = decltype(r);
        launch_pin_start<REAL>(3 * p->m, take ? real<REAL>(p->start) : real<REAL>(p->rhs), p->kind.p, real<REAL>(p->lo),
                               real<REAL>(p->hi), real<REAL>(p->start), p->ctx->stream);
      });
      take = true;
    }
    p->start_active = take;
  }
  ~StartScope() { p->start_active = false; }
};

// The longest launch of a fixed-sweep solve: tickets are 32-bit counters that advance by cnt per sweep, and the static
// timetable counts time steps in a 32-bit int (see do_solve)
int fixed_chunk_max(const Plan &pl_used) {
  const int64_t by_ticket = (int64_t)0xF0000000u / (int64_t)std::max(1, pl_used.max_cnt) - 2;
  const int64_t by_clock = ((int64_t)0x7fffffff - 2 * (int64_t)std::max(1, pl_used.max_depth) - 2) / (int64_t)std::max(1, pl_used.max_period) - 2;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(by_ticket, by_clock), 0x7fffffff));
}

// every ensemble's residual of the states xs / as / ws into B.err
void batch_residual(egs_problem *p, BatchSolveState &B, double cfm, const int32_t *running, const void *xs, const void *as,
                    const void *ws, int sweeps) {
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    launch_seg_residual<REAL>(solve_args(p, (REAL)cfm, true), B.segs, running, static_cast<const REAL *>(xs),
                              static_cast<const REAL *>(as), static_cast<const REAL *>(ws), sweeps, B.err.p, p->ctx->stream);
  });
}

// the stopping test over B.err for the states xs / as (strides in elements per entry)
void batch_select(egs_problem *p, BatchSolveState &B, const egs_solve_params *prm, int sweeps, int first, int all_checked,
                  int init, const void *xs, size_t xstride, const void *as, size_t astride) {
  hipStream_t s = p->ctx->stream;
  HIPCHK(hipMemsetAsync(B.stop().n_running, 0, sizeof(int32_t), s));
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    launch_seg_select<REAL>(B.segs, B.stop(), B.err.p, sweeps, first, prm->max_iters, prm->check_every, prm->tol, all_checked,
                            init, static_cast<const REAL *>(xs), xstride, static_cast<const REAL *>(as), astride,
                            real<REAL>(B.fin_x), real<REAL>(B.fin_acc), s);
  });
}

// ONE read-back: the number of ensembles still running and the stall flag (cleared once seen).  Synchronises.
int batch_read_running(egs_problem *p, BatchSolveState &B, int *flag) {
  hipStream_t s = p->ctx->stream;
  const int E = B.segs.n_ens;
  HIPCHK(hipMemcpyAsync(B.h_ints.p + E, B.stop().n_running, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(B.h_ints.p + E + 1, p->error_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *flag = B.h_ints.p[E + 1];
  if (*flag) HIPCHK(hipMemsetAsync(p->error_flag.p, 0, sizeof(int32_t), s));
  return B.h_ints.p[E];
}

}  // namespace

void launch_residual(egs_problem *p) {
  ensure_system(p);   // the metric sorts the rows by lo, hi and is_eq
  const int rows = 3 * p->m;
  hipStream_t s = p->ctx->stream;
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    launch_residual_partials<REAL>(rows, real<REAL>(p->wres), real<REAL>(p->x), real<REAL>(p->lo), real<REAL>(p->hi), p->is_eq.p,
                                   p->friction ? real<REAL>(p->mu) : nullptr, p->res_partials.p, kResidualBlocks, s);
  });
}

// synchronises; returns the reference's residual metric and the error flag
double read_residual(egs_problem *p, int *err_flag) {
  double part[4 * kResidualBlocks];
  int32_t flag = 0;
  hipStream_t s = p->ctx->stream;
  HIPCHK(hipMemcpyAsync(part, p->res_partials.p, sizeof part, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&flag, p->error_flag.p, sizeof flag, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (flag) {   // reported to the caller now: clear the sticky word
    HIPCHK(hipMemsetAsync(p->error_flag.p, 0, sizeof(int32_t), s));
    HIPCHK(hipStreamSynchronize(s));
    *p->h_flag.p = 0;
  }
  if (err_flag) *err_flag = flag;
  return residual_metric(part);
}

egs_status validate_params(egs_context *ctx, const egs_solve_params *prm) {
  if (!prm) return fail(ctx, EGS_ERR_INVALID, "params is NULL");
  if (prm->method < 0 || prm->method > 2) return fail(ctx, EGS_ERR_INVALID, "unknown method");
  if (prm->max_iters < 0) return fail(ctx, EGS_ERR_INVALID, "max_iters < 0");
  if (prm->method == EGS_SOR && !(prm->omega > 0 && prm->omega < 2))
    return fail(ctx, EGS_ERR_INVALID, "SOR needs 0 < omega < 2 (sparse_iterations.cc:15)");
  return EGS_OK;
}

void fill_stats(egs_problem *p, egs_solve_stats *st) {
  if (!p->use_quad) ensure_tile_plan(p);
  const Plan &pl = p->use_quad ? p->planq : p->plan;   // islands and ticket periods agree between the two
  st->n_islands = pl.n_islands;
  st->n_tiles = pl.n_tiles;
  st->n_global = (int32_t)pl.global.size();
  st->reserved = p->use_quad ? 1 : 0;  // 1: 4-lanes-per-constraint schedule for GS/SOR
  st->schedule = (p->use_quad ? EGS_SCHED_QUAD : 0) | (p->last_sched & ~(egs_problem::kSchedRefinements | egs_problem::kSchedFullOnly | egs_problem::kSchedFormsOnly));
  if (!p->use_quad && !pl.global.empty())
    st->schedule |= p->oversize == kQuadPatches ? EGS_SCHED_QUAD_PATCHES : p->oversize == kLanePatches ? EGS_SCHED_LANE_PATCHES : EGS_SCHED_ALL_GLOBAL;
  st->tile_constraints = pl.block;
}

// The solve driver: sparse_iterations.cc:148-226.  assemble: egs_problem_step hands the assembly to the first launch
// (step_fuses_assembly).
egs_status do_solve(egs_problem *p, const egs_solve_params *prm, egs_solve_stats *stats, const AssembleArgs *assemble) {
  egs_context *ctx = p->ctx;
  if (egs_status st = validate_params(ctx, prm)) return st;
  if (!p->have_blocks) return fail(ctx, EGS_ERR_INVALID, "no system uploaded (set_blocks or assemble first)");
  if (p->m == 0) {  // sparse_iterations.cc:152-154
    p->last_iterations = 0;
    if (stats) { std::memset(stats, 0, sizeof *stats); fill_stats(p, stats); }
    return EGS_OK;
  }
  if (!assemble) ensure_system(p);   // this solve reads the stored system
  ensure_minv_real(p);   // also decides the isotropic fast path, hence the tile size
  if (!p->use_quad || prm->method == EGS_JACOBI) ensure_tile_plan(p);
  if (stall_seen(p)) return report_stall(p);   // an earlier asynchronous solve timed out
  const StartScope start(p, prm->tol > 0 && p->sliders);
  if (!(prm->tol > 0)) {
    // tickets are 32-bit counters that advance by cnt per sweep: very long runs
    // are cut into resumed launches so they cannot wrap
    // ... and the static timetable counts time steps in a 32-bit int (t_end = depth + period x sweeps,
    // step_device.h / quad_solve.hip): the chunk also keeps that below INT_MAX.  64-bit arithmetic, then the clamp.
    const int chunk_max = fixed_chunk_max(p->use_quad ? p->planq : p->plan);
    int done = 0;
    do {
      const int chunk = std::min(chunk_max, prm->max_iters - done);
      launch_solve(p, *prm, chunk, done > 0 ? 1 : 0, done > 0 ? nullptr : assemble);
      done += chunk;
    } while (done < prm->max_iters);
    p->last_iterations = prm->max_iters;
    p->have_lambda = true;
    p->residual_pending = !stats;   // nobody is looking: the reduction runs when egs_problem_get_stats asks
    // ... and a stall shows up at the next call or the next synchronising getter.  A solve that was one FACE launch
    // posts no copy: its kernel stores to the page-locked word itself (step_face.hip; the unsplit form has no wait)
    const bool face_alone = prm->max_iters <= chunk_max && (p->last_sched & EGS_SCHED_FACE) != 0;
    if (!stats && !face_alone) post_flag_copy(p);
    if (stats) {
      int flag = 0;
      launch_residual(p);
      stats->residual = read_residual(p, &flag);
      stats->iterations = prm->max_iters;
      stats->status = flag ? EGS_ERR_STALL : EGS_OK;
      fill_stats(p, stats);
      if (flag) return fail(ctx, EGS_ERR_STALL, "device ordering wait timed out");
    }
    return EGS_OK;
  }
  // tol > 0: x0 = rhs (or the problem's start), residual before iterating, then the reference's loop: one sweep,
  // one residual, stop at the first err <= tol (sparse_iterations.cc:204-221).
  const int every = prm->check_every > 0 ? prm->check_every : 1;
  int it = 0, flag = 0;
  launch_solve(p, *prm, 0, 0);
  launch_residual(p);
  // Should x0 already satisfy the test when its residual is deferred (from x0 = rhs it never does in practice; a
  // start taken from the previous step's lambda can) its state is simply produced again.
  const bool defer_first = defer_first_residual(prm);
  double err = 0.0;
  // one more kernel evaluates the stopping test of every recorded sweep and ONE read-back per chunk finds the
  // first sweep that satisfies it (use_history)
  const bool history = use_history(p, prm);
  const bool deferred = history && defer_first;
  if (!deferred) err = read_residual(p, &flag);
  if (history) {
    const size_t rs = p->real_size(), m = (size_t)p->m;
    ChunkSchedule sched(p, prm);
    const int K = sched.K;
    prepare_history(p, K);
    p->hist_out.alloc((size_t)K * kResidualBlocks * 4);
    // read-backs land in page-locked memory: a pageable destination makes each of the two copies per launch a
    // synchronous bounce through the runtime's staging buffer
    const size_t part_len = (size_t)K * kResidualBlocks * 4, first_len = (size_t)kResidualBlocks * 4;
    if (p->h_hist.cap < part_len + 1 + first_len) {
      if (p->h_hist.p) HIPCHK(hipStreamSynchronize(ctx->stream));   // the stream may still write to the old one
      p->h_hist.alloc(part_len + 1 + first_len);
    }
    double *part = p->h_hist.p;
    int32_t *h_f32 = reinterpret_cast<int32_t *>(part + part_len);
    double *first_part = part + part_len + 1;
    bool first_pending = deferred;
    if (deferred) {
      HIPCHK(hipMemcpyAsync(first_part, p->res_partials.p, first_len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      err = std::numeric_limits<double>::infinity();
    }
    while (!flag && err > prm->tol && it < prm->max_iters) {
      const int chunk = sched.next(prm->max_iters - it);
      p->hist_sweeps = chunk;
      launch_solve(p, *prm, chunk, 1);
      p->hist_sweeps = 0;
      auto residual_pass = [&](int write_sweep) {
        with_real(p, [&](auto r) {
          using REAL = decltype(r);
          launch_hist_residual<REAL>(solve_args(p, (REAL)prm->cfm, true), chunk, kResidualBlocks, p->hist_out.p, write_sweep, ctx->stream);
        });
      };
      residual_pass(0);
      HIPCHK(hipMemcpyAsync(part, p->hist_out.p, (size_t)chunk * kResidualBlocks * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipMemcpyAsync(h_f32, p->error_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      flag = *h_f32;
      if (flag) { HIPCHK(hipMemsetAsync(p->error_flag.p, 0, sizeof(int32_t), ctx->stream)); break; }
      if (first_pending) {      // the residual of x0, read with this chunk
        first_pending = false;
        const double e0 = residual_metric(first_part);
        if (!(e0 > prm->tol)) {      // x0 was the answer: produce its state again (lambda, accumulators, w, partial sums)
          launch_solve(p, *prm, 0, 0);
          launch_residual(p);
          err = e0;
          break;
        }
      }
      int stop = 0;   // first recorded sweep (1-based) at which the reference would stop
      double err_stop = 0, err_last = err;
      for (int sw = 1; sw <= chunk; ++sw) {
        const bool checked = ((it + sw) % every == 0) || (it + sw == prm->max_iters);
        if (!checked) continue;
        const double e = residual_metric(part + (size_t)(sw - 1) * kResidualBlocks * 4);
        err_last = e;
        if (!(e > prm->tol)) { stop = sw; err_stop = e; break; }   // as the loop condition: a NaN residual stops it too
      }
      if (stop > 0 && stop < chunk) {
        // the answer is the snapshot of sweep `stop`: lambda, accumulators, w
        const size_t off_x = (size_t)(stop - 1) * 3 * m * rs, off_a = (size_t)(stop - 1) * 6 * (size_t)p->n * rs;
        HIPCHK(hipMemcpyAsync(p->x.p, p->hist_x.p + off_x, 3 * m * rs, hipMemcpyDeviceToDevice, ctx->stream));
        if (p->n > 0)
          HIPCHK(hipMemcpyAsync(p->acc.p, p->hist_acc.p + off_a, 6 * (size_t)p->n * rs, hipMemcpyDeviceToDevice, ctx->stream));
        residual_pass(stop);
        it += stop;
        err = err_stop;
        break;
      }
      it += chunk;
      err = err_last;
      if (stop == chunk) break;   // the launch's own epilogue state is the answer
    }
    p->residual_pending = it > 0;   // res_partials still hold the sums of x0; x / wres are final
    release_large_history(p);
  } else {
    while (!flag && err > prm->tol && it < prm->max_iters) {
      const int chunk = std::min(every, prm->max_iters - it);
      launch_solve(p, *prm, chunk, 1);
      launch_residual(p);
      err = read_residual(p, &flag);
      it += chunk;
    }
  }
  p->last_iterations = it;
  p->have_lambda = !flag;
  if (stats) {
    stats->residual = err;
    stats->iterations = it;
    stats->status = flag ? EGS_ERR_STALL : EGS_OK;
    fill_stats(p, stats);
  }
  if (flag) return fail(ctx, EGS_ERR_STALL, "device ordering wait timed out");
  return EGS_OK;
}

// ---- batched worlds: the per-ensemble stopping rule ----------------------------
// A world of E > 1 independent ensembles (egs_world_create_batch) solves them in one system, and each
// ensemble must end with the lambda, sweep count and residual of a world holding only it.  Sweeps
// never cross ensembles, so every ensemble is swept until the last one stops; the stopping test runs
// per ensemble on the device (launch_seg_residual / launch_seg_select, kernels.h) and copies each
// ensemble's chosen state into fin_x / fin_acc, which become x / acc at the end.
// The solve of a batched world: do_solve's loops, each ensemble stopping on its own (sparse_iterations.cc:204-221).
// Enqueues the copy of the per-ensemble results into B.h_ints / B.h_res; the caller synchronises before reading them.
// active [E] (device, may be NULL): only these ensembles run the stopping test; the others are not checked and no
// state of theirs is selected (egs_world_stabilize's finished ensembles).  The sweeps still cover every ensemble, as
// they do for an ensemble that has stopped (section 4c of DESIGN.md); a fixed sweep count ignores active.
egs_status do_solve_batch(egs_problem *p, const egs_solve_params *prm, BatchSolveState &B, const int32_t *active) {
  egs_context *ctx = p->ctx;
  hipStream_t s = ctx->stream;
  if (egs_status st = validate_params(ctx, prm)) return st;
  if (!p->have_blocks) return fail(ctx, EGS_ERR_INVALID, "no system uploaded (set_blocks or assemble first)");
  const int E = B.segs.n_ens;
  const size_t rs = p->real_size(), m = (size_t)p->m, n = (size_t)(p->n > 0 ? p->n : 1);
  ensure_system(p);
  auto finish = [&]() {
    HIPCHK(hipMemcpyAsync(B.h_ints.p, B.stop().iterations, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(B.h_res.p, B.stop().residual, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, s));
  };
  B.err.alloc((size_t)E);
  if (!(prm->tol > 0)) {   // fixed sweep count: do_solve as it is, then every ensemble's residual of the final state
    if (egs_status st = do_solve(p, prm, nullptr)) return st;
    batch_residual(p, B, prm->cfm, nullptr, p->x.p, nullptr, p->wres.p, 1);
    launch_seg_fixed(B.segs, B.stop(), B.err.p, prm->max_iters, s);
    HIPCHK(hipGetLastError());
    finish();
    return EGS_OK;
  }
  ensure_minv_real(p);
  if (!p->use_quad || prm->method == EGS_JACOBI) ensure_tile_plan(p);
  if (stall_seen(p)) return report_stall(p);
  const StartScope start(p, p->sliders);   // (tol > 0 here)
  // the schedule of do_solve: same recorded-chunk decision, chunk sizes and deferred residual of x0
  const bool defer_first = defer_first_residual(prm);
  const bool history = use_history(p, prm);
  ChunkSchedule sched(p, prm);
  const int K = sched.K;
  // before the first launch: a growing DevBuf frees the old one
  B.err.alloc((size_t)std::max(K, 1) * E);
  B.fin_x.alloc(3 * m * rs);
  B.fin_acc.alloc(6 * n * rs);
  auto residual = [&](const int32_t *running, const void *xs, const void *as, const void *ws, int sweeps) {
    batch_residual(p, B, prm->cfm, running, xs, as, ws, sweeps);
  };
  // x0 = rhs (or the problem's start): every ensemble's residual before iterating; those that already pass stop at 0 sweeps
  launch_solve(p, *prm, 0, 0);
  residual(nullptr, p->x.p, nullptr, p->wres.p, 1);
  batch_select(p, B, prm, 1, 0, 1, 1, p->x.p, 0, p->acc.p, 0);
  if (active) launch_stab_seed_running(E, active, B.stop().running, B.stop().n_running, s);
  int it = 0, flag = 0;
  // as do_solve: with recorded chunks the count of x0 rides on the first chunk's read-back
  int running = (history && defer_first) ? E : batch_read_running(p, B, &flag);
  const int32_t *d_running = B.stop().running;
  if (history) {
    prepare_history(p, K);
    while (!flag && running > 0 && it < prm->max_iters) {
      const int chunk = sched.next(prm->max_iters - it);
      p->hist_sweeps = chunk;
      launch_solve(p, *prm, chunk, 1);
      p->hist_sweeps = 0;
      residual(d_running, p->hist_x.p, p->hist_acc.p, nullptr, chunk);
      batch_select(p, B, prm, chunk, it + 1, 0, 0, p->hist_x.p, 3 * m, p->hist_acc.p, 6 * n);
      running = batch_read_running(p, B, &flag);
      it += chunk;
    }
    release_large_history(p);
  } else {
    while (!flag && running > 0 && it < prm->max_iters) {
      const int chunk = std::min(prm->check_every > 0 ? prm->check_every : 1, prm->max_iters - it);
      launch_solve(p, *prm, chunk, 1);
      it += chunk;
      residual(d_running, p->x.p, nullptr, p->wres.p, 1);
      batch_select(p, B, prm, 1, it, 1, 0, p->x.p, 0, p->acc.p, 0);
      running = batch_read_running(p, B, &flag);
    }
  }
  if (flag) return fail(ctx, EGS_ERR_STALL, "device ordering wait timed out");
  // every ensemble has stopped: its state is in fin_x / fin_acc
  if (m > 0) HIPCHK(hipMemcpyAsync(p->x.p, B.fin_x.p, 3 * m * rs, hipMemcpyDeviceToDevice, s));
  if (p->n > 0) HIPCHK(hipMemcpyAsync(p->acc.p, B.fin_acc.p, 6 * (size_t)p->n * rs, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipGetLastError());
  p->last_iterations = it;
  p->have_lambda = true;
  p->residual_pending = false;
  finish();
  return EGS_OK;
}

// egs_problem_step assembles in the prologue of the solve launch (step_solve.hip: ASSEMBLE) exactly when do_solve is
// about to make ONE launch -- a fixed sweep count in one chunk -- and choose_sweep hands that launch the assembly.
// Anything else -- tol > 0, invalid parameters, more sweeps than one launch takes -- keeps assemble_kernel.
bool step_fuses_assembly(egs_problem *p, const egs_solve_params *prm) {
  if (p->m <= 0 || validate_params(nullptr, prm) != EGS_OK || prm->tol > 0) return false;
  ensure_minv_real(p);   // what do_solve does first: isotropy, LINSYM's body check, hence the tile plan
  return choose_sweep(p, prm->method, prm->max_iters, false, false, true).assemble && prm->max_iters <= fixed_chunk_max(p->plan);
}

// lambda -> the accumulators a_b = M_b^-1 sum_i J_ib^T lambda_i the velocity update reads: the solve
// kernels' own list-order accumulation (a launch without sweeps builds them from x0 = rhs, so lambda
// is lent to it as the rhs).
void accumulators_from_lambda(egs_problem *p) {
  egs_solve_params prm;
  egs_default_params(&prm);
  prm.method = EGS_GAUSS_SEIDEL; prm.tol = 0.0; prm.max_iters = 0;
  hipStream_t s = p->ctx->stream;
  ensure_system(p);
  const size_t bytes = (size_t)p->m * 3 * p->real_size();
  p->tmp_rows.alloc(bytes > 0 ? bytes : 1);
  HIPCHK(hipMemcpyAsync(p->tmp_rows.p, p->rhs.p, bytes, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(p->rhs.p, p->x.p, bytes, hipMemcpyDeviceToDevice, s));
  launch_solve(p, prm, 0, 0);     // x = "rhs" (= lambda), acc = sum B x in list order
  HIPCHK(hipMemcpyAsync(p->rhs.p, p->tmp_rows.p, bytes, hipMemcpyDeviceToDevice, s));
}

}  // namespace egs
