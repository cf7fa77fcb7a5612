// step_solve.hip -- projected Gauss-Seidel / backward SOR on a STATIC, time-stepped schedule.
//
// tile_solve_kernel finds the list order at run time: every lane polls its two bodies' tickets
// until it is its turn.  For a tile whose islands are regular (a pile of columns) that order is a
// fixed timetable: with level(c) = depth of constraint c in the list-order dependency DAG of one
// sweep and P = the largest level span of a body in the tile (plan.h), constraint c may run its
// update of sweep s at time
//     T(c, s) = level(c) + P * s                      (forward sweep; s = 0 is the x0 = rhs accumulation)
// because per body those times increase in list order and the first update of sweep s + 1 comes
// after the last one of sweep s.  The kernel walks the time steps with ONE workgroup barrier per
// step: the lanes due at that step run their update (accumulators in LDS, constants in VGPRs, the
// device functions of tile_solve_kernel: same arithmetic, same bits), everyone else goes straight to
// the barrier.  No tickets, no polling, no sleeping, no bounded spins -- and all lanes that are due
// together run in ONE pass (phase-major lane order puts them in the same wavefront), which the
// ticket kernel only approximates (23 of 32 lanes per pass).
// Backward SOR: the accumulation phase runs the list forward (steps 0 .. depth - 1), then the
// sweeps run it backward at depth + (depth - 1 - level) + P * (s - 1).
//
// GROUP > 1: one workgroup walks GROUP tiles on the same clock (the CU holds that many tiles anyway:
// registers).  Tiles that step independently collide on the SIMDs -- a pass is ~75 % instruction
// issue, two passes on one SIMD take 1.7 x as long (profiles/r02/microbench.json: update_iso_w8) --
// and in a regular tile the due wavefront is the same in every tile.  Sharing the barrier and
// rotating the lane -> wavefront assignment by the tile's number inside the group puts the GROUP
// passes of a time step on GROUP different SIMDs.
//
// LINSYM: the isotropic fp64 sweep when every two-body constraint has J1_lin = -J0_lin bit for bit and both bodies
// the same linear weight wl (a pile of equal boxes: contact.cc:66-99 builds [-Rn, ..] / [Rn, ..]), and every
// constraint has a body on side 1.  Then wl0 J0_lin = -(wl1 J1_lin) exactly (negation commutes with rounding), so
// load_cons leaves ONE linear block Jl = -J1_lin in J0_lin's registers and Bl = wl1 Jl, precomputed, in J1_lin's:
// side 1's linear residual products take -Jl and the linear accumulator updates take +Bl (side 0) / -Bl (side 1), all
// as source negations, which cost nothing.  An update forms only the 18 angular products w J on the fly instead of
// 36.  Same roundings in the same order as the plain kernel: the same bits (solve.cpp decides the preconditions).
//
// ASSEMBLE (LINSYM only): the prologue assembles the lane's constraint itself (assemble_device.h, the body of
// assemble_kernel) instead of reading back what assemble_kernel wrote: the blocks go from the assembly's registers into
// Cons, and load_cons (ASSEMBLED) finishes them.  The lane also stores J0, J1 (staged through LDS, stage_blocks), rhs,
// lo, hi, err and is_eq where assemble_kernel puts them, with the same bits, for whatever reads the system after the
// solve (get_blocks, the residual, matvec, later solves).  Nothing waits for these stores: they drain while the
// timetable runs.  Every constraint of the problem is a lane of some tile (solve.cpp: no oversize islands), so all of
// them are written.
// Every lane of this form is a contact (solve.cpp: choose_sweep requires a list without joints), so its sweep carries no
// lo, hi or eq: the projection takes a contact's bounds as literals (solve_device.h: project_contact, the same value
// as project() for every input).  The registers that frees hold side 0's nine angular products wa0 J0_ang, formed once
// after load_cons with the multiply an update would use (AngProducts below): the same bits, nine multiplies less per
// update.
// The steady-state loop (GROUP == 1, no snapshots, LINSYM or not ISO): between the first depth steps of a launch (the
// fill: lanes still wait for their first turn, or run the accumulation) and its last ones (the drain: lanes have run
// out of sweeps) every lane whose level matches the clock modulo P is due, in some sweep 1 .. sweeps.  There the
// kernel walks a second loop without the per-lane timetable: the clock, its phase t mod P and the loop bounds are
// scalar, a lane compares its phase with the clock's, and `due`, `sweep`, the accumulation branch and the history
// test are gone from the pass.  The bounds are the same for every lane of the workgroup (the tile's depth and period,
// the launch's sweeps): every wavefront meets the same barriers as in the single loop.  SolveArgs::steady = 0 (solve.cpp:
// EGS_STEP_STEADY=0) keeps the single loop.  The arithmetic of an update is the same code: the same bits.
//
// STORE_SYSTEM = false: none of that is stored -- a step reads none of it (the sweeps run from registers) -- and the
// problem remembers that its system is not materialised (problem.h: ensure_system runs assemble_kernel on demand).
//
// PAIR (ASSEMBLE only): an update runs on a lane pair, each lane holding one side of two constraints; described where
// it is written, before the kernel.  CHAIN (PAIR only): where the pair's two constraints are consecutive updates of the
// same two bodies, the steady loop hands their accumulators from the first update to the second in registers.  SHARE
// (CHAIN only): where the two also have one contact normal, the lane keeps their linear block and weights once.  FACE
// (a kernel of its own, step_solve_face_kernel): where the plan lays the four contact points of a face 32 lanes apart,
// a thread pair holds all four and runs their updates behind one barrier.  Where its tiles leave the last round of
// resident slots half empty or emptier, that launch is split in time (step_solve_face_pieces_kernel: a tile as two
// pieces, sweeps 1 .. s1 and s1 + 1 .. S, taken by ticket on persistent workgroups; policy.h: face_split_policy).
#include <algorithm>

#include "kernels.h"
#include "policy.h"
#include "solve_device.h"
#include "assemble_device.h"

namespace egs {

namespace {

// row_dot of row r with side 1's linear products taken as -Jl (dot3h's order, row_dot's sum order)
template <typename REAL>
__device__ __forceinline__ REAL linsym_row_dot(const Cons<REAL> &c, int r, const REAL *a0, const REAL *a1) {
  const REAL *j = c.J0 + 6 * r;
  const REAL p0 = dot3h(j, a0), p1 = dot3h(j + 3, a0 + 3);
  REAL p2 = (-j[0]) * a1[0];
  p2 = tfma(-j[1], a1[1], p2);
  p2 = tfma(-j[2], a1[2], p2);
  const REAL p3 = dot3h(c.J1 + 6 * r + 3, a1 + 3);
  return (p0 + p1) + (p2 + p3);
}
// row_residuals on the LINSYM registers
template <typename REAL>
__device__ __forceinline__ void linsym_residuals(const Cons<REAL> &c, const REAL *a0, const REAL *a1, const REAL *x,
                                                 REAL cfm, REAL *res) {
#pragma unroll
  for (int r = 0; r < 3; ++r) res[r] = c.rhs[r] - tfma(cfm, x[r], linsym_row_dot(c, r, a0, a1));
}

// How many of the 18 angular products wa J_ang of an update an ASSEMBLE instantiation forms once, after load_cons, and
// holds in registers through both loops (AngProducts): the largest count at which the instantiation keeps scratch 0
// and at most 168 VGPRs (three wavefronts per SIMD), found by compiling every count.  The
// registers are those the literal bounds of the contact projection freed (solve_device.h: project_contact).
// Nine = all of side 0, after which wa0 is not live in the loops; ten spill 12 bytes in every one of the four.
constexpr int kAngFree[2] = {9, 9};    // store-free (the headline): GS, backward SOR
constexpr int kAngStore[2] = {9, 9};   // storing
template <int METHOD, bool STORE_SYSTEM>
constexpr int ang_products() {
  return STORE_SYSTEM ? kAngStore[METHOD - 1] : kAngFree[METHOD - 1];
}

// Held products in the order side 0 then side 1, per side column-major as linsym_acc_add uses them: product i of a
// side is wa J[6 (i % 3) + 3 + i / 3].  HELD = 0: nothing is held.
template <typename REAL, int HELD>
struct AngProducts {
  REAL p[HELD > 0 ? HELD : 1];
  template <int SIDE>
  __device__ __forceinline__ void form(const REAL *J, REAL wa) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (9 * SIDE + i < HELD) {
        p[9 * SIDE + i] = wa * J[6 * (i % 3) + 3 + i / 3];   // the one multiply of linsym_acc_add: the same rounding
        asm volatile("" : "+v"(p[9 * SIDE + i]));             // opaque: held, not formed again where it is used
      }
    }
  }
};

// The weights of the products formed on the fly, opaque to the optimiser in place: the products stay in the update
// (not hoisted into registers of the compiler's choosing).  A side whose nine products are held needs no wa.
template <int HELD, typename REAL>
__device__ __forceinline__ void opaque_wa(Cons<REAL> &c) {
  if constexpr (HELD < 9) asm volatile("" : "+v"(c.wa0), "+v"(c.wa1));
  else if constexpr (HELD < 18) asm volatile("" : "+v"(c.wa1));
}

// acc_add_iso with the linear half from +-Bl (NEG: side 1) and the angular half w J formed on the fly, or taken from
// the held products (SIDE's first of them).  wa is the loop-carried register itself, made opaque by the caller: no
// copy per update.
template <bool NEG, int HELD = 0, typename REAL>
__device__ __forceinline__ void linsym_acc_add(REAL *a, const Cons<REAL> &c, const REAL *Ja, REAL wa, const REAL *d,
                                               const AngProducts<REAL, HELD> &h = AngProducts<REAL, HELD>()) {
  constexpr int SIDE = NEG ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const REAL *B = c.J1 + k;   // Bl[r][k] at B[6 r]
    REAL t = tfma(NEG ? -B[0] : B[0], d[0], a[k]);
    t = tfma(NEG ? -B[6] : B[6], d[1], t);
    a[k] = tfma(NEG ? -B[12] : B[12], d[2], t);
  }
#pragma unroll
  for (int k = 3; k < 6; ++k) {
    const int i = 9 * SIDE + 3 * (k - 3);
    REAL t = tfma(i < HELD ? h.p[i] : wa * Ja[k], d[0], a[k]);
    t = tfma(i + 1 < HELD ? h.p[i + 1] : wa * Ja[6 + k], d[1], t);
    a[k] = tfma(i + 2 < HELD ? h.p[i + 2] : wa * Ja[12 + k], d[2], t);
  }
}

// The ASSEMBLE prologue of one lane: K1-K4 for constraint cidx (J0 / J1 into c, for stage_blocks and load_cons), rhs,
// err, lo, hi and is_eq to global memory where assemble_kernel puts them (24 B per lane and array: a few lines per
// store instruction), rhs into c.  STORE = false: into c only.  The bounds do not go into c: the sweep of this form
// projects with a contact's literals.
template <bool STORE, bool REST>
__device__ __forceinline__ void assemble_lane(const AssembleArgs &G, int cidx, Cons<double> &c) {
  double e[3], lo[3], hi[3], u0[6], u1[6];
  bool eq[3];
  assemble_one<false>(G, cidx, c.J0, c.J1, e, lo, hi, eq, u0, u1);   // contacts only (choose_sweep): no angular block
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    // REST: restitution on the normal row (G.rest is set), here in the prologue only
    if (REST && r == 2) c.rhs[r] = assemble_rhs_bounce_t<false>(G, cidx, 0.0, 0.0, c.J0, c.J1, e, u0, u1);
    else c.rhs[r] = assemble_rhs(G, c.J0, c.J1, e, u0, u1, r);
    if constexpr (STORE) {
      reinterpret_cast<double *>(G.rhs)[(size_t)cidx * 3 + r] = c.rhs[r];
      G.err[(size_t)cidx * 3 + r] = e[r];
      reinterpret_cast<double *>(G.lo)[(size_t)cidx * 3 + r] = lo[r];
      reinterpret_cast<double *>(G.hi)[(size_t)cidx * 3 + r] = hi[r];
      G.is_eq[(size_t)cidx * 3 + r] = eq[r] ? 1 : 0;
    }
  }
}

// LDS per wavefront for stage_blocks: 64 rows of 18 doubles at a stride of 19 (conflict-free column walks)
constexpr int kStageWave = 64 * 19;

// J0 and J1 of the wavefront's lanes to global memory in assemble_kernel's layout, through LDS: stored from the lanes'
// registers, one instruction writes 64 rows 144 B apart, 64 cache lines; staged, lane l stores elements l, l + 64, ..
// of the wavefront's 64 x 18 block, about four whole rows per instruction.  The whole wavefront takes part (the
// inactive lanes store nothing); the staging area is the tile's LDS before the accumulators are set up.
__device__ __forceinline__ void stage_blocks(const AssembleArgs &G, double *stg, int lane, int cidx, bool active,
                                             const Cons<double> &c) {
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const double *J = side ? c.J1 : c.J0;
    double *out = reinterpret_cast<double *>(side ? G.J1 : G.J0);
    if (active) {
#pragma unroll
      for (int k = 0; k < 18; ++k) stg[lane * 19 + k] = J[k];
    }
    asm volatile("" ::: "memory");   // the wavefront's LDS operations run in order: no wait, only no reordering
#pragma unroll
    for (int it = 0; it < 18; ++it) {
      const int e = it * 64 + lane, row = e / 18, k = e - 18 * row;
      const double v = stg[row * 19 + k];
      const int ci = __shfl(cidx, row);
      if (ci >= 0) out[(size_t)ci * 18 + k] = v;
    }
    asm volatile("" ::: "memory");
  }
}

template <int METHOD>
__device__ __forceinline__ int timetable_end(int depth, int P, int sweeps, int resume) {
  if (METHOD == 2) return (resume ? 0 : depth) + (sweeps >= 1 ? depth + P * (sweeps - 1) : 0);
  const int n_phases = sweeps + (resume ? 0 : 1);   // updates per lane: the accumulation shares the forward timetable
  return n_phases >= 1 ? depth + P * (n_phases - 1) : 0;
}

// ---- PAIR (ASSEMBLE only): one update on a lane pair --------------------------------------------------------------
// In a regular pile tile a time step has 32 due lanes, all in one wavefront, and a pass costs the same with 32 active
// lanes as with 64.  Here thread l of wavefront w plays side s = l & 1 of TWO constraints, A = plan lane 64 w + (l >> 1)
// and B = plan lane 64 w + 32 + (l >> 1): it holds side s's block J_s, weights and accumulator address of both, and the
// even lane owns A's rhs, x, D and inv, the odd lane B's.  An update of A runs on both lanes of the pair: each forms its
// side's half of the three row sums, the halves cross by DPP, the owner alone projects, dx goes back by DPP and each
// lane updates and stores its own side's accumulator.  256 threads still hold 256 constraints, at the same registers.
// Same bits: the row sum keeps (p0 + p1) + (p2 + p3) (the odd owner adds the halves the other way round: commutative);
// side 1's linear terms take J1_lin itself, bit-equal to the -Jl of LINSYM, and its products wl1 J1_lin are -(wl1 Jl);
// side 0's take J0_lin = Jl and wl0 = wl1 (LINSYM's preconditions); a side without a body holds zeros and reads the
// world slot, whose half sums to the same +0.  The form is right for any plan; it pays where each half-wavefront of
// plan lanes shares one phase (plan.h: Plan::pairable), which is where solve.cpp takes it.

// How many of a side's 18 products w J (column-major as the accumulator update takes them: the nine linear first) a
// lane holds per constraint: the largest count at which the instantiation keeps scratch 0 and at most 168 VGPRs, found
// by compiling every count.  Six spill 12 to 20 bytes in every one of the four.
constexpr int kPairHeldFree[2] = {5, 5};    // store-free: GS, backward SOR
constexpr int kPairHeldStore[2] = {5, 5};   // storing
// ... and in the CHAIN form (below), whose steady loop carries a pair's six accumulators across a barrier: five spill
// 20 (GS) and 28 bytes (backward SOR), four 12 bytes in backward SOR
constexpr int kPairHeldChainFree[2] = {4, 3};
constexpr int kPairHeldChainStore[2] = {4, 3};
template <int METHOD, bool STORE_SYSTEM, bool CHAIN>
constexpr int pair_products() {
  if (CHAIN) return STORE_SYSTEM ? kPairHeldChainStore[METHOD - 1] : kPairHeldChainFree[METHOD - 1];
  return STORE_SYSTEM ? kPairHeldStore[METHOD - 1] : kPairHeldFree[METHOD - 1];
}

// one side of one constraint, as its lane holds it
template <int HELD>
struct PairSide {
  double J[18];   // 3x6 row-major; zeros where the constraint has no body on this side
  double wl, wa;
  double p[HELD > 0 ? HELD : 1];   // product i = w J[6 (i % 3) + i / 3]
  __device__ __forceinline__ void form() {
#pragma unroll
    for (int i = 0; i < 18; ++i) {
      if (i < HELD) {
        p[i] = (i < 9 ? wl : wa) * J[6 * (i % 3) + i / 3];   // the one multiply of acc_add_iso: the same rounding
        asm volatile("" : "+v"(p[i]));
      }
    }
  }
  // acc_add_iso with the held products taken from registers; the weights opaque in place, as in linsym_acc_add
  __device__ __forceinline__ void acc_add(double *a, const double *d) {
    if constexpr (HELD < 9) asm volatile("" : "+v"(wl), "+v"(wa));
    else if constexpr (HELD < 18) asm volatile("" : "+v"(wa));
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double w = k < 3 ? wl : wa;
      double t = tfma(3 * k < HELD ? p[3 * k] : w * J[k], d[0], a[k]);
      t = tfma(3 * k + 1 < HELD ? p[3 * k + 1] : w * J[6 + k], d[1], t);
      a[k] = tfma(3 * k + 2 < HELD ? p[3 * k + 2] : w * J[12 + k], d[2], t);
    }
  }
  // this side's half of row r's sum: p0 + p1 resp. p2 + p3 of row_dot
  __device__ __forceinline__ double half_dot(int r, const double *a) const {
    return dot3h(J + 6 * r, a) + dot3h(J + 6 * r + 3, a + 3);
  }
};

// SHARE (CHAIN only; solve.cpp takes it where problem.h: share_normals holds): A and B of a thread pair are contact
// points of one face pair of the same two bodies, with one normal.  A contact's linear block is -+Rn, and Rn comes from
// the normal alone (assemble_device.h: align_to_z(d + 3, Rn)), so on each side A's nine linear entries and B's are the
// same bits, and so are the weights: the same body.  The lane keeps them ONCE (PairLin: A's), with the linear products
// wl Jl, which then serve both constraints, and per constraint only the angular 3x3 with its held products (PairAng).
// Every operand is the double the CHAIN form reads in its place, every multiply the one PairSide does: the same bits.
// The registers that frees hold products: how many of the nine shared linear ones, and how many of the nine angular
// ones per constraint, found as the counts above were: all nine linear ones fit everywhere; a
// sixth angular one spills 12 (GS) or 20 bytes (backward SOR).
constexpr int kShareLinFree[2] = {9, 9};    // store-free: GS, backward SOR
constexpr int kShareLinStore[2] = {9, 9};   // storing
constexpr int kShareAngFree[2] = {5, 5};
constexpr int kShareAngStore[2] = {5, 5};
template <int METHOD, bool STORE_SYSTEM>
constexpr int share_lin_products() {
  return STORE_SYSTEM ? kShareLinStore[METHOD - 1] : kShareLinFree[METHOD - 1];
}
template <int METHOD, bool STORE_SYSTEM>
constexpr int share_ang_products() {
  return STORE_SYSTEM ? kShareAngStore[METHOD - 1] : kShareAngFree[METHOD - 1];
}

// the linear part of one side, for both constraints of the lane
template <int HELD>
struct PairLin {
  double J[9];    // the three rows' linear columns: PairSide's J[6 r + k] at 3 r + k
  double wl, wa;
  double p[HELD > 0 ? HELD : 1];   // product i = wl J[3 (i % 3) + i / 3]: PairSide's product i
  __device__ __forceinline__ void form() {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (i < HELD) {
        p[i] = wl * J[3 * (i % 3) + i / 3];
        asm volatile("" : "+v"(p[i]));
      }
    }
  }
};
// the angular part of one side of one constraint
template <int HELD>
struct PairAng {
  double J[9];    // PairSide's J[6 r + 3 + k] at 3 r + k
  double p[HELD > 0 ? HELD : 1];   // product i = wa J[3 (i % 3) + i / 3]: PairSide's product 9 + i
  __device__ __forceinline__ void form(double wa) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (i < HELD) {
        p[i] = wa * J[3 * (i % 3) + i / 3];
        asm volatile("" : "+v"(p[i]));
      }
    }
  }
};
// one side of one constraint as PairSide's users take it, from the two parts
template <int LHELD, int AHELD>
struct PairShared {
  PairLin<LHELD> &L;
  PairAng<AHELD> &G;
  __device__ __forceinline__ void acc_add(double *a, const double *d) const {
    if constexpr (LHELD < 9) asm volatile("" : "+v"(L.wl));
    if constexpr (AHELD < 9) asm volatile("" : "+v"(L.wa));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double t = tfma(3 * k < LHELD ? L.p[3 * k] : L.wl * L.J[k], d[0], a[k]);
      t = tfma(3 * k + 1 < LHELD ? L.p[3 * k + 1] : L.wl * L.J[3 + k], d[1], t);
      a[k] = tfma(3 * k + 2 < LHELD ? L.p[3 * k + 2] : L.wl * L.J[6 + k], d[2], t);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double t = tfma(3 * k < AHELD ? G.p[3 * k] : L.wa * G.J[k], d[0], a[3 + k]);
      t = tfma(3 * k + 1 < AHELD ? G.p[3 * k + 1] : L.wa * G.J[3 + k], d[1], t);
      a[3 + k] = tfma(3 * k + 2 < AHELD ? G.p[3 * k + 2] : L.wa * G.J[6 + k], d[2], t);
    }
  }
  __device__ __forceinline__ double half_dot(int r, const double *a) const {
    return dot3h(L.J + 3 * r, a) + dot3h(G.J + 3 * r, a + 3);
  }
};

// One update of a pair's constraint on both lanes.  own: this lane holds the constraint's scalars (c, x); BCAST: the
// quad_perm that hands the owner's value to both; GENERAL: the update may be the accumulation (sweep 0: dx = x).
// a: this lane's side's accumulator.  LOAD: read from LDS first; otherwise the caller hands it over in registers, as
// the pair's previous update left it.  STORE: written back to LDS; otherwise it stays in a for the pair's next update.
template <int METHOD, int BCAST, bool GENERAL, bool LOAD, bool STORE, typename SIDE>
__device__ __forceinline__ void pair_pass(SIDE &S, unsigned ac, double (&a)[6], bool has, bool own,
                                          const Cons<double> &c, double (&x)[3], int sweep, double cfm) {
  double dx[3];
  if constexpr (LOAD) load6(ac, a);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double h = S.half_dot(r, a);
    dx[r] = h + dpp_all<kQuadSwap>(h);   // the row sum, until the owner puts dx there
  }
  if (own) {
    if (GENERAL && sweep == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) dx[r] = x[r];
    } else {
      double res[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) res[r] = c.rhs[r] - tfma(cfm, x[r], dx[r]);
      update_rows<double, METHOD, true, false>(c, res, x, dx);
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) dx[r] = dpp_all<BCAST>(dx[r]);
  if (has) {
    S.acc_add(a, dx);
    if constexpr (STORE) store6(ac, a);
  }
}
// ... from LDS to LDS
template <int METHOD, int BCAST, bool GENERAL, typename SIDE>
__device__ __forceinline__ void pair_pass(SIDE &S, unsigned ac, bool has, bool own, const Cons<double> &c,
                                          double (&x)[3], int sweep, double cfm) {
  double a[6];
  pair_pass<METHOD, BCAST, GENERAL, true, true>(S, ac, a, has, own, c, x, sweep, cfm);
}

// lambda and w = A x - rhs of a pair's constraint, written by its owner
template <typename SIDE>
__device__ __forceinline__ void pair_epilogue(const SolveArgs<double> &A, const SIDE &S, unsigned ac, bool own,
                                              int cidx, const Cons<double> &c, const double *x) {
  double a[6];
  load6(ac, a);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double h = S.half_dot(r, a);
    const double ax = h + dpp_all<kQuadSwap>(h);
    if (own) {
      A.x[(size_t)cidx * 3 + r] = x[r];
      A.wres[(size_t)cidx * 3 + r] = tfma(A.cfm, x[r], ax) - c.rhs[r];
    }
  }
}

// a constraint's side as the loops take it: the PairSide, or (SHARE) the view of the shared parts
template <bool SHARE, typename P, typename V>
__device__ __forceinline__ auto &pair_side(P &p, V &v) {
  if constexpr (SHARE) return v;
  else return p;
}

// CHAIN (plans that are Plan::chained, plan.h; solve.cpp launches it on no other): A and B of a thread pair are
// consecutive updates of the same two bodies, so both lanes have ONE accumulator address for the two, and in the steady
// window the pair's first update (A forward, B in backward SOR) is due at even steps and its second at the step after
// (plan.cpp derives it).  The steady loop then walks two steps per iteration: the first's pass reads the accumulators
// and stores nothing, the second's takes them from the first's registers and stores.  Nothing else in the tile touches
// the two bodies in between (per body the timetable runs one update per step), so LDS holds the same doubles at every
// point where another lane reads them: the same bits.  A pair with an A and no B reads and stores in A's own step.
// The barrier between the two steps of an iteration stays, although on such a plan it orders nothing (the lanes due at
// steps 2 j and 2 j + 1 are the firsts and seconds of the same pairs): without it the step measured no faster
// (DESIGN.md section 5).
template <int METHOD, bool STORE_SYSTEM, bool CHAIN, bool REST, bool SHARE>
__device__ __forceinline__ void pair_step_solve(const SolveArgs<double> &A, unsigned char *smem) {
  constexpr int BLOCK = 256;
  const int tid = (int)threadIdx.x, tile = blockIdx.x;
  const int side = tid & 1, laneA = (tid & ~63) + ((tid & 63) >> 1), laneB = laneA + 32;
  const bool ownA = side == 0, ownB = side == 1;
  double *s_acc = reinterpret_cast<double *>(smem);
  const int nslots = A.tile_nslots[tile];
  const int32_t *slot_body = A.slot_body + A.tile_slot_off[tile];

  const int P = A.tile_period[tile], depth = A.tile_depth[tile];
  // the constraint this lane assembles and owns (A on the even lane, B on the odd one), and this lane's side of both;
  // of the descriptors only that stays: the epilogue reads the constraint numbers again
  const LaneDesc d = A.lanes[(size_t)tile * BLOCK + (side ? laneB : laneA)];
  const bool active = d.cidx >= 0;
  const bool has0 = active && d.slot0 != 0, has1 = active && d.slot1 != 0;
  bool activeA, activeB;
  unsigned acA, acB;
  {
    const LaneDesc o = A.lanes[(size_t)tile * BLOCK + (side ? laneA : laneB)];
    const bool other = o.cidx >= 0;
    const int mine = active ? (side ? d.slot1 : d.slot0) : 0, theirs = other ? (side ? o.slot1 : o.slot0) : 0;
    activeA = side ? other : active;
    activeB = side ? active : other;
    acA = lds_addr(s_acc + (side ? theirs : mine) * 6);
    acB = lds_addr(s_acc + (side ? mine : theirs) * 6);
    if constexpr (CHAIN) acB = acA;   // the same two bodies wherever B is active, and unused where it is not
  }
  const unsigned ac_world = lds_addr(s_acc);   // slot 0: no body on this side

  Cons<double> c = {};
  double x[3] = {0.0, 0.0, 0.0};
  if (active) assemble_lane<STORE_SYSTEM, REST>(A.assemble, d.cidx, c);
  if constexpr (STORE_SYSTEM) {
    stage_blocks(A.assemble, reinterpret_cast<double *>(smem) + (tid >> 6) * kStageWave, tid & 63, d.cidx, active, c);
    __syncthreads();   // every wavefront has read its staging area back
  }
  for (int s = tid; s < nslots; s += BLOCK) {   // a fresh solve: the accumulators start from zero
#pragma unroll
    for (int k = 0; k < 6; ++k) s_acc[s * 6 + k] = 0.0;
  }
  // D, inv and the weights from the whole constraint, as the one-lane form has them (no LINSYM rewrite: each side keeps
  // its own linear block)
  if (active) {
    load_cons<double, true, false, true>(A, d.cidx, has0, has1, has0 ? slot_body[d.slot0] : 0, has1 ? slot_body[d.slot1] : 0, c);
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = c.rhs[r];
  }
  // the sides change hands once: the even lane gives A's side 1 for B's side 0
  static_assert(CHAIN || !SHARE, "SHARE is a form of the CHAIN kernel");
  constexpr int HELD = pair_products<METHOD, STORE_SYSTEM, CHAIN>();
  constexpr int LHELD = share_lin_products<METHOD, STORE_SYSTEM>(), AHELD = share_ang_products<METHOD, STORE_SYSTEM>();
  PairSide<HELD> PA, PB;        // not SHARE
  PairLin<LHELD> L;             // SHARE: one linear part under two angular ones
  PairAng<AHELD> GA, GB;
  PairShared<LHELD, AHELD> VA{L, GA}, VB{L, GB};
  auto &SA = pair_side<SHARE>(PA, VA);
  auto &SB = pair_side<SHARE>(PB, VB);
  if constexpr (SHARE) {
    // the linear block and the weights move once, A's: B's are the same bits wherever B is active (solve.cpp)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double gl = dpp_all<kQuadSwap>(c.J1[6 * r + k]);
        const double ga = dpp_all<kQuadSwap>(side ? c.J0[6 * r + 3 + k] : c.J1[6 * r + 3 + k]);
        L.J[3 * r + k] = side ? gl : c.J0[6 * r + k];
        GA.J[3 * r + k] = side ? ga : c.J0[6 * r + 3 + k];
        GB.J[3 * r + k] = side ? c.J1[6 * r + 3 + k] : ga;
      }
    }
    const double gl = dpp_all<kQuadSwap>(c.wl1), ga = dpp_all<kQuadSwap>(c.wa1);
    L.wl = side ? gl : c.wl0;
    L.wa = side ? ga : c.wa0;
    L.form();
    GA.form(L.wa);
    GB.form(L.wa);
  } else {
#pragma unroll
    for (int k = 0; k < 18; ++k) {
      const double got = dpp_all<kQuadSwap>(side ? c.J0[k] : c.J1[k]);
      SA.J[k] = side ? got : c.J0[k];
      SB.J[k] = side ? c.J1[k] : got;
    }
    {
      const double gl = dpp_all<kQuadSwap>(side ? c.wl0 : c.wl1), ga = dpp_all<kQuadSwap>(side ? c.wa0 : c.wa1);
      SA.wl = side ? gl : c.wl0; SA.wa = side ? ga : c.wa0;
      SB.wl = side ? c.wl1 : gl; SB.wa = side ? c.wa1 : ga;
    }
    SA.form();
    SB.form();
  }
  int t_end = __builtin_amdgcn_readfirstlane(timetable_end<METHOD>(depth, P, A.sweeps, 0));
  __syncthreads();

  // the timetable of step_solve_kernel, once per constraint of the pair (identical in both lanes); the levels are read
  // here, behind the barrier, so that they occupy no register through the prologue
  const int levelA = A.lane_level[(size_t)tile * BLOCK + laneA], levelB = A.lane_level[(size_t)tile * BLOCK + laneB];
  int sweepA = 0, sweepB = 0;
  const int t0 = METHOD == 2 ? depth : 0;
  int dueA = (activeA && A.sweeps >= 0) ? levelA : 0x7fffffff, dueB = (activeB && A.sweeps >= 0) ? levelB : 0x7fffffff;
  constexpr int grid_acc = METHOD == 1 ? 1 : 0;
  int t_s = 0, t_e = 0;
  const int Ps = __builtin_amdgcn_readfirstlane(P);
  if (A.steady && Ps > 0) {
    const int ds = __builtin_amdgcn_readfirstlane(depth), t0s = METHOD == 2 ? ds : 0;
    t_s = grid_acc ? ds : t0s + ds - 1;
    t_e = min(t0s + Ps * (A.sweeps + grid_acc), t_end);
    if constexpr (CHAIN) {
      // whole pairs of steps from an even one (the period is even: a step's parity is its phase's): an odd t_s leaves
      // one more step to the fill, an odd length one more to the drain -- both loops take any step of the timetable
      t_s += t_s & 1;
      t_e -= (t_e - t_s) & 1;
    }
    if (t_e <= t_s) t_s = t_e = 0;
  }
  int t = 0, stop = t_e > t_s ? t_s : t_end;
  for (;;) {
    for (; t < stop; ++t) {
      if (dueA == t) {
        pair_pass<METHOD, kQuadEven, true>(SA, acA, acA != ac_world, ownA, c, x, sweepA, A.cfm);
        dueA = (METHOD == 2 && sweepA == 0) ? t0 + (depth - 1 - levelA) : dueA + P;
        if (++sweepA > A.sweeps) dueA = 0x7fffffff;
      }
      if (dueB == t) {   // after A's where both are due: they share no body then
        pair_pass<METHOD, kQuadOdd, true>(SB, acB, acB != ac_world, ownB, c, x, sweepB, A.cfm);
        dueB = (METHOD == 2 && sweepB == 0) ? t0 + (depth - 1 - levelB) : dueB + P;
        if (++sweepB > A.sweeps) dueB = 0x7fffffff;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    if (t >= t_end) break;
    if constexpr (CHAIN) {
      // steady, two steps per iteration behind one compare: the even phase of the pair's first update with the clock's
      const int bA = (METHOD == 2) ? t0 + depth - 1 - levelA : levelA;
      const int phF = activeA ? (bA % Ps) & ~1 : -1;   // backward, A is the second: its phase is odd, B's one less
      const bool has = acA != ac_world;
      int tp = t % Ps;
      double a[6];
      for (; t < t_e; t += 2) {
        const bool go = phF == tp;
        if constexpr (METHOD == 1) {
          if (go) {
            pair_pass<METHOD, kQuadEven, false, true, false>(SA, acA, a, has, ownA, c, x, 1, A.cfm);
            if (!activeB && has) store6(acA, a);   // an A without a B
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // that store
          __builtin_amdgcn_s_barrier();
          if (go && activeB) pair_pass<METHOD, kQuadOdd, false, false, true>(SB, acA, a, has, ownB, c, x, 1, A.cfm);
        } else {
          if (go && activeB) pair_pass<METHOD, kQuadOdd, false, true, false>(SB, acA, a, has, ownB, c, x, 1, A.cfm);
          __builtin_amdgcn_s_barrier();   // nothing was stored in this step
          if (go) {
            if (!activeB) load6(acA, a);   // an A without a B
            pair_pass<METHOD, kQuadEven, false, false, true>(SA, acA, a, has, ownA, c, x, 1, A.cfm);
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        tp = tp + 2 == Ps ? 0 : tp + 2;
      }
    } else {
      // steady: the two passes as two code copies, each behind one compare of the constraint's phase with the clock's
      const int phaseA = activeA ? ((METHOD == 2) ? t0 + depth - 1 - levelA : levelA) % Ps : -1;
      const int phaseB = activeB ? ((METHOD == 2) ? t0 + depth - 1 - levelB : levelB) % Ps : -1;
      int tp = t % Ps;
      for (; t < t_e; ++t) {
        if (phaseA == tp) pair_pass<METHOD, kQuadEven, false>(SA, acA, acA != ac_world, ownA, c, x, 1, A.cfm);
        if (phaseB == tp) pair_pass<METHOD, kQuadOdd, false>(SB, acB, acB != ac_world, ownB, c, x, 1, A.cfm);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        tp = tp + 1 == Ps ? 0 : tp + 1;
      }
    }
    // drain: each constraint's next update at or after t_e, from its level (read again: not held through the window)
    const int lvA = A.lane_level[(size_t)tile * BLOCK + laneA], lvB = A.lane_level[(size_t)tile * BLOCK + laneB];
    const int bA = (METHOD == 2) ? t0 + depth - 1 - lvA : lvA, bB = (METHOD == 2) ? t0 + depth - 1 - lvB : lvB;
    const int kA = t_e > bA ? (t_e - bA + Ps - 1) / Ps : 0, kB = t_e > bB ? (t_e - bB + Ps - 1) / Ps : 0;
    sweepA = kA + 1 - grid_acc;
    sweepB = kB + 1 - grid_acc;
    dueA = (!activeA || sweepA > A.sweeps) ? 0x7fffffff : bA + P * kA;
    dueB = (!activeB || sweepB > A.sweeps) ? 0x7fffffff : bB + P * kB;
    stop = t_end;
  }

  const int cidx = A.lanes[(size_t)tile * BLOCK + (side ? laneB : laneA)].cidx;   // the owner's: the one that is used
  if (activeA) pair_epilogue(A, SA, acA, ownA, cidx, c, x);
  if (activeB) pair_epilogue(A, SB, acB, ownB, cidx, c, x);
  for (int s = tid + 1; s < nslots; s += BLOCK) {
    const int body = slot_body[s];
    if (body < 0) continue;   // unused slot number
#pragma unroll
    for (int k = 0; k < 6; ++k) A.acc[(size_t)body * 6 + k] = s_acc[s * 6 + k];
  }
}

// ---- FACE (a refinement of SHARE; GS, store-free, no restitution): four updates on a thread pair ------------------
// A face pair of a pile has four contact points: four consecutive updates of the same two bodies, which the phase-major
// plan lays 32 lanes apart (plan.h: Plan::faced).  CHAIN keeps points 0 and 1 on one thread pair and hands the
// accumulators to points 2 and 3, in the next wavefront, through LDS and a barrier.  Here a tile's 256 plan lanes run on
// 128 threads: thread l of wavefront W plays side s = l & 1 of the FOUR constraints at plan lanes 128 W + 32 k + (l >> 1),
// k = 0 .. 3 (members A, B, C, D).  The even lane owns A and C (rhs, x, inv, D's off-diagonal), the odd lane B and D; the
// lane holds ONE linear part (A's: all four carry one normal, problem.h: face_normals) and four angular ones.  The steady
// loop walks four steps per iteration behind one compare: load, pass A, B, C, D on the same six registers, store, ONE
// barrier.  Inside a block of four steps nothing else in the tile touches the group's two bodies (Plan::faced says so
// per block and slot), so LDS holds the same doubles wherever another lane reads them, and the three barriers that
// stood inside the block ordered nothing.  Every operand is the double the SHARE form reads in its place, every product
// the multiply it does, in its order: the same bits.  A group with fewer than four members runs those it has.
// The fill, the drain and the accumulation take the general loop, which walks blocks the same way with `due` and `sweep`
// per group: right on any block of the timetable.
// Registers: up to 256 VGPRs at two wavefronts per SIMD (four 128-thread tiles per CU).  Held products: all nine linear ones
// and kFaceAng of the nine angular ones per member, the largest count that keeps scratch 0.
#ifndef EGS_FACE_ANG_PRODUCTS
#define EGS_FACE_ANG_PRODUCTS 6
#endif
constexpr int kFaceLin = 9, kFaceAng = EGS_FACE_ANG_PRODUCTS;
constexpr int kFaceThreads = 128, kFaceLanes = 256;

// The prologue in stages: each stage's loads are issued together, branch-free, and waited for once.
//   1. the four members' descriptors and member 0's level;
//   2. data[7] of both owned constraints and the group's two body numbers, taken ONCE, from member 0's slots through
//      slot_body (every active member of a faced plan has member 0's slots: plan.h, Plan::faced) -- neither body0 /
//      body1 nor kind is read: the launch is contacts only (solve.cpp: choose_sweep);
//   3. the two bodies' state once per lane: pos, v, w, Wf, Minv[0], Minv[21] of each side;
//   4. u0 and u1 once, then the two assemblies from those values (assemble_device.h: contact_blocks, side_u,
//      assemble_rhs -- the operations of assemble_one in their order) and load_cons for D and inv.
// An index that would not be valid is clamped to one that is (body 0 for a world side, constraint 0 for an idle
// member) and the value selected away afterwards: a world side gets the zeros it always got, an idle member zeros
// throughout.
struct FaceBodies {
  double pos0[3], pos1[3];
  double u0[6], u1[6];     // v/dt + W f per side, zeros for a world side
  double wl0, wa0, wl1, wa1;
  bool has0, has1;         // the group's: member 0 is active and has a body on the side
};
// stage 3 and the first half of stage 4; b0 / b1: the sides' body numbers, negative where there is none
__device__ __forceinline__ void face_bodies(const SolveArgs<double> &A, int b0, int b1, FaceBodies &B) {
  const AssembleArgs &G = A.assemble;
  const size_t i0 = (size_t)max(b0, 0), i1 = (size_t)max(b1, 0);
  double vw0[6], vw1[6], wf0[6], wf1[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    B.pos0[k] = G.pos[i0 * 3 + k];
    B.pos1[k] = G.pos[i1 * 3 + k];
    vw0[k] = G.v[i0 * 3 + k];
    vw1[k] = G.v[i1 * 3 + k];
    vw0[3 + k] = G.w[i0 * 3 + k];
    vw1[3 + k] = G.w[i1 * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    wf0[k] = G.Wf[i0 * 6 + k];
    wf1[k] = G.Wf[i1 * 6 + k];
  }
  B.wl0 = A.Minv[i0 * 36];
  B.wa0 = A.Minv[i0 * 36 + 21];
  B.wl1 = A.Minv[i1 * 36];
  B.wa1 = A.Minv[i1 * 36 + 21];
  __builtin_amdgcn_sched_barrier(0);   // every load above is issued before the first use below
  side_u(vw0, wf0, G.dt, B.u0);
  side_u(vw1, wf1, G.dt, B.u1);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    B.u0[k] = B.has0 ? B.u0[k] : 0.0;
    B.u1[k] = B.has1 ? B.u1[k] : 0.0;
  }
}
// one owned constraint from its descriptor d and the bodies' values: assembled and finished as the one-lane form does
// (the same J, rhs, D and inv); idle: zeros
__device__ __forceinline__ void face_assemble(const SolveArgs<double> &A, const double (&d)[7], const FaceBodies &B, bool active,
                                              Cons<double> &c, double (&x)[3]) {
  const bool has0 = active && B.has0, has1 = active && B.has1;
  double e[3];
  contact_blocks(d, B.pos0, B.pos1, has0, has1, c.J0, c.J1, e);
#pragma unroll
  for (int r = 0; r < 3; ++r) c.rhs[r] = assemble_rhs(A.assemble, c.J0, c.J1, e, B.u0, B.u1, r);
  c.wl0 = B.wl0; c.wa0 = B.wa0; c.wl1 = B.wl1; c.wa1 = B.wa1;
  load_cons<double, true, false, true, false, true>(A, 0, has0, has1, 0, 0, c);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    c.rhs[r] = active ? c.rhs[r] : 0.0;
    c.inv[r] = active ? c.inv[r] : 0.0;
    // opaque: formed here, in the prologue, as when loads pinned the assembly -- not sunk to the loops that use them
    asm volatile("" : "+v"(c.rhs[r]), "+v"(c.inv[r]));
    x[r] = c.rhs[r];
  }
  asm volatile("" : "+v"(c.D[3]), "+v"(c.D[6]), "+v"(c.D[7]));   // the off-diagonal entries a forward update takes
}
// the sides of the pair's two owned constraints (the even lane's c is E's, the odd lane's O's) change hands once: this
// lane's side of both; LIN: E's linear block and weights too
template <bool LIN>
__device__ __forceinline__ void face_sides(const Cons<double> &c, int side, PairLin<kFaceLin> &L, PairAng<kFaceAng> &GE,
                                           PairAng<kFaceAng> &GO) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double ga = dpp_all<kQuadSwap>(side ? c.J0[6 * r + 3 + k] : c.J1[6 * r + 3 + k]);
      GE.J[3 * r + k] = side ? ga : c.J0[6 * r + 3 + k];
      GO.J[3 * r + k] = side ? c.J1[6 * r + 3 + k] : ga;
      if constexpr (LIN) {
        const double gl = dpp_all<kQuadSwap>(c.J1[6 * r + k]);
        L.J[3 * r + k] = side ? gl : c.J0[6 * r + k];
      }
    }
  }
  if constexpr (LIN) {
    const double gl = dpp_all<kQuadSwap>(c.wl1), ga = dpp_all<kQuadSwap>(c.wa1);
    L.wl = side ? gl : c.wl0;
    L.wa = side ? ga : c.wa0;
  }
}

//
// PIECES: the launch split in time (policy.h: face_split_policy).  A workgroup is not a tile but a PIECE of the list W.pieces:
// a whole tile, or the first or the second part of a tile cut after sweep s1.  A first part runs the accumulation and
// sweeps 1 .. s1, stores lambda and the accumulators where the epilogue stores them anyway, and publishes the tile:
// every thread's stores, an agent-scope release, then one store of the launch's epoch to W.flags[tile].  A second part
// runs the same prologue (the same J, rhs, inv), then one thread waits for the flag (agent-scope acquire loads, a
// sleep between them, at most A.spin_limit of them: on overrun the workgroup sets A.error_flag and returns), and it
// resumes as step_solve_kernel resumes: x from A.x, the accumulators from A.acc, sweep 1 first, no accumulation, on the
// timetable of a resumed launch of S - s1 sweeps.  Each body's accumulator sees the same updates in the same order:
// the same bits.  Pieces are taken by ticket (one atomicAdd per piece on a counter that is never reset: the host
// passes what it stood at), not by blockIdx: a second part stands behind its first part in the list, so whoever holds
// the first part's ticket is already running and waits for nothing -- whatever order the workgroups are dispatched in.
// The workgroups are persistent: as many as the GPU holds at once (or as there are pieces), each taking piece after
// piece until a ticket is past the list.  With one workgroup per piece the hardware refilled the freed slots late and
// unevenly (a tenth of them stood empty while workgroups were pending) and the launch was no shorter than the unsplit
// one.
// Only the prologue, the loop bounds and the epilogue differ from the unsplit kernel: n_sweeps and resume are scalar.
// Returns false once the list is exhausted: the workgroup is done.
template <bool PIECES>
__device__ __forceinline__ bool face_step(const SolveArgs<double> &A, const FaceWork &W, unsigned char *smem, const int tid) {
  constexpr int METHOD = 1;
  int tile = blockIdx.x, n_sweeps = A.sweeps, resume = 0, kind = kFaceWhole;
  if constexpr (PIECES) {
    unsigned *s_word = reinterpret_cast<unsigned *>(smem);
    if (tid == 0) *s_word = atomicAdd(W.counter, 1u) - W.ticket_base;
    __syncthreads();
    const unsigned ticket = (unsigned)__builtin_amdgcn_readfirstlane((int)*s_word);
    __syncthreads();   // read by everyone before the prologue takes this LDS
    if (ticket >= (unsigned)W.n_pieces) return false;   // no piece left; nothing is read past the list
    const FacePiece pc = W.pieces[ticket];
    tile = __builtin_amdgcn_readfirstlane(pc.tile);
    resume = __builtin_amdgcn_readfirstlane(pc.resume);
    n_sweeps = __builtin_amdgcn_readfirstlane(pc.sweeps);
    kind = __builtin_amdgcn_readfirstlane(pc.kind);
  }
  const int side = tid & 1;
  const bool even = side == 0, odd = side == 1;
  // member k of this thread pair's group: plan lane lane0 + 32 k
  const size_t lane0 = (size_t)tile * kFaceLanes + (tid >> 6) * 128 + ((tid & 63) >> 1);
  double *s_acc = reinterpret_cast<double *>(smem);
  const int nslots = A.tile_nslots[tile];
  const int32_t *slot_body = A.slot_body + A.tile_slot_off[tile];
  const int P = A.tile_period[tile], depth = A.tile_depth[tile];

  // stage 1: the four members' descriptors and the group's level.  How many members the group has (member k is not
  // active without member k - 1), and this lane's side's accumulator: one address for all of them
  LaneDesc dm[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) dm[k] = A.lanes[lane0 + 32 * k];
  const int levelA = A.lane_level[lane0];
  int nm = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (dm[k].cidx >= 0) nm = k + 1;
  const int slot0 = dm[0].cidx >= 0 ? dm[0].slot0 : 0, slot1 = dm[0].cidx >= 0 ? dm[0].slot1 : 0;
  const unsigned ac = lds_addr(s_acc + (side ? slot1 : slot0) * 6);
  const bool has = ac != lds_addr(s_acc);   // slot 0, the world: no body on this side

  // the two constraints this lane owns: A and C on the even lane, B and D on the odd one
  const int own0 = side ? dm[1].cidx : dm[0].cidx, own1 = side ? dm[3].cidx : dm[2].cidx;
  // stage 2: their descriptors and the group's bodies (slot 0 holds -1)
  double d0[7], d1[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    d0[k] = A.assemble.data[(size_t)max(own0, 0) * 7 + k];
    d1[k] = A.assemble.data[(size_t)max(own1, 0) * 7 + k];
  }
  const int body0 = slot_body[slot0], body1 = slot_body[slot1];
  __builtin_amdgcn_sched_barrier(0);   // issued together, before the first wait
  // stage 3: the bodies' state, once per lane
  FaceBodies B;
  B.has0 = slot0 != 0;
  B.has1 = slot1 != 0;
  face_bodies(A, body0, body1, B);

  // stage 4: one assembly after the other.  The first's blocks wait in LDS (the accumulators' place, before they are
  // set up; element e of thread i at e * 128 + i) while the second is assembled from the same body values.
  PairLin<kFaceLin> L;
  PairAng<kFaceAng> GA, GB, GC, GD;
  Cons<double> c0 = {}, c1 = {};
  double x0[3], x1[3];
  face_assemble(A, d0, B, own0 >= 0, c0, x0);
  face_sides<true>(c0, side, L, GA, GB);
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    s_acc[e * kFaceThreads + tid] = L.J[e];
    s_acc[(9 + e) * kFaceThreads + tid] = GA.J[e];
    s_acc[(18 + e) * kFaceThreads + tid] = GB.J[e];
  }
  asm volatile("" ::: "memory");   // stored here, loaded below: not carried in registers
  // ... and the second assembly, which no longer loads, is not scheduled into the first: one at a time in the registers
  __builtin_amdgcn_sched_barrier(0);
  face_assemble(A, d1, B, own1 >= 0, c1, x1);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    L.J[e] = s_acc[e * kFaceThreads + tid];
    GA.J[e] = s_acc[(9 + e) * kFaceThreads + tid];
    GB.J[e] = s_acc[(18 + e) * kFaceThreads + tid];
  }
  face_sides<false>(c1, side, L, GC, GD);
  __syncthreads();   // every thread has its blocks back
  if (PIECES && resume) {
    // the second part of a split tile: behind both assemblies, so whatever waiting there is overlaps the prologue
    unsigned *s_word = reinterpret_cast<unsigned *>(smem);
    if (tid == 0) {
      uint32_t spins = 0;
      unsigned ok = 1;
      while (__hip_atomic_load(W.flags + tile, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != W.epoch) {
        if (++spins > A.spin_limit) { ok = 0; break; }
        __builtin_amdgcn_s_sleep(8);
      }
      *s_word = ok;
    }
    __syncthreads();
    const bool ok = __builtin_amdgcn_readfirstlane((int)*s_word) != 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every thread reads what the first part stored
    __syncthreads();   // the word is read before the accumulators take its place
    if (!ok) {
      // the piece is given up and the launch reports a stall; the workgroup goes on drawing, so that the counter ends
      // where the host expects it whatever happened
      if (tid == 0) atomicOr(A.error_flag, 1);
      return true;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      if (own0 >= 0) x0[r] = A.x[(size_t)own0 * 3 + r];
      if (own1 >= 0) x1[r] = A.x[(size_t)own1 * 3 + r];
    }
    for (int s = tid; s < nslots; s += kFaceThreads) {
      const int body = slot_body[s];
#pragma unroll
      for (int k = 0; k < 6; ++k) s_acc[s * 6 + k] = body >= 0 ? A.acc[(size_t)body * 6 + k] : 0.0;
    }
  } else {
    for (int s = tid; s < nslots; s += kFaceThreads) {   // a fresh solve: the accumulators start from zero
#pragma unroll
      for (int k = 0; k < 6; ++k) s_acc[s * 6 + k] = 0.0;
    }
  }
  // the held products, formed behind both assemblies: fewer registers live through the second one
  L.form();
  GA.form(L.wa);
  GB.form(L.wa);
  GC.form(L.wa);
  GD.form(L.wa);
  PairShared<kFaceLin, kFaceAng> SA{L, GA}, SB{L, GB}, SC{L, GC}, SD{L, GD};
  const int t_end = __builtin_amdgcn_readfirstlane(timetable_end<METHOD>(depth, P, n_sweeps, resume));
  __syncthreads();

  // The timetable of step_solve_kernel per GROUP: member k's level is A's + k and the period a multiple of 4, so the
  // four members are due at the four steps of one block, in one sweep (0: the accumulation), and the group's next
  // block comes a period later.  Both loops walk a block per iteration behind ONE barrier: what holds for the steady
  // window holds for the fill and the drain (Plan::faced is about every block), and a block past the timetable's end
  // finds no group due.
  // (a resumed piece starts at sweep 1: its grid has no accumulation, one update less)
  int sweep = resume, due = (nm > 0 && n_sweeps >= resume) ? levelA : 0x7fffffff;
  int t_s = 0, t_e = 0;
  const int Ps = __builtin_amdgcn_readfirstlane(P);
  if (A.steady && Ps > 0) {
    // whole blocks from a step = 0 (mod 4): a step's residue is its phase's
    t_s = (__builtin_amdgcn_readfirstlane(depth) + 3) & ~3;
    t_e = min(Ps * (n_sweeps + 1 - resume), t_end);
    t_e -= (t_e - t_s) & 3;
    if (t_e <= t_s) t_s = t_e = 0;
  }
  int t = 0, stop = t_e > t_s ? t_s : t_end;
  double a[6];
  for (;;) {
    for (; t < stop; t += 4) {
      if (due == t) {
        pair_pass<METHOD, kQuadEven, true, true, false>(SA, ac, a, has, even, c0, x0, sweep, A.cfm);
        if (nm > 1) pair_pass<METHOD, kQuadOdd, true, false, false>(SB, ac, a, has, odd, c0, x0, sweep, A.cfm);
        if (nm > 2) pair_pass<METHOD, kQuadEven, true, false, false>(SC, ac, a, has, even, c1, x1, sweep, A.cfm);
        if (nm > 3) pair_pass<METHOD, kQuadOdd, true, false, false>(SD, ac, a, has, odd, c1, x1, sweep, A.cfm);
        if (has) store6(ac, a);   // after the group's last active member
        due += P;
        if (++sweep > n_sweeps) due = 0x7fffffff;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    if (t >= t_end) break;
    {
      // steady: one compare of the phase of the group's first update with the clock's; no `due`, no `sweep`, no
      // accumulation branch
      const int phF = nm > 0 ? levelA % Ps : -1;
      int tp = t % Ps;
      for (; t < t_e; t += 4) {
        if (phF == tp) {
          pair_pass<METHOD, kQuadEven, false, true, false>(SA, ac, a, has, even, c0, x0, 1, A.cfm);
          if (nm > 1) pair_pass<METHOD, kQuadOdd, false, false, false>(SB, ac, a, has, odd, c0, x0, 1, A.cfm);
          if (nm > 2) pair_pass<METHOD, kQuadEven, false, false, false>(SC, ac, a, has, even, c1, x1, 1, A.cfm);
          if (nm > 3) pair_pass<METHOD, kQuadOdd, false, false, false>(SD, ac, a, has, odd, c1, x1, 1, A.cfm);
          if (has) store6(ac, a);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        tp = tp + 4 == Ps ? 0 : tp + 4;
      }
    }
    // drain: the group's next block at or after t_e, from its level (read again: not held through the window)
    const int lv = A.lane_level[lane0];
    const int n = t_e > lv ? (t_e - lv + Ps - 1) / Ps : 0;
    sweep = n + resume;   // update n on a grid whose update 0 is the accumulation, or (resumed) sweep 1
    due = (nm == 0 || sweep > n_sweeps) ? 0x7fffffff : lv + P * n;
    stop = t_end;
  }

  // the owner's constraint numbers, read again: not held through the loops
  const int cidx0 = A.lanes[lane0 + 32 * side].cidx, cidx1 = A.lanes[lane0 + 64 + 32 * side].cidx;
  if (nm > 0) pair_epilogue(A, SA, ac, even, cidx0, c0, x0);
  if (nm > 1) pair_epilogue(A, SB, ac, odd, cidx0, c0, x0);
  if (nm > 2) pair_epilogue(A, SC, ac, even, cidx1, c1, x1);
  if (nm > 3) pair_epilogue(A, SD, ac, odd, cidx1, c1, x1);
  for (int s = tid + 1; s < nslots; s += kFaceThreads) {
    const int body = slot_body[s];
    if (body < 0) continue;   // unused slot number
#pragma unroll
    for (int k = 0; k < 6; ++k) A.acc[(size_t)body * 6 + k] = s_acc[s * 6 + k];
  }
  if (PIECES && kind == kFaceFirst) {
    // publish: this thread's stores of lambda and the accumulators, released to the agent, before the tile's flag
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(W.flags + tile, W.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  return true;
}

__global__ void __launch_bounds__(kFaceThreads, 2) step_solve_face_kernel(const SolveArgs<double> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  face_step<false>(A, FaceWork{}, smem, (int)threadIdx.x);
}
// ... persistent workgroups, as many as the GPU holds at once: each takes piece after piece until the list is exhausted
__global__ void __launch_bounds__(kFaceThreads, 2) step_solve_face_pieces_kernel(const SolveArgs<double> A, const FaceWork W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int tid = (int)threadIdx.x;
  for (;;) {
    // A piece is compiled as the unsplit kernel's body is: the thread number and the launch's scalars are opaque per
    // piece, so nothing formed from them is carried in registers from one piece to the next (scratch stays 0).
    SolveArgs<double> B = A;
    asm volatile("" : "+v"(tid), "+s"(B.assemble.dt), "+s"(B.assemble.erp), "+s"(B.cfm));
    if (!face_step<true>(B, W, smem, tid)) break;
    __syncthreads();   // the epilogue has read the accumulators before the next ticket lands there
  }
}

// FRIC: the Coulomb pyramid on the constraints with mu >= 0 (solve_device.h: project_pyramid), A.mu not NULL.  The
// ASSEMBLE form has none (solve.cpp: choose_sweep).
template <typename REAL, int BLOCK, int METHOD, bool ISO, int GROUP, bool HIST, bool LINSYM = false, bool ASSEMBLE = false,
          bool STORE_SYSTEM = true, bool FRIC = false, bool PAIR = false, bool CHAIN = false, bool REST = false, bool SHARE = false>
__global__ void __launch_bounds__(BLOCK * GROUP, (ISO && GROUP == 1) ? (sizeof(REAL) == 4 ? 4 : 3) : 1) step_solve_kernel(const SolveArgs<REAL> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if constexpr (PAIR) {   // ASSEMBLE, fp64, 256-lane tiles (launch_step_solve_assemble)
    pair_step_solve<METHOD, STORE_SYSTEM, CHAIN, REST, SHARE>(A, smem);
    return;
  }
  constexpr int WAVES = BLOCK / 64;
  const int sub = GROUP > 1 ? (int)threadIdx.x / BLOCK : 0;                 // wavefront-uniform
  const int phys = GROUP > 1 ? (int)threadIdx.x % BLOCK : (int)threadIdx.x;
  // lane of the tile this thread plays: wavefront j of sub-tile k plays the tile's wavefront (j + k) mod WAVES
  const int tid = (GROUP > 1 && WAVES > 1) ? (((phys >> 6) + sub) % WAVES) * 64 + (phys & 63) : phys;
  const int tile = blockIdx.x * GROUP + sub;
  const bool valid = GROUP == 1 || tile < A.n_tiles;
  const int resume = ASSEMBLE ? 0 : A.resume;   // the ASSEMBLE form starts a solve (launch_step_solve_assemble)
  REAL *s_acc = reinterpret_cast<REAL *>(smem) + (size_t)sub * A.max_slots * 6;

  const int nslots = valid ? A.tile_nslots[tile] : 0;
  const int32_t *slot_body = A.slot_body + (valid ? A.tile_slot_off[tile] : 0);
  if constexpr (!ASSEMBLE) {   // the ASSEMBLE form stages its blocks in this LDS first (below)
    for (int s = tid; s < nslots; s += BLOCK) {
      const int body = slot_body[s];
#pragma unroll
      for (int k = 0; k < 6; ++k) s_acc[s * 6 + k] = (resume && body >= 0) ? A.acc[(size_t)body * 6 + k] : REAL(0);
    }
  }
  LaneDesc d;
  d.cidx = -1;
  if (valid) d = A.lanes[(size_t)tile * BLOCK + tid];
  const bool active = d.cidx >= 0;
  const bool has0 = active && d.slot0 != 0, has1 = active && d.slot1 != 0;
  const int slot0 = active ? d.slot0 : 0, slot1 = active ? d.slot1 : 0;
  const int level = valid ? A.lane_level[(size_t)tile * BLOCK + tid] : 0;
  const int P = valid ? A.tile_period[tile] : 1, depth = valid ? A.tile_depth[tile] : 1;

  Cons<REAL> c;
  REAL x[3] = {REAL(0), REAL(0), REAL(0)};
  // where x starts: the previous launch's x, a given start (A.x0), or NULL: rhs (Q7; always so in the ASSEMBLE form)
  const REAL *xs = ASSEMBLE ? nullptr : resume ? A.x : A.x0;
  if constexpr (ASSEMBLE) {
    if (active) assemble_lane<STORE_SYSTEM, REST>(A.assemble, d.cidx, c);
    if constexpr (STORE_SYSTEM) {
      stage_blocks(A.assemble, reinterpret_cast<double *>(smem) + (tid >> 6) * kStageWave, tid & 63, d.cidx, active, c);
      __syncthreads();   // every wavefront has read its staging area back
    }
    for (int s = tid; s < nslots; s += BLOCK) {   // a fresh solve: the accumulators start from zero
#pragma unroll
      for (int k = 0; k < 6; ++k) s_acc[s * 6 + k] = REAL(0);
    }
  }
  // ASSEMBLE: every lane is a contact (solve.cpp: choose_sweep), so the projection takes its bounds as literals, and
  // some of the angular products of B are formed once, after load_cons
  constexpr int HELD = ASSEMBLE ? ang_products<METHOD, STORE_SYSTEM>() : 0;
  AngProducts<REAL, HELD> held;
  if (active) {
    if constexpr (ASSEMBLE) load_cons<REAL, true, true, true>(A, d.cidx, has0, has1, has0 ? slot_body[slot0] : 0, has1 ? slot_body[slot1] : 0, c);
    else load_cons<REAL, ISO, LINSYM, false, FRIC>(A, d.cidx, has0, has1, has0 ? slot_body[slot0] : 0, has1 ? slot_body[slot1] : 0, c);
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = xs ? xs[(size_t)d.cidx * 3 + r] : c.rhs[r];
    if constexpr (HELD > 0) {
      held.template form<0>(c.J0, c.wa0);
      held.template form<1>(c.J1, c.wa1);
    }
  }
  const unsigned ac0 = lds_addr(s_acc + slot0 * 6), ac1 = lds_addr(s_acc + slot1 * 6);
  // snapshots for the per-sweep stopping test (kernels.h): is this lane the last update of its body in a sweep?
  const bool hist = HIST && A.hist_x != nullptr;   // isotropic variant: a separate instantiation, the plain one keeps its registers
  const bool last0 = (METHOD == 2) ? d.pos0 == 0 : d.pos0 + 1 == d.cnt0, last1 = (METHOD == 2) ? d.pos1 == 0 : d.pos1 + 1 == d.cnt1;

  // the clock runs until the longest timetable of the group has ended
  int t_end = 0;
#pragma unroll
  for (int k = 0; k < GROUP; ++k) {
    const int tk = blockIdx.x * GROUP + k;
    if (GROUP == 1 || tk < A.n_tiles) t_end = max(t_end, timetable_end<METHOD>(A.tile_depth[tk], A.tile_period[tk], A.sweeps, resume));
  }
  __syncthreads();

  // the timetable: `due` = the step of this lane's next update, `sweep` = which sweep that is (0 = accumulation)
  int sweep = resume ? 1 : 0;
  const int t0 = (METHOD == 2 && !resume) ? depth : 0;       // backward sweeps start after the forward accumulation
  int due = (METHOD == 2 && resume) ? depth - 1 - level : level;
  if (!active || sweep > A.sweeps) due = 0x7fffffff;
  // The steady window [t_s, t_e) (GROUP == 1, no snapshots; A.steady): with b = the step of the lane's first update on
  // the sweeps' grid (forward: level, the accumulation being update 0 of a fresh solve; backward: t0 + depth - 1 -
  // level) a lane is due at b + P k.  From t_s on every lane has b <= t, and on a fresh forward solve b + P <= t: the
  // accumulation is behind it; before t_e = t0 + P * (updates on the grid) even a lane with b = t0 + (t mod P), the
  // smallest b a tile can hold, has an update left, so a tile whose first level is not 0 only ends its sweeps later.
  // In between, the due lanes are exactly the active ones with b = t (mod P), all in a sweep 1 .. A.sweeps.  The
  // bounds come from the tile's depth and period and the launch's sweeps alone: every wavefront of the workgroup
  // meets the same t_end barriers.
  // The isotropic kernels without LINSYM sit at their register limit (168 / 128 VGPRs): a second loop would spill.
  constexpr bool STEADY = GROUP == 1 && (LINSYM || !ISO);
  const int grid_acc = (METHOD == 1 && !resume) ? 1 : 0;
  int t_s = 0, t_e = 0, Ps = 1;
  if constexpr (STEADY) {
    // workgroup-uniform by construction; said so, the clock and its bounds live in scalar registers
    t_end = __builtin_amdgcn_readfirstlane(t_end);
    Ps = __builtin_amdgcn_readfirstlane(P);
    if (A.steady && !hist && Ps > 0) {
      const int ds = __builtin_amdgcn_readfirstlane(depth), t0s = (METHOD == 2 && !resume) ? ds : 0;
      t_s = grid_acc ? ds : t0s + ds - 1;
      t_e = min(t0s + Ps * (A.sweeps + grid_acc), t_end);
      if (t_e <= t_s) t_s = t_e = 0;   // an empty window: the general loop alone
    }
  }
  int t = 0, stop = t_e > t_s ? t_s : t_end;
  for (;;) {
    for (; t < stop; ++t) {
      if (due == t) {
        REAL a0[6], a1[6];
        load12(ac0, ac1, a0, a1);
        REAL dx[3] = {REAL(0), REAL(0), REAL(0)};
        if (sweep == 0) {
#pragma unroll
          for (int r = 0; r < 3; ++r) dx[r] = x[r];
        } else {
          REAL res[3];
          if (LINSYM) linsym_residuals(c, a0, a1, x, A.cfm, res);
          else row_residuals(c, a0, a1, x, A.cfm, res);
          update_rows<REAL, METHOD, ASSEMBLE, FRIC>(c, res, x, dx);
        }
        if (LINSYM) {
          opaque_wa<HELD>(c);
          if (has0) { linsym_acc_add<false, HELD>(a0, c, c.J0, c.wa0, dx, held); store6(ac0, a0); }
          if (has1) { linsym_acc_add<true, HELD>(a1, c, c.J1, c.wa1, dx, held); store6(ac1, a1); }
        } else {
          if (has0) { acc_add_side0<ISO>(a0, c, dx); store6(ac0, a0); }
          if (has1) { acc_add_side1<ISO>(a1, c, dx); store6(ac1, a1); }
        }
        if (hist && sweep >= 1) {
          REAL *hx = A.hist_x + ((size_t)(sweep - 1) * A.m + d.cidx) * 3;
          hx[0] = x[0]; hx[1] = x[1]; hx[2] = x[2];
          if (has0 && last0) {
            REAL *ha = A.hist_acc + ((size_t)(sweep - 1) * A.n_bodies + slot_body[slot0]) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) ha[k] = a0[k];
          }
          if (has1 && last1) {
            REAL *ha = A.hist_acc + ((size_t)(sweep - 1) * A.n_bodies + slot_body[slot1]) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) ha[k] = a1[k];
          }
        }
        // next: the first backward sweep starts at t0 and runs the list from its end
        due = (METHOD == 2 && sweep == 0) ? t0 + (depth - 1 - level) : due + P;
        if (++sweep > A.sweeps) due = 0x7fffffff;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wavefront's accumulator stores have landed
      __builtin_amdgcn_s_barrier();
    }
    if (!STEADY || t >= t_end) break;
    // steady: one compare of the lane's phase with the clock's (scalar), no `due`, no `sweep`, no accumulation branch
    const int b = (METHOD == 2) ? t0 + depth - 1 - level : level;
    const int phase = active ? b % Ps : -1;
    int tp = t % Ps;
    for (; t < t_e; ++t) {
      if (phase == tp) {
        REAL a0[6], a1[6], res[3], dx[3];
        load12(ac0, ac1, a0, a1);
        if (LINSYM) linsym_residuals(c, a0, a1, x, A.cfm, res);
        else row_residuals(c, a0, a1, x, A.cfm, res);
        update_rows<REAL, METHOD, ASSEMBLE, FRIC>(c, res, x, dx);
        if (LINSYM) {
          opaque_wa<HELD>(c);
          if (has0) { linsym_acc_add<false, HELD>(a0, c, c.J0, c.wa0, dx, held); store6(ac0, a0); }
          linsym_acc_add<true, HELD>(a1, c, c.J1, c.wa1, dx, held);   // every active lane has side 1 (solve.cpp)
          store6(ac1, a1);
        } else {
          if (has0) { acc_add_side0<ISO>(a0, c, dx); store6(ac0, a0); }
          if (has1) { acc_add_side1<ISO>(a1, c, dx); store6(ac1, a1); }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      tp = tp + 1 == Ps ? 0 : tp + 1;
    }
    // drain: the lane's next update at or after t_e, from its level (read again: not held through the window)
    const int lv = A.lane_level[(size_t)tile * BLOCK + tid];
    const int bd = (METHOD == 2) ? t0 + depth - 1 - lv : lv;
    const int k = t_e > bd ? (t_e - bd + Ps - 1) / Ps : 0;
    sweep = k + 1 - grid_acc;
    due = (!active || sweep > A.sweeps) ? 0x7fffffff : bd + P * k;
    stop = t_end;
  }

  // epilogue: lambda, w = A x - rhs, accumulators
  if (active) {
    REAL a0[6], a1[6];
    lds_load6(s_acc + slot0 * 6, a0);
    lds_load6(s_acc + slot1 * 6, a1);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const REAL ax = LINSYM ? linsym_row_dot(c, r, a0, a1) : row_dot(c.J0 + 6 * r, a0, c.J1 + 6 * r, a1);
      REAL w = tfma(A.cfm, x[r], ax) - c.rhs[r];
      A.x[(size_t)d.cidx * 3 + r] = x[r];
      A.wres[(size_t)d.cidx * 3 + r] = w;
    }
  }
  for (int s = tid + 1; s < nslots; s += BLOCK) {
    const int body = slot_body[s];
    if (body < 0) continue;   // unused slot number
#pragma unroll
    for (int k = 0; k < 6; ++k) A.acc[(size_t)body * 6 + k] = s_acc[s * 6 + k];
  }
}

}  // namespace

template <typename REAL>
void launch_step_solve(const SolveArgs<REAL> &a, int method, int n_tiles, int block, int group, bool linsym, hipStream_t s) {
  if (n_tiles <= 0) return;
  SolveArgs<REAL> b = a;
  b.n_tiles = n_tiles;
#define EGS_LAUNCH_S(BLK, ISO, GRP) EGS_LAUNCH_SH(BLK, ISO, GRP, !ISO, false)
#define EGS_LAUNCH_SH(BLK, ISO, GRP, HIST, LINSYM)                                                             \
  {                                                                                                            \
    if (b.mu != nullptr) EGS_LAUNCH_SF(BLK, ISO, GRP, HIST, LINSYM, true)                                      \
    else EGS_LAUNCH_SF(BLK, ISO, GRP, HIST, LINSYM, false)                                                     \
  }
#define EGS_LAUNCH_SF(BLK, ISO, GRP, HIST, LINSYM, FRIC)                                                       \
  {                                                                                                            \
    const size_t lds = (size_t)b.max_slots * 6 * sizeof(REAL) * GRP;                                           \
    const dim3 g((n_tiles + GRP - 1) / GRP), t(BLK * GRP);                                                     \
    auto k1 = step_solve_kernel<REAL, BLK, 1, ISO, GRP, HIST, LINSYM, false, true, FRIC>;                      \
    auto k2 = step_solve_kernel<REAL, BLK, 2, ISO, GRP, HIST, LINSYM, false, true, FRIC>;                      \
    if (lds > 48 * 1024) {                                                                                     \
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(method == 1 ? k1 : k2),                            \
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                               \
    }                                                                                                          \
    if (method == 1) hipLaunchKernelGGL(k1, g, t, lds, s, b);                                                  \
    else hipLaunchKernelGGL(k2, g, t, lds, s, b);                                                              \
  }
  if (block == 256 && a.iso) {
    if (b.hist_x != nullptr) EGS_LAUNCH_SH(256, true, 1, true, false)      // per-sweep snapshots of the stopping loop (kernels.h)
    else if constexpr (sizeof(REAL) == 4) {
      if (group == 4) EGS_LAUNCH_S(256, true, 4)
      else if (group == 2) EGS_LAUNCH_S(256, true, 2)
      else EGS_LAUNCH_S(256, true, 1)
    } else {
      if (group == 3) EGS_LAUNCH_S(256, true, 3)
      else if (linsym) EGS_LAUNCH_SH(256, true, 1, false, true)   // one linear block for both sides (LINSYM above)
      else EGS_LAUNCH_S(256, true, 1)
    }
  }
  else if (block == 256) EGS_LAUNCH_S(256, false, 1)
  else if (block == 128) EGS_LAUNCH_S(128, false, 1)
  else if (block == 64) EGS_LAUNCH_S(64, false, 1)
  else EGS_LAUNCH_S(512, false, 1)
#undef EGS_LAUNCH_S
#undef EGS_LAUNCH_SH
#undef EGS_LAUNCH_SF
}

namespace {
template <bool STORE_SYSTEM, bool PAIR, bool CHAIN, bool REST, bool SHARE>
void launch_step_solve_assemble_r(const SolveArgs<double> &b, int method, int n_tiles, hipStream_t s) {
  // the accumulators; the storing form stages its blocks in the same LDS first
  size_t lds = (size_t)b.max_slots * 6 * sizeof(double);
  if (STORE_SYSTEM) lds = std::max(lds, (size_t)4 * kStageWave * sizeof(double));
  auto k1 = step_solve_kernel<double, 256, 1, true, 1, false, true, true, STORE_SYSTEM, false, PAIR, CHAIN, REST, SHARE>;
  auto k2 = step_solve_kernel<double, 256, 2, true, 1, false, true, true, STORE_SYSTEM, false, PAIR, CHAIN, REST, SHARE>;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(method == 1 ? k1 : k2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (method == 1) hipLaunchKernelGGL(k1, dim3(n_tiles), dim3(256), lds, s, b);
  else hipLaunchKernelGGL(k2, dim3(n_tiles), dim3(256), lds, s, b);
}
// restitution (b.assemble.rest is set) has instantiations of its own: the launches without it run the code they ran
template <bool STORE_SYSTEM, bool PAIR, bool CHAIN = false, bool SHARE = false>
void launch_step_solve_assemble_t(const SolveArgs<double> &b, int method, int n_tiles, hipStream_t s) {
  if (b.assemble.rest != nullptr) launch_step_solve_assemble_r<STORE_SYSTEM, PAIR, CHAIN, true, SHARE>(b, method, n_tiles, s);
  else launch_step_solve_assemble_r<STORE_SYSTEM, PAIR, CHAIN, false, SHARE>(b, method, n_tiles, s);
}
}  // namespace

void launch_step_solve_assemble(const SolveArgs<double> &a, int method, int n_tiles, bool store_system, bool pair, bool chain,
                                bool share, hipStream_t s) {
  SolveArgs<double> b = a;
  b.n_tiles = n_tiles;
  if (pair && chain && share) {
    if (store_system) launch_step_solve_assemble_t<true, true, true, true>(b, method, n_tiles, s);
    else launch_step_solve_assemble_t<false, true, true, true>(b, method, n_tiles, s);
  } else if (pair && chain) {
    if (store_system) launch_step_solve_assemble_t<true, true, true>(b, method, n_tiles, s);
    else launch_step_solve_assemble_t<false, true, true>(b, method, n_tiles, s);
  } else if (store_system) {
    if (pair) launch_step_solve_assemble_t<true, true>(b, method, n_tiles, s);
    else launch_step_solve_assemble_t<true, false>(b, method, n_tiles, s);
  } else {
    if (pair) launch_step_solve_assemble_t<false, true>(b, method, n_tiles, s);
    else launch_step_solve_assemble_t<false, false>(b, method, n_tiles, s);
  }
}

void launch_step_solve_face(const SolveArgs<double> &a, int n_tiles, int tiles_per_cu, const FaceWork *w, hipStream_t s) {
  if (n_tiles <= 0) return;
  SolveArgs<double> b = a;
  b.n_tiles = n_tiles;
  // the accumulators; the prologue keeps 27 doubles per thread in the same LDS first
  size_t lds = std::max((size_t)b.max_slots * 6, (size_t)27 * kFaceThreads) * sizeof(double);
  // the registers allow four tiles per CU; a request above a quarter of the CU's 160 KiB of LDS leaves room for three
  constexpr size_t kQuarterLds = 160 * 1024 / 4;
  if (tiles_per_cu == 3) lds = std::max(lds, kQuarterLds + 1024);
  if (w) {   // split in time: persistent workgroups that take the pieces by ticket
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(step_solve_face_pieces_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(step_solve_face_pieces_kernel, dim3(w->n_workgroups), dim3(kFaceThreads), lds, s, b, *w);
    return;
  }
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(step_solve_face_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(step_solve_face_kernel, dim3(n_tiles), dim3(kFaceThreads), lds, s, b);
}

template void launch_step_solve<double>(const SolveArgs<double> &, int, int, int, int, bool, hipStream_t);
template void launch_step_solve<float>(const SolveArgs<float> &, int, int, int, int, bool, hipStream_t);

}  // namespace egs
