// step_device.h -- projected Gauss-Seidel / backward SOR on a STATIC, time-stepped schedule: the timetable, and the
// device functions that more than one of its kernel families takes (step_solve.hip: one lane per constraint;
// step_pair.hip: a lane pair per update; step_face.hip: a thread pair per box face).
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
// The steady-state loop (GROUP == 1, no snapshots, LINSYM or not ISO): between the first depth steps of a launch (the
// fill: lanes still wait for their first turn, or run the accumulation) and its last ones (the drain: lanes have run
// out of sweeps) every lane whose level matches the clock modulo P is due, in some sweep 1 .. sweeps.  There the
// kernel walks a second loop without the per-lane timetable: the clock, its phase t mod P and the loop bounds are
// scalar, a lane compares its phase with the clock's, and `due`, `sweep`, the accumulation branch and the history
// test are gone from the pass.  The bounds are the same for every lane of the workgroup (the tile's depth and period,
// the launch's sweeps): every wavefront meets the same barriers as in the single loop.  SolveArgs::steady = 0 (solve.cpp:
// EGS_STEP_STEADY=0) keeps the single loop.  The arithmetic of an update is the same code: the same bits.
#pragma once
#include <algorithm>
#include <type_traits>

#include "kernels.h"
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

// ---- the host side of the step units ---------------------------------------------------------------------------------
// The dynamic LDS of an ASSEMBLE launch on 256-lane tiles: the accumulators; the storing form stages its blocks in the
// same LDS first
inline size_t assemble_lds_bytes(const SolveArgs<double> &b, bool store_system) {
  const size_t lds = (size_t)b.max_slots * 6 * sizeof(double);
  return store_system ? std::max(lds, (size_t)4 * kStageWave * sizeof(double)) : lds;
}
// Runtime bools as types: f(std::true_type{} or std::false_type{}, ..) with one argument per bool, in their order (as
// problem.h: with_real does for the precision).  The one place that turns a launch's switches into template arguments.
template <typename F>
void with_bools(F &&f) { f(); }
template <typename F, typename... BOOLS>
void with_bools(F &&f, bool b, BOOLS... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// A launch with `lds` bytes of dynamic LDS: above the 48 KiB a kernel may ask for unprepared, its limit is raised first
template <typename... PARAMS, typename... ARGS>
void launch_lds(void (*kernel)(PARAMS...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const ARGS &...args) {
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

}  // namespace
}  // namespace egs
