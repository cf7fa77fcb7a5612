// step_pair_device.h -- one update of the timetable step on a lane pair: what a lane holds of a constraint's side, the
// pass and the epilogue.  The PAIR / CHAIN / SHARE kernel (step_pair.hip) and the FACE kernels (step_face.hip) take them.
#pragma once
#include "solve_device.h"

namespace egs {
namespace {

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

}  // namespace
}  // namespace egs
