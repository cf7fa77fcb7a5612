// step_face.hip -- the FACE form of the fused step launch (the timetable: step_device.h; the lane-pair structs and the
// pass: step_pair_device.h; the SHARE form it refines: step_pair.hip).
//
// FACE (kernels of its own, step_solve_face_kernel): where the plan lays the four contact points of a face 32 lanes apart,
// a thread pair holds all four and runs their updates behind one barrier.  Where its tiles leave the last round of
// resident slots half empty or emptier, that launch is split in time (step_solve_face_pieces_kernel: a tile as two
// pieces, sweeps 1 .. s1 and s1 + 1 .. S, taken by ticket on persistent workgroups; policy.h: face_split_policy).
// Both kernels have a LEAN twin from the same source (step_solve_face_lean_kernel, ..._lean_pieces_kernel): fewer held
// products and the owner's scalars in LDS, 168 VGPRs, six tiles per CU instead of four -- slower blocks, taken where six
// tiles per CU save a round (policy.h: face_form_policy).
#include <algorithm>
#include <stdexcept>

#include "kernels.h"
#include "policy.h"
#include "step_device.h"
#include "step_pair_device.h"

namespace egs {

namespace {

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
// LEAN (168 VGPRs, three wavefronts per SIMD, six tiles per CU): no angular products and as many of the nine linear ones,
// which serve all four members, as keep scratch out of the timetable loops with the owner's scalars parked in LDS
// (face_park): all nine in the unsplit kernel, six in the pieces kernel (nine reload two doubles per block there).
constexpr int kFaceLeanLin = 9, kFaceLeanLinPieces = 6;

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
template <bool LIN, int NL, int NA>
__device__ __forceinline__ void face_sides(const Cons<double> &c, int side, PairLin<NL> &L, PairAng<NA> &GE, PairAng<NA> &GO) {
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

constexpr int kFaceOff[3] = {3, 6, 7};   // D's off-diagonal entries that a forward update takes
// LEAN: the parked values of owned constraint K (0, 1), to LDS and back (element e of this thread at park[e * 128])
template <bool LEAN, int K>
__device__ __forceinline__ void face_park(double *park, const Cons<double> &c) {
  if constexpr (LEAN) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      park[(9 * K + r) * kFaceThreads] = c.rhs[r];
      park[(9 * K + 3 + r) * kFaceThreads] = c.D[kFaceOff[r]];
      park[(9 * K + 6 + r) * kFaceThreads] = c.inv[r];
    }
  }
}
template <bool LEAN, int K>
__device__ __forceinline__ void face_unpark(const double *park, Cons<double> &c) {
  if constexpr (LEAN) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      c.rhs[r] = park[(9 * K + r) * kFaceThreads];
      c.D[kFaceOff[r]] = park[(9 * K + 3 + r) * kFaceThreads];
      c.inv[r] = park[(9 * K + 6 + r) * kFaceThreads];
    }
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
// one.  Nor does workgroup k start with piece k to save its first draw: measured, the headline's
// launch then took 461 us where it takes 444 (supposedly the list's even mix of first parts and
// whole tiles no longer reaches every CU once the hardware's placement of workgroup numbers decides who gets which).
// Only the prologue, the loop bounds and the epilogue differ from the unsplit kernel: n_sweeps and resume are scalar.
// Returns false once the list is exhausted: the workgroup is done.
template <bool PIECES, bool LEAN>
__device__ __forceinline__ bool face_step(const SolveArgs<double> &A, const FaceWork &W, unsigned char *smem, const int tid) {
  constexpr int METHOD = 1;
  constexpr int NL = LEAN ? (PIECES ? kFaceLeanLinPieces : kFaceLeanLin) : kFaceLin, NA = LEAN ? 0 : kFaceAng;
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
  PairLin<NL> L;
  PairAng<NA> GA, GB, GC, GD;
  Cons<double> c0 = {}, c1 = {};
  double x0[3], x1[3];
  face_assemble(A, d0, B, own0 >= 0, c0, x0);
  face_sides<true>(c0, side, L, GA, GB);
  // (LEAN: the last linear entry stays in its register, so that six tiles' staging fits a CU: 26 doubles per thread are
  // the 26 KiB a tile may ask for -- policy.h: face_lds_bytes)
  constexpr int SL = LEAN ? 8 : 9;
  static_assert(SL + 18 == (LEAN ? kFaceLeanStaged : kFaceStaged), "policy.h sizes the staging");
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    if (e < SL) s_acc[e * kFaceThreads + tid] = L.J[e];
    s_acc[(SL + e) * kFaceThreads + tid] = GA.J[e];
    s_acc[(SL + 9 + e) * kFaceThreads + tid] = GB.J[e];
  }
  asm volatile("" ::: "memory");   // stored here, loaded below: not carried in registers
  // ... and the second assembly, which no longer loads, is not scheduled into the first: one at a time in the registers
  __builtin_amdgcn_sched_barrier(0);
  face_assemble(A, d1, B, own1 >= 0, c1, x1);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    if (e < SL) L.J[e] = s_acc[e * kFaceThreads + tid];
    GA.J[e] = s_acc[(SL + e) * kFaceThreads + tid];
    GB.J[e] = s_acc[(SL + 9 + e) * kFaceThreads + tid];
  }
  face_sides<false>(c1, side, L, GC, GD);
  __syncthreads();   // every thread has its blocks back
  // LEAN: the owner's rhs, D's off-diagonals and inv of both constraints, which the loops would otherwise reload from
  // scratch, are parked in LDS behind the accumulators (element e of thread i at e * 128 + i) and read in the block, each
  // constraint's ahead of its two passes
  static_assert(kFaceLeanParked == 18, "policy.h sizes the parked values");
  double *s_park = nullptr;
  if constexpr (LEAN) {
    s_park = s_acc + (size_t)A.max_slots * 6 + tid;
    face_park<LEAN, 0>(s_park, c0);
    face_park<LEAN, 1>(s_park, c1);
  }
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
      // where the host expects it whatever happened.  The host's page-locked copy of the flag is set from here (no copy
      // is posted behind a FACE launch): system scope, so the host sees it once the launch has ended at the latest
      if (tid == 0) {
        atomicOr(A.error_flag, 1);
        __hip_atomic_store(W.host_stall, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
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
  PairShared<NL, NA> SA{L, GA}, SB{L, GB}, SC{L, GC}, SD{L, GD};
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
        face_unpark<LEAN, 0>(s_park, c0);
        pair_pass<METHOD, kQuadEven, true, true, false>(SA, ac, a, has, even, c0, x0, sweep, A.cfm);
        if (nm > 1) pair_pass<METHOD, kQuadOdd, true, false, false>(SB, ac, a, has, odd, c0, x0, sweep, A.cfm);
        face_unpark<LEAN, 1>(s_park, c1);
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
          face_unpark<LEAN, 0>(s_park, c0);
          pair_pass<METHOD, kQuadEven, false, true, false>(SA, ac, a, has, even, c0, x0, 1, A.cfm);
          if (nm > 1) pair_pass<METHOD, kQuadOdd, false, false, false>(SB, ac, a, has, odd, c0, x0, 1, A.cfm);
          face_unpark<LEAN, 1>(s_park, c1);
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
  face_unpark<LEAN, 0>(s_park, c0);
  face_unpark<LEAN, 1>(s_park, c1);
  if (nm > 0) pair_epilogue(A, SA, ac, even, cidx0, c0, x0);
  if (nm > 1) pair_epilogue(A, SB, ac, odd, cidx0, c0, x0);
  if (nm > 2) pair_epilogue(A, SC, ac, even, cidx1, c1, x1);
  if (nm > 3) pair_epilogue(A, SD, ac, odd, cidx1, c1, x1);
  for (int s = tid + 1; s < nslots; s += kFaceThreads) {
    const int body = slot_body[s];
    if (body < 0) continue;   // unused slot number
    double acc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) A.acc[(size_t)body * 6 + k] = acc[k] = s_acc[s * 6 + k];
    // the step's velocity of the body, velocity_kernel's expression (kernels.hip) on the accumulator just stored: the
    // same bits.  A first part's accumulators are not the step's: its tile's second part writes.
    if (W.v6 && kind != kFaceFirst) {
      const AssembleArgs &G = A.assemble;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const double vel = k < 3 ? G.v[(size_t)body * 3 + k] : G.w[(size_t)body * 3 + k - 3];
        W.v6[(size_t)body * 6 + k] = vel + G.dt * (G.Wf[(size_t)body * 6 + k] + acc[k]);
      }
    }
  }
  if (PIECES && kind == kFaceFirst) {
    // publish: this thread's stores of lambda and the accumulators, released to the agent, before the tile's flag
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(W.flags + tile, W.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  return true;
}

// (W: the velocity pointer alone is read)
__global__ void __launch_bounds__(kFaceThreads, 2) step_solve_face_kernel(const SolveArgs<double> A, const FaceWork W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  face_step<false, false>(A, W, smem, (int)threadIdx.x);
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
    if (!face_step<true, false>(B, W, smem, tid)) break;
    __syncthreads();   // the epilogue has read the accumulators before the next ticket lands there
  }
}
// the LEAN twins: the same source at three wavefronts per SIMD (six tiles per CU)
__global__ void __launch_bounds__(kFaceThreads, 3) step_solve_face_lean_kernel(const SolveArgs<double> A, const FaceWork W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  face_step<false, true>(A, W, smem, (int)threadIdx.x);
}
__global__ void __launch_bounds__(kFaceThreads, 3) step_solve_face_lean_pieces_kernel(const SolveArgs<double> A, const FaceWork W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int tid = (int)threadIdx.x;
  for (;;) {
    SolveArgs<double> B = A;
    asm volatile("" : "+v"(tid), "+s"(B.assemble.dt), "+s"(B.assemble.erp), "+s"(B.cfm));
    if (!face_step<true, true>(B, W, smem, tid)) break;
    __syncthreads();
  }
}

}  // namespace

void launch_step_solve_face(const SolveArgs<double> &a, int n_tiles, int tiles_per_cu, bool lean, const FaceWork &w,
                            hipStream_t s) {
  if (n_tiles <= 0) return;
  SolveArgs<double> b = a;
  b.n_tiles = n_tiles;
  // the accumulators, the lean form's parked values behind them; the prologue keeps its blocks in the same LDS first
  // (policy.h: face_lds_bytes).  A lean tile whose request does not fit six to a CU is the caller's to refuse (solve.cpp:
  // choose_sweep asks face_lds_bytes before it sizes the slots, the split and the grid for the form): no falling back
  // here, where the work list is already the lean form's
  static_assert(kFaceThreads == kFaceTileThreads, "policy.h sizes the LDS request for this many threads");
  const size_t lds = face_lds_bytes(b.max_slots, lean, tiles_per_cu);
  if (lds == 0) throw std::logic_error("a lean FACE launch asked for where a tile's LDS request does not fit");
  // a piece list: persistent workgroups that take its pieces
  auto *kernel = w.pieces ? (lean ? step_solve_face_lean_pieces_kernel : step_solve_face_pieces_kernel)
                          : (lean ? step_solve_face_lean_kernel : step_solve_face_kernel);
  launch_lds(kernel, w.pieces ? dim3(w.n_workgroups) : dim3(n_tiles), dim3(kFaceThreads), lds, s, b, w);
}

}  // namespace egs
