// step_pair.hip -- the lane-pair forms of the fused step launch (the timetable: step_device.h; ASSEMBLE, STORE_SYSTEM
// and REST: step_solve.hip, whose one-lane ASSEMBLE form this one replaces where the plan is pairable).
//
// PAIR (ASSEMBLE only): an update runs on a lane pair, each lane holding one side of two constraints; described where
// it is written (step_pair_device.h).  CHAIN (PAIR only): where the pair's two constraints are consecutive updates of the
// same two bodies, the steady loop hands their accumulators from the first update to the second in registers.  SHARE
// (CHAIN only): where the two also have one contact normal, the lane keeps their linear block and weights once.
#include <stdexcept>

#include "kernels.h"
#include "step_device.h"
#include "step_pair_device.h"

namespace egs {

namespace {

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

// ASSEMBLE, fp64, 256-lane tiles (launch_step_solve_pair); the registers of step_solve_kernel's isotropic fp64 forms:
// three wavefronts per SIMD
template <int METHOD, bool STORE_SYSTEM, bool CHAIN, bool REST, bool SHARE>
__global__ void __launch_bounds__(256, 3) step_solve_pair_kernel(const SolveArgs<double> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  pair_step_solve<METHOD, STORE_SYSTEM, CHAIN, REST, SHARE>(A, smem);
}

}  // namespace

void launch_step_solve_pair(const SolveArgs<double> &a, int method, int n_tiles, bool store_system, bool chain, bool share,
                            hipStream_t s) {
  if (share && !chain) throw std::logic_error("the SHARE form asked for without the CHAIN form it is a form of");
  SolveArgs<double> b = a;
  b.n_tiles = n_tiles;
  // restitution (b.assemble.rest is set) has instantiations of its own: the launches without it run the code they ran
  with_bools([&](auto store, auto chain_c, auto share_c, auto rest) {
    constexpr bool STORE = decltype(store)::value, CHAIN = decltype(chain_c)::value, SHARE = decltype(share_c)::value,
                   REST = decltype(rest)::value;
    if constexpr (CHAIN || !SHARE)   // the other combination was rejected above
      launch_lds(method == 1 ? step_solve_pair_kernel<1, STORE, CHAIN, REST, SHARE> : step_solve_pair_kernel<2, STORE, CHAIN, REST, SHARE>,
                 dim3(n_tiles), dim3(256), assemble_lds_bytes(b, STORE), s, b);
  }, store_system, chain, share, b.assemble.rest != nullptr);
}

}  // namespace egs
