// step_solve.hip -- the timetable sweep with one lane per constraint (the timetable itself: step_device.h): every tile
// size, stored-B and isotropic bodies, GROUP, the per-sweep snapshots, LINSYM, friction, and the one-lane ASSEMBLE form.
// The lane-pair forms of the ASSEMBLE launch are kernels of their own (step_pair.hip: PAIR, CHAIN, SHARE; step_face.hip:
// FACE).
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
//
// STORE_SYSTEM = false: none of that is stored -- a step reads none of it (the sweeps run from registers) -- and the
// problem remembers that its system is not materialised (problem.h: ensure_system runs assemble_kernel on demand).
#include "kernels.h"
#include "step_device.h"

namespace egs {

namespace {

// FRIC: the Coulomb pyramid on the constraints with mu >= 0 (solve_device.h: project_pyramid), A.mu not NULL.  The
// ASSEMBLE form has none (solve.cpp: choose_sweep).
// REST: the ASSEMBLE prologue bounces the normal rows (step_device.h: assemble_lane).
template <typename REAL, int BLOCK, int METHOD, bool ISO, int GROUP, bool HIST, bool LINSYM = false, bool ASSEMBLE = false,
          bool STORE_SYSTEM = true, bool FRIC = false, bool REST = false>
__global__ void __launch_bounds__(BLOCK * GROUP, (ISO && GROUP == 1) ? (sizeof(REAL) == 4 ? 4 : 3) : 1) step_solve_kernel(const SolveArgs<REAL> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
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

namespace {
// one instantiation pair (GS, backward SOR) of the stored-system sweep, with or without friction (b.mu)
template <int BLK, bool ISO, int GRP, bool HIST, bool LINSYM, typename REAL>
void launch_step_form(const SolveArgs<REAL> &b, int method, hipStream_t s) {
  const size_t lds = (size_t)b.max_slots * 6 * sizeof(REAL) * GRP;
  const dim3 g((b.n_tiles + GRP - 1) / GRP), t(BLK * GRP);
  with_bools([&](auto fric) {
    constexpr bool FRIC = decltype(fric)::value;
    launch_lds(method == 1 ? step_solve_kernel<REAL, BLK, 1, ISO, GRP, HIST, LINSYM, false, true, FRIC>
                           : step_solve_kernel<REAL, BLK, 2, ISO, GRP, HIST, LINSYM, false, true, FRIC>, g, t, lds, s, b);
  }, b.mu != nullptr);
}
}  // namespace

template <typename REAL>
void launch_step_solve(const SolveArgs<REAL> &a, int method, int n_tiles, int block, int group, bool linsym, hipStream_t s) {
  if (n_tiles <= 0) return;
  SolveArgs<REAL> b = a;
  b.n_tiles = n_tiles;
  if (block == 256 && a.iso) {
    if (b.hist_x != nullptr) launch_step_form<256, true, 1, true, false>(b, method, s);   // per-sweep snapshots of the stopping loop (kernels.h)
    else if constexpr (sizeof(REAL) == 4) {
      if (group == 4) launch_step_form<256, true, 4, false, false>(b, method, s);
      else if (group == 2) launch_step_form<256, true, 2, false, false>(b, method, s);
      else launch_step_form<256, true, 1, false, false>(b, method, s);
    } else {
      if (group == 3) launch_step_form<256, true, 3, false, false>(b, method, s);
      else if (linsym) launch_step_form<256, true, 1, false, true>(b, method, s);   // one linear block for both sides (LINSYM above)
      else launch_step_form<256, true, 1, false, false>(b, method, s);
    }
  }
  // stored B: the snapshots are part of the one instantiation
  else if (block == 256) launch_step_form<256, false, 1, true, false>(b, method, s);
  else if (block == 128) launch_step_form<128, false, 1, true, false>(b, method, s);
  else if (block == 64) launch_step_form<64, false, 1, true, false>(b, method, s);
  else launch_step_form<512, false, 1, true, false>(b, method, s);
}

void launch_step_solve_assemble(const SolveArgs<double> &a, int method, int n_tiles, bool store_system, hipStream_t s) {
  SolveArgs<double> b = a;
  b.n_tiles = n_tiles;
  // restitution (b.assemble.rest is set) has instantiations of its own: the launches without it run the code they ran
  with_bools([&](auto store, auto rest) {
    constexpr bool STORE = decltype(store)::value, REST = decltype(rest)::value;
    launch_lds(method == 1 ? step_solve_kernel<double, 256, 1, true, 1, false, true, true, STORE, false, REST>
                           : step_solve_kernel<double, 256, 2, true, 1, false, true, true, STORE, false, REST>,
               dim3(n_tiles), dim3(256), assemble_lds_bytes(b, STORE), s, b);
  }, store_system, b.assemble.rest != nullptr);
}

template void launch_step_solve<double>(const SolveArgs<double> &, int, int, int, int, bool, hipStream_t);
template void launch_step_solve<float>(const SolveArgs<float> &, int, int, int, int, bool, hipStream_t);

}  // namespace egs
