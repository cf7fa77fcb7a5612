// kernels.hip -- gfx950 (CDNA4, wave64) kernels of the constraint-solve path.
//
//   assemble_kernel        K1-K4: Jacobian blocks, error, bounds, ODE rhs
//                          (joints.cc:3-35, contact.cc:14-117, ensembles.cc:569)
//   tile_solve_kernel      K5-K8: projected Jacobi / Gauss-Seidel / backward
//                          SOR over J W J^T + cfm I, one workgroup per tile of
//                          whole islands, body accumulators in LDS
//                          (sparse_iterations.cc:148-226)
//   global_solve_kernel    the same sweep for islands larger than a workgroup
//   residual_partials      K8 reduction (sparse_iterations.cc:51-69)
//   velocity_kernel        K9 (ensembles.cc:535, 572)
//
// Built with -ffp-contract=off: the only fused operations are the explicit
// fma() calls, in the order fixed by the CPU oracle (oracle/pgs_fast.inc), so
// the results can be compared bit for bit.
//
// How list order is kept without global barriers.  The reference sweeps the
// constraint list strictly in order.  Two constraints only interact through a
// shared body, so it is enough that, per body, its constraints run in list
// order, sweep after sweep.  Every body carries a ticket counter; constraint c
// with rank `pos` among the `cnt` constraints of that body may run in sweep s
// when ticket == s*cnt + pos (cnt-1-pos for the backward sweep) on BOTH of
// its bodies, and bumps both tickets when done.  The dependency graph is
// acyclic ((sweep, index) is a topological order), so there is always a lane
// that can run; consecutive sweeps pipeline through an island as a wavefront.
#include "kernels.h"
#include "solve_device.h"
#include "assemble_device.h"
#include "rotation_device.h"

#ifndef EGS_POLL_SLEEP
#define EGS_POLL_SLEEP 32  // s_sleep units (64 cycles) of a wavefront none of whose lanes is ready; s_wakeup ends it early
#endif

namespace egs {

namespace {

// Ticket-ordered a += B dx for every lane of the workgroup (list order per
// body).  Used for the initial accumulators (dx = x0) and the Jacobi sweep.
template <bool ISO, typename REAL>
__device__ __forceinline__ bool ordered_accumulate(REAL *s_acc, unsigned *s_tick, const Cons<REAL> &c,
                                                   const REAL *dx, bool active, bool has0, bool has1,
                                                   int slot0, int slot1, unsigned want0, unsigned want1,
                                                   unsigned spin_limit) {
  bool pending = active;
  bool ok = true;
  unsigned spins = 0;
  while (pending) {
    const unsigned t0 = has0 ? lds_load_acquire(s_tick + slot0) : want0;
    const unsigned t1 = has1 ? lds_load_acquire(s_tick + slot1) : want1;
    if (t0 == want0 && t1 == want1) {
      REAL a0[6], a1[6];
      if (has0) {
        lds_load6(s_acc + slot0 * 6, a0);
        acc_add_side0<ISO>(a0, c, dx);
        lds_store6(s_acc + slot0 * 6, a0);
      }
      if (has1) {
        lds_load6(s_acc + slot1 * 6, a1);
        acc_add_side1<ISO>(a1, c, dx);
        lds_store6(s_acc + slot1 * 6, a1);
      }
      if (has0) lds_store_release(s_tick + slot0, want0 + 1);
      if (has1) lds_store_release(s_tick + slot1, want1 + 1);
      pending = false;
    } else if (++spins > spin_limit) {
      ok = false;
      pending = false;
    }
  }
  return ok;
}

// ISO: every body's M^-1 block is diag(a, a, a, b, b, b) (boxes with I = c*Identity at
// their rest orientation -- every BASELINE pile).  B = M^-1 J^T is then w * J entry by
// entry and is formed on the fly instead of living in 72 VGPRs: 164 instead of 232 VGPRs,
// three wavefronts per SIMD instead of two, i.e. 768 instead of 512 constraints resident
// per CU.  Same products, same roundings, same bits.
// FRIC: the Coulomb pyramid on the constraints with mu >= 0 (solve_device.h: project_pyramid), A.mu not NULL.
template <typename REAL, int BLOCK, int METHOD, bool ISO, bool FRIC = false>
__global__ void __launch_bounds__(BLOCK, ISO ? (sizeof(REAL) == 4 ? 4 : 3) : 1) tile_solve_kernel(const SolveArgs<REAL> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  REAL *s_acc = reinterpret_cast<REAL *>(smem);
  unsigned *s_tick = reinterpret_cast<unsigned *>(smem + (size_t)A.max_slots * 6 * sizeof(REAL));

  const int tile = blockIdx.x, tid = threadIdx.x;
  const int nslots = A.tile_nslots[tile];
  const int32_t *slot_body = A.slot_body + A.tile_slot_off[tile];

  for (int s = tid; s < nslots; s += BLOCK) {
    const int body = slot_body[s];
#pragma unroll
    for (int k = 0; k < 6; ++k)
      s_acc[s * 6 + k] = (A.resume && body >= 0) ? A.acc[(size_t)body * 6 + k] : REAL(0);
    s_tick[s] = 0u;
  }

  const LaneDesc d = A.lanes[(size_t)tile * BLOCK + tid];
  const bool active = d.cidx >= 0;
  const bool has0 = active && d.slot0 != 0, has1 = active && d.slot1 != 0;
  const int slot0 = d.slot0, slot1 = d.slot1;
  const unsigned cnt0 = d.cnt0, cnt1 = d.cnt1;
  const unsigned pos0 = d.pos0, pos1 = d.pos1;

  Cons<REAL> c;
  REAL x[3] = {REAL(0), REAL(0), REAL(0)};
  const REAL *xs = A.resume ? A.x : A.x0;   // the previous launch's x, a given start, or NULL: rhs (Q7)
  if (active) {
    load_cons<REAL, ISO, false, false, FRIC>(A, d.cidx, has0, has1, has0 ? slot_body[slot0] : 0, has1 ? slot_body[slot1] : 0, c);
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = xs ? xs[(size_t)d.cidx * 3 + r] : c.rhs[r];
  }
  __syncthreads();

  bool ok = true;
  // Tickets count completed updates per body.  Sweep s (1-based) waits for
  // base + (s-1)*cnt + ord; the initial accumulation (x0 = rhs,
  // sparse_iterations.cc:202) takes tickets 0..cnt-1 unless resuming.
  const unsigned base0 = A.resume ? 0u : cnt0, base1 = A.resume ? 0u : cnt1;
  if (!A.resume) {
    ok = ordered_accumulate<ISO>(s_acc, s_tick, c, x, active, has0, has1, slot0, slot1, pos0, pos1, A.spin_limit);
    __syncthreads();
  }

  if (METHOD == 0) {
    for (int s = 1; s <= A.sweeps; ++s) {
      REAL dx[3] = {REAL(0), REAL(0), REAL(0)};
      if (active) {
        REAL a0[6], a1[6], res[3];
        lds_load6(s_acc + slot0 * 6, a0);
        lds_load6(s_acc + slot1 * 6, a1);
        row_residuals(c, a0, a1, x, A.cfm, res);
        update_rows<REAL, 0, false, FRIC>(c, res, x, dx);
      }
      __syncthreads();  // every lane has read the old accumulators
      ok &= ordered_accumulate<ISO>(s_acc, s_tick, c, dx, active, has0, has1, slot0, slot1,
                               base0 + (unsigned)(s - 1) * cnt0 + pos0,
                               base1 + (unsigned)(s - 1) * cnt1 + pos1, A.spin_limit);
      __syncthreads();
      if (!ISO && A.hist_x) {   // snapshots for the per-sweep stopping test: the sweep is complete here
        if (active) {
          REAL *hx = A.hist_x + ((size_t)(s - 1) * A.m + d.cidx) * 3;
          hx[0] = x[0]; hx[1] = x[1]; hx[2] = x[2];
        }
        for (int q = tid + 1; q < nslots; q += BLOCK) {
          if (slot_body[q] < 0) continue;   // slot numbers have gaps (plan.cpp, bank-aware numbering)
          REAL *ha = A.hist_acc + ((size_t)(s - 1) * A.n_bodies + slot_body[q]) * 6;
#pragma unroll
          for (int k = 0; k < 6; ++k) ha[k] = s_acc[q * 6 + k];
        }
      }
    }
  } else {
    const unsigned ord0 = (METHOD == 2) ? cnt0 - 1u - pos0 : pos0;
    const unsigned ord1 = (METHOD == 2) ? cnt1 - 1u - pos1 : pos1;
    unsigned want0 = base0 + ord0, want1 = base1 + ord1;
    int sweep = 1;
    unsigned spins = 0;
    bool alive = active && A.sweeps >= 1;
    const unsigned tk0 = lds_addr(s_tick + slot0), tk1 = lds_addr(s_tick + slot1);
    const unsigned ac0 = lds_addr(s_acc + slot0 * 6), ac1 = lds_addr(s_acc + slot1 * 6);
    while (alive) {
      unsigned t0, t1;
      REAL a0[6], a1[6];
      // Two stages: every wavefront of the (two) resident tiles polls, so the poll reads the
      // tickets only (8 B per lane); the 96 B of accumulators follow for the lanes whose turn
      // it is.  One extra LDS round trip on the hand-off, but 13x less polling traffic in front
      // of the working wavefront's LDS operations: +5 % on the batched C3 solve.  A wavefront
      // with no ready lane sleeps (up to 2048 cycles) and is woken by the s_wakeup that follows
      // every ticket store in its workgroup: another +7 %.
      poll_ticks(tk0, tk1, t0, t1);                 // world slot 0: ticket ignored, zeros
      const bool ready = (!has0 || t0 == want0) && (!has1 || t1 == want1);
      if (ready) load12(ac0, ac1, a0, a1);
      if (ready) {
        REAL res[3], dx[3] = {REAL(0), REAL(0), REAL(0)};
        row_residuals(c, a0, a1, x, A.cfm, res);
        update_rows<REAL, METHOD, false, FRIC>(c, res, x, dx);
        if (has0) { acc_add_side0<ISO>(a0, c, dx); store6(ac0, a0); }
        if (has1) { acc_add_side1<ISO>(a1, c, dx); store6(ac1, a1); }
        if (has0) store_tick(tk0, want0 + 1);
        if (has1) store_tick(tk1, want1 + 1);
        // the workgroup's sleeping wavefronts poll now instead of when their s_sleep expires
        asm volatile("s_wakeup");
        if (!ISO && A.hist_x) {   // snapshots for the per-sweep stopping test (kernels.h)
          REAL *hx = A.hist_x + ((size_t)(sweep - 1) * A.m + d.cidx) * 3;
          hx[0] = x[0]; hx[1] = x[1]; hx[2] = x[2];
          if (has0 && ord0 == cnt0 - 1u) {      // this was body0's last update of the sweep
            REAL *ha = A.hist_acc + ((size_t)(sweep - 1) * A.n_bodies + slot_body[slot0]) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) ha[k] = a0[k];
          }
          if (has1 && ord1 == cnt1 - 1u) {
            REAL *ha = A.hist_acc + ((size_t)(sweep - 1) * A.n_bodies + slot_body[slot1]) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) ha[k] = a1[k];
          }
        }
        want0 += cnt0; want1 += cnt1;
        spins = 0;
        alive = ++sweep <= A.sweeps;
      } else if (++spins > A.spin_limit) {
        ok = false;
        alive = false;
      }
      if (!__any(ready)) __builtin_amdgcn_s_sleep(EGS_POLL_SLEEP);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
  }

  if (!ok) atomicOr(A.error_flag, 1);

  // epilogue: lambda, w = A x - rhs, accumulators
  if (active) {
    REAL a0[6], a1[6];
    lds_load6(s_acc + slot0 * 6, a0);
    lds_load6(s_acc + slot1 * 6, a1);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      REAL w = tfma(A.cfm, x[r], row_dot(c.J0 + 6 * r, a0, c.J1 + 6 * r, a1)) - c.rhs[r];
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

// --------------------------------------------------------------------------
// residual partial sums (sparse_iterations.cc:51-69): per block 4 sums of w^2
// over {equality, at lo & w<0, at hi & w>0, strictly inside}.  A row pinned by lo == hi (a free hinge's axis row) has
// its multiplier fixed and w free of either sign: it violates nothing and is in none of the four (in all three kernels
// below; a row with lo < hi is sorted as ever).
// FRIC: rows 0 and 1 of a constraint with mu >= 0 by the pyramid's rule (solve_device.h: pyramid_residual), the
// normal multiplier being row 3i + 2 of the same x.  Without FRIC mu is not read.
template <typename REAL, bool FRIC = false>
__global__ void __launch_bounds__(256) residual_partials_kernel(int rows, const REAL *wres, const REAL *x,
                                                                const REAL *lo, const REAL *hi,
                                                                const uint8_t *is_eq, double *out, const REAL *mu = nullptr) {
  __shared__ double red[4][256];
  double e = 0, a = 0, b = 0, c = 0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256) {
    const double w = (double)wres[r];
    const REAL xv = x[r], l = lo[r], h = hi[r];
    if (FRIC && r % 3 < 2 && mu[r / 3] >= REAL(0)) pyramid_residual(xv, w, mu[r / 3], x[r - r % 3 + 2], a, b, c);
    else if (is_eq[r]) e += w * w;
    else {
      if (xv == l && w < 0 && l != h) a += w * w;
      if (xv == h && w > 0 && l != h) b += w * w;
      if (xv > l && xv < h) c += w * w;
    }
  }
  red[0][threadIdx.x] = e; red[1][threadIdx.x] = a; red[2][threadIdx.x] = b; red[3][threadIdx.x] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 4) out[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// The same four sums for every sweep of a recorded chunk (SolveArgs::hist_x / hist_acc):
// w = cfm x + J a - rhs from the snapshots, evaluated with the solve kernels' own epilogue
// expression, then the reduction of residual_partials_kernel -- so each sweep's value is the
// one a launch stopped after that sweep would have produced, bit for bit.
// One block walks its rows ONCE per group of G recorded sweeps: the row's J blocks, bounds and rhs are read
// once and serve G sweeps (per sweep only lambda and the two accumulators change), instead of re-streaming
// 300 B of J per row and sweep.  Per sweep every thread adds the same rows in the same order and the block
// reduces them the same way as before, so the sums have the same bits.
template <typename REAL, int G, bool FRIC = false>
__global__ void __launch_bounds__(256) hist_residual_kernel(const SolveArgs<REAL> A, double *out, int write_sweep, int sweeps) {
  __shared__ double red[4][256];
  const int s0 = blockIdx.y * G;          // first sweep of the group, 0-based
  const int rows = 3 * A.m;
  double acc[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g) { acc[g][0] = 0; acc[g][1] = 0; acc[g][2] = 0; acc[g][3] = 0; }
  for (int r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256) {
    const int i = r / 3, rr = r - 3 * i;
    const int b0 = A.body0[i], b1 = A.body1[i];
    REAL j0[6], j1[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      j0[k] = b0 >= 0 ? A.J0[(size_t)i * 18 + 6 * rr + k] : REAL(0);
      j1[k] = b1 >= 0 ? A.J1[(size_t)i * 18 + 6 * rr + k] : REAL(0);
    }
    const REAL l = A.lo[r], h = A.hi[r], rhs = A.rhs[r];
    const bool eq = A.is_eq[r] != 0;
    const REAL mu = (FRIC && rr < 2) ? A.mu[i] : REAL(-1);   // < 0: the stored bounds
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int sweep = s0 + g;
      if (sweep >= sweeps) break;
      const REAL *ha = A.hist_acc + (size_t)sweep * A.n_bodies * 6;
      REAL a0[6], a1[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        a0[k] = b0 >= 0 ? ha[(size_t)b0 * 6 + k] : REAL(0);
        a1[k] = b1 >= 0 ? ha[(size_t)b1 * 6 + k] : REAL(0);
      }
      const REAL xv = A.hist_x[(size_t)sweep * A.m * 3 + r];
      const REAL wr = tfma(A.cfm, xv, row_dot(j0, a0, j1, a1)) - rhs;
      if (write_sweep == sweep + 1) A.wres[r] = wr;
      const double w = (double)wr;
      if (FRIC && mu >= REAL(0)) {
        double s_lo = 0, s_hi = 0, s_in = 0;
        pyramid_residual(xv, w, mu, A.hist_x[(size_t)sweep * A.m * 3 + 3 * i + 2], s_lo, s_hi, s_in);
        acc[g][1] += s_lo; acc[g][2] += s_hi; acc[g][3] += s_in;
      } else if (eq) acc[g][0] += w * w;
      else {
        if (xv == l && w < 0 && l != h) acc[g][1] += w * w;
        if (xv == h && w > 0 && l != h) acc[g][2] += w * w;
        if (xv > l && xv < h) acc[g][3] += w * w;
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int sweep = s0 + g;
    if (sweep >= sweeps) break;
    __syncthreads();
    red[0][threadIdx.x] = acc[g][0]; red[1][threadIdx.x] = acc[g][1]; red[2][threadIdx.x] = acc[g][2]; red[3][threadIdx.x] = acc[g][3];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s)
        for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x < 4) out[((size_t)sweep * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = red[threadIdx.x][0];
  }
}

// --------------------------------------------------------------------------
// Batched worlds: the residual of each ensemble on its own (kernels.h, launch_seg_residual).  One
// workgroup per (ensemble, sweep) replays the stand-alone reduction: local row lr of the ensemble is
// added by thread lr % 256 of block (lr / 256) % kResidualBlocks in ascending lr, each block reduces as
// residual_partials_kernel does, and the block sums are added in block order as read_residual adds them.
// Blocks beyond the ensemble's rows would contribute +0.0 to sums that are >= 0 (or NaN): skipped.
template <typename REAL, bool FRIC = false>
__global__ void __launch_bounds__(256) seg_residual_kernel(const SolveArgs<REAL> A, const EnsembleSegs S, const int32_t *running,
                                                           const REAL *xs, const REAL *as, const REAL *ws, double *err) {
  __shared__ double red[4][256];
  const int e = blockIdx.x, sweep = blockIdx.y, t = threadIdx.x;
  if (running && !running[e]) return;
  const int j0 = S.jo[e], mje = S.jo[e + 1] - j0;
  const int c0 = S.mj + S.co[e], mce = S.co[e + 1] - S.co[e];
  const int rows = 3 * (mje + mce), jrows = 3 * mje;
  const REAL *hx = xs + (size_t)sweep * A.m * 3;
  const REAL *ha = ws ? nullptr : as + (size_t)sweep * A.n_bodies * 6;
  const int nblk = min(kResidualBlocks, (rows + 255) / 256);
  double sum[4] = {0, 0, 0, 0};
  for (int blk = 0; blk < nblk; ++blk) {
    double acc[4] = {0, 0, 0, 0};
    for (int lr = blk * 256 + t; lr < rows; lr += kResidualBlocks * 256) {
      const int r = lr < jrows ? 3 * j0 + lr : 3 * c0 + (lr - jrows);
      const REAL xv = hx[r], l = A.lo[r], h = A.hi[r];
      double w;
      if (ws) {
        w = (double)ws[r];
      } else {   // hist_residual_kernel's expression
        const int i = r / 3, rr = r - 3 * i;
        const int b0 = A.body0[i], b1 = A.body1[i];
        REAL j0v[6], j1v[6], a0[6], a1[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          j0v[k] = b0 >= 0 ? A.J0[(size_t)i * 18 + 6 * rr + k] : REAL(0);
          j1v[k] = b1 >= 0 ? A.J1[(size_t)i * 18 + 6 * rr + k] : REAL(0);
          a0[k] = b0 >= 0 ? ha[(size_t)b0 * 6 + k] : REAL(0);
          a1[k] = b1 >= 0 ? ha[(size_t)b1 * 6 + k] : REAL(0);
        }
        w = (double)(tfma(A.cfm, xv, row_dot(j0v, a0, j1v, a1)) - A.rhs[r]);
      }
      if (FRIC && r % 3 < 2 && A.mu[r / 3] >= REAL(0)) {
        double s_lo = 0, s_hi = 0, s_in = 0;
        pyramid_residual(xv, w, A.mu[r / 3], hx[r - r % 3 + 2], s_lo, s_hi, s_in);
        acc[1] += s_lo; acc[2] += s_hi; acc[3] += s_in;
      } else if (A.is_eq[r]) acc[0] += w * w;
      else {
        if (xv == l && w < 0 && l != h) acc[1] += w * w;
        if (xv == h && w > 0 && l != h) acc[2] += w * w;
        if (xv > l && xv < h) acc[3] += w * w;
      }
    }
    __syncthreads();   // thread 0 has read the previous block's sums
    red[0][t] = acc[0]; red[1][t] = acc[1]; red[2][t] = acc[2]; red[3][t] = acc[3];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s)
        for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + s];
      __syncthreads();
    }
    if (t == 0)
      for (int k = 0; k < 4; ++k) sum[k] += red[k][0];
  }
  if (t == 0) err[(size_t)sweep * S.n_ens + e] = sqrt(sum[0]) + (sqrt(sum[1]) + sqrt(sum[2]) + sqrt(sum[3]));
}

// One workgroup per ensemble: the stopping test (thread 0), then the chosen state's rows (all threads).
// Only thread 0 reads or writes the ensemble's state; the other threads learn the outcome from s_pick
// after the barrier (-1: still running or already stopped, nothing to copy).
template <typename REAL>
__global__ void __launch_bounds__(256) seg_select_kernel(const EnsembleSegs S, const EnsembleStop T, const double *err, int sweeps,
                                                         int first, int max_iters, int every, double tol, int all_checked,
                                                         int init, const REAL *xs, size_t xstride, const REAL *as,
                                                         size_t astride, REAL *fin_x, REAL *fin_acc) {
  __shared__ int s_pick;
  const int e = blockIdx.x, t = threadIdx.x;
  if (t == 0) s_pick = -1;
  if (t == 0 && (init || T.running[e])) {
    int pick = -1;
    double res = init ? 0.0 : T.residual[e];
    for (int k = 0; k < sweeps; ++k) {
      const int sw = first + k;
      if (!(all_checked || sw % every == 0 || sw == max_iters)) continue;
      res = err[(size_t)k * S.n_ens + e];
      if (!(res > tol)) { pick = k; break; }   // as the reference's loop condition: NaN stops too
    }
    if (pick < 0 && first + sweeps - 1 >= max_iters) pick = sweeps - 1;
    T.residual[e] = res;
    if (pick >= 0) { T.iterations[e] = first + pick; T.running[e] = 0; }
    else { T.running[e] = 1; atomicAdd(T.n_running, 1); }
    s_pick = pick;
  }
  __syncthreads();
  const int pick = s_pick;
  if (pick < 0) return;
  const REAL *x = xs + (size_t)pick * xstride, *a = as + (size_t)pick * astride;
  const size_t jb = (size_t)3 * S.jo[e], jn = (size_t)3 * (S.jo[e + 1] - S.jo[e]);
  const size_t cb = (size_t)3 * (S.mj + S.co[e]), cn = (size_t)3 * (S.co[e + 1] - S.co[e]);
  const size_t bb = (size_t)6 * S.bo[e], bn = (size_t)6 * (S.bo[e + 1] - S.bo[e]);
  for (size_t r = t; r < jn; r += 256) fin_x[jb + r] = x[jb + r];
  for (size_t r = t; r < cn; r += 256) fin_x[cb + r] = x[cb + r];
  for (size_t q = t; q < bn; q += 256) fin_acc[bb + q] = a[bb + q];
}

__global__ void __launch_bounds__(256) seg_fixed_kernel(const EnsembleSegs S, const EnsembleStop T, const double *err, int sweeps) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= S.n_ens) return;
  const bool any = S.jo[e + 1] > S.jo[e] || S.co[e + 1] > S.co[e];
  T.iterations[e] = any ? sweeps : 0;   // a world without constraints does not solve (sparse_iterations.cc:152-154)
  T.residual[e] = err[e];
  T.running[e] = 0;
}

// --------------------------------------------------------------------------
// K9: v_new = v + dt (W f_ext + a)        (ensembles.cc:535, 572)
template <typename REAL>
__global__ void __launch_bounds__(256) velocity_kernel(int n, const double *v, const double *w, const double *Wf,
                                                       const REAL *acc, double dt, double *v6) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // one lane per (body, component): every access contiguous
  if (e >= 6 * n) return;
  const int b = e / 6, r = e - 6 * b;
  const double vel = r < 3 ? v[(size_t)b * 3 + r] : w[(size_t)b * 3 + r - 3];
  v6[e] = vel + dt * (Wf[e] + (double)acc[e]);
}
// ... with each body's own dt (egs_world_step_each); a body that sits the step out keeps its velocity
template <typename REAL>
__global__ void __launch_bounds__(256) velocity_each_kernel(int n, const double *v, const double *w, const double *Wf,
                                                            const REAL *acc, const int32_t *body_ens, const double *dt_each,
                                                            double *v6) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 6 * n) return;
  const int b = e / 6, r = e - 6 * b;
  const double vel = r < 3 ? v[(size_t)b * 3 + r] : w[(size_t)b * 3 + r - 3];
  const double dt = dt_each[body_ens[b]];
  v6[e] = dt == 0.0 ? vel : vel + dt * (Wf[e] + (double)acc[e]);
}

// Wf = M^-1 f_ext per body, the expression of ComputeVDot's M_inverse_ * external_force_torque_
// restricted to the diagonal block (ensembles.cc:535)
__global__ void __launch_bounds__(256) mass_times_force_kernel(int n, const double *Minv, const double *f_ext, double *Wf) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 6 * n) return;
  const int b = e / 6, r = e - 6 * b;
  const double *M = Minv + (size_t)b * 36 + 6 * r, *f = f_ext + (size_t)b * 6;
  Wf[e] = ((((M[0] * f[0] + M[1] * f[1]) + M[2] * f[2]) + M[3] * f[3]) + M[4] * f[4]) + M[5] * f[5];
}

// Live inertia: what Ensemble::Init (ensembles.cc:202-222) would compute at the R and w the
// device holds now, for every body the mask selects (inertia_body not a multiple of the identity).  One lane per body.
// Operation order is that of orc_minv_blocks / orc_external_force (oracle/model.c) with mat3_inv (oracle/linalg.h):
// I_g = (R I_b) R^T, its inverse by cofactors, the gyroscopic torque ((-[w]x) I_g) w.  The lane writes the angular
// 3x3 of its fp64 block and of the working-precision one (the (REAL) of the fp64 value, as convert_kernel gives),
// f_ext[3:6] (+ torque[b] where an applied torque is given) and its six rows of Wf in mass_times_force_kernel's
// expression.  The linear rows of M^-1 and f_ext are read, never written.
template <typename REAL>
__global__ void __launch_bounds__(256) live_mass_kernel(int n, const double *R, const double *w, const double *inertia_body,
                                                        const double *torque, const uint8_t *live_mask, double *Minv,
                                                        REAL *Minv_r, double *f_ext, double *Wf) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n || !live_mask[b]) return;
  double Rb[9], Ib[9], wb[3], RI[9], Rt[9], Ig[9], cm[9], t[9], tq[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) { Rb[k] = R[(size_t)b * 9 + k]; Ib[k] = inertia_body[(size_t)b * 9 + k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) wb[k] = w[(size_t)b * 3 + k];
  mm3(Rb, Ib, RI);   // body.h:58: R I R^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rt[3 * i + j] = Rb[3 * j + i];
  mm3(RI, Rt, Ig);
  double *M = Minv + (size_t)b * 36;
  REAL *Mr = Minv_r + (size_t)b * 36;
  {  // mat3_inv
    const double c00 = Ig[4] * Ig[8] - Ig[5] * Ig[7];
    const double c10 = Ig[5] * Ig[6] - Ig[3] * Ig[8];
    const double c20 = Ig[3] * Ig[7] - Ig[4] * Ig[6];
    const double det = (Ig[0] * c00 + Ig[1] * c10) + Ig[2] * c20;
    const double id = 1.0 / det;
    double inv[9];
    inv[0] = c00 * id;
    inv[1] = (Ig[2] * Ig[7] - Ig[1] * Ig[8]) * id;
    inv[2] = (Ig[1] * Ig[5] - Ig[2] * Ig[4]) * id;
    inv[3] = c10 * id;
    inv[4] = (Ig[0] * Ig[8] - Ig[2] * Ig[6]) * id;
    inv[5] = (Ig[2] * Ig[3] - Ig[0] * Ig[5]) * id;
    inv[6] = c20 * id;
    inv[7] = (Ig[1] * Ig[6] - Ig[0] * Ig[7]) * id;
    inv[8] = (Ig[0] * Ig[4] - Ig[1] * Ig[3]) * id;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        M[6 * (3 + r) + 3 + c] = inv[3 * r + c];
        Mr[6 * (3 + r) + 3 + c] = (REAL)inv[3 * r + c];
      }
  }
  crossmat(wb, cm);
#pragma unroll
  for (int k = 0; k < 9; ++k) cm[k] = -1.0 * cm[k];
  mm3(cm, Ig, t);
  mv3(t, wb, tq);
  double f[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f[k] = f_ext[(size_t)b * 6 + k];
    f[3 + k] = torque ? torque[(size_t)b * 3 + k] + tq[k] : tq[k];
    f_ext[(size_t)b * 6 + 3 + k] = f[3 + k];
  }
  // the block as it stands now: its own stores above are visible to the lane that made them
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double *Mrow = M + 6 * r;
    Wf[(size_t)b * 6 + r] = ((((Mrow[0] * f[0] + Mrow[1] * f[1]) + Mrow[2] * f[2]) + Mrow[3] * f[3]) + Mrow[4] * f[4]) + Mrow[5] * f[5];
  }
}

// StepPositions_ODE (ensembles.cc:577-591): p += dt (v + v_new)/2,
// R = Q(dt (w + w_new)/2) R with Q = WtoQ (utils.cc:82-89); then the new
// velocities become the body state for the next step.
// The state is read from `in` and written to `out`: the same arrays (in place), or a second set, which leaves the state
// the step started from intact (egs_problem_advance after a step whose system is deferred).
// EACH: in place (in == out), body b by dt_each[body_ens[b]]; dt 0 = the body is left alone
template <bool EACH>
__device__ __forceinline__ void advance_body(int n, const BodyState &in, const BodyState &out, const double *v6, double dt,
                                             const int32_t *body_ens, const double *dt_each) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  if (EACH) {
    dt = dt_each[body_ens[b]];
    if (dt == 0.0) return;
  }
  double wm[3], Rb[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rb[k] = in.R[(size_t)b * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vm = (in.v[(size_t)b * 3 + k] + v6[(size_t)b * 6 + k]) / 2.0;
    out.pos[(size_t)b * 3 + k] = in.pos[(size_t)b * 3 + k] + dt * vm;
    wm[k] = (in.w[(size_t)b * 3 + k] + v6[(size_t)b * 6 + 3 + k]) / 2.0;
  }
  rotate_by_w(wm, dt, Rb);
#pragma unroll
  for (int k = 0; k < 9; ++k) out.R[(size_t)b * 9 + k] = Rb[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { out.v[(size_t)b * 3 + k] = v6[(size_t)b * 6 + k]; out.w[(size_t)b * 3 + k] = v6[(size_t)b * 6 + 3 + k]; }
}
__global__ void __launch_bounds__(256) advance_kernel(int n, const BodyState in, const BodyState out, const double *v6, double dt) {
  advance_body<false>(n, in, out, v6, dt, nullptr, nullptr);
}
__global__ void __launch_bounds__(256) advance_each_kernel(int n, const BodyState state, const double *v6,
                                                           const int32_t *body_ens, const double *dt_each) {
  advance_body<true>(n, state, state, v6, 0.0, body_ens, dt_each);
}

template <typename REAL>
__global__ void __launch_bounds__(256) fill_friction_kernel(int m, int mj, const int32_t *body0, const int32_t *body1,
                                                            const int32_t *body_ens, const double *mu_ens, REAL *mu) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int b = body0[i] >= 0 ? body0[i] : body1[i];   // as constraint_rates: the first body's ensemble
  mu[i] = i < mj ? REAL(-1) : (REAL)mu_ens[body_ens ? body_ens[b] : 0];
}

template <typename REAL>
__global__ void __launch_bounds__(256) convert_kernel(int count, const double *src, REAL *dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < count) dst[i] = (REAL)src[i];
}

// flag &= every 6x6 block is diag(a, a, a, b, b, b) exactly (the tile kernel's ISO variant)
template <typename REAL>
__global__ void __launch_bounds__(256) minv_iso_kernel(int n, const REAL *W, int *flag) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  bool iso = true;
  if (b < n) {
    const REAL *w = W + (size_t)b * 36;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        const REAL v = w[6 * r + c];
        if (r != c) iso &= (v == REAL(0));
        else iso &= (v == w[r < 3 ? 0 : 21]);
      }
  }
  if (!iso) atomicAnd(flag, 0);
}

__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }
__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

template <typename REAL>
__global__ void __launch_bounds__(256) linsym_bodies_kernel(int m, const int32_t *body0, const int32_t *body1, const REAL *W, int *flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool ok = true;
  if (i < m) {
    const int b0 = body0[i], b1 = body1[i];
    ok = b1 >= 0;
    if (ok && b0 >= 0) ok = same_bits(W[(size_t)b0 * 36], W[(size_t)b1 * 36]);
  }
  if (!ok) atomicAnd(flag, 0);
}

// thread i = pair l of wavefront w of tile t, i = (4 t + w) * 32 + l: plan lanes 64 w + l and 64 w + 32 + l.
// Bit 0 of *flag: every pair carries one normal (SHARE); bit 1, read with bit 0: the first of an odd w's pair also
// carries that of the pair 64 lanes below, member 0 of its group of four (FACE: plan.h, plan_faces_normals).
__global__ void __launch_bounds__(256) share_normals_kernel(int n_pairs, const LaneDesc *lanes, const double *data, int *flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pairs) return;
  const size_t ia = (size_t)(i >> 5) * 64 + (i & 31);
  const int a = lanes[ia].cidx, b = lanes[ia + 32].cidx;
  if (a < 0 || b < 0) return;
  const double *na = data + (size_t)a * 7 + 3, *nb = data + (size_t)b * 7 + 3;
  if (!(same_bits(na[0], nb[0]) && same_bits(na[1], nb[1]) && same_bits(na[2], nb[2]))) atomicAnd(flag, 0);
}
// ... the pairs' firsts: a group's member 2 against its member 0 (a member 2 without a member 3 is no pair above)
__global__ void __launch_bounds__(256) face_normals_kernel(int n_pairs, const LaneDesc *lanes, const double *data, int *flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pairs || !((i >> 5) & 1)) return;
  const size_t ic = (size_t)(i >> 5) * 64 + (i & 31);
  const int a = lanes[ic - 64].cidx, c = lanes[ic].cidx;
  if (a < 0 || c < 0) return;
  const double *na = data + (size_t)a * 7 + 3, *nc = data + (size_t)c * 7 + 3;
  if (!(same_bits(na[0], nc[0]) && same_bits(na[1], nc[1]) && same_bits(na[2], nc[2]))) atomicAnd(flag, ~2);
}

// --------------------------------------------------------------------------
// K1-K4 assembly: the per-constraint body lives in assemble_device.h.
struct NoRates {};   // the scalar form's (empty) second argument
// EACH: dt and erp per constraint from its ensemble's (T); an ensemble that sits the step out (dt 0) gets rhs rows of
// exactly 0, its blocks, err, bounds and row types as always.  REST: restitution on the normal rows (A.rest is set);
// an instantiation of its own, so that the launches without it keep their registers.  motor: the hinge motors'
// table (assemble_device.h: motor_row), NULL = off; read by hinge-axis lanes only.  ANGULAR: the list holds an angular
// block (LOCK, HINGE_AXIS); without one the launch runs the instantiation that leaves them and the motors out, with
// the registers and the occupancy it had before they existed.  LIMITS: the hinge limits' table (assemble_device.h:
// limit_row) is set; an instantiation of the ANGULAR form of its own, so that the lists without a stop run the code
// they ran before the limits.  A row whose stop is active is the limit's for the step: the motor leaves it alone.
// SLIDER: the list holds an EGS_JOINT_SLIDER_AXIS; the form with the slider block beside every other, launched for such
// a list only.  Its tables are run-time pointers, NULL = off: motor (hinges and sliders), limit (the hinge limits) and
// travel (the sliders' stops, assemble_device.h: slider_stop_row), the last an argument of this form alone (SliderArg).
struct NoTravel {};
template <bool SLIDER> struct SliderArg { using type = NoTravel; };
template <> struct SliderArg<true> { using type = const double *; };
template <typename REAL, bool EACH, typename RATES, bool REST, bool ANGULAR, bool LIMITS = false, bool SLIDER = false>
__global__ void __launch_bounds__(256) assemble_kernel(const AssembleArgs A, const RATES T, const double *motor,
                                                       const double *limit, const typename SliderArg<SLIDER>::type travel) {
  // J blocks leave through LDS: a lane's 18 values are 144 B apart from its neighbour's, so direct
  // stores hit 64 lines per instruction; staged, the workgroup writes its 256 x 18 block contiguously
  __shared__ REAL stage[256 * 19];   // row stride 19: conflict-free column walks
  const int i_raw = blockIdx.x * 256 + threadIdx.x;
  const bool live = i_raw < A.m;
  const int i = live ? i_raw : A.m - 1;   // the tail lanes recompute the last constraint and store nothing
  double j0[18], j1[18], e[3], lo[3], hi[3], u0[6], u1[6];
  bool eq[3];
  double dt = 0.0, erp = 0.0;   // EACH: the constraint's own; otherwise A.dt / A.erp where they are used
  if constexpr (EACH) constraint_rates(A, T, i, dt, erp);
  // the stop's row first, while nothing else is live: three values and a flag wait for the block
  bool stopped = false;
  double stop_err = 0.0, stop_lo = 0.0, stop_hi = 0.0;
  if constexpr (LIMITS) stopped = limit_row(A, limit, i, stop_err, stop_lo, stop_hi);
  if constexpr (SLIDER) {
    if (limit != nullptr) stopped = limit_row(A, limit, i, stop_err, stop_lo, stop_hi);
    if (travel != nullptr && !stopped) stopped = slider_stop_row(A, travel, i, stop_err, stop_lo, stop_hi);
  }
  assemble_one_t<EACH, ANGULAR, SLIDER>(A, i, dt, j0, j1, e, lo, hi, eq, u0, u1);
  if ((LIMITS || SLIDER) && stopped) { e[2] = stop_err; lo[2] = stop_lo; hi[2] = stop_hi; }
  REAL *J0o = reinterpret_cast<REAL *>(A.J0), *J1o = reinterpret_cast<REAL *>(A.J1);
  REAL *loo = reinterpret_cast<REAL *>(A.lo), *hio = reinterpret_cast<REAL *>(A.hi);
  REAL *rhso = reinterpret_cast<REAL *>(A.rhs);
  {
    const int first = blockIdx.x * 256;
    const int count = (A.m - first) < 256 ? (A.m - first) : 256;
#pragma unroll
    for (int k = 0; k < 18; ++k) stage[threadIdx.x * 19 + k] = (REAL)j0[k];
    __syncthreads();
    for (int e = threadIdx.x; e < count * 18; e += 256) J0o[(size_t)first * 18 + e] = stage[(e / 18) * 19 + e % 18];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 18; ++k) stage[threadIdx.x * 19 + k] = (REAL)j1[k];
    __syncthreads();
    for (int e = threadIdx.x; e < count * 18; e += 256) J1o[(size_t)first * 18 + e] = stage[(e / 18) * 19 + e % 18];
  }
  if (!live) return;
  double motor_rhs = 0.0;
  const bool motored = ANGULAR && !stopped && motor != nullptr && motor_row<EACH, SLIDER>(A, motor, i, dt, j0, j1, u0, u1, lo, hi, motor_rhs);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (r == 2 && motored)
      rhso[(size_t)i * 3 + r] = (EACH && dt == 0.0) ? REAL(0) : (REAL)motor_rhs;
    else if (REST && r == 2)
      rhso[(size_t)i * 3 + r] = (EACH && dt == 0.0) ? REAL(0) : (REAL)assemble_rhs_bounce_t<EACH>(A, i, dt, erp, j0, j1, e, u0, u1);
    else
      rhso[(size_t)i * 3 + r] = (EACH && dt == 0.0) ? REAL(0) : (REAL)assemble_rhs_t<EACH>(A, dt, erp, j0, j1, e, u0, u1, r);
    A.err[(size_t)i * 3 + r] = e[r];
    loo[(size_t)i * 3 + r] = (REAL)lo[r];
    hio[(size_t)i * 3 + r] = (REAL)hi[r];
    A.is_eq[(size_t)i * 3 + r] = eq[r] ? 1 : 0;
  }
}


// --------------------------------------------------------------------------
// Cross-workgroup path: islands larger than a tile.  Same ticket protocol, but
// body accumulators and tickets live in global memory and the lanes of a
// persistent grid (<= one 256-thread workgroup per CU, so every workgroup is
// resident) each own a strided slice of the constraint list.  Hand-off between
// workgroups: sc1 (write-through) payload stores -> s_waitcnt vmcnt(0) -> sc1
// ticket store; sc1 ticket poll -> sc1 payload loads, all by the same lane.
// Every wait is bounded.
// B = W J^T, D, den per global constraint; x0 = rhs or the given start; dx workspace = x0.
template <typename REAL>
__global__ void __launch_bounds__(256) global_prepare_kernel(const GlobalArgs<REAL> A) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= A.mg) return;
  const GlobalDesc d = A.cons[g];
  SolveArgs<REAL> S;
  S.Minv = A.Minv; S.J0 = A.J0; S.J1 = A.J1; S.is_eq = A.is_eq; S.lo = A.lo; S.hi = A.hi; S.rhs = A.rhs;
  S.cfm = A.cfm; S.kscale = A.kscale;
  Cons<REAL> c;
  load_cons(S, d.cidx, d.body0 >= 0, d.body1 >= 0, d.body0, d.body1, c);
#pragma unroll
  for (int k = 0; k < 18; ++k) { A.B0[(size_t)g * 18 + k] = c.B0[k]; A.B1[(size_t)g * 18 + k] = c.B1[k]; }
#pragma unroll
  for (int k = 0; k < 9; ++k) A.D[(size_t)g * 9 + k] = c.D[k];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    A.den[(size_t)g * 3 + r] = c.inv[r];
    const REAL x0 = A.x0 ? A.x0[(size_t)d.cidx * 3 + r] : c.rhs[r];   // a given start, or rhs (Q7)
    if (!A.resume) A.x[(size_t)d.cidx * 3 + r] = x0;
    A.dx[(size_t)g * 3 + r] = A.resume ? REAL(0) : x0;
  }
}

// B = W J^T, D, 1/den for every constraint, indexed by list position (quad path).
template <typename REAL>
__global__ void __launch_bounds__(256) cons_prepare_kernel(const SolveArgs<REAL> A) {
  __shared__ REAL stage[256 * 19];   // the outputs leave through LDS, contiguously (see assemble_kernel)
  const int i_raw = blockIdx.x * 256 + threadIdx.x;
  const int i = i_raw < A.m ? i_raw : A.m - 1;
  const int first = blockIdx.x * 256;
  const int count = (A.m - first) < 256 ? (A.m - first) : 256;
  const int b0 = A.body0[i], b1 = A.body1[i];
  Cons<REAL> c;
  load_cons(A, i, b0 >= 0, b1 >= 0, b0, b1, c);
  auto flush = [&](const REAL *vals, int per, REAL *out) {
    for (int k = 0; k < per; ++k) stage[threadIdx.x * 19 + k] = vals[k];
    __syncthreads();
    for (int e = threadIdx.x; e < count * per; e += 256) out[(size_t)first * per + e] = stage[(e / per) * 19 + e % per];
    __syncthreads();
  };
  flush(c.B0, 18, A.wsB0);
  flush(c.B1, 18, A.wsB1);
  flush(c.D, 9, A.wsD);
  flush(c.inv, 3, A.wsInv);
}

template <typename REAL, bool FRIC = false>
__device__ __forceinline__ void gload_cons(const GlobalArgs<REAL> &A, int g, const GlobalDesc &d, Cons<REAL> &c) {
  const bool has0 = d.body0 >= 0, has1 = d.body1 >= 0;
#pragma unroll
  for (int k = 0; k < 18; ++k) {
    c.J0[k] = has0 ? A.J0[(size_t)d.cidx * 18 + k] : REAL(0);
    c.J1[k] = has1 ? A.J1[(size_t)d.cidx * 18 + k] : REAL(0);
    c.B0[k] = A.B0[(size_t)g * 18 + k];
    c.B1[k] = A.B1[(size_t)g * 18 + k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) c.D[k] = A.D[(size_t)g * 9 + k];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    c.inv[r] = A.den[(size_t)g * 3 + r];
    c.rhs[r] = A.rhs[(size_t)d.cidx * 3 + r];
    c.lo[r] = A.lo[(size_t)d.cidx * 3 + r];
    c.hi[r] = A.hi[(size_t)d.cidx * 3 + r];
    c.eq[r] = A.is_eq[(size_t)d.cidx * 3 + r] != 0;
    clamp_bounds(c.eq[r], c.lo[r], c.hi[r]);
  }
  if (FRIC) {
    const REAL mu = A.mu[d.cidx];
    c.pyr = mu >= REAL(0);
    if (c.pyr) c.lo[0] = mu;
  }
}

template <typename REAL, int METHOD, bool FRIC = false>
__global__ void __launch_bounds__(256) global_solve_kernel(const GlobalArgs<REAL> A) {
  const int L = gridDim.x * 256, lane = blockIdx.x * 256 + threadIdx.x;
  const int per_lane = A.per_lane;
  const bool rel = A.resume || A.mode == 1;  // tickets start at 0 for this launch's first phase
  int p = (A.resume && A.mode == 0) ? 1 : 0; // phase 0 = ordered accumulate of dx
  const int p_last = A.mode == 1 ? 0 : A.sweeps;
  int k = 0;
  bool ok = true;
  unsigned spins = 0;
  bool alive = p <= p_last;
  while (alive) {
    const bool backward = (METHOD == 2) && p >= 1;
    const int kk = backward ? per_lane - 1 - k : k;
    const int g = kk * L + lane;
    bool advance = false, ready = false;
    if (g >= A.mg) {
      advance = true;
    } else {
      const GlobalDesc d = A.cons[g];
      const bool has0 = d.body0 >= 0, has1 = d.body1 >= 0;
      const unsigned cnt0 = d.cnt0, cnt1 = d.cnt1, pos0 = d.pos0, pos1 = d.pos1;
      unsigned want0, want1;
      const unsigned o0 = backward ? cnt0 - 1u - pos0 : pos0, o1 = backward ? cnt1 - 1u - pos1 : pos1;
      if (p == 0) { want0 = pos0; want1 = pos1; }
      else {
        want0 = (rel ? 0u : cnt0) + (unsigned)(p - 1) * cnt0 + o0;
        want1 = (rel ? 0u : cnt1) + (unsigned)(p - 1) * cnt1 + o1;
      }
      const unsigned t0 = has0 ? gld(A.tickets + d.body0) : want0;
      const unsigned t1 = has1 ? gld(A.tickets + d.body1) : want1;
      ready = (t0 == want0) && (t1 == want1);
      if (ready) {
        // Every hand-off byte is stored sc1 (write-through, gst) and loaded sc1
        // (L1-bypassing, gld), and the storing lane drains vmcnt before it bumps
        // the ticket, so no L1 invalidate / L2 write-back is needed (guide G16,
        // "sc1 both sides"); the wavefront-scope fence only pins compiler order.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        REAL a0[6], a1[6], dx[3];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          a0[q] = has0 ? gld(A.acc + (size_t)d.body0 * 6 + q) : REAL(0);
          a1[q] = has1 ? gld(A.acc + (size_t)d.body1 * 6 + q) : REAL(0);
        }
        Cons<REAL> c;
        gload_cons<REAL, FRIC>(A, g, d, c);
        if (p == 0) {
#pragma unroll
          for (int r = 0; r < 3; ++r) dx[r] = A.dx[(size_t)g * 3 + r];
        } else {
          REAL x[3], res[3];
#pragma unroll
          for (int r = 0; r < 3; ++r) { x[r] = A.x[(size_t)d.cidx * 3 + r]; dx[r] = REAL(0); }
          row_residuals(c, a0, a1, x, A.cfm, res);
          update_rows<REAL, METHOD, false, FRIC>(c, res, x, dx);
#pragma unroll
          for (int r = 0; r < 3; ++r) A.x[(size_t)d.cidx * 3 + r] = x[r];
        }
        if (has0) {
          acc_add(a0, c.B0, dx);
#pragma unroll
          for (int q = 0; q < 6; ++q) gst(A.acc + (size_t)d.body0 * 6 + q, a0[q]);
        }
        if (has1) {
          acc_add(a1, c.B1, dx);
#pragma unroll
          for (int q = 0; q < 6; ++q) gst(A.acc + (size_t)d.body1 * 6 + q, a1[q]);
        }
        if (A.hist_x && p >= 1) {   // snapshots for the per-sweep stopping test (kernels.h)
          const size_t sw = (size_t)(p - 1);
#pragma unroll
          for (int r = 0; r < 3; ++r) A.hist_x[(sw * A.m + d.cidx) * 3 + r] = A.x[(size_t)d.cidx * 3 + r];
          if (has0 && o0 == cnt0 - 1u) {   // this was the body's last update of the sweep
#pragma unroll
            for (int q = 0; q < 6; ++q) A.hist_acc[(sw * A.n_bodies + d.body0) * 6 + q] = a0[q];
          }
          if (has1 && o1 == cnt1 - 1u) {
#pragma unroll
            for (int q = 0; q < 6; ++q) A.hist_acc[(sw * A.n_bodies + d.body1) * 6 + q] = a1[q];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (has0) gst(A.tickets + d.body0, want0 + 1u);
        if (has1) gst(A.tickets + d.body1, want1 + 1u);
        advance = true;
        spins = 0;
      } else if (++spins > A.spin_limit) {
        ok = false;
        alive = false;
      }
    }
    if (advance) {
      if (++k == per_lane) { k = 0; ++p; }
      alive = alive && p <= p_last;
    }
    if (!__any(ready)) __builtin_amdgcn_s_sleep(2);
  }
  if (!ok) atomicOr(A.error_flag, 1);
}

// Jacobi compute phase for the cross-workgroup path: x_new and dx from the
// accumulators of the previous sweep (no ordering needed: read-only on acc).
template <typename REAL, bool FRIC = false>
__global__ void __launch_bounds__(256) global_jacobi_kernel(const GlobalArgs<REAL> A) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= A.mg) return;
  const GlobalDesc d = A.cons[g];
  Cons<REAL> c;
  gload_cons<REAL, FRIC>(A, g, d, c);
  REAL a0[6], a1[6], x[3], res[3], dx[3];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    a0[q] = d.body0 >= 0 ? A.acc[(size_t)d.body0 * 6 + q] : REAL(0);
    a1[q] = d.body1 >= 0 ? A.acc[(size_t)d.body1 * 6 + q] : REAL(0);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) x[r] = A.x[(size_t)d.cidx * 3 + r];
  row_residuals(c, a0, a1, x, A.cfm, res);
  update_rows<REAL, 0, false, FRIC>(c, res, x, dx);
#pragma unroll
  for (int r = 0; r < 3; ++r) { A.x[(size_t)d.cidx * 3 + r] = x[r]; A.dx[(size_t)g * 3 + r] = dx[r]; }
}

// w = A x - rhs for the cross-workgroup constraints, after the last sweep.
template <typename REAL>
__global__ void __launch_bounds__(256) global_wres_kernel(const GlobalArgs<REAL> A) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= A.mg) return;
  const GlobalDesc d = A.cons[g];
  REAL a0[6], a1[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    a0[q] = d.body0 >= 0 ? A.acc[(size_t)d.body0 * 6 + q] : REAL(0);
    a1[q] = d.body1 >= 0 ? A.acc[(size_t)d.body1 * 6 + q] : REAL(0);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    REAL j0[6], j1[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      j0[q] = d.body0 >= 0 ? A.J0[(size_t)d.cidx * 18 + 6 * r + q] : REAL(0);
      j1[q] = d.body1 >= 0 ? A.J1[(size_t)d.cidx * 18 + 6 * r + q] : REAL(0);
    }
    A.wres[(size_t)d.cidx * 3 + r] = tfma(A.cfm, A.x[(size_t)d.cidx * 3 + r], row_dot(j0, a0, j1, a1)) - A.rhs[(size_t)d.cidx * 3 + r];
  }
}

}  // namespace

// --------------------------------------------------------------------------
// Dense J M^-1 J^T + cfm I (ensembles.cc:510, 513-521) from the block-sparse form: one lane per
// pair of constraints writes the 3x3 block (zero when the two share no body).  O(m^2) like the
// reference's dense product, for the sizes its dense solver is meant for (Chain / Cairn).
__global__ void __launch_bounds__(256) dense_system_kernel(int m, const int32_t *body0, const int32_t *body1,
                                                           const double *J0, const double *J1, const double *Minv,
                                                           double cfm, double *A) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)m * m) return;
  const int i = (int)(idx / m), j = (int)(idx % m);
  double blk[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int si = 0; si < 2; ++si) {
    const int bi = si ? body1[i] : body0[i];
    if (bi < 0) continue;
    for (int sj = 0; sj < 2; ++sj) {
      const int bj = sj ? body1[j] : body0[j];
      if (bj != bi) continue;
      const double *Ji = (si ? J1 : J0) + (size_t)i * 18, *Jj = (sj ? J1 : J0) + (size_t)j * 18, *W = Minv + (size_t)bi * 36;
      double t[18];   // W Jj^T, 6x3
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          double v = W[6 * k] * Jj[6 * q];
#pragma unroll
          for (int l = 1; l < 6; ++l) v = __builtin_fma(W[6 * k + l], Jj[6 * q + l], v);
          t[3 * k + q] = v;
        }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          double v = blk[3 * r + q];
#pragma unroll
          for (int k = 0; k < 6; ++k) v = __builtin_fma(Ji[6 * r + k], t[3 * k + q], v);
          blk[3 * r + q] = v;
        }
    }
  }
  if (i == j) { blk[0] += cfm; blk[4] += cfm; blk[8] += cfm; }
  const size_t N = (size_t)3 * m;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) A[((size_t)3 * i + r) * N + 3 * j + q] = blk[3 * r + q];
}

// ---- launchers ------------------------------------------------------------
void launch_dense_system(int m, const int32_t *body0, const int32_t *body1, const double *J0, const double *J1,
                         const double *Minv, double cfm, double *A, hipStream_t s) {
  if (m <= 0) return;
  const size_t pairs = (size_t)m * m;
  hipLaunchKernelGGL(dense_system_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, m, body0, body1, J0, J1, Minv, cfm, A);
}

template <typename REAL>
void launch_tile_solve(const SolveArgs<REAL> &a, int method, int n_tiles, int block, hipStream_t s) {
  if (n_tiles <= 0) return;
  const size_t lds = (size_t)a.max_slots * (6 * sizeof(REAL) + sizeof(unsigned));
  const dim3 g(n_tiles), b(block);
#define EGS_LAUNCH_TF(BLK, ISO, FRIC)                                                                     \
  switch (method) {                                                                                       \
    case 0: hipLaunchKernelGGL((tile_solve_kernel<REAL, BLK, 0, ISO, FRIC>), g, b, lds, s, a); break;     \
    case 1: hipLaunchKernelGGL((tile_solve_kernel<REAL, BLK, 1, ISO, FRIC>), g, b, lds, s, a); break;     \
    default: hipLaunchKernelGGL((tile_solve_kernel<REAL, BLK, 2, ISO, FRIC>), g, b, lds, s, a); break;    \
  }
#define EGS_LAUNCH_T(BLK, ISO) \
  if (a.mu != nullptr) { EGS_LAUNCH_TF(BLK, ISO, true) } else { EGS_LAUNCH_TF(BLK, ISO, false) }
#define EGS_LAUNCH(BLK) EGS_LAUNCH_T(BLK, false)
  if (block == 256 && a.iso) { EGS_LAUNCH_T(256, true) }
  else if (block == 256) { EGS_LAUNCH(256) }
  else if (block == 128) { EGS_LAUNCH(128) }
  else if (block == 64) { EGS_LAUNCH(64) }
  else { EGS_LAUNCH(512) }
#undef EGS_LAUNCH
#undef EGS_LAUNCH_T
#undef EGS_LAUNCH_TF
}

template <typename REAL>
void launch_assemble(const AssembleArgs &a, bool angular, const HingeTables &h, hipStream_t s) {
  if (a.m <= 0) return;
  const dim3 g((a.m + 255) / 256), t(256);
  if (h.slider) {
    if (a.rest) hipLaunchKernelGGL((assemble_kernel<REAL, false, NoRates, true, true, false, true>), g, t, 0, s, a, NoRates{}, h.motor, h.limit, h.travel);
    else hipLaunchKernelGGL((assemble_kernel<REAL, false, NoRates, false, true, false, true>), g, t, 0, s, a, NoRates{}, h.motor, h.limit, h.travel);
  } else if (angular && h.limit) {
    if (a.rest) hipLaunchKernelGGL((assemble_kernel<REAL, false, NoRates, true, true, true>), g, t, 0, s, a, NoRates{}, h.motor, h.limit, NoTravel{});
    else hipLaunchKernelGGL((assemble_kernel<REAL, false, NoRates, false, true, true>), g, t, 0, s, a, NoRates{}, h.motor, h.limit, NoTravel{});
  } else if (angular) {
    if (a.rest) hipLaunchKernelGGL((assemble_kernel<REAL, false, NoRates, true, true>), g, t, 0, s, a, NoRates{}, h.motor, nullptr, NoTravel{});
    else hipLaunchKernelGGL((assemble_kernel<REAL, false, NoRates, false, true>), g, t, 0, s, a, NoRates{}, h.motor, nullptr, NoTravel{});
  } else if (a.rest) hipLaunchKernelGGL((assemble_kernel<REAL, false, NoRates, true, false>), g, t, 0, s, a, NoRates{}, nullptr, nullptr, NoTravel{});
  else hipLaunchKernelGGL((assemble_kernel<REAL, false, NoRates, false, false>), g, t, 0, s, a, NoRates{}, nullptr, nullptr, NoTravel{});
}

template <typename REAL>
void launch_assemble_each(const AssembleArgs &a, const EnsembleRates &t, bool angular, const HingeTables &h, hipStream_t s) {
  if (a.m <= 0) return;
  const dim3 g((a.m + 255) / 256), b(256);
  if (h.slider) {
    if (a.rest) hipLaunchKernelGGL((assemble_kernel<REAL, true, EnsembleRates, true, true, false, true>), g, b, 0, s, a, t, h.motor, h.limit, h.travel);
    else hipLaunchKernelGGL((assemble_kernel<REAL, true, EnsembleRates, false, true, false, true>), g, b, 0, s, a, t, h.motor, h.limit, h.travel);
  } else if (angular && h.limit) {
    if (a.rest) hipLaunchKernelGGL((assemble_kernel<REAL, true, EnsembleRates, true, true, true>), g, b, 0, s, a, t, h.motor, h.limit, NoTravel{});
    else hipLaunchKernelGGL((assemble_kernel<REAL, true, EnsembleRates, false, true, true>), g, b, 0, s, a, t, h.motor, h.limit, NoTravel{});
  } else if (angular) {
    if (a.rest) hipLaunchKernelGGL((assemble_kernel<REAL, true, EnsembleRates, true, true>), g, b, 0, s, a, t, h.motor, nullptr, NoTravel{});
    else hipLaunchKernelGGL((assemble_kernel<REAL, true, EnsembleRates, false, true>), g, b, 0, s, a, t, h.motor, nullptr, NoTravel{});
  } else if (a.rest) hipLaunchKernelGGL((assemble_kernel<REAL, true, EnsembleRates, true, false>), g, b, 0, s, a, t, nullptr, nullptr, NoTravel{});
  else hipLaunchKernelGGL((assemble_kernel<REAL, true, EnsembleRates, false, false>), g, b, 0, s, a, t, nullptr, nullptr, NoTravel{});
}

template <typename REAL>
__global__ void __launch_bounds__(256) pin_start_kernel(int rows, const REAL *src, const int32_t *kind, const REAL *lo,
                                                        const REAL *hi, REAL *dst) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const REAL l = lo[r];
  dst[r] = (r % 3 == 2 && kind[r / 3] == 5 && l == hi[r]) ? l : src[r];
}

template <typename REAL>
void launch_pin_start(int rows, const REAL *src, const int32_t *kind, const REAL *lo, const REAL *hi, REAL *dst, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL((pin_start_kernel<REAL>), dim3((rows + 255) / 256), dim3(256), 0, s, rows, src, kind, lo, hi, dst);
}

template <typename REAL>
void launch_residual_partials(int rows, const REAL *wres, const REAL *x, const REAL *lo, const REAL *hi,
                              const uint8_t *is_eq, const REAL *mu, double *out, int blocks, hipStream_t s) {
  if (mu) hipLaunchKernelGGL((residual_partials_kernel<REAL, true>), dim3(blocks), dim3(256), 0, s, rows, wres, x, lo, hi, is_eq, out, mu);
  else hipLaunchKernelGGL((residual_partials_kernel<REAL>), dim3(blocks), dim3(256), 0, s, rows, wres, x, lo, hi, is_eq, out, mu);
}

template <typename REAL>
void launch_hist_residual(const SolveArgs<REAL> &a, int sweeps, int blocks, double *out, int write_sweep, hipStream_t s) {
  if (sweeps <= 0 || a.m <= 0) return;
  constexpr int G = 8;   // recorded sweeps that share one pass over the J blocks
  const dim3 grid(blocks, (sweeps + G - 1) / G);
  if (a.mu) hipLaunchKernelGGL((hist_residual_kernel<REAL, G, true>), grid, dim3(256), 0, s, a, out, write_sweep, sweeps);
  else hipLaunchKernelGGL((hist_residual_kernel<REAL, G>), grid, dim3(256), 0, s, a, out, write_sweep, sweeps);
}

template <typename REAL>
void launch_seg_residual(const SolveArgs<REAL> &a, const EnsembleSegs &S, const int32_t *running, const REAL *xs,
                         const REAL *as, const REAL *ws, int sweeps, double *err, hipStream_t s) {
  if (S.n_ens <= 0 || sweeps <= 0) return;
  if (a.mu) hipLaunchKernelGGL((seg_residual_kernel<REAL, true>), dim3(S.n_ens, sweeps), dim3(256), 0, s, a, S, running, xs, as, ws, err);
  else hipLaunchKernelGGL((seg_residual_kernel<REAL>), dim3(S.n_ens, sweeps), dim3(256), 0, s, a, S, running, xs, as, ws, err);
}

template <typename REAL>
void launch_seg_select(const EnsembleSegs &S, const EnsembleStop &T, const double *err, int sweeps, int first, int max_iters,
                       int every, double tol, int all_checked, int init, const REAL *xs, size_t xstride, const REAL *as,
                       size_t astride, REAL *fin_x, REAL *fin_acc, hipStream_t s) {
  if (S.n_ens <= 0) return;
  hipLaunchKernelGGL((seg_select_kernel<REAL>), dim3(S.n_ens), dim3(256), 0, s, S, T, err, sweeps, first, max_iters,
                     every > 0 ? every : 1, tol, all_checked, init, xs, xstride, as, astride, fin_x, fin_acc);
}

void launch_seg_fixed(const EnsembleSegs &S, const EnsembleStop &T, const double *err, int sweeps, hipStream_t s) {
  if (S.n_ens <= 0) return;
  hipLaunchKernelGGL(seg_fixed_kernel, dim3((S.n_ens + 255) / 256), dim3(256), 0, s, S, T, err, sweeps);
}

template <typename REAL>
void launch_velocity(int n, const double *v, const double *w, const double *Wf, const REAL *acc, double dt, double *v6,
                     hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL((velocity_kernel<REAL>), dim3((6 * n + 255) / 256), dim3(256), 0, s, n, v, w, Wf, acc, dt, v6);
}

template <typename REAL>
void launch_velocity_each(int n, const double *v, const double *w, const double *Wf, const REAL *acc, const int32_t *body_ens,
                          const double *dt_each, double *v6, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL((velocity_each_kernel<REAL>), dim3((6 * n + 255) / 256), dim3(256), 0, s, n, v, w, Wf, acc, body_ens,
                     dt_each, v6);
}

void launch_mass_times_force(int n, const double *Minv, const double *f_ext, double *Wf, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(mass_times_force_kernel, dim3((6 * n + 255) / 256), dim3(256), 0, s, n, Minv, f_ext, Wf);
}

template <typename REAL>
void launch_live_mass(int n, const double *R, const double *w, const double *inertia_body, const double *torque,
                      const uint8_t *live_mask, double *Minv, REAL *Minv_r, double *f_ext, double *Wf, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL((live_mass_kernel<REAL>), dim3((n + 255) / 256), dim3(256), 0, s, n, R, w, inertia_body, torque,
                     live_mask, Minv, Minv_r, f_ext, Wf);
}

void launch_advance(int n, const BodyState &in, const BodyState &out, const double *v6, double dt, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(advance_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, in, out, v6, dt);
}

void launch_advance_each(int n, const BodyState &state, const double *v6, const int32_t *body_ens, const double *dt_each,
                         hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(advance_each_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, state, v6, body_ens, dt_each);
}

template <typename REAL>
void launch_fill_friction(int m, int mj, const int32_t *body0, const int32_t *body1, const int32_t *body_ens,
                          const double *mu_ens, REAL *mu, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL((fill_friction_kernel<REAL>), dim3((m + 255) / 256), dim3(256), 0, s, m, mj, body0, body1, body_ens, mu_ens, mu);
}

template <typename REAL>
void launch_convert_minv(int count, const double *src, REAL *dst, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL((convert_kernel<REAL>), dim3((count + 255) / 256), dim3(256), 0, s, count, src, dst);
}

template <typename REAL>
void launch_minv_iso(int n, const REAL *W, int *flag, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL((minv_iso_kernel<REAL>), dim3((n + 255) / 256), dim3(256), 0, s, n, W, flag);
}

template <typename REAL>
void launch_linsym_bodies(int m, const int32_t *body0, const int32_t *body1, const REAL *W, int *flag, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL((linsym_bodies_kernel<REAL>), dim3((m + 255) / 256), dim3(256), 0, s, m, body0, body1, W, flag);
}


void launch_share_normals(int n_tiles, const LaneDesc *lanes, const double *data, int *flag, hipStream_t s) {
  if (n_tiles <= 0) return;
  const int n_pairs = n_tiles * 128;
  hipLaunchKernelGGL(share_normals_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, s, n_pairs, lanes, data, flag);
  hipLaunchKernelGGL(face_normals_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, s, n_pairs, lanes, data, flag);
}

template <typename REAL>
int occupancy_global_solve() {
  int best = 1 << 30, nb = 0;   // the friction forms included: the persistent grid is sized once for all of them
#define EGS_OCC(M, F)                                                                                               \
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, global_solve_kernel<REAL, M, F>, 256, 0) != hipSuccess) return 0; \
  best = nb < best ? nb : best;
  EGS_OCC(1, false) EGS_OCC(2, false) EGS_OCC(1, true) EGS_OCC(2, true)
#undef EGS_OCC
  return best;
}
template int occupancy_global_solve<double>();
template int occupancy_global_solve<float>();

template <typename REAL>
void launch_global_solve(const GlobalArgs<REAL> &a0, int max_blocks, hipStream_t s) {
  if (a0.mg <= 0) return;
  GlobalArgs<REAL> a = a0;
  const int flat_blocks = (a.mg + 255) / 256;
  // the persistent grid's workgroups wait on each other: never more than are resident together
  // (max_blocks = occupancy x CUs, capped at one per CU; the lanes take more constraints each instead)
  const int cap = max_blocks > 0 ? max_blocks : 1;
  const int grid = flat_blocks < cap ? flat_blocks : cap;
  a.per_lane = (a.mg + grid * 256 - 1) / (grid * 256);
  const size_t tick_bytes = sizeof(uint32_t) * (size_t)(a.n_bodies > 0 ? a.n_bodies : 1);
  hipLaunchKernelGGL((global_prepare_kernel<REAL>), dim3(flat_blocks), dim3(256), 0, s, a);
  const bool fric = a.mu != nullptr;   // the ordered accumulation (mode 1) projects nothing: it has no friction form
  if (a.method == 0) {
    if (!a.resume) {  // accumulators from x0
      a.mode = 1;
      (void)hipMemsetAsync(a.tickets, 0, tick_bytes, s);
      hipLaunchKernelGGL((global_solve_kernel<REAL, 1>), dim3(grid), dim3(256), 0, s, a);
    }
    for (int it = 0; it < a.sweeps; ++it) {
      if (fric) hipLaunchKernelGGL((global_jacobi_kernel<REAL, true>), dim3(flat_blocks), dim3(256), 0, s, a);
      else hipLaunchKernelGGL((global_jacobi_kernel<REAL>), dim3(flat_blocks), dim3(256), 0, s, a);
      a.mode = 1;
      (void)hipMemsetAsync(a.tickets, 0, tick_bytes, s);
      hipLaunchKernelGGL((global_solve_kernel<REAL, 1>), dim3(grid), dim3(256), 0, s, a);
    }
  } else {
    a.mode = 0;
    (void)hipMemsetAsync(a.tickets, 0, tick_bytes, s);
    if (a.method == 1 && fric) hipLaunchKernelGGL((global_solve_kernel<REAL, 1, true>), dim3(grid), dim3(256), 0, s, a);
    else if (a.method == 1) hipLaunchKernelGGL((global_solve_kernel<REAL, 1>), dim3(grid), dim3(256), 0, s, a);
    else if (fric) hipLaunchKernelGGL((global_solve_kernel<REAL, 2, true>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((global_solve_kernel<REAL, 2>), dim3(grid), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL((global_wres_kernel<REAL>), dim3(flat_blocks), dim3(256), 0, s, a);
}

template <typename REAL>
void launch_global_wres(const GlobalArgs<REAL> &a, hipStream_t s) {
  if (a.mg <= 0) return;
  hipLaunchKernelGGL((global_wres_kernel<REAL>), dim3((a.mg + 255) / 256), dim3(256), 0, s, a);
}

template <typename REAL>
void launch_cons_prepare(const SolveArgs<REAL> &a, hipStream_t s) {
  if (a.m <= 0) return;
  hipLaunchKernelGGL((cons_prepare_kernel<REAL>), dim3((a.m + 255) / 256), dim3(256), 0, s, a);
}

#define EGS_INSTANTIATE(REAL)                                                                                \
  template void launch_tile_solve<REAL>(const SolveArgs<REAL> &, int, int, int, hipStream_t);                \
  template void launch_global_solve<REAL>(const GlobalArgs<REAL> &, int, hipStream_t);                            \
  template void launch_cons_prepare<REAL>(const SolveArgs<REAL> &, hipStream_t);                             \
  template void launch_global_wres<REAL>(const GlobalArgs<REAL> &, hipStream_t);                            \
  template void launch_assemble<REAL>(const AssembleArgs &, bool, const HingeTables &, hipStream_t);                               \
  template void launch_assemble_each<REAL>(const AssembleArgs &, const EnsembleRates &, bool, const HingeTables &, hipStream_t);   \
  template void launch_pin_start<REAL>(int, const REAL *, const int32_t *, const REAL *, const REAL *, REAL *, hipStream_t);  \
  template void launch_residual_partials<REAL>(int, const REAL *, const REAL *, const REAL *, const REAL *,  \
                                               const uint8_t *, const REAL *, double *, int, hipStream_t);   \
  template void launch_velocity<REAL>(int, const double *, const double *, const double *, const REAL *, double,   \
                                      double *, hipStream_t);                          \
  template void launch_velocity_each<REAL>(int, const double *, const double *, const double *, const REAL *,      \
                                           const int32_t *, const double *, double *, hipStream_t);                 \
  template void launch_convert_minv<REAL>(int, const double *, REAL *, hipStream_t);                         \
  template void launch_live_mass<REAL>(int, const double *, const double *, const double *, const double *,  \
                                       const uint8_t *, double *, REAL *, double *, double *, hipStream_t);  \
  template void launch_fill_friction<REAL>(int, int, const int32_t *, const int32_t *, const int32_t *,      \
                                           const double *, REAL *, hipStream_t);                             \
  template void launch_minv_iso<REAL>(int, const REAL *, int *, hipStream_t);                               \
  template void launch_linsym_bodies<REAL>(int, const int32_t *, const int32_t *, const REAL *, int *, hipStream_t);                               \
  template void launch_hist_residual<REAL>(const SolveArgs<REAL> &, int, int, double *, int, hipStream_t);   \
  template void launch_seg_residual<REAL>(const SolveArgs<REAL> &, const EnsembleSegs &, const int32_t *, const REAL *, \
                                          const REAL *, const REAL *, int, double *, hipStream_t);                      \
  template void launch_seg_select<REAL>(const EnsembleSegs &, const EnsembleStop &, const double *, int, int, int, int,  \
                                        double, int, int, const REAL *, size_t, const REAL *, size_t, REAL *, REAL *,   \
                                        hipStream_t);
EGS_INSTANTIATE(double)
EGS_INSTANTIATE(float)

}  // namespace egs
