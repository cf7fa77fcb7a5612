// problem.cpp -- the device-resident problem: its topology and plans (problem_set_topology, ensure_tile_plan),
// mass blocks, the sticky stall flag, assembly and velocity update, the stand-alone mat-vec, and the egs_problem_*
// entries of the C ABI with the stateless egs_solve_blocks / egs_matvec_blocks on top of them.
#include <chrono>
#include <cmath>

#include "matvec.h"
#include "policy.h"
#include "problem.h"

using namespace egs;

namespace {

// host double <-> the problem's REAL: fp32 problems convert on the host, through a temporary
void upload_real(egs_problem *p, DevBuf<unsigned char> &dst, const double *src, size_t count) {
  if (!src || count == 0) return;
  hipStream_t s = p->ctx->stream;
  std::vector<float> tmp;
  const void *h = src;
  if (p->precision == EGS_F32) {
    tmp.resize(count);
    for (size_t i = 0; i < count; ++i) tmp[i] = (float)src[i];
    h = tmp.data();
  }
  HIPCHK(hipMemcpyAsync(dst.p, h, count * p->real_size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
}

void download_real(egs_problem *p, const DevBuf<unsigned char> &src, double *dst, size_t count) {
  if (!dst || count == 0) return;
  hipStream_t s = p->ctx->stream;
  const bool f32 = p->precision == EGS_F32;
  std::vector<float> tmp(f32 ? count : 0);
  HIPCHK(hipMemcpyAsync(f32 ? (void *)tmp.data() : (void *)dst, src.p, count * p->real_size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (size_t i = 0; f32 && i < count; ++i) dst[i] = (double)tmp[i];
}

// Once per M^-1 upload or topology change (4 bytes back): may the fp64 isotropic timetable sweep keep one linear block
// for both sides (step_solve.hip: LINSYM)?  The body half of the preconditions -- every constraint has a body on
// side 1, and where it has one on side 0 as well, the same linear weight -- is decided here, on the device; the
// Jacobian half (lin_neg) where the blocks are made.
void decide_linsym_bodies(egs_problem *p) {
  p->linsym_bodies = 0;
  if (p->precision != EGS_F64 || !p->minv_iso || p->m <= 0) return;
  hipStream_t s = p->ctx->stream;
  int one = 1, flag = 0;
  int32_t *scratch = p->error_flag.p + 1;
  HIPCHK(hipMemcpyAsync(scratch, &one, sizeof(int), hipMemcpyHostToDevice, s));
  launch_linsym_bodies<double>(p->m, p->body0.p, p->body1.p, real<double>(p->Minv_r), scratch, s);
  HIPCHK(hipMemcpyAsync(&flag, scratch, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  p->linsym_bodies = flag != 0 ? 1 : 0;
}

}  // namespace

namespace egs {
void decide_share_normals(egs_problem *p) {
  if (p->share_normals != egs_problem::kShareUndecided) return;
  p->share_normals = 0;
  p->face_normals = false;
  if (!p->tile_plan_ready || !p->plan.chained || p->plan.block != 256 || !p->have_constraints) return;
  hipStream_t s = p->ctx->stream;
  int both = 3, flag = 0;   // bit 0: SHARE's answer, bit 1 with it: FACE's
  int32_t *scratch = p->error_flag.p + 1;
  HIPCHK(hipMemcpyAsync(scratch, &both, sizeof(int), hipMemcpyHostToDevice, s));
  launch_share_normals(p->plan.n_tiles, p->tile.lanes.p, p->data.p, scratch, s);
  HIPCHK(hipMemcpyAsync(&flag, scratch, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  p->share_normals = (flag & 1) ? 1 : 0;
  p->face_normals = flag == 3 && p->plan.faced;
}
}  // namespace egs

namespace {

// two device buffers change places (DevBuf owns its allocation: members, not objects, are exchanged)
template <typename T>
void swap_buffers(DevBuf<T> &a, DevBuf<T> &b) {
  std::swap(a.p, b.p);
  std::swap(a.count, b.count);
  std::swap(a.cap, b.cap);
}

void ensure_wf(egs_problem *p) {
  if (p->wf_valid) return;
  p->Wf.alloc((size_t)(p->n > 0 ? p->n : 1) * 6);
  launch_mass_times_force(p->n, p->Minv_d.p, p->f_ext.p, p->Wf.p, p->ctx->stream);
  p->wf_valid = true;
}

// The schedule of the stand-alone products (matvec_plan.h), built on first use.
void ensure_matvec_plan(egs_problem *p) {
  if (p->mv_ready) return;
  // 128 constraints per tile: 37 KB of LDS, four workgroups per CU keep loads in flight while others
  // compute (measured on 1 M contacts: 5.2-5.4 TB/s against 4.9-5.0 with 256).  EGS_MV_TILE=256 for experiments.
  const char *te = std::getenv("EGS_MV_TILE");
  const int forced = te ? std::atoi(te) : 0;
  p->mvplan = build_matvec_plan(p->n, p->m, p->h_body0.data(), p->h_body1.data(), forced == 256 ? 256 : 128);
  const MatvecPlan &pl = p->mvplan;
  stage(p->ctx, p->mv_lanes, pl.lanes);
  stage(p->ctx, p->mv_tiles, pl.tiles);
  stage(p->ctx, p->mv_slots, pl.slots);
  stage(p->ctx, p->mv_ents, pl.ents);
  stage(p->ctx, p->mv_boundary, pl.boundary);
  const size_t rs = p->real_size(), mm = (size_t)(p->m > 0 ? p->m : 1);
  p->mv_T.alloc((size_t)(pl.n_shared_entries > 0 ? pl.n_shared_entries : 1) * 6 * rs);
  p->mv_x.alloc(mm * 3 * rs);
  p->mv_y.alloc(mm * 3 * rs);
  HIPCHK(hipStreamSynchronize(p->ctx->stream));
  p->mv_ready = true;
}

template <typename REAL>
void launch_matvec_t(egs_problem *p, int parts, REAL eps, REAL scale, const REAL *x) {
  const MatvecPlan &pl = p->mvplan;
  MatvecArgs<REAL> a;
  a.lanes = p->mv_lanes.p; a.tiles = p->mv_tiles.p; a.slots = p->mv_slots.p; a.ents = p->mv_ents.p;
  a.boundary = p->mv_boundary.p; a.n_boundary = (int32_t)pl.boundary.size();
  a.max_slots = pl.max_slots;
  a.Minv = real<REAL>(p->Minv_r);
  a.J0 = real<REAL>(p->J0); a.J1 = real<REAL>(p->J1);
  a.x = x; a.y = real<REAL>(p->mv_y); a.T = real<REAL>(p->mv_T);
  a.eps = eps; a.scale = scale; a.accumulate = 0;
  { const char *ne = std::getenv("EGS_MV_NT"); a.stream_nt = ne ? (std::atoi(ne) != 0) : 1; }   // +2-8 % measured
  record_kernel_event(p->ctx, true);
  if (parts == EGS_MV_FULL) {
    launch_matvec<REAL>(a, 8, pl.n_tiles, pl.block, p->ctx->stream);
  } else {   // Lx + Ux, Ux + Dx, Lx + Dx as the reference adds them (sparse_iterations_utils.cc:563-569, 606-622)
    for (int bit = 1; bit <= 4; bit <<= 1) {
      if (!(parts & bit)) continue;
      launch_matvec<REAL>(a, bit, pl.n_tiles, pl.block, p->ctx->stream);
      a.accumulate = 1;
    }
  }
  record_kernel_event(p->ctx, false);
  HIPCHK(hipGetLastError());
}

egs_status do_matvec(egs_problem *p, int32_t parts, double eps, double scale, const double *x, double *y) {
  egs_context *ctx = p->ctx;
  if (!(parts == EGS_MV_FULL || (parts >= 1 && parts <= 7)))
    return fail(ctx, EGS_ERR_INVALID, "parts must be EGS_MV_FULL or a combination of LOWER / UPPER / DIAG");
  if (!p->have_blocks) return fail(ctx, EGS_ERR_INVALID, "no system uploaded (set_blocks or assemble first)");
  if (p->m == 0) return EGS_OK;
  ensure_system(p);
  ensure_minv_real(p);
  ensure_matvec_plan(p);
  if (x) upload_real(p, p->mv_x, x, (size_t)p->m * 3);
  // x = NULL: the device-resident lambda of the last solve
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    launch_matvec_t<REAL>(p, parts, (REAL)eps, (REAL)scale, real<REAL>(x ? p->mv_x : p->x));
  });
  if (y) download_real(p, p->mv_y, y, (size_t)p->m * 3);
  return EGS_OK;
}

// egs_solve_blocks / egs_matvec_blocks are stateless for their caller; the context keeps the
// last problem (schedule + device buffers) and reuses it while the constraint graph is unchanged.
egs_status oneshot_problem(egs_context *ctx, int32_t n, int32_t m, const int32_t *body0, const int32_t *body1,
                           int32_t precision, egs_problem **out) {
  egs_problem *p = ctx->oneshot;
  const bool reuse = p && p->n == n && p->m == m && p->precision == precision &&
                     (m == 0 || (std::memcmp(p->h_body0.data(), body0, (size_t)m * sizeof(int32_t)) == 0 &&
                                 std::memcmp(p->h_body1.data(), body1, (size_t)m * sizeof(int32_t)) == 0));
  if (!reuse) {
    if (p) { egs_problem_destroy(p); ctx->oneshot = nullptr; }
    egs_status st = egs_problem_create(ctx, n, m, body0, body1, precision, &p);
    if (st != EGS_OK) return st;
    ctx->oneshot = p;
  }
  *out = p;
  return EGS_OK;
}
}  // namespace

namespace egs {

void ensure_minv_real(egs_problem *p) {
  if (p->minv_r_valid) {
    if (p->linsym_bodies < 0) decide_linsym_bodies(p);
    return;
  }
  const int count = p->n * 36;
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    launch_convert_minv<REAL>(count, p->Minv_d.p, real<REAL>(p->Minv_r), p->ctx->stream);
  });
  p->minv_r_valid = true;
  // isotropy of the blocks, checked once per upload (4 bytes back)
  const char *ie = std::getenv("EGS_ISO");
  if (p->n > 0 && !(ie && std::atoi(ie) == 0)) {
    hipStream_t s = p->ctx->stream;
    int one = 1, flag = 0;
    int32_t *scratch = p->error_flag.p + 1;
    HIPCHK(hipMemcpyAsync(scratch, &one, sizeof(int), hipMemcpyHostToDevice, s));
    with_real(p, [&](auto r) { using REAL = decltype(r); launch_minv_iso<REAL>(p->n, real<REAL>(p->Minv_r), scratch, s); });
    HIPCHK(hipMemcpyAsync(&flag, scratch, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // live inertia rewrites the angular blocks of its bodies every step: whatever the upload held, they are not isotropic
    const bool iso = flag != 0 && !p->live_any;
    if (iso != p->minv_iso) p->tile_plan_ready = false;   // the preferred tile size depends on it
    p->minv_iso = iso;
  }
  decide_linsym_bodies(p);
}

void refresh_live_mass(egs_problem *p) {
  if (!p->live_any || p->n <= 0) return;
  ensure_system(p);      // a deferred system is made from the Wf of the state its step read: before that Wf changes
  ensure_minv_real(p);   // an upload not converted yet (the one place with a read-back: once per upload, not per step)
  ensure_wf(p);
  record_kernel_event(p->ctx, true);
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    launch_live_mass<REAL>(p->n, p->R.p, p->w.p, p->live_inertia.p, p->live_has_torque ? p->live_torque.p : nullptr,
                           p->live_mask.p, p->Minv_d.p, real<REAL>(p->Minv_r), p->f_ext.p, p->Wf.p, p->ctx->stream);
  });
  record_kernel_event(p->ctx, false);
  HIPCHK(hipGetLastError());
}

egs_status set_live_inertia(egs_problem *p, const double *inertia_body, const double *torque) {
  egs_context *ctx = p->ctx;
  const size_t n = (size_t)p->n;
  std::vector<uint8_t> mask(n, 0);
  bool any = false;
  for (size_t b = 0; inertia_body && b < n; ++b) {
    const double *I = inertia_body + 9 * b;
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(I[k])) return fail(ctx, EGS_ERR_INVALID, "body " + std::to_string(b) + ": non-finite inertia_body");
    for (int k = 0; torque && k < 3; ++k)
      if (!std::isfinite(torque[3 * b + k])) return fail(ctx, EGS_ERR_INVALID, "body " + std::to_string(b) + ": non-finite torque");
    if (I[1] != I[3] || I[2] != I[6] || I[5] != I[7])
      return fail(ctx, EGS_ERR_INVALID, "body " + std::to_string(b) + ": inertia_body is not symmetric");
    // Sylvester: the three leading minors
    const double m2 = I[0] * I[4] - I[1] * I[3];
    const double m3 = (I[0] * (I[4] * I[8] - I[5] * I[7]) + I[1] * (I[5] * I[6] - I[3] * I[8])) + I[2] * (I[3] * I[7] - I[4] * I[6]);
    if (!(I[0] > 0) || !(m2 > 0) || !(m3 > 0))
      return fail(ctx, EGS_ERR_INVALID, "body " + std::to_string(b) + ": inertia_body is not positive definite");
    const bool multiple = I[1] == 0 && I[2] == 0 && I[5] == 0 && I[0] == I[4] && I[0] == I[8];   // a I_3: skipped
    mask[b] = multiple ? 0 : 1;
    any |= !multiple;
  }
  return guarded(ctx, [&]() -> egs_status {
    hipStream_t s = ctx->stream;
    HIPCHK(hipStreamSynchronize(s));   // a step in flight may still read the old arrays
    const bool was = p->live_any;
    if (any) {
      p->live_inertia.alloc(n * 9); p->live_mask.alloc(n);
      upload(p->live_inertia, inertia_body, n * 9, s);
      upload(p->live_mask, mask.data(), n, s);
      if (torque) { p->live_torque.alloc(n * 3); upload(p->live_torque, torque, n * 3, s); }
      p->live_has_torque = torque != nullptr;
      p->live_any = true;
      if (p->minv_iso) {   // once: the isotropic schedules are not for these blocks, and the tile size follows
        p->minv_iso = false;
        p->tile_plan_ready = false;
        p->linsym_bodies = 0;
      }
    } else {
      p->live_any = false;
      p->live_has_torque = false;
      if (was) p->minv_r_valid = false;   // the blocks stay what the last refresh left: the isotropy check decides again
    }
    return EGS_OK;
  });
}

// Ball joints that join two bodies are assembled with +0 in J1_lin where J0_lin holds +0 (joints.cc:17-31): their
// J1_lin is -J0_lin in value but not in bits.  Contacts are [-Rn, ..] / [Rn, ..], negated bit for bit.
// A list without any joint holds contacts only: the fused step's sweep takes their bounds as literals (solve.cpp:
// choose_sweep).
// The angular blocks (EGS_JOINT_LOCK, EGS_JOINT_HINGE_AXIS) are joints here: one between two bodies counts as a two-body
// ball joint (its J1 is -1.0 * J0 only in value where J0 holds +0, and the LINSYM forms keep one linear block, which
// these do not have), so a list that holds one runs none of LINSYM, FUSED_ASSEMBLY, PAIR or CHAIN.
// A slider (EGS_JOINT_SLIDER_AXIS) has a lever arm on body0 alone, J1 = [-Rn | 0]: whichever sides it joins, the list
// that holds one counts as holding a two-body joint, and none of LINSYM, FUSED_ASSEMBLY, PAIR, CHAIN, SHARE, FACE runs.
void note_kinds(egs_problem *p, const int32_t *kind) {
  bool jp = false, joint = false;
  p->angular = false;
  p->sliders = false;
  for (int i = 0; i < p->m; ++i) {
    joint = joint || kind[i] != EGS_CONTACT_BOX;
    p->angular = p->angular || kind[i] == EGS_JOINT_LOCK || kind[i] == EGS_JOINT_HINGE_AXIS;
    p->sliders = p->sliders || kind[i] == EGS_JOINT_SLIDER_AXIS;
    jp = jp || (kind[i] != EGS_CONTACT_BOX && p->h_body0[i] >= 0 && p->h_body1[i] >= 0) || kind[i] == EGS_JOINT_SLIDER_AXIS;
  }
  p->joint_pairs = jp;
  p->contacts_only = !joint;
  p->h_kind.assign(kind, kind + p->m);
  note_hinges(p, nullptr);
}

void note_hinges(egs_problem *p, const double *motor) {
  p->hinges = p->hinges_pinned = false;
  p->pinned_slider = -1;
  for (int i = 0; i < p->m && i < (int)p->h_kind.size(); ++i) {
    if (p->h_kind[i] == EGS_JOINT_SLIDER_AXIS) {   // its rail row is a box row of the dense steps, as a hinge's axis row
      p->hinges = true;
      if ((!motor || !(motor[2 * (size_t)i + 1] > 0)) && p->pinned_slider < 0) p->pinned_slider = i;
      continue;
    }
    if (p->h_kind[i] != EGS_JOINT_HINGE_AXIS) continue;
    p->hinges = true;
    if (!motor || !(motor[2 * (size_t)i + 1] > 0)) p->hinges_pinned = true;
  }
}

// ---- the sticky stall flag ---------------------------------------------------
// asynchronous refresh of the page-locked copy (4 bytes), enqueued behind a solve
void post_flag_copy(egs_problem *p) {
  HIPCHK(hipMemcpyAsync(p->h_flag.p, p->error_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, p->ctx->stream));
}

// A stall was seen: clear it (it is being reported now) and fail.  Synchronises.
egs_status report_stall(egs_problem *p) {
  hipStream_t s = p->ctx->stream;
  HIPCHK(hipMemsetAsync(p->error_flag.p, 0, sizeof(int32_t), s));
  HIPCHK(hipStreamSynchronize(s));
  *p->h_flag.p = 0;
  p->ctx->error = "device ordering wait timed out";
  return EGS_ERR_STALL;
}

// What is wrong with a list of kinds and descriptors (nothing: NULL): an unknown kind; for the angular blocks a side 0
// without a body, non-finite data, a LOCK quaternion or a hinge axis whose squared norm is not within 1e-12 of 1; for
// a slider a side 0 without a body, non-finite data, a rail direction a0 that is no unit vector within 1e-12.
const char *constraints_fault(int m, const int32_t *kind, const int32_t *body0, const double *data) {
  auto unit = [](const double *v, int k) {
    double n = 0.0;
    for (int q = 0; q < k; ++q) n += v[q] * v[q];
    return std::fabs(n - 1.0) <= 1e-12;   // false for a NaN
  };
  for (int i = 0; i < m; ++i) {
    const double *d = data + 7 * (size_t)i;
    switch (kind[i]) {
      case EGS_JOINT_BALL: case EGS_CONTACT_BOX: break;
      case EGS_JOINT_LOCK: case EGS_JOINT_HINGE_AXIS:
        if (body0[i] < 0) return "an angular joint needs a body on side 0";
        for (int k = 0; k < 7; ++k)
          if (!std::isfinite(d[k])) return "non-finite angular joint data";
        if (kind[i] == EGS_JOINT_LOCK ? !unit(d, 4) : !(unit(d, 3) && unit(d + 3, 3)))
          return kind[i] == EGS_JOINT_LOCK ? "the lock quaternion is not a unit quaternion" : "a hinge axis is not a unit vector";
        break;
      case EGS_JOINT_SLIDER_AXIS:
        if (body0[i] < 0) return "a slider needs a body on side 0";
        for (int k = 0; k < 7; ++k)
          if (!std::isfinite(d[k])) return "non-finite slider data";
        if (!unit(d, 3)) return "a slider's rail direction is not a unit vector";
        break;
      default: return "unknown constraint kind";
    }
  }
  return nullptr;
}

// What is wrong with a limit table: a non-finite entry anywhere; on a HINGE_AXIS row with a stop a q that is not a unit
// quaternion within 1e-12 (constraints_fault's bound), a (sin, cos) pair that is neither (0, 0) nor on the unit circle
// within 1e-12, a stop at +-pi (1 + cos <= 0: tan(limit / 2) has no value there), or lo above hi in the half-angle order
// tan(lo / 2) > tan(hi / 2), cross-multiplied as limit_row compares.
const char *limits_fault(size_t m, const int32_t *kind, const double *lim, int *first) {
  *first = -1;
  for (size_t i = 0; lim && i < m; ++i) {
    const double *L = lim + 8 * i;
    for (int k = 0; k < 8; ++k)
      if (!std::isfinite(L[k])) return "non-finite hinge limit entry";
    if (kind[i] != EGS_JOINT_HINGE_AXIS) continue;
    const bool lower = L[4] != 0.0 || L[5] != 0.0, upper = L[6] != 0.0 || L[7] != 0.0;
    if (!lower && !upper) continue;
    if (!(std::fabs(((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]) + L[3] * L[3] - 1.0) <= 1e-12))
      return "the hinge limit's reference quaternion is not a unit quaternion";
    for (int k = 4; k < 8; k += 2) {
      if (L[k] == 0.0 && L[k + 1] == 0.0) continue;
      if (!(std::fabs(L[k] * L[k] + L[k + 1] * L[k + 1] - 1.0) <= 1e-12)) return "a hinge limit's (sin, cos) pair is not on the unit circle";
      if (1.0 + L[k + 1] <= 0.0) return "a hinge limit at +-pi";
    }
    if (lower && upper && L[4] * (1.0 + L[7]) > L[6] * (1.0 + L[5])) return "a hinge's lower limit is above its upper limit";
    if (*first < 0) *first = (int)i;
  }
  return nullptr;
}

const char *travel_fault(size_t m, const int32_t *kind, const double *lim, int *first) {
  *first = -1;
  for (size_t i = 0; lim && i < m; ++i) {
    const double xlo = lim[2 * i], xhi = lim[2 * i + 1];
    if (xlo != xlo || xhi != xhi) return "NaN slider limit entry";
    if (kind[i] != EGS_JOINT_SLIDER_AXIS) continue;
    if (xlo == INFINITY || xhi == -INFINITY) return "a slider's lower limit is +inf or its upper limit -inf";
    if (xlo > xhi) return "a slider's lower limit is above its upper limit";
    if (*first < 0 && (std::isfinite(xlo) || std::isfinite(xhi))) *first = (int)i;
  }
  return nullptr;
}

AssembleArgs assemble_args(egs_problem *p, double dt, double erp) {
  AssembleArgs a;
  a.n = p->n; a.m = p->m;
  a.pos = p->pos.p; a.R = p->R.p; a.v = p->v.p; a.w = p->w.p;
  ensure_wf(p);
  a.Wf = p->Wf.p;
  a.kind = p->kind.p; a.body0 = p->body0.p; a.body1 = p->body1.p;
  a.data = p->data.p;
  a.dt = dt; a.erp = erp;
  a.J0 = p->J0.p; a.J1 = p->J1.p; a.lo = p->lo.p; a.hi = p->hi.p; a.rhs = p->rhs.p;
  a.err = p->err.p; a.is_eq = p->is_eq.p;
  a.rest = p->restitution ? p->rest.p : nullptr;
  a.vth = p->rest_vth;
  return a;
}

// what the device assembly tells about the blocks it makes
void note_assembled(egs_problem *p) {
  p->have_blocks = true;
  p->lin_neg = !p->joint_pairs;   // contact.cc:66-99 builds [-Rn, ..] / [Rn, ..]; two-body ball joints: note_kinds
}

void do_assemble(egs_problem *p, double dt, double erp) {
  const AssembleArgs a = assemble_args(p, dt, erp);
  with_real(p, [&](auto r) { launch_assemble<decltype(r)>(a, p->angular, hinge_tables(p), p->ctx->stream); });
  HIPCHK(hipGetLastError());
  note_assembled(p);
  p->sys_deferred = false;   // every array is written: a deferred system is superseded
}

void do_assemble_each(egs_problem *p, const EnsembleRates &r) {
  const AssembleArgs a = assemble_args(p, 0.0, 0.0);   // the scalar pair is not read
  with_real(p, [&](auto t) { launch_assemble_each<decltype(t)>(a, r, p->angular, hinge_tables(p), p->ctx->stream); });
  HIPCHK(hipGetLastError());
  note_assembled(p);
  p->sys_deferred = false;
}

// The deferred step's system, now: assemble_kernel on the state that step read, with its dt and erp.
void ensure_system(egs_problem *p) {
  if (!p->sys_deferred) return;
  AssembleArgs a = assemble_args(p, p->deferred_dt, p->deferred_erp);
  if (p->deferred_prev) { a.pos = p->prev_pos.p; a.R = p->prev_R.p; a.v = p->prev_v.p; a.w = p->prev_w.p; }
  with_real(p, [&](auto r) { launch_assemble<decltype(r)>(a, p->angular, hinge_tables(p), p->ctx->stream); });
  HIPCHK(hipGetLastError());
  p->sys_deferred = false;
}

void do_velocity(egs_problem *p, double dt) {
  ensure_wf(p);
  with_real(p, [&](auto r) {
    using REAL = decltype(r);
    launch_velocity<REAL>(p->n, p->v.p, p->w.p, p->Wf.p, real<REAL>(p->acc), dt, p->v6.p, p->ctx->stream);
  });
  HIPCHK(hipGetLastError());
}

void do_velocity_each(egs_problem *p, const EnsembleRates &r) {
  ensure_wf(p);
  with_real(p, [&](auto t) {
    using REAL = decltype(t);
    launch_velocity_each<REAL>(p->n, p->v.p, p->w.p, p->Wf.p, real<REAL>(p->acc), r.body_ens, r.dt, p->v6.p, p->ctx->stream);
  });
  HIPCHK(hipGetLastError());
}

// no constraints: v_dot = M^-1 f (ensembles.cc:504-505), the accumulators the velocity update reads are zero
void zero_accumulators(egs_problem *p) {
  HIPCHK(hipMemsetAsync(p->acc.p, 0, (size_t)(p->n > 0 ? p->n : 1) * 6 * p->real_size(), p->ctx->stream));
}

// The 1-lane-per-constraint schedule (tile / patch / global kernels).  Built on
// demand: a problem that runs on the quad schedule only needs it for Jacobi.
void ensure_tile_plan(egs_problem *p) {
  if (p->tile_plan_ready) return;
  hipStream_t s = p->ctx->stream;
  const int n = p->n, m = p->m;
  {
    // 256 constraints per tile; 512 once there are enough tiles to give every CU two
    // anyway (all 64 lanes of the working wavefront busy: +3-4 % on 16 batched C3 piles) --
    // but not for isotropic bodies, whose register-light kernel fits THREE 256-thread tiles per CU.
    // Oversize islands (patch / global kernels) always use 256 -- unless 512 makes every island fit.
    const char *te = std::getenv("EGS_TILE");   // experiment knob: 64/128/256/512 constraints per tile
    const int forced = te ? std::atoi(te) : 0;
    int tile = (forced == 64 || forced == 128 || forced == 256 || forced == 512) ? forced : (m >= kBigTileMinConstraints && p->precision == EGS_F64 && !(p->minv_iso && iso_schedule_pays(m, p->ctx->cu_count, p->precision)) ? 512 : 256);
    p->plan = build_plan(n, m, p->h_body0.data(), p->h_body1.data(), tile);
    if (!p->plan.global.empty()) {
      if (tile == 256 && !forced) {   // islands of 257..512 constraints: one 512-thread workgroup, all hand-offs in LDS
        Plan big = build_plan(n, m, p->h_body0.data(), p->h_body1.data(), 512);
        if (big.global.empty()) p->plan = std::move(big);
      } else if (tile != 256) {       // the patch kernels are 256-constraint workgroups, forced size or not
        p->plan = build_plan(n, m, p->h_body0.data(), p->h_body1.data(), 256);
      }
    }
  }
  const Plan &pl = p->plan;
  {
    std::vector<char> in_tile((size_t)(n > 0 ? n : 1), 0);
    for (const int32_t b : pl.slot_body)
      if (b >= 0) in_tile[(size_t)b] = 1;
    p->plan_covers_bodies = n > 0 && std::count(in_tile.begin(), in_tile.end(), 1) == n;
  }
  p->tile.stage(p->ctx, pl);
  stage(p->ctx, p->gcons, pl.global);
  if (pl.n_patch_tiles > 0) p->patch.stage(p->ctx, pl);
  {
    const char *pe = std::getenv("EGS_PATCH"), *qp = std::getenv("EGS_QUAD_PATCH");
    const size_t lds = (size_t)pl.patch_max_slots * (6 * p->real_size() + sizeof(unsigned));
    int occ_quad = 0, occ_lane = 0, occ_glob = 1;
    with_real(p, [&](auto r) {
      using REAL = decltype(r);
      if (pl.n_patch_tiles > 0) { occ_quad = occupancy_quad_patch_solve<REAL>(lds); occ_lane = occupancy_patch_solve<REAL>(lds); }
      if (!pl.global.empty()) occ_glob = occupancy_global_solve<REAL>();
    });
    p->oversize = choose_oversize_schedule(pl.n_patch_tiles, occ_quad, occ_lane, p->ctx->cu_count, !(pe && std::atoi(pe) == 0),
                                           pl.block == 256 && !(qp && std::atoi(qp) == 0));
    // (a patch plan with runs is for the 4-lane kernel only: plan.cpp builds it when that kernel will take it; should it
    //  not -- no LDS left for a resident workgroup -- the island goes the all-global way rather than to a kernel that
    //  does not know the placeholders)
    if (pl.patch_runs && p->oversize == kLanePatches) p->oversize = kAllGlobal;
    p->global_max_blocks = std::max(1, std::min(occ_glob, 1) * p->ctx->cu_count);
    if (p->oversize == kQuadPatches) {
      const size_t rsz = p->real_size(), mm2 = (size_t)m;
      p->wsB0.alloc(mm2 * 18 * rsz); p->wsB1.alloc(mm2 * 18 * rsz); p->wsD.alloc(mm2 * 9 * rsz); p->wsInv.alloc(mm2 * 3 * rsz);
    }
  }
  const size_t mg = pl.global.size(), rsz = p->real_size();
  p->gB0.alloc(mg * 18 * rsz); p->gB1.alloc(mg * 18 * rsz); p->gD.alloc(mg * 9 * rsz);
  p->gden.alloc(mg * 3 * rsz); p->gdx.alloc(mg * 3 * rsz);
  HIPCHK(hipStreamSynchronize(s));
  p->tile_plan_ready = true;
  if (p->share_normals >= 0) p->share_normals = egs_problem::kShareUndecided;   // the answer was the old plan's
}

// (Re)build everything that depends on the constraint topology.  Body state
// (pos, R, v, w, M^-1, f_ext) is kept when n is unchanged; buffers only grow.
void problem_set_topology(egs_problem *p, int32_t m, const int32_t *body0, const int32_t *body1, bool fresh) {
  egs_context *ctx = p->ctx;
  const int n = p->n;
  hipStream_t s = ctx->stream;
  const auto t_top0 = std::chrono::steady_clock::now();
  HIPCHK(hipStreamSynchronize(s));   // nothing may still read the pinned arena
  ctx->pinned.reset();
  p->m = m;
  p->h_body0.assign(body0, body0 + m);
  p->h_body1.assign(body1, body1 + m);
  p->tile_plan_ready = false;
  p->linsym_bodies = -1;
  p->share_normals = egs_problem::kShareDeviceData;   // no descriptors yet: egs_problem_set_constraints brings them
  p->mv_ready = false;
  p->dense_cfm = -1.0;
  p->h_rows_valid = false;
  p->use_quad = false;
  p->have_blocks = false;
  p->sys_deferred = false;
  p->have_constraints = false;
  p->last_iterations = 0;
  // the rows changed: x holds no lambda of this list, and a GIVEN start has the wrong length
  p->have_lambda = false;
  if (p->start_mode == EGS_START_GIVEN) p->start_mode = EGS_START_RHS;
  p->friction = false;   // the coefficients were those of the old list (the world refills them: world_step.cpp)
  p->restitution = false;   // likewise
  p->motors = false;        // likewise
  p->limits = false;        // likewise
  p->limited_hinge = -1;
  p->travels = false;       // likewise
  p->stopped_slider = -1;
  p->hinges = p->hinges_pinned = p->angular = p->sliders = false;
  p->pinned_slider = -1;
  p->h_kind.clear();
  {  // quad schedule: small problems whose islands all fit 64-constraint tiles
    const char *env = std::getenv("EGS_QUAD");
    const int force = env ? std::atoi(env) : -1;
    if (m > 0 && force != 0 && (force == 1 || (long)m <= 64L * quad_tiles_per_cu_max(p->precision) * p->ctx->cu_count)) {
      const char *qe = std::getenv("EGS_QUAD_TILE");   // experiment knob: force 64 or 256
      const int qt = qe ? std::atoi(qe) : 0;
      // 64-constraint tiles when every island fits, else 1024-thread tiles of 256
      // runs (plan.h) while there is about one tile per CU
      const auto t_pl0 = std::chrono::steady_clock::now();
      p->planq = build_plan(n, m, body0, body1, (qt == 64 || qt == 128 || qt == 256) ? qt : kAutoQuadBlock, &p->planq,
                            p->ctx->cu_count);
      if (std::getenv("EGS_PLAN_TRACE"))
        std::fprintf(stderr, "plan trace: build_plan(quad) %.1f us for %d constraints\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_pl0).count(), m);
      bool one_round = true;
      if (force != 1 && p->planq.global.empty()) {
        const size_t qlds = (size_t)p->planq.max_slots * 6 * p->real_size();
        const int occ = with_real(p, [&](auto r) { return occupancy_step_quad<decltype(r)>(p->planq.block, qlds); });
        one_round = (long)p->planq.n_tiles <= (long)occ * p->ctx->cu_count;
      }
      if (p->planq.global.empty() && one_round) {
        p->use_quad = true;
        p->quad.stage(p->ctx, p->planq);
        const size_t rsz = p->real_size(), mm2 = (size_t)m;
        p->wsB0.alloc(mm2 * 18 * rsz); p->wsB1.alloc(mm2 * 18 * rsz); p->wsD.alloc(mm2 * 9 * rsz); p->wsInv.alloc(mm2 * 3 * rsz);
      }
    }
  }
  stage(p->ctx, p->body0, p->h_body0);
  stage(p->ctx, p->body1, p->h_body1);
  const size_t rs = p->real_size();
  const size_t nn = (size_t)(n > 0 ? n : 1), mm = (size_t)(m > 0 ? m : 1);
  p->kind.alloc(mm); p->data.alloc(mm * 7);
  p->err.alloc(mm * 3);
  p->J0.alloc(mm * 18 * rs); p->J1.alloc(mm * 18 * rs);
  p->lo.alloc(mm * 3 * rs); p->hi.alloc(mm * 3 * rs); p->rhs.alloc(mm * 3 * rs);
  p->x.alloc(mm * 3 * rs); p->wres.alloc(mm * 3 * rs);
  p->is_eq.alloc(mm * 3);
  HIPCHK(hipMemsetAsync(p->acc.p, 0, nn * 6 * rs, s));
  if (fresh) {   // a re-planned world overwrites both in its next solve; a new problem reads as zeros
    HIPCHK(hipMemsetAsync(p->x.p, 0, mm * 3 * rs, s));
    HIPCHK(hipMemsetAsync(p->wres.p, 0, mm * 3 * rs, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  if (std::getenv("EGS_PLAN_TRACE"))
    std::fprintf(stderr, "plan trace: problem_set_topology %.1f us in all\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_top0).count());
  // the 1-lane schedule is built at the first solve that needs it (ensure_tile_plan):
  // its tile size depends on the mass blocks, which arrive after the topology
}

egs_status check_topology(egs_context *ctx, int32_t n, int32_t m, const int32_t *body0, const int32_t *body1) {
  if (n < 0 || m < 0 || (m > 0 && (!body0 || !body1))) return fail(ctx, EGS_ERR_INVALID, "bad sizes / NULL topology");
  for (int i = 0; i < m; ++i) {
    // (the schedule builder checks the range too, but the 1-lane schedule is built lazily)
    if (body0[i] < -1 || body0[i] >= n || body1[i] < -1 || body1[i] >= n)
      return fail(ctx, EGS_ERR_INVALID, "body index out of range");
    if (body0[i] >= 0 && body0[i] == body1[i])
      return fail(ctx, EGS_ERR_INVALID, "constraint with the same body on both sides");
  }
  return EGS_OK;
}
}  // namespace egs

extern "C" {

egs_status egs_problem_create(egs_context *ctx, int32_t n, int32_t m, const int32_t *body0,
                              const int32_t *body1, int32_t precision, egs_problem **out) {
  if (!ctx || !out) return EGS_ERR_INVALID;
  *out = nullptr;
  if (egs_status st = check_topology(ctx, n, m, body0, body1)) return st;
  if (precision != EGS_F64 && precision != EGS_F32) return fail(ctx, EGS_ERR_INVALID, "unknown precision");
  egs_problem *p = new (std::nothrow) egs_problem;
  if (!p) return fail(ctx, EGS_ERR_HIP, "host allocation failed");
  p->ctx = ctx; p->n = n; p->m = m; p->precision = precision;
  egs_status st = guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    const size_t rs = p->real_size(), nn = (size_t)(n > 0 ? n : 1);
    p->gtickets.alloc(nn);
    p->pos.alloc(nn * 3); p->R.alloc(nn * 9); p->v.alloc(nn * 3); p->w.alloc(nn * 3);
    p->Minv_d.alloc(nn * 36); p->f_ext.alloc(nn * 6); p->v6.alloc(nn * 6);
    p->res_partials.alloc(4 * kResidualBlocks);
    p->Minv_r.alloc(nn * 36 * rs);
    p->acc.alloc(nn * 6 * rs);
    p->error_flag.alloc(2);
    HIPCHK(hipMemsetAsync(p->error_flag.p, 0, 2 * sizeof(int32_t), ctx->stream));
    p->h_flag.alloc(16);   // 64 bytes
    *p->h_flag.p = 0;
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&p->h_flag_dev), p->h_flag.p, 0));
    problem_set_topology(p, m, body0, body1);
    return EGS_OK;
  });
  if (st != EGS_OK) { delete p; return st; }
  *out = p;
  return EGS_OK;
}

egs_status egs_problem_create_batch(egs_context *ctx, int32_t n_ensembles, const int32_t *n_bodies,
                                    const int32_t *n_constraints, const int32_t *body0, const int32_t *body1,
                                    int32_t precision, egs_problem **out, int32_t *body_offset,
                                    int32_t *constraint_offset) {
  if (!ctx || !out) return EGS_ERR_INVALID;
  *out = nullptr;
  if (n_ensembles < 0 || (n_ensembles > 0 && (!n_bodies || !n_constraints)))
    return fail(ctx, EGS_ERR_INVALID, "bad ensemble count / NULL size tables");
  long nb = 0, nc = 0;
  for (int e = 0; e < n_ensembles; ++e) {
    if (n_bodies[e] < 0 || n_constraints[e] < 0) return fail(ctx, EGS_ERR_INVALID, "negative ensemble size");
    nb += n_bodies[e]; nc += n_constraints[e];
  }
  if (nb > INT32_MAX || nc > INT32_MAX) return fail(ctx, EGS_ERR_INVALID, "batch too large for 32-bit indices");
  if (nc > 0 && (!body0 || !body1)) return fail(ctx, EGS_ERR_INVALID, "NULL topology");
  std::vector<int32_t> g0, g1;
  try {
    g0.resize((size_t)nc); g1.resize((size_t)nc);
  } catch (const std::bad_alloc &) {
    return fail(ctx, EGS_ERR_HIP, "host allocation failed");
  }
  long bo = 0, co = 0;
  for (int e = 0; e < n_ensembles; ++e) {
    if (body_offset) body_offset[e] = (int32_t)bo;
    if (constraint_offset) constraint_offset[e] = (int32_t)co;
    for (int i = 0; i < n_constraints[e]; ++i) {
      const int32_t a = body0[co + i], b = body1[co + i];
      if (a < -1 || a >= n_bodies[e] || b < -1 || b >= n_bodies[e])
        return fail(ctx, EGS_ERR_INVALID, "ensemble-local body index out of range");
      g0[(size_t)(co + i)] = a < 0 ? -1 : (int32_t)(bo + a);
      g1[(size_t)(co + i)] = b < 0 ? -1 : (int32_t)(bo + b);
    }
    bo += n_bodies[e]; co += n_constraints[e];
  }
  if (body_offset) body_offset[n_ensembles] = (int32_t)bo;
  if (constraint_offset) constraint_offset[n_ensembles] = (int32_t)co;
  return egs_problem_create(ctx, (int32_t)nb, (int32_t)nc, g0.data(), g1.data(), precision, out);
}

void egs_problem_destroy(egs_problem *p) {
  if (!p) return;
  if (p->ctx && p->ctx->stream) (void)hipStreamSynchronize(p->ctx->stream);
  delete p;
}

egs_status egs_problem_set_blocks(egs_problem *p, const double *Minv, const double *J0, const double *J1,
                                  const uint8_t *is_eq, const double *lo, const double *hi, const double *rhs) {
  if (!p) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    const size_t n = p->n, m = p->m;
    ensure_system(p);   // the arrays not given here keep the deferred step's values; M^-1 is one of its inputs
    if (Minv && n) { upload(p->Minv_d, Minv, n * 36, p->ctx->stream); p->minv_r_valid = false; p->wf_valid = false; }
    upload_real(p, p->J0, J0, m * 18);
    upload_real(p, p->J1, J1, m * 18);
    if (J0 || J1) {
      // step_solve_kernel's LINSYM form keeps ONE linear block per constraint: J1_lin = -J0_lin wherever both sides
      // exist, equal in value (a NaN refuses it) and bit for bit
      bool neg = J0 && J1 && p->precision == EGS_F64 && p->h_body0.size() == m && p->h_body1.size() == m;
      for (size_t i = 0; neg && i < m; ++i) {
        if (p->h_body0[i] < 0 || p->h_body1[i] < 0) continue;
        for (int r = 0; r < 3 && neg; ++r)
          for (int k = 0; k < 3 && neg; ++k) {
            const double a = J0[i * 18 + 6 * r + k], b = -J1[i * 18 + 6 * r + k];
            neg = a == b && std::memcmp(&a, &b, sizeof a) == 0;
          }
      }
      p->lin_neg = neg;
    }
    if (is_eq && m) upload(p->is_eq, is_eq, m * 3, p->ctx->stream);
    upload_real(p, p->lo, lo, m * 3);
    upload_real(p, p->hi, hi, m * 3);
    upload_real(p, p->rhs, rhs, m * 3);
    p->have_blocks = true;
    return EGS_OK;
  });
}

egs_status egs_problem_solve(egs_problem *p, const egs_solve_params *params, egs_solve_stats *stats) {
  if (!p) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status { return do_solve(p, params, stats); });
}

egs_status egs_problem_set_start(egs_problem *p, int32_t mode, const double *x0) {
  if (!p) return EGS_ERR_INVALID;
  if (mode != EGS_START_RHS && mode != EGS_START_GIVEN && mode != EGS_START_PREVIOUS)
    return fail(p->ctx, EGS_ERR_INVALID, "unknown start mode");
  const size_t rows = (size_t)p->m * 3;
  if (mode == EGS_START_GIVEN) {
    if (!x0 && rows > 0) return fail(p->ctx, EGS_ERR_INVALID, "EGS_START_GIVEN needs the 3m rows of x0");
    for (size_t i = 0; i < rows; ++i)
      if (x0[i] != x0[i]) return fail(p->ctx, EGS_ERR_INVALID, "NaN in x0");
  }
  return guarded(p->ctx, [&]() -> egs_status {
    if (mode == EGS_START_GIVEN) {
      HIPCHK(hipStreamSynchronize(p->ctx->stream));   // a solve in flight may still read the old start
      p->start.alloc((rows > 0 ? rows : 1) * p->real_size());
      upload_real(p, p->start, x0, rows);
    }
    p->start_mode = mode;
    return EGS_OK;
  });
}

egs_status egs_problem_set_friction(egs_problem *p, const double *mu) {
  if (!p) return EGS_ERR_INVALID;
  const size_t m = (size_t)p->m;
  bool any = false;
  for (size_t i = 0; mu && i < m; ++i) {
    if (mu[i] != mu[i]) return fail(p->ctx, EGS_ERR_INVALID, "NaN friction coefficient");
    any |= mu[i] >= 0;
  }
  return guarded(p->ctx, [&]() -> egs_status {
    HIPCHK(hipStreamSynchronize(p->ctx->stream));   // a solve in flight may still read the old coefficients
    if (any) {
      p->mu.alloc(m * p->real_size());
      upload_real(p, p->mu, mu, m);
    }
    p->friction = any;
    return EGS_OK;
  });
}

egs_status egs_problem_set_restitution(egs_problem *p, const double *rest, double vth) {
  if (!p) return EGS_ERR_INVALID;
  if (!(vth >= 0) || std::isinf(vth)) return fail(p->ctx, EGS_ERR_INVALID, "the restitution threshold must be finite and >= 0");
  const size_t m = (size_t)p->m;
  bool any = false;
  for (size_t i = 0; rest && i < m; ++i) {
    if (rest[i] != rest[i] || std::isinf(rest[i])) return fail(p->ctx, EGS_ERR_INVALID, "NaN or infinite restitution coefficient");
    any |= rest[i] >= 0;
  }
  return guarded(p->ctx, [&]() -> egs_status {
    ensure_system(p);   // a deferred system is the one of the table its step ran with
    HIPCHK(hipStreamSynchronize(p->ctx->stream));   // an assembly in flight may still read the old coefficients
    if (any) {
      p->rest.alloc(m);
      upload(p->rest, rest, m, p->ctx->stream);
    }
    p->restitution = any;
    p->rest_vth = vth;
    return EGS_OK;
  });
}

egs_status egs_problem_set_motors(egs_problem *p, const double *motor) {
  if (!p) return EGS_ERR_INVALID;
  const size_t m = (size_t)p->m;
  bool any = false;
  for (size_t i = 0; motor && i < m; ++i) {
    const double speed = motor[2 * i], tau = motor[2 * i + 1];
    if (speed != speed || std::isinf(speed)) return fail(p->ctx, EGS_ERR_INVALID, "NaN or infinite motor speed");
    if (tau != tau) return fail(p->ctx, EGS_ERR_INVALID, "NaN motor torque limit");
    any |= tau >= 0 && i < p->h_kind.size() && (p->h_kind[i] == EGS_JOINT_HINGE_AXIS || p->h_kind[i] == EGS_JOINT_SLIDER_AXIS);
  }
  return guarded(p->ctx, [&]() -> egs_status {
    ensure_system(p);   // a deferred system is the one of the table its step ran with
    HIPCHK(hipStreamSynchronize(p->ctx->stream));   // an assembly in flight may still read the old table
    if (any) {
      p->motor.alloc(m * 2);
      upload(p->motor, motor, m * 2, p->ctx->stream);
    }
    p->motors = any;
    note_hinges(p, any ? motor : nullptr);
    p->h_rows_valid = false;   // the axis rows' bounds follow the table
    return EGS_OK;
  });
}

egs_status egs_problem_set_hinge_limits(egs_problem *p, const double *lim) {
  if (!p) return EGS_ERR_INVALID;
  const size_t m = (size_t)p->m;
  int first = -1;
  if (lim && p->h_kind.size() != m) return fail(p->ctx, EGS_ERR_INVALID, "egs_problem_set_constraints first: the limits go with its kinds");
  if (lim)
    if (const char *fault = limits_fault(m, p->h_kind.data(), lim, &first)) return fail(p->ctx, EGS_ERR_INVALID, fault);
  return guarded(p->ctx, [&]() -> egs_status {
    ensure_system(p);   // a deferred system is the one of the table its step ran with
    HIPCHK(hipStreamSynchronize(p->ctx->stream));   // an assembly in flight may still read the old table
    if (first >= 0) {
      p->limit.alloc(m * 8);
      upload(p->limit, lim, m * 8, p->ctx->stream);
    }
    p->limits = first >= 0;
    p->limited_hinge = first;
    p->h_rows_valid = false;   // the axis rows' bounds follow the table
    return EGS_OK;
  });
}

egs_status egs_problem_set_slider_limits(egs_problem *p, const double *lim) {
  if (!p) return EGS_ERR_INVALID;
  const size_t m = (size_t)p->m;
  int first = -1;
  if (lim && p->h_kind.size() != m) return fail(p->ctx, EGS_ERR_INVALID, "egs_problem_set_constraints first: the limits go with its kinds");
  if (lim)
    if (const char *fault = travel_fault(m, p->h_kind.data(), lim, &first)) return fail(p->ctx, EGS_ERR_INVALID, fault);
  return guarded(p->ctx, [&]() -> egs_status {
    ensure_system(p);   // a deferred system is the one of the table its step ran with
    HIPCHK(hipStreamSynchronize(p->ctx->stream));   // an assembly in flight may still read the old table
    if (first >= 0) {
      p->travel.alloc(m * 2);
      upload(p->travel, lim, m * 2, p->ctx->stream);
    }
    p->travels = first >= 0;
    p->stopped_slider = first;
    p->h_rows_valid = false;   // the rail rows' bounds follow the table
    return EGS_OK;
  });
}

egs_status egs_problem_get_lambda(egs_problem *p, double *x) {
  if (!p || !x) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    download_real(p, p->x, x, (size_t)p->m * 3);
    return stall_seen(p) ? report_stall(p) : EGS_OK;   // the download synchronised: every earlier solve is accounted for
  });
}

egs_status egs_problem_get_accumulators(egs_problem *p, double *a) {
  if (!p || !a) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    download_real(p, p->acc, a, (size_t)p->n * 6);
    return stall_seen(p) ? report_stall(p) : EGS_OK;
  });
}

egs_status egs_problem_set_state(egs_problem *p, const double *pos, const double *R, const double *v,
                                 const double *w, const double *Minv, const double *f_ext) {
  if (!p) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    const size_t n = p->n;
    hipStream_t s = p->ctx->stream;
    ensure_system(p);   // before its inputs change
    if (pos) upload(p->pos, pos, n * 3, s);
    if (R) upload(p->R, R, n * 9, s);
    if (v) upload(p->v, v, n * 3, s);
    if (w) upload(p->w, w, n * 3, s);
    if (Minv) { upload(p->Minv_d, Minv, n * 36, s); p->minv_r_valid = false; p->wf_valid = false; }
    if (f_ext) { upload(p->f_ext, f_ext, n * 6, s); p->wf_valid = false; }
    p->have_state = true;
    return EGS_OK;
  });
}

egs_status egs_problem_set_mass(egs_problem *p, const double *inv_mass, const double *inv_inertia) {
  if (!p) return EGS_ERR_INVALID;
  if (p->n > 0 && (!inv_mass || !inv_inertia)) return fail(p->ctx, EGS_ERR_INVALID, "NULL mass arrays");
  return guarded(p->ctx, [&]() -> egs_status {
    const size_t n = (size_t)p->n;
    std::vector<double> blocks(n * 36, 0.0);
    for (size_t b = 0; b < n; ++b) {
      double *W = blocks.data() + b * 36;
      for (int k = 0; k < 3; ++k) W[7 * k] = inv_mass[b];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) W[6 * (3 + r) + 3 + c] = inv_inertia[b * 9 + 3 * r + c];
    }
    ensure_system(p);   // before its inputs change
    if (n) { upload(p->Minv_d, blocks.data(), n * 36, p->ctx->stream); p->minv_r_valid = false; p->wf_valid = false; }
    return EGS_OK;
  });
}

egs_status egs_problem_set_live_inertia(egs_problem *p, const double *inertia_body, const double *torque) {
  if (!p) return EGS_ERR_INVALID;
  return set_live_inertia(p, inertia_body, torque);
}

egs_status egs_problem_get_mass(egs_problem *p, double *Minv, double *f_ext) {
  if (!p) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    const size_t n = (size_t)p->n;
    hipStream_t s = p->ctx->stream;
    if (p->have_state) refresh_live_mass(p);   // live inertia: the arrays of the state the device holds now
    if (Minv && n) HIPCHK(hipMemcpyAsync(Minv, p->Minv_d.p, n * 36 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (f_ext && n) HIPCHK(hipMemcpyAsync(f_ext, p->f_ext.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return EGS_OK;
  });
}

egs_status egs_problem_set_constraints(egs_problem *p, const int32_t *kind, const double *data) {
  if (!p) return EGS_ERR_INVALID;
  if (p->m > 0 && (!kind || !data)) return fail(p->ctx, EGS_ERR_INVALID, "NULL constraint descriptors");
  if (const char *fault = constraints_fault(p->m, kind, p->h_body0.data(), data)) return fail(p->ctx, EGS_ERR_INVALID, fault);
  return guarded(p->ctx, [&]() -> egs_status {
    ensure_system(p);   // before its inputs change
    upload(p->kind, kind, (size_t)p->m, p->ctx->stream);
    upload(p->data, data, (size_t)p->m * 7, p->ctx->stream);
    note_kinds(p, kind);
    p->share_normals = egs_problem::kShareUndecided;
    p->motors = false;   // the table was given for the kinds before these
    p->limits = false;   // likewise
    p->limited_hinge = -1;
    p->travels = false;  // likewise
    p->stopped_slider = -1;
    p->have_constraints = true;
    p->h_rows_valid = false;
    return EGS_OK;
  });
}

egs_status egs_problem_assemble(egs_problem *p, double dt, double erp) {
  if (!p) return EGS_ERR_INVALID;
  if (!p->have_state || !p->have_constraints) return fail(p->ctx, EGS_ERR_INVALID, "set_state and set_constraints first");
  if (!(dt > 0)) return fail(p->ctx, EGS_ERR_INVALID, "dt must be > 0");
  return guarded(p->ctx, [&]() -> egs_status { refresh_live_mass(p); do_assemble(p, dt, erp); return EGS_OK; });
}

egs_status egs_problem_step(egs_problem *p, double dt, double erp, const egs_solve_params *params,
                            egs_solve_stats *stats) {
  if (!p) return EGS_ERR_INVALID;
  if (!p->have_state || !p->have_constraints) return fail(p->ctx, EGS_ERR_INVALID, "set_state and set_constraints first");
  if (!(dt > 0)) return fail(p->ctx, EGS_ERR_INVALID, "dt must be > 0");
  return guarded(p->ctx, [&]() -> egs_status {
    if (stall_seen(p)) return report_stall(p);   // an earlier (asynchronous) step timed out
    refresh_live_mass(p);
    note_assembled(p);   // what choose_sweep reads of the blocks this step makes
    egs_status st;
    // the solve's launch may write the velocities itself (problem.h: step_velocity); whatever happens in the solve, the
    // offer ends with it
    struct Offer {
      egs_problem *p;
      ~Offer() { p->step_velocity = egs_problem::kVelocityNone; }
    } offer{p};
    if (step_fuses_assembly(p, params)) {
      const AssembleArgs a = assemble_args(p, dt, erp);
      p->step_velocity = egs_problem::kVelocityOffered;
      st = do_solve(p, params, stats, &a);
    } else {
      do_assemble(p, dt, erp);
      st = do_solve(p, params, stats);
    }
    if (st != EGS_OK) return st;
    if (p->step_velocity != egs_problem::kVelocityWritten) do_velocity(p, dt);
    return EGS_OK;
  });
}

egs_status egs_problem_get_blocks(egs_problem *p, double *J0, double *J1, uint8_t *is_eq, double *lo,
                                  double *hi, double *rhs, double *err) {
  if (!p) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    const size_t m = p->m;
    ensure_system(p);
    download_real(p, p->J0, J0, m * 18);
    download_real(p, p->J1, J1, m * 18);
    download_real(p, p->lo, lo, m * 3);
    download_real(p, p->hi, hi, m * 3);
    download_real(p, p->rhs, rhs, m * 3);
    hipStream_t s = p->ctx->stream;
    if (is_eq && m) HIPCHK(hipMemcpyAsync(is_eq, p->is_eq.p, m * 3, hipMemcpyDeviceToHost, s));
    if (err && m) HIPCHK(hipMemcpyAsync(err, p->err.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return EGS_OK;
  });
}

egs_status egs_problem_get_velocity(egs_problem *p, double *v6) {
  if (!p || !v6) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    if (p->n) HIPCHK(hipMemcpyAsync(v6, p->v6.p, (size_t)p->n * 6 * sizeof(double), hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    return stall_seen(p) ? report_stall(p) : EGS_OK;
  });
}

egs_status egs_problem_advance(egs_problem *p, double dt) {
  if (!p) return EGS_ERR_INVALID;
  if (!p->have_state) return fail(p->ctx, EGS_ERR_INVALID, "set_state and step first");
  return guarded(p->ctx, [&]() -> egs_status {
    if (stall_seen(p)) return report_stall(p);   // do not integrate a lambda that came out of a timed-out wait
    // a second advance would overwrite the one old state set that is kept
    if (p->sys_deferred && p->deferred_prev) ensure_system(p);
    const BodyState cur{p->pos.p, p->R.p, p->v.p, p->w.p};
    if (!p->sys_deferred) {
      launch_advance(p->n, cur, cur, p->v6.p, dt, p->ctx->stream);
    } else {
      // the deferred system is assembled from the state the step read: the new state goes to the other set of buffers
      // and the sets change places (no copy, no extra launch)
      const size_t nn = (size_t)(p->n > 0 ? p->n : 1);
      p->prev_pos.alloc(nn * 3); p->prev_R.alloc(nn * 9); p->prev_v.alloc(nn * 3); p->prev_w.alloc(nn * 3);
      launch_advance(p->n, cur, BodyState{p->prev_pos.p, p->prev_R.p, p->prev_v.p, p->prev_w.p}, p->v6.p, dt, p->ctx->stream);
      swap_buffers(p->pos, p->prev_pos); swap_buffers(p->R, p->prev_R);
      swap_buffers(p->v, p->prev_v); swap_buffers(p->w, p->prev_w);
      p->deferred_prev = true;
    }
    HIPCHK(hipGetLastError());
    return EGS_OK;
  });
}

egs_status egs_problem_get_state(egs_problem *p, double *pos, double *R, double *v, double *w) {
  if (!p) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    const size_t n = p->n;
    hipStream_t s = p->ctx->stream;
    if (pos && n) HIPCHK(hipMemcpyAsync(pos, p->pos.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (R && n) HIPCHK(hipMemcpyAsync(R, p->R.p, n * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (v && n) HIPCHK(hipMemcpyAsync(v, p->v.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (w && n) HIPCHK(hipMemcpyAsync(w, p->w.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return stall_seen(p) ? report_stall(p) : EGS_OK;
  });
}

egs_status egs_problem_get_stats(egs_problem *p, egs_solve_stats *stats) {
  if (!p || !stats) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    std::memset(stats, 0, sizeof *stats);
    fill_stats(p, stats);
    stats->iterations = p->last_iterations;
    if (p->m == 0) return EGS_OK;
    int flag = 0;
    if (p->residual_pending) { launch_residual(p); p->residual_pending = false; }
    stats->residual = read_residual(p, &flag);
    stats->status = flag ? EGS_ERR_STALL : EGS_OK;
    return flag ? fail(p->ctx, EGS_ERR_STALL, "device ordering wait timed out") : EGS_OK;
  });
}

egs_status egs_problem_get_schedule(egs_problem *p, int32_t *schedule) {
  if (!p || !schedule) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    egs_solve_stats st;
    std::memset(&st, 0, sizeof st);
    fill_stats(p, &st);
    *schedule = st.schedule | (int32_t)(p->last_sched & egs_problem::kSchedRefinements);
    return EGS_OK;
  });
}

egs_status egs_problem_get_schedule_full(egs_problem *p, int32_t *schedule) {
  if (!p || !schedule) return EGS_ERR_INVALID;
  const egs_status st = egs_problem_get_schedule(p, schedule);
  if (st == EGS_OK) *schedule |= (int32_t)(p->last_sched & egs_problem::kSchedFullOnly);
  return st;
}

egs_status egs_problem_get_schedule_forms(egs_problem *p, int32_t *schedule) {
  if (!p || !schedule) return EGS_ERR_INVALID;
  const egs_status st = egs_problem_get_schedule_full(p, schedule);
  if (st == EGS_OK) *schedule |= (int32_t)(p->last_sched & egs_problem::kSchedFormsOnly);
  return st;
}

egs_status egs_solve_blocks(egs_context *ctx, int32_t n, const double *Minv, int32_t m, const int32_t *body0,
                            const int32_t *body1, const double *J0, const double *J1, const uint8_t *is_eq,
                            const double *lo, const double *hi, const double *rhs, const egs_solve_params *params,
                            int32_t precision, double *x, egs_solve_stats *stats) {
  if (!ctx) return EGS_ERR_INVALID;
  if (m > 0 && (!Minv || !body0 || !body1 || !J0 || !J1 || !is_eq || !lo || !hi || !rhs || !x))
    return fail(ctx, EGS_ERR_INVALID, "NULL array");
  egs_problem *p = nullptr;
  egs_status st = oneshot_problem(ctx, n, m, body0, body1, precision, &p);
  if (st != EGS_OK) return st;
  st = egs_problem_set_blocks(p, Minv, J0, J1, is_eq, lo, hi, rhs);
  egs_solve_stats local;
  if (st == EGS_OK) st = egs_problem_solve(p, params, stats ? stats : &local);
  if (st == EGS_OK && m > 0) st = egs_problem_get_lambda(p, x);
  return st;
}

egs_status egs_problem_matvec(egs_problem *p, int32_t parts, double eps, double scale, const double *x, double *y) {
  if (!p) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status { return do_matvec(p, parts, eps, scale, x, y); });
}

egs_status egs_problem_get_matvec(egs_problem *p, double *y) {
  if (!p || !y) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    if (!p->mv_ready) return fail(p->ctx, EGS_ERR_INVALID, "egs_problem_matvec first");
    download_real(p, p->mv_y, y, (size_t)p->m * 3);
    return EGS_OK;
  });
}

egs_status egs_problem_get_wres(egs_problem *p, double *w) {
  if (!p || !w) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    download_real(p, p->wres, w, (size_t)p->m * 3);
    return stall_seen(p) ? report_stall(p) : EGS_OK;
  });
}

egs_status egs_matvec_blocks(egs_context *ctx, int32_t n, const double *Minv, int32_t m, const int32_t *body0,
                             const int32_t *body1, const double *J0, const double *J1, int32_t parts, double eps,
                             double scale, int32_t precision, const double *x, double *y) {
  if (!ctx) return EGS_ERR_INVALID;
  if (m > 0 && (!Minv || !body0 || !body1 || !J0 || !J1 || !x || !y)) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  egs_problem *p = nullptr;
  egs_status st = oneshot_problem(ctx, n, m, body0, body1, precision, &p);
  if (st != EGS_OK) return st;
  st = egs_problem_set_blocks(p, Minv, J0, J1, nullptr, nullptr, nullptr, nullptr);
  if (st == EGS_OK) st = egs_problem_matvec(p, parts, eps, scale, x, y);
  return st;
}

egs_status egs_problem_debug_trace(egs_problem *p, uint64_t *out, int64_t count, int32_t *sweeps) {
  if (!p || !out) return EGS_ERR_INVALID;
  return guarded(p->ctx, [&]() -> egs_status {
    if (sweeps) *sweeps = p->trace_sweeps;
    const int64_t have = (int64_t)p->trace_sweeps * p->m;
    if (have <= 0 || count < have) return fail(p->ctx, EGS_ERR_INVALID, "no trace recorded (EGS_TRACE_UPDATES=1, an island on 4-lane patches) or buffer too small");
    HIPCHK(hipMemcpyAsync(out, p->trace.p, (size_t)have * sizeof(uint64_t), hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    return EGS_OK;
  });
}

}  // extern "C"
