// world.cpp -- the core of the egs_world_* entries of the C ABI, with the stateless egs_update_contacts[_joints]:
// Ensemble::Step (ensembles.cc:390-427) resident on the device, for one ensemble or a batch of them.  Here: create and
// destroy, the set and get entries, the contact update and the re-plan.  The stepping entries are in world_step.cpp
// (the sparse sweeps, with the warm start) and world_dense.cpp (the dense path), the stabilisation passes in
// world_stabilize.cpp; struct egs_world and what crosses these units is in world.h.
#include <cmath>
#include <limits>

#include "world.h"

using namespace egs;

namespace {

void world_fill_motors(egs_world *w);
void world_fill_limits(egs_world *w);
void world_fill_travel(egs_world *w);

void world_make_problem(egs_world *w, const int32_t *b0, const int32_t *b1, int m) {
  hipStream_t s = w->ctx->stream;
  if (!w->prob) {
    egs_problem *created = nullptr;
    egs_status st = egs_problem_create(w->ctx, w->n, m, b0, b1, w->precision, &created);
    if (st != EGS_OK) throw HipError(std::string("world: egs_problem_create: ") + egs_last_error(w->ctx));
    w->prob = created;
  } else {  // same bodies, new constraint list: the body state stays where it is
    if (check_topology(w->ctx, w->n, m, b0, b1) != EGS_OK)
      throw std::invalid_argument(egs_last_error(w->ctx));
    problem_set_topology(w->prob, m, b0, b1, /*fresh=*/false);
  }
  egs_problem *np = w->prob;
  // constraint kinds: joints first, then contacts; joint descriptors are static
  std::vector<int32_t> kind((size_t)(m > 0 ? m : 1), EGS_CONTACT_BOX);
  const int mj = (int)w->jb0.size();
  for (int i = 0; i < mj; ++i) kind[i] = w->jkind[(size_t)i];
  if (m > 0) {
    kind.resize((size_t)m);
    stage(w->ctx, np->kind, kind);   // through the pinned arena (reset only after a synchronise): no wait here
    note_kinds(np, kind.data());
    if (mj > 0) upload(np->data, w->jdata.data(), (size_t)mj * 7, s);
  }
  world_fill_motors(w);
  world_fill_limits(w);
  world_fill_travel(w);
  np->have_constraints = true;
  np->h_rows_valid = false;
  w->topo_b0.assign(b0, b0 + m); w->topo_b1.assign(b1, b1 + m);
  ++w->replans;
}

// The problem's motor table for its current list from the joints' (the joints come first; no contact row is read:
// assemble_device.h, motor_row).  The new topology has turned the problem's table off.
void world_fill_motors(egs_world *w) {
  egs_problem *p = w->prob;
  const size_t mj = w->jb0.size();
  p->motors = false;
  if (w->jmotor.empty() || p->m <= 0) { note_hinges(p, nullptr); return; }
  std::vector<double> t((size_t)p->m * 2, -1.0);
  std::copy(w->jmotor.begin(), w->jmotor.end(), t.begin());
  bool any = false;
  for (size_t i = 0; i < mj; ++i) any |= (w->jkind[i] == EGS_JOINT_HINGE_AXIS || w->jkind[i] == EGS_JOINT_SLIDER_AXIS) && t[2 * i + 1] >= 0;
  if (any) {
    p->motor.alloc(t.size());
    upload(p->motor, t.data(), t.size(), w->ctx->stream);
    p->motors = true;
  }
  note_hinges(p, any ? t.data() : nullptr);
  p->h_rows_valid = false;
}

// The problem's limit table for its current list from the joints' (the joints come first; the contacts' rows are
// zeros, which limit_row never reads: it returns on the kind).  The new topology has turned the problem's table off.
void world_fill_limits(egs_world *w) {
  egs_problem *p = w->prob;
  const size_t mj = w->jb0.size();
  p->limits = false;
  p->limited_hinge = -1;
  if (w->jlimit.empty() || p->m <= 0) return;
  std::vector<double> t((size_t)p->m * 8, 0.0);
  std::copy(w->jlimit.begin(), w->jlimit.end(), t.begin());
  int first = -1;
  limits_fault(mj, w->jkind.data(), w->jlimit.data(), &first);   // validated when it was set: the first stop only
  if (first >= 0) {
    p->limit.alloc(t.size());
    upload(p->limit, t.data(), t.size(), w->ctx->stream);
    p->limits = true;
    p->limited_hinge = first;
  }
  p->h_rows_valid = false;
}

// The problem's travel table for its current list from the joints' (the joints come first; the contacts' rows are
// (-inf, +inf), which slider_stop_row never reads: it returns on the kind).  The new topology has turned the problem's
// table off.
void world_fill_travel(egs_world *w) {
  egs_problem *p = w->prob;
  const size_t mj = w->jb0.size();
  p->travels = false;
  p->stopped_slider = -1;
  if (w->jtravel.empty() || p->m <= 0) return;
  std::vector<double> t((size_t)p->m * 2);
  for (size_t i = 0; i < t.size(); ++i) t[i] = i % 2 ? INFINITY : -INFINITY;
  std::copy(w->jtravel.begin(), w->jtravel.end(), t.begin());
  int first = -1;
  travel_fault(mj, w->jkind.data(), w->jtravel.data(), &first);   // validated when it was set: the first stop only
  if (first >= 0) {
    p->travel.alloc(t.size());
    upload(p->travel, t.data(), t.size(), w->ctx->stream);
    p->travels = true;
    p->stopped_slider = first;
  }
  p->h_rows_valid = false;
}

bool holds_capsule(const std::vector<int32_t> &shape) {
  for (int32_t v : shape) if (v == EGS_SHAPE_CAPSULE) return true;
  return false;
}

egs_status update_contacts_entry(egs_context *ctx, int32_t n, const double *pos, const double *R, const double *side,
                                 int32_t m_joints, const int32_t *jb0, const int32_t *jb1, const double *jdata,
                                 const int32_t *shape, int32_t max_contacts, int32_t *m_out, int32_t *body0,
                                 int32_t *body1, double *data) {
  if (!ctx) return EGS_ERR_INVALID;
  if (n < 0 || m_joints < 0 || !m_out || (n > 0 && (!pos || !R || !side)) || (m_joints > 0 && (!jb0 || !jb1 || !jdata)) ||
      (max_contacts > 0 && (!body0 || !body1 || !data)))
    return fail(ctx, EGS_ERR_INVALID, "NULL array");
  for (int q = 0; q < m_joints; ++q)
    if (jb0[q] < -1 || jb0[q] >= n || jb1[q] < -1 || jb1[q] >= n) return fail(ctx, EGS_ERR_INVALID, "joint body index out of range");
  if (shape) {
    const std::string fault = shapes_fault(n, shape, side);
    if (!fault.empty()) return fail(ctx, EGS_ERR_INVALID, fault);
  }
  *m_out = 0;
  // only body-body joints can prune (the pair scan never visits the ground, quirk Q4)
  std::vector<int32_t> b0, b1; std::vector<double> jd;
  for (int q = 0; q < m_joints; ++q)
    if (jb0[q] >= 0 && jb1[q] >= 0) { b0.push_back(jb0[q]); b1.push_back(jb1[q]); jd.insert(jd.end(), jdata + 7 * (size_t)q, jdata + 7 * (size_t)q + 7); }
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    *m_out = update_contacts(ctx->stream, n, pos, R, side, max_contacts, body0, body1, data, nullptr, nullptr,
                             (int)b0.size(), b0.data(), b1.data(), jd.data(), shape);
    return EGS_OK;
  });
}

// egs_world_set_friction / egs_world_set_restitution: the table's checks -- NULL, n_ensembles, then the entry's own
// (check) -- its upload, and any: is some coefficient >= 0?
template <typename CHECK>
egs_status world_set_table(egs_world *w, CoeffTable &t, int32_t n_ensembles, const double *values, const char *null_msg,
                           CHECK &&check) {
  if (!values) return fail(w->ctx, EGS_ERR_INVALID, null_msg);
  if (egs_status st = world_check_ensembles(w, n_ensembles)) return st;
  if (egs_status st = check()) return st;
  bool any = false;
  for (int e = 0; e < n_ensembles; ++e) any |= values[e] >= 0;
  return guarded(w->ctx, [&]() -> egs_status {
    hipStream_t s = w->ctx->stream;
    HIPCHK(hipStreamSynchronize(s));   // a step in flight may still read the old table
    t.d.alloc((size_t)n_ensembles);
    t.h.assign(values, values + n_ensembles);
    HIPCHK(hipMemcpyAsync(t.d.p, values, (size_t)n_ensembles * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // values is the caller's
    t.any = any;
    return EGS_OK;
  });
}

}  // namespace

namespace egs {

// What is wrong with a shape array (nothing: an empty string): a value that is no egs_shape, or -- where the side lengths are
// known (side != NULL) -- a sphere whose side row is not three equal positive numbers, a capsule whose side row is not
// (d, d, l) with 0 < d < l, both finite.
std::string shapes_fault(int n, const int32_t *shape, const double *side) {
  for (int b = 0; b < n; ++b) {
    if (shape[b] != EGS_SHAPE_BOX && shape[b] != EGS_SHAPE_SPHERE && shape[b] != EGS_SHAPE_CAPSULE)
      return "body " + std::to_string(b) + ": unknown shape " + std::to_string(shape[b]);
    if (shape[b] == EGS_SHAPE_BOX || !side) continue;
    const double *d = side + 3 * (size_t)b;
    if (shape[b] == EGS_SHAPE_SPHERE) {
      if (!(d[0] > 0) || d[1] != d[0] || d[2] != d[0])
        return "body " + std::to_string(b) + ": a sphere's side_lengths must be (d, d, d) with d > 0";
    } else if (!(d[0] > 0) || d[1] != d[0] || !(d[2] > d[0]) || !std::isfinite(d[0]) || !std::isfinite(d[2])) {
      return "body " + std::to_string(b) + ": a capsule's side_lengths must be (d, d, l) with 0 < d < l, both finite" +
             (d[2] == d[0] ? " (l == d is a sphere: use EGS_SHAPE_SPHERE)" : "");
    }
  }
  return std::string();
}

void world_update_contacts(egs_world *w, PhaseTimer *lap) {
  hipStream_t s = w->ctx->stream;
  const int mj = (int)w->jb0.size();
  // the pruning takes the ball joints alone
  const int mc = w->col.run(s, w->n, w->prob->pos.p, w->prob->R.p, w->dside.p, w->mj_ball, w->djb0.p, w->djb1.p, w->djdata.p,
                            w->shapes ? w->dshape.p : nullptr, w->shapes && w->capsules);
  if (lap) (*lap)(0);
  const size_t mt = (size_t)mj + (size_t)mc;
  if (mt > w->h_cap) {   // grow-only; the stream is idle here (col.run synchronised)
    w->topo_pinned.reset();
    w->h_cap = mt + mt / 4 + 64;
    w->h_b0 = static_cast<int32_t *>(w->topo_pinned.take(2 * w->h_cap * sizeof(int32_t)));
    w->h_b1 = w->h_b0 + w->h_cap;
  }
  std::copy(w->jb0.begin(), w->jb0.end(), w->h_b0);
  std::copy(w->jb1.begin(), w->jb1.end(), w->h_b1);
  if (mc > 0) {   // the GPU writes the 8 bytes per contact straight into page-locked host memory
    w->col.export_topology(s, mc, w->h_b0 + mj, w->h_b1 + mj);
    HIPCHK(hipStreamSynchronize(s));
  }
  const bool changed = mt != w->topo_b0.size() || (mt > 0 && (
                       std::memcmp(w->h_b0, w->topo_b0.data(), mt * sizeof(int32_t)) != 0 ||
                       std::memcmp(w->h_b1, w->topo_b1.data(), mt * sizeof(int32_t)) != 0));
  if (lap) (*lap)(1);
  if (changed) world_make_problem(w, w->h_b0, w->h_b1, (int)mt);  // host plan only on topology change
  if (lap) (*lap)(2);
  w->prob->share_normals = egs_problem::kShareDeviceData;   // the contacts' descriptors are written on the device
  if (mc > 0)
    HIPCHK(hipMemcpyAsync(w->prob->data.p + (size_t)mj * 7, w->col.data(), (size_t)mc * 7 * sizeof(double),
                          hipMemcpyDeviceToDevice, s));
  w->m_contacts = mc;
}

}  // namespace egs

extern "C" {

egs_status egs_update_contacts_joints(egs_context *ctx, int32_t n, const double *pos, const double *R,
                                      const double *side, int32_t m_joints, const int32_t *jb0, const int32_t *jb1,
                                      const double *jdata, int32_t max_contacts, int32_t *m_out, int32_t *body0,
                                      int32_t *body1, double *data) {
  return update_contacts_entry(ctx, n, pos, R, side, m_joints, jb0, jb1, jdata, nullptr, max_contacts, m_out, body0, body1, data);
}

egs_status egs_update_contacts_shapes(egs_context *ctx, int32_t n, const double *pos, const double *R,
                                      const double *side, int32_t m_joints, const int32_t *jb0, const int32_t *jb1,
                                      const double *jdata, const int32_t *shape, int32_t max_contacts, int32_t *m_out,
                                      int32_t *body0, int32_t *body1, double *data) {
  return update_contacts_entry(ctx, n, pos, R, side, m_joints, jb0, jb1, jdata, shape, max_contacts, m_out, body0, body1, data);
}

egs_status egs_update_contacts(egs_context *ctx, int32_t n, const double *pos, const double *R, const double *side,
                               int32_t max_contacts, int32_t *m_out, int32_t *body0, int32_t *body1, double *data) {
  return egs_update_contacts_joints(ctx, n, pos, R, side, 0, nullptr, nullptr, nullptr, max_contacts, m_out, body0, body1, data);
}

egs_status egs_world_create(egs_context *ctx, int32_t n_bodies, int32_t precision, egs_world **out) {
  if (!ctx || !out || n_bodies < 0) return EGS_ERR_INVALID;
  *out = nullptr;
  if (precision != EGS_F64 && precision != EGS_F32) return fail(ctx, EGS_ERR_INVALID, "unknown precision");
  egs_world *w = new (std::nothrow) egs_world;
  if (!w) return fail(ctx, EGS_ERR_HIP, "host allocation failed");
  w->ctx = ctx; w->n = n_bodies; w->precision = precision;
  { const char *te = std::getenv("EGS_WORLD_TRACE"); w->trace = te && std::atoi(te) != 0; }
  egs_status st = guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    w->dside.alloc((size_t)(n_bodies > 0 ? n_bodies : 1) * 3);
    return EGS_OK;
  });
  if (st != EGS_OK) { delete w; return st; }
  *out = w;
  return EGS_OK;
}

void egs_world_destroy(egs_world *w) {
  if (!w) return;
  if (w->trace && w->t_phase[4] > 0) {
    const double k = 1.0 / w->t_phase[4];
    std::fprintf(stderr, "egs_world trace (%d steps, %d re-plans), us/step: collide %.1f  topology %.1f  re-plan %.1f  solve+integrate %.1f\n",
                 (int)w->t_phase[4], w->replans, w->t_phase[0] * k, w->t_phase[1] * k, w->t_phase[2] * k, w->t_phase[3] * k);
  }
  if (w->trace && w->t_stab[5] > 0) {
    const double k = 1.0 / w->t_stab[5];
    std::fprintf(stderr, "egs_world stabilize trace (%d passes), us/pass: detect+re-plan %.1f  relaxation re-topology %.1f  "
                 "assemble+test %.1f  solve %.1f  J^T y+relax %.1f\n", (int)w->t_stab[5], w->t_stab[0] * k, w->t_stab[1] * k,
                 w->t_stab[2] * k, w->t_stab[3] * k, w->t_stab[4] * k);
  }
  delete w;   // every member releases what it owns
}

egs_status egs_world_set_bodies(egs_world *w, const double *pos, const double *R, const double *v, const double *wv,
                                const double *Minv, const double *f_ext, const double *side_lengths) {
  if (!w) return EGS_ERR_INVALID;
  // the first call needs everything; afterwards NULL = keep (M^-1, f_ext and the side lengths
  // are frozen at Init in the reference, Q5)
  if (w->n > 0 && !w->have_bodies && (!pos || !R || !v || !wv || !Minv || !f_ext || !side_lengths))
    return fail(w->ctx, EGS_ERR_INVALID, "NULL array on the first egs_world_set_bodies");
  if (w->shapes && side_lengths) {   // new side lengths under the shapes in force: nothing changes if they do not fit
    const std::string fault = shapes_fault(w->n, w->h_shape.data(), side_lengths);
    if (!fault.empty()) return fail(w->ctx, EGS_ERR_INVALID, fault);
  }
  return guarded(w->ctx, [&]() -> egs_status {
    if (!w->prob) world_make_problem(w, w->jb0.data(), w->jb1.data(), (int)w->jb0.size());
    egs_status st = egs_problem_set_state(w->prob, pos, R, v, wv, Minv, f_ext);
    if (st != EGS_OK) return st;
    world_drop_history(w);
    if (side_lengths) {
      upload(w->dside, side_lengths, (size_t)w->n * 3, w->ctx->stream);
      w->h_side.assign(side_lengths, side_lengths + (size_t)w->n * 3);
    }
    w->have_bodies = true;
    return EGS_OK;
  });
}

egs_status egs_world_set_live_inertia(egs_world *w, const double *inertia_body, const double *torque) {
  if (!w) return EGS_ERR_INVALID;
  egs_status made = guarded(w->ctx, [&]() -> egs_status {   // valid before egs_world_set_bodies, as set_bodies itself is
    if (!w->prob) world_make_problem(w, w->jb0.data(), w->jb1.data(), (int)w->jb0.size());
    return EGS_OK;
  });
  if (made != EGS_OK) return made;
  return set_live_inertia(w->prob, inertia_body, torque);
}

egs_status egs_world_get_mass(egs_world *w, double *Minv, double *f_ext) {
  if (!w) return EGS_ERR_INVALID;
  if (!w->have_bodies) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  return egs_problem_get_mass(w->prob, Minv, f_ext);
}

egs_status egs_world_set_shapes(egs_world *w, const int32_t *shape) {
  if (!w) return EGS_ERR_INVALID;
  if (shape) {   // against the side lengths if egs_world_set_bodies has given them, else there when it does
    const std::string fault = shapes_fault(w->n, shape, w->h_side.empty() ? nullptr : w->h_side.data());
    if (!fault.empty()) return fail(w->ctx, EGS_ERR_INVALID, fault);
  }
  return guarded(w->ctx, [&]() -> egs_status {
    if (shape && w->n > 0) {
      w->dshape.alloc((size_t)w->n);
      upload(w->dshape, shape, (size_t)w->n, w->ctx->stream);
      w->h_shape.assign(shape, shape + w->n);
    }
    w->shapes = shape && w->n > 0;
    if (!w->shapes) w->h_shape.clear();
    w->capsules = holds_capsule(w->h_shape);
    world_drop_history(w);
    return EGS_OK;
  });
}

egs_status egs_world_create_batch(egs_context *ctx, int32_t n_ensembles, const int32_t *n_bodies, int32_t precision,
                                  egs_world **out, int32_t *body_offset) {
  if (!ctx || !out) return EGS_ERR_INVALID;
  *out = nullptr;
  if (n_ensembles < 1 || !n_bodies) return fail(ctx, EGS_ERR_INVALID, "bad ensemble count / NULL size table");
  std::vector<int32_t> off((size_t)n_ensembles + 1, 0);
  long nb = 0;
  for (int e = 0; e < n_ensembles; ++e) {
    if (n_bodies[e] < 0) return fail(ctx, EGS_ERR_INVALID, "negative ensemble size");
    nb += n_bodies[e];
    if (nb > INT32_MAX) return fail(ctx, EGS_ERR_INVALID, "batch too large for 32-bit indices");
    off[(size_t)e + 1] = (int32_t)nb;
  }
  if (body_offset) std::copy(off.begin(), off.end(), body_offset);
  egs_status st = egs_world_create(ctx, (int32_t)nb, precision, out);
  if (st != EGS_OK || n_ensembles == 1) return st;   // one ensemble: the plain world, nothing else
  egs_world *w = *out;
  st = guarded(ctx, [&]() -> egs_status {
    const size_t E = (size_t)n_ensembles;
    EnsembleLayout &L = w->ens;
    L.n_ens = n_ensembles;
    L.body_off = off;
    L.joint_off.assign(E + 1, 0);
    std::vector<int32_t> ens((size_t)(nb > 0 ? nb : 1), 0);
    for (size_t e = 0; e < E; ++e)
      for (int32_t b = off[e]; b < off[e + 1]; ++b) ens[(size_t)b] = (int32_t)e;
    L.d_ens.alloc(ens.size()); upload(L.d_ens, ens.data(), ens.size(), ctx->stream);
    L.d_boff.alloc(E + 1); upload(L.d_boff, off.data(), E + 1, ctx->stream);
    L.d_joff.alloc(E + 1); upload(L.d_joff, L.joint_off.data(), E + 1, ctx->stream);
    L.d_coff.alloc(E + 1); upload(L.d_coff, L.joint_off.data(), E + 1, ctx->stream);   // no contacts yet
    L.batch.segs = EnsembleSegs{n_ensembles, 0, L.d_joff.p, L.d_coff.p, L.d_boff.p};
    L.batch.ensure(n_ensembles);
    std::fill(L.batch.h_ints.p, L.batch.h_ints.p + E + 2, 0);
    std::fill(L.batch.h_res.p, L.batch.h_res.p + E, 0.0);
    w->col.set_ensembles(n_ensembles, L.d_ens.p, L.d_boff.p, L.d_coff.p);
    return EGS_OK;
  });
  if (st != EGS_OK) { egs_world_destroy(w); *out = nullptr; }
  return st;
}

egs_status egs_world_set_joints_kinds(egs_world *w, int32_t m_joints, const int32_t *kind, const int32_t *body0,
                                      const int32_t *body1, const double *data) {
  if (!w || m_joints < 0 || (m_joints > 0 && (!body0 || !body1 || !data))) return EGS_ERR_INVALID;
  for (int i = 0; kind && i < m_joints; ++i)
    if (kind[i] == EGS_CONTACT_BOX) return fail(w->ctx, EGS_ERR_INVALID, "a contact is not a joint");
  if (kind)
    if (const char *fault = constraints_fault(m_joints, kind, body0, data)) return fail(w->ctx, EGS_ERR_INVALID, fault);
  EnsembleLayout &L = w->ens;
  std::vector<int32_t> joint_off;
  if (L.n_ens > 1) {   // every joint inside one ensemble, the joints grouped by ensemble (order within kept)
    joint_off.assign((size_t)L.n_ens + 1, 0);
    int last = 0;
    for (int i = 0; i < m_joints; ++i) {
      const int32_t a = body0[i], b = body1[i];
      if (a < -1 || a >= w->n || b < -1 || b >= w->n || (a < 0 && b < 0))
        return fail(w->ctx, EGS_ERR_INVALID, "joint body index out of range");
      const int ea = a >= 0 ? L.ensemble_of(a) : -1, eb = b >= 0 ? L.ensemble_of(b) : -1;
      if (ea >= 0 && eb >= 0 && ea != eb) return fail(w->ctx, EGS_ERR_INVALID, "joint between two ensembles");
      const int e = ea >= 0 ? ea : eb;
      if (e < last) return fail(w->ctx, EGS_ERR_INVALID, "joints not grouped by ensemble");
      last = e;
      ++joint_off[(size_t)e + 1];
    }
    for (int e = 0; e < L.n_ens; ++e) joint_off[(size_t)e + 1] += joint_off[(size_t)e];
  }
  w->jb0.assign(body0, body0 + m_joints);
  w->jb1.assign(body1, body1 + m_joints);
  w->jdata.assign(data, data + (size_t)m_joints * 7);
  if (kind) w->jkind.assign(kind, kind + m_joints);
  else w->jkind.assign((size_t)m_joints, EGS_JOINT_BALL);
  w->jmotor.clear();   // the motors were those of the old list
  w->jlimit.clear();   // and the limits
  w->jtravel.clear();  // and the sliders' travel stops
  // the ball joints, in list order: what the collider prunes against
  std::vector<int32_t> bb0, bb1;
  std::vector<double> bd;
  for (int i = 0; i < m_joints; ++i) {
    if (w->jkind[(size_t)i] != EGS_JOINT_BALL) continue;
    bb0.push_back(body0[i]); bb1.push_back(body1[i]);
    bd.insert(bd.end(), data + 7 * (size_t)i, data + 7 * (size_t)i + 7);
  }
  const size_t mb = bb0.size();
  w->mj_ball = (int)mb;
  return guarded(w->ctx, [&]() -> egs_status {
    w->djb0.alloc(mb); w->djb1.alloc(mb); w->djdata.alloc(mb * 7);
    if (mb > 0) {
      upload(w->djb0, bb0.data(), mb, w->ctx->stream);
      upload(w->djb1, bb1.data(), mb, w->ctx->stream);
      upload(w->djdata, bd.data(), mb * 7, w->ctx->stream);
    }
    world_make_problem(w, w->jb0.data(), w->jb1.data(), m_joints);   // contacts are re-detected by the next step
    w->m_contacts = 0;
    world_drop_history(w);
    if (L.n_ens > 1) {
      const size_t E1 = (size_t)L.n_ens + 1;
      L.joint_off = joint_off;
      upload(L.d_joff, joint_off.data(), E1, w->ctx->stream);
      HIPCHK(hipMemsetAsync(L.d_coff.p, 0, E1 * sizeof(int32_t), w->ctx->stream));
      L.batch.segs.mj = m_joints;
    }
    return EGS_OK;
  });
}

egs_status egs_world_set_joints(egs_world *w, int32_t m_joints, const int32_t *body0, const int32_t *body1,
                                const double *data) {
  return egs_world_set_joints_kinds(w, m_joints, nullptr, body0, body1, data);
}

egs_status egs_world_set_joint_motors(egs_world *w, const double *motor) {
  if (!w) return EGS_ERR_INVALID;
  const size_t mj = w->jb0.size();
  for (size_t i = 0; motor && i < mj; ++i) {
    const double speed = motor[2 * i], tau = motor[2 * i + 1];
    if (speed != speed || std::isinf(speed)) return fail(w->ctx, EGS_ERR_INVALID, "NaN or infinite motor speed");
    if (tau != tau) return fail(w->ctx, EGS_ERR_INVALID, "NaN motor torque limit");
  }
  return guarded(w->ctx, [&]() -> egs_status {
    if (w->prob) {
      ensure_system(w->prob);
      HIPCHK(hipStreamSynchronize(w->ctx->stream));   // an assembly in flight may still read the old table
    }
    if (motor) w->jmotor.assign(motor, motor + 2 * mj);
    else w->jmotor.clear();
    if (w->prob) world_fill_motors(w);
    return EGS_OK;
  });
}

egs_status egs_world_set_joint_limits(egs_world *w, const double *lim) {
  if (!w) return EGS_ERR_INVALID;
  const size_t mj = w->jb0.size();
  int first = -1;
  if (const char *fault = limits_fault(mj, w->jkind.data(), lim, &first)) return fail(w->ctx, EGS_ERR_INVALID, fault);
  return guarded(w->ctx, [&]() -> egs_status {
    if (w->prob) {
      ensure_system(w->prob);
      HIPCHK(hipStreamSynchronize(w->ctx->stream));   // an assembly in flight may still read the old table
    }
    if (lim && first >= 0) w->jlimit.assign(lim, lim + 8 * mj);
    else w->jlimit.clear();
    if (w->prob) world_fill_limits(w);
    return EGS_OK;
  });
}

egs_status egs_world_set_slider_limits(egs_world *w, const double *lim) {
  if (!w) return EGS_ERR_INVALID;
  const size_t mj = w->jb0.size();
  int first = -1;
  if (const char *fault = travel_fault(mj, w->jkind.data(), lim, &first)) return fail(w->ctx, EGS_ERR_INVALID, fault);
  return guarded(w->ctx, [&]() -> egs_status {
    if (w->prob) {
      ensure_system(w->prob);
      HIPCHK(hipStreamSynchronize(w->ctx->stream));   // an assembly in flight may still read the old table
    }
    if (lim && first >= 0) w->jtravel.assign(lim, lim + 2 * mj);
    else w->jtravel.clear();
    if (w->prob) world_fill_travel(w);
    return EGS_OK;
  });
}

egs_status egs_world_get_bodies(egs_world *w, double *pos, double *R, double *v, double *wv) {
  if (!w || !w->prob) return EGS_ERR_INVALID;
  return egs_problem_get_state(w->prob, pos, R, v, wv);
}

egs_status egs_world_get_contacts(egs_world *w, int32_t max_contacts, int32_t *m_out, int32_t *body0, int32_t *body1,
                                  double *data) {
  if (!w || !m_out) return EGS_ERR_INVALID;
  *m_out = w->m_contacts;
  if (w->m_contacts > max_contacts) return fail(w->ctx, EGS_ERR_INVALID, "max_contacts too small");
  return guarded(w->ctx, [&]() -> egs_status {
    const size_t mc = (size_t)w->m_contacts;
    hipStream_t s = w->ctx->stream;
    if (mc && body0) HIPCHK(hipMemcpyAsync(body0, w->col.body0(), mc * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (mc && body1) HIPCHK(hipMemcpyAsync(body1, w->col.body1(), mc * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (mc && data) HIPCHK(hipMemcpyAsync(data, w->col.data(), mc * 7 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return EGS_OK;
  });
}

egs_status egs_world_get_lambda(egs_world *w, int32_t max_rows, int32_t *rows_out, double *lambda) {
  if (!w || !w->prob || !rows_out) return EGS_ERR_INVALID;
  *rows_out = 3 * w->prob->m;
  if (w->lambda_stale)
    return fail(w->ctx, EGS_ERR_INVALID, "no step lambda for the constraint list egs_world_stabilize left: step first");
  if (3 * w->prob->m > max_rows) return fail(w->ctx, EGS_ERR_INVALID, "max_rows too small");
  if (w->prob->m == 0) return EGS_OK;
  return egs_problem_get_lambda(w->prob, lambda);
}

egs_status egs_world_get_blocks(egs_world *w, double *J0, double *J1, uint8_t *is_eq, double *lo, double *hi, double *rhs,
                                double *err) {
  if (!w || !w->prob) return EGS_ERR_INVALID;
  if (w->prob->m == 0) return EGS_OK;
  if (!w->prob->have_blocks) return fail(w->ctx, EGS_ERR_INVALID, "no step has assembled the world's list yet");
  return egs_problem_get_blocks(w->prob, J0, J1, is_eq, lo, hi, rhs, err);
}

egs_status egs_world_set_friction(egs_world *w, int32_t n_ensembles, const double *mu) {
  if (!w) return EGS_ERR_INVALID;
  egs_status st = world_set_table(w, w->friction, n_ensembles, mu, "NULL friction table", [&]() -> egs_status {
    for (int e = 0; e < n_ensembles; ++e)
      if (mu[e] != mu[e]) return fail(w->ctx, EGS_ERR_INVALID, "NaN friction coefficient");
    return EGS_OK;
  });
  if (st != EGS_OK) return st;
  if (!w->friction.any && w->prob) w->prob->friction = false;
  return EGS_OK;
}

egs_status egs_world_set_restitution(egs_world *w, int32_t n_ensembles, const double *rest, double vth) {
  if (!w) return EGS_ERR_INVALID;
  egs_status st = world_set_table(w, w->restitution, n_ensembles, rest, "NULL restitution table", [&]() -> egs_status {
    if (!(vth >= 0) || std::isinf(vth)) return fail(w->ctx, EGS_ERR_INVALID, "the restitution threshold must be finite and >= 0");
    for (int e = 0; e < n_ensembles; ++e)
      if (rest[e] != rest[e] || std::isinf(rest[e])) return fail(w->ctx, EGS_ERR_INVALID, "NaN or infinite restitution coefficient");
    return EGS_OK;
  });
  if (st != EGS_OK) return st;
  w->rest_vth = vth;
  if (!w->restitution.any && w->prob) w->prob->restitution = false;
  return EGS_OK;
}

egs_status egs_world_batch_info(egs_world *w, int32_t n_ensembles, int32_t *joint_offset, int32_t *contact_offset,
                                int32_t *iterations, double *residual) {
  if (!w) return EGS_ERR_INVALID;
  if (egs_status st = world_check_ensembles(w, n_ensembles)) return st;
  const EnsembleLayout &L = w->ens;
  const size_t E = (size_t)L.n_ens;
  if (L.n_ens > 1) {
    if (joint_offset) std::copy(L.joint_off.begin(), L.joint_off.end(), joint_offset);
    return guarded(w->ctx, [&]() -> egs_status {
      if (contact_offset) {
        HIPCHK(hipMemcpyAsync(contact_offset, L.d_coff.p, (E + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, w->ctx->stream));
        HIPCHK(hipStreamSynchronize(w->ctx->stream));
      }
      if (iterations) std::copy(L.batch.h_ints.p, L.batch.h_ints.p + E, iterations);
      if (residual) std::copy(L.batch.h_res.p, L.batch.h_res.p + E, residual);
      return EGS_OK;
    });
  }
  // one ensemble: the plain world's own figures
  if (joint_offset) { joint_offset[0] = 0; joint_offset[1] = (int32_t)w->jb0.size(); }
  if (contact_offset) { contact_offset[0] = 0; contact_offset[1] = w->m_contacts; }
  if (!iterations && !residual) return EGS_OK;
  egs_solve_stats st{};
  const bool dense = w->dense.was_last;
  if (w->prob && !dense) {
    if (egs_status r = egs_problem_get_stats(w->prob, &st)) return r;
  }
  if (iterations) iterations[0] = dense ? w->dense.info[0].pivots : st.iterations;
  if (residual) residual[0] = dense ? std::numeric_limits<double>::quiet_NaN() : st.residual;
  return EGS_OK;
}

egs_status egs_world_info(egs_world *w, int32_t *n_constraints, int32_t *n_contacts, int32_t *replans) {
  if (!w) return EGS_ERR_INVALID;
  if (n_constraints) *n_constraints = w->prob ? w->prob->m : 0;
  if (n_contacts) *n_contacts = w->m_contacts;
  if (replans) *replans = w->replans;
  return EGS_OK;
}

}  // extern "C"
