// rays.cpp -- the ray entries of the C ABI: egs_cast_rays (stateless, host arrays, one ensemble) and the world's
// egs_world_set_rays / egs_world_cast_rays (a table kept on the device, cast against the state the device holds).  Both
// go through the one kernel of raycast.hip.  Casting reads the world's pos / R / side / shape and writes only the ray
// table's own output buffer: nothing a step reads.
#include <cmath>

#include "world.h"

using namespace egs;

namespace {

// What is wrong with the rays themselves (nothing: NULL): a non-finite origin or direction, a zero direction, a negative
// or NaN tmax (+inf is a ray without an end).
const char *rays_fault(int n_rays, const double *origin, const double *dir, const double *tmax) {
  for (size_t i = 0; i < (size_t)n_rays; ++i) {
    const double *o = origin + 3 * i, *d = dir + 3 * i;
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(o[k]) || !std::isfinite(d[k])) return "a ray's origin and direction must be finite";
    if (d[0] == 0 && d[1] == 0 && d[2] == 0) return "a ray's direction must not be zero";
    if (!(tmax[i] >= 0)) return "a ray's tmax must be >= 0 (+inf allowed)";
  }
  return nullptr;
}

// t [n] | normal [n][3] | hit [n]: the layout of a cast's output block
size_t out_bytes(size_t n) { return n * (4 * sizeof(double) + sizeof(int32_t)); }
double *out_t(unsigned char *p) { return reinterpret_cast<double *>(p); }
double *out_normal(unsigned char *p, size_t n) { return reinterpret_cast<double *>(p) + n; }
int32_t *out_hit(unsigned char *p, size_t n) { return reinterpret_cast<int32_t *>(p + n * 4 * sizeof(double)); }

void copy_out(unsigned char *h, size_t n, int32_t *hit_body, double *t, double *normal) {
  std::memcpy(t, out_t(h), n * sizeof(double));
  if (normal) std::memcpy(normal, out_normal(h, n), 3 * n * sizeof(double));
  std::memcpy(hit_body, out_hit(h, n), n * sizeof(int32_t));
}

}  // namespace

extern "C" {

egs_status egs_cast_rays(egs_context *ctx, int32_t n_bodies, const double *pos, const double *R, const double *side_lengths,
                         const int32_t *shape, int32_t n_rays, const int32_t *ray_body, const double *origin,
                         const double *dir, const double *tmax, int32_t *hit_body, double *t, double *normal) {
  if (!ctx) return EGS_ERR_INVALID;
  if (n_bodies < 0 || n_rays < 0 || (n_bodies > 0 && (!pos || !R || !side_lengths)))
    return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (shape) {
    const std::string fault = shapes_fault(n_bodies, shape, side_lengths);
    if (!fault.empty()) return fail(ctx, EGS_ERR_INVALID, fault);
  }
  if (n_rays == 0) return EGS_OK;
  if (!origin || !dir || !tmax || !hit_body || !t) return fail(ctx, EGS_ERR_INVALID, "NULL array");
  if (const char *fault = rays_fault(n_rays, origin, dir, tmax)) return fail(ctx, EGS_ERR_INVALID, fault);
  for (int i = 0; ray_body && i < n_rays; ++i)
    if (ray_body[i] < -1 || ray_body[i] >= n_bodies) return fail(ctx, EGS_ERR_INVALID, "ray_body out of range");
  return guarded(ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nb = (size_t)n_bodies, nr = (size_t)n_rays;
    // one block of doubles and one of ints up, one block down
    std::vector<double> hd(15 * nb + 7 * nr);
    if (nb) {
      std::memcpy(hd.data(), pos, 3 * nb * sizeof(double));
      std::memcpy(hd.data() + 3 * nb, R, 9 * nb * sizeof(double));
      std::memcpy(hd.data() + 12 * nb, side_lengths, 3 * nb * sizeof(double));
    }
    double *rays = hd.data() + 15 * nb;
    std::memcpy(rays, origin, 3 * nr * sizeof(double));
    std::memcpy(rays + 3 * nr, dir, 3 * nr * sizeof(double));
    std::memcpy(rays + 6 * nr, tmax, nr * sizeof(double));
    std::vector<int32_t> hi;
    if (shape) hi.insert(hi.end(), shape, shape + nb);
    if (ray_body) hi.insert(hi.end(), ray_body, ray_body + nr);
    ScopedDevBuf<double> dd(hd.size());
    ScopedDevBuf<int32_t> di(hi.size());
    ScopedDevBuf<unsigned char> dout(out_bytes(nr));
    HIPCHK(hipMemcpyAsync(dd.p, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice, s));
    if (!hi.empty()) HIPCHK(hipMemcpyAsync(di.p, hi.data(), hi.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int32_t *dshape = shape ? di.p : nullptr;
    const int32_t *dbody = ray_body ? di.p + (shape ? nb : 0) : nullptr;
    const double *drays = dd.p + 15 * nb;
    cast_rays_device(s, n_bodies, dd.p, dd.p + 3 * nb, dd.p + 12 * nb, dshape, n_rays, nullptr, nullptr, 1, dbody, drays,
                     drays + 3 * nr, drays + 6 * nr, out_hit(dout.p, nr), out_t(dout.p), out_normal(dout.p, nr));
    std::vector<unsigned char> ho(out_bytes(nr));
    HIPCHK(hipMemcpyAsync(ho.data(), dout.p, ho.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    copy_out(ho.data(), nr, hit_body, t, normal);
    return EGS_OK;
  });
}

egs_status egs_world_set_rays(egs_world *w, int32_t n_rays, const int32_t *ray_ens, const int32_t *ray_body,
                              const double *origin, const double *dir, const double *tmax) {
  if (!w) return EGS_ERR_INVALID;
  if (n_rays < 0) return fail(w->ctx, EGS_ERR_INVALID, "negative ray count");
  RayTable &T = w->rays;
  if (n_rays == 0) { T.n = 0; return EGS_OK; }
  const EnsembleLayout &L = w->ens;
  if (!origin || !dir || !tmax || (L.n_ens > 1 && !ray_ens)) return fail(w->ctx, EGS_ERR_INVALID, "NULL array");
  if (const char *fault = rays_fault(n_rays, origin, dir, tmax)) return fail(w->ctx, EGS_ERR_INVALID, fault);
  bool attached = false;
  for (int i = 0; i < n_rays; ++i) {
    const int e = ray_ens ? ray_ens[i] : 0;
    if (e < 0 || e >= L.n_ens) return fail(w->ctx, EGS_ERR_INVALID, "ray_ens out of range");
    if (i > 0 && ray_ens && e < ray_ens[i - 1]) return fail(w->ctx, EGS_ERR_INVALID, "ray_ens must be non-decreasing");
    const int b = ray_body ? ray_body[i] : -1;
    if (b == -1) continue;
    const int lo = L.n_ens > 1 ? L.body_off[(size_t)e] : 0, hi = L.n_ens > 1 ? L.body_off[(size_t)e + 1] : w->n;
    if (b < lo || b >= hi) return fail(w->ctx, EGS_ERR_INVALID, "ray_body out of range or outside the ray's ensemble");
    attached = true;
  }
  return guarded(w->ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(w->ctx->device));
    hipStream_t s = w->ctx->stream;
    const size_t nr = (size_t)n_rays;
    const bool grouped = L.n_ens > 1;
    // every buffer first, so that a failed allocation leaves the old table whole
    T.geom.alloc(7 * nr);
    T.out.alloc(out_bytes(nr));
    T.h.alloc(out_bytes(nr));
    if (grouped) T.ens.alloc(nr);
    if (attached) T.body.alloc(nr);
    T.n = 0;
    std::vector<double> g(7 * nr);
    std::memcpy(g.data(), origin, 3 * nr * sizeof(double));
    std::memcpy(g.data() + 3 * nr, dir, 3 * nr * sizeof(double));
    std::memcpy(g.data() + 6 * nr, tmax, nr * sizeof(double));
    upload(T.geom, g.data(), g.size(), s);
    if (grouped) upload(T.ens, ray_ens, nr, s);
    if (attached) upload(T.body, ray_body, nr, s);
    T.grouped = grouped; T.attached = attached;
    T.n = n_rays;
    return EGS_OK;
  });
}

egs_status egs_world_cast_rays(egs_world *w, int32_t max_rays, int32_t *n_out, int32_t *hit_body, double *t, double *normal) {
  if (!w) return EGS_ERR_INVALID;
  RayTable &T = w->rays;
  if (n_out) *n_out = T.n;
  if (T.n == 0) return fail(w->ctx, EGS_ERR_INVALID, "no ray table: egs_world_set_rays first");
  if (!w->have_bodies || !w->prob) return fail(w->ctx, EGS_ERR_INVALID, "egs_world_set_bodies first");
  if (max_rays < T.n) return fail(w->ctx, EGS_ERR_INVALID, "max_rays too small");
  if (!hit_body || !t) return fail(w->ctx, EGS_ERR_INVALID, "NULL array");
  return guarded(w->ctx, [&]() -> egs_status {
    HIPCHK(hipSetDevice(w->ctx->device));
    hipStream_t s = w->ctx->stream;
    const size_t nr = (size_t)T.n;
    const double *g = T.geom.p;
    cast_rays_device(s, w->n, w->prob->pos.p, w->prob->R.p, w->dside.p, w->shapes ? w->dshape.p : nullptr, T.n,
                     T.grouped ? T.ens.p : nullptr, T.grouped ? w->ens.d_boff.p : nullptr, w->ens.n_ens, T.attached ? T.body.p : nullptr, g,
                     g + 3 * nr, g + 6 * nr, out_hit(T.out.p, nr), out_t(T.out.p), out_normal(T.out.p, nr));
    HIPCHK(hipMemcpyAsync(T.h.p, T.out.p, out_bytes(nr), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    copy_out(T.h.p, nr, hit_body, t, normal);
    return EGS_OK;
  });
}

}  // extern "C"
