// raycast.hip -- ray casts against the ground and the three shapes, one ray per lane.
//
// The rules are stated above egs_cast_rays in eggshell_amd.h; the arithmetic below is restated line for line in
// tests/ray_twin.py (fp64, -ffp-contract=off, one rounding per operation, IEEE sqrt and /), so the device's hit, t and
// normal are that twin's bits.  They share conventions with collide.hip, not code.
//
// Form.  256-thread workgroups, one ray per lane.  Rays arrive grouped by non-decreasing ensemble, so a workgroup's
// rays belong to the ensembles [ens(first ray), ens(last ray)] and it walks that stretch of bodies in chunks of
// kRayChunk.  A chunk is staged into LDS as 18-double records (pos, R, side, bounding radius^2, shape; 144 bytes, so a
// record starts 16-byte aligned) by the first kRayChunk threads, then every lane scans the staged bodies of its own
// ensemble in ascending index order: the lanes of a wavefront read the same record, which the LDS broadcasts.  The
// running best is replaced only by a strictly smaller t, and the ground is tested first, so "minimum, ties to the
// ground and then to the lowest index" needs no second pass.
//
// Cull.  Before the exact test a body is skipped if the ray's line misses its bounding sphere, or the sphere lies
// behind the origin.  Both are decided against radius^2 (1 + 1e-6) + 1e-20 |o - c|^2: the first term covers the
// rounding of the exact tests' own accept / reject decisions at the surface (relative 1e-15), the second the
// cancellation in the perpendicular offset for a far origin (its absolute error is a few ulp of |o - c|, squared and
// weighted by 1e6 to pair with the 1e-6: (a + b)^2 <= (1 + k) a^2 + (1 + 1 / k) b^2).  A skipped body could not have
// been hit or held the origin, so the cull never changes a result.  It is a launch choice (cast_rays_device): on where
// an ensemble holds more than a chunk of bodies, EGS_RAY_CULL=0 / 1 forces the form without / with it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "raycast.h"
#include "runtime.h"

namespace egs {
namespace {

constexpr int kRayThreads = 256;
constexpr int kRec = 18;   // doubles per staged body: pos 0-2, R 3-11, side 12-14, bound 15, shape 16, pad 17

struct RayArgs {
  int n_bodies, n_rays;
  const double *pos, *R, *side;
  const int32_t *shape;
  const int32_t *ray_ens, *body_off, *ray_body;
  const double *origin, *dir, *tmax;
  int32_t *hit;
  double *t, *normal;
};

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// the running result of one ray
struct Best {
  double t, n0, n1, n2;
  int body;   // -2: nothing yet
};

// a solid that holds the origin: t = 0, no normal
__device__ __forceinline__ void take_inside(Best &b, double tmax, int body) {
  if (b.body == -2 ? 0.0 <= tmax : 0.0 < b.t) { b.t = 0.0; b.n0 = 0.0; b.n1 = 0.0; b.n2 = 0.0; b.body = body; }
}

__device__ __forceinline__ bool wins(const Best &b, double tmax, double t) {
  return b.body == -2 ? t <= tmax : t < b.t;
}

// The entering root of |w + t d|^2 = r2 / scale (scale = d.d for a ball, the perpendicular d.d for a cylinder side) in
// the perpendicular-offset form, which does not cancel for a far origin: -1 where there is none or it is negative.
__device__ __forceinline__ double enter_root(double w0, double w1, double w2, double d0, double d1, double d2, double dd,
                                             double r2) {
  const double s = dot3(w0, w1, w2, d0, d1, d2) / dd;
  const double m0 = w0 - s * d0, m1 = w1 - s * d1, m2 = w2 - s * d2;
  const double disc = r2 - dot3(m0, m1, m2, m0, m1, m2);
  if (!(disc >= 0.0)) return -1.0;
  const double h = sqrt(disc / dd);
  const double t = -s - h;
  return t >= 0.0 ? t : -1.0;
}

// (w + t d) normalised
__device__ __forceinline__ void radial_normal(Best &b, double w0, double w1, double w2, double d0, double d1, double d2,
                                              double t) {
  const double q0 = w0 + t * d0, q1 = w1 + t * d1, q2 = w2 + t * d2;
  const double L = sqrt(dot3(q0, q1, q2, q0, q1, q2));
  b.n0 = q0 / L; b.n1 = q1 / L; b.n2 = q2 / L;
}

__device__ __forceinline__ void test_sphere(Best &b, const double *rec, int body, double o0, double o1, double o2, double d0,
                                            double d1, double d2, double dd, double tmax) {
  const double w0 = o0 - rec[0], w1 = o1 - rec[1], w2 = o2 - rec[2];
  const double r = rec[12] * 0.5;
  const double r2 = r * r;
  if (dot3(w0, w1, w2, w0, w1, w2) < r2) { take_inside(b, tmax, body); return; }
  const double t = enter_root(w0, w1, w2, d0, d1, d2, dd, r2);
  if (t >= 0.0 && wins(b, tmax, t)) {
    b.t = t; b.body = body;
    radial_normal(b, w0, w1, w2, d0, d1, d2, t);
  }
}

__device__ __forceinline__ void test_box(Best &b, const double *rec, int body, double o0, double o1, double o2, double d0,
                                         double d1, double d2, double tmax) {
  const double w0 = o0 - rec[0], w1 = o1 - rec[1], w2 = o2 - rec[2];
  double tin = -INFINITY, tout = INFINITY;
  int kin = 0;
  bool sign_in = false, miss = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double p = (rec[3 + k] * w0 + rec[6 + k] * w1) + rec[9 + k] * w2;
    const double q = (rec[3 + k] * d0 + rec[6 + k] * d1) + rec[9 + k] * d2;
    const double h = rec[12 + k] * 0.5;
    if (q == 0.0) {
      if (fabs(p) > h) miss = true;
    } else {
      const double ta = (-h - p) / q, tb = (h - p) / q;
      const double tn = fmin(ta, tb), tf = fmax(ta, tb);
      if (tn > tin) { tin = tn; kin = k; sign_in = q > 0.0; }
      if (tf < tout) tout = tf;
    }
  }
  if (miss || !(tin <= tout) || !(tout > 0.0)) return;
  if (tin < 0.0) { take_inside(b, tmax, body); return; }
  if (!wins(b, tmax, tin)) return;
  const double c0 = kin == 0 ? rec[3] : (kin == 1 ? rec[4] : rec[5]);
  const double c1 = kin == 0 ? rec[6] : (kin == 1 ? rec[7] : rec[8]);
  const double c2 = kin == 0 ? rec[9] : (kin == 1 ? rec[10] : rec[11]);
  b.t = tin; b.body = body;
  b.n0 = sign_in ? -c0 : c0; b.n1 = sign_in ? -c1 : c1; b.n2 = sign_in ? -c2 : c2;
}

__device__ __forceinline__ void test_capsule(Best &b, const double *rec, int body, double o0, double o1, double o2, double d0,
                                             double d1, double d2, double dd, double tmax) {
  const double w0 = o0 - rec[0], w1 = o1 - rec[1], w2 = o2 - rec[2];
  const double u0 = rec[5], u1 = rec[8], u2 = rec[11];
  const double r = rec[12] * 0.5;
  const double e = (rec[14] - rec[12]) * 0.5;
  const double r2 = r * r;
  const double wu = dot3(w0, w1, w2, u0, u1, u2);
  {   // the origin against the segment, by the collider's clamp
    const double s = fmin(fmax(wu, -e), e);
    const double v0 = w0 - s * u0, v1 = w1 - s * u1, v2 = w2 - s * u2;
    if (dot3(v0, v1, v2, v0, v1, v2) < r2) { take_inside(b, tmax, body); return; }
  }
  // the side, in the components perpendicular to u
  const double du = dot3(d0, d1, d2, u0, u1, u2);
  const double wp0 = w0 - wu * u0, wp1 = w1 - wu * u1, wp2 = w2 - wu * u2;
  const double dp0 = d0 - du * u0, dp1 = d1 - du * u1, dp2 = d2 - du * u2;
  const double a = dot3(dp0, dp1, dp2, dp0, dp1, dp2);
  double t = -1.0;
  int part = 0;
  if (a != 0.0) {
    const double ts = enter_root(wp0, wp1, wp2, dp0, dp1, dp2, a, r2);
    if (ts >= 0.0) {
      const double ax = wu + ts * du;
      if (ax >= -e && ax <= e) t = ts;
    }
  }
  // the balls at end 0 and end 1, centred at c -+ e u
  const double ne = -e;
  const double a0 = o0 - (rec[0] + ne * u0), a1 = o1 - (rec[1] + ne * u1), a2 = o2 - (rec[2] + ne * u2);
  const double t0 = enter_root(a0, a1, a2, d0, d1, d2, dd, r2);
  if (t0 >= 0.0 && (t < 0.0 || t0 < t)) { t = t0; part = 1; }
  const double b0 = o0 - (rec[0] + e * u0), b1 = o1 - (rec[1] + e * u1), b2 = o2 - (rec[2] + e * u2);
  const double t1 = enter_root(b0, b1, b2, d0, d1, d2, dd, r2);
  if (t1 >= 0.0 && (t < 0.0 || t1 < t)) { t = t1; part = 2; }
  if (!(t >= 0.0) || !wins(b, tmax, t)) return;
  b.t = t; b.body = body;
  if (part == 0) radial_normal(b, wp0, wp1, wp2, dp0, dp1, dp2, t);
  else if (part == 1) radial_normal(b, a0, a1, a2, d0, d1, d2, t);
  else radial_normal(b, b0, b1, b2, d0, d1, d2, t);
}

template <bool CULL>
__global__ __launch_bounds__(kRayThreads) void raycast_kernel(RayArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[kRayChunk * kRec];
  const int tid = (int)threadIdx.x;
  const int first = (int)blockIdx.x * kRayThreads;
  const int i = first + tid;
  const bool live = i < a.n_rays;
  // the bodies this workgroup walks: those of the ensembles of its first and last ray, and of all between
  int lo = 0, hi = a.n_bodies;
  if (a.ray_ens) {
    const int last = min(first + kRayThreads, a.n_rays) - 1;
    lo = a.body_off[a.ray_ens[first]];
    hi = a.body_off[a.ray_ens[last] + 1];
  }
  int mylo = 0, myhi = 0, skip = -1;
  double o0 = 0, o1 = 0, o2 = 0, d0 = 0, d1 = 0, d2 = 1, tmax = 0;
  if (live) {
    mylo = a.ray_ens ? a.body_off[a.ray_ens[i]] : 0;
    myhi = a.ray_ens ? a.body_off[a.ray_ens[i] + 1] : a.n_bodies;
    o0 = a.origin[3 * (size_t)i]; o1 = a.origin[3 * (size_t)i + 1]; o2 = a.origin[3 * (size_t)i + 2];
    d0 = a.dir[3 * (size_t)i]; d1 = a.dir[3 * (size_t)i + 1]; d2 = a.dir[3 * (size_t)i + 2];
    tmax = a.tmax[i];
    skip = a.ray_body ? a.ray_body[i] : -1;
    if (skip >= 0) {   // the ray rides on body skip: o_w = c + R o, d_w = R d
      const double *c = a.pos + 3 * (size_t)skip, *R = a.R + 9 * (size_t)skip;
      const double x0 = c[0] + ((R[0] * o0 + R[1] * o1) + R[2] * o2);
      const double x1 = c[1] + ((R[3] * o0 + R[4] * o1) + R[5] * o2);
      const double x2 = c[2] + ((R[6] * o0 + R[7] * o1) + R[8] * o2);
      const double y0 = (R[0] * d0 + R[1] * d1) + R[2] * d2;
      const double y1 = (R[3] * d0 + R[4] * d1) + R[5] * d2;
      const double y2 = (R[6] * d0 + R[7] * d1) + R[8] * d2;
      o0 = x0; o1 = x1; o2 = x2; d0 = y0; d1 = y1; d2 = y2;
    }
  }
  const double dd = dot3(d0, d1, d2, d0, d1, d2);
  Best b{tmax, 0.0, 0.0, 0.0, -2};
  if (live) {   // the ground: the half space z < 0
    if (o2 < 0.0) take_inside(b, tmax, -1);
    else if (d2 < 0.0) {
      const double t = o2 / (-d2);
      if (wins(b, tmax, t)) { b.t = t; b.n0 = 0.0; b.n1 = 0.0; b.n2 = 1.0; b.body = -1; }
    }
  }
  for (int base = lo; base < hi; base += kRayChunk) {
    const int cnt = min(kRayChunk, hi - base);
    __syncthreads();   // every lane is done with the chunk before
    if (tid < cnt) {
      const size_t g = (size_t)(base + tid);
      double *rec = lds + tid * kRec;
#pragma unroll
      for (int k = 0; k < 3; ++k) rec[k] = a.pos[3 * g + k];
#pragma unroll
      for (int k = 0; k < 9; ++k) rec[3 + k] = a.R[9 * g + k];
      const double s0 = a.side[3 * g], s1 = a.side[3 * g + 1], s2 = a.side[3 * g + 2];
      rec[12] = s0; rec[13] = s1; rec[14] = s2;
      const int sh = a.shape ? a.shape[g] : EGS_SHAPE_BOX;
      // the bounding sphere about the centre: the box's half diagonal, the ball's r, the capsule's half length l / 2
      double bound;
      if (sh == EGS_SHAPE_BOX) bound = 0.25 * ((s0 * s0 + s1 * s1) + s2 * s2);
      else if (sh == EGS_SHAPE_SPHERE) bound = 0.25 * (s0 * s0);
      else bound = 0.25 * (s2 * s2);
      rec[15] = bound * (1.0 + 1e-6);
      rec[16] = (double)sh;
      rec[17] = 0.0;
    }
    __syncthreads();
    if (live) {
      const int jlo = max(base, mylo), jhi = min(base + cnt, myhi);
      for (int j = jlo; j < jhi; ++j) {
        if (j == skip) continue;
        const double *rec = lds + (j - base) * kRec;
        if (CULL) {
          const double w0 = o0 - rec[0], w1 = o1 - rec[1], w2 = o2 - rec[2];
          const double ww = dot3(w0, w1, w2, w0, w1, w2);
          const double wd = dot3(w0, w1, w2, d0, d1, d2);
          const double lim = rec[15] + 1e-20 * ww;
          const double s = wd / dd;
          const double m0 = w0 - s * d0, m1 = w1 - s * d1, m2 = w2 - s * d2;
          if (dot3(m0, m1, m2, m0, m1, m2) > lim) continue;   // the line passes the bounding sphere by
          if (wd > 0.0 && ww > lim) continue;                 // the bounding sphere is behind the origin
        }
        const int sh = (int)rec[16];
        if (sh == EGS_SHAPE_BOX) test_box(b, rec, j, o0, o1, o2, d0, d1, d2, tmax);
        else if (sh == EGS_SHAPE_SPHERE) test_sphere(b, rec, j, o0, o1, o2, d0, d1, d2, dd, tmax);
        else test_capsule(b, rec, j, o0, o1, o2, d0, d1, d2, dd, tmax);
      }
    }
  }
  if (live) {
    a.hit[i] = b.body;
    a.t[i] = b.t;
    if (a.normal) { a.normal[3 * (size_t)i] = b.n0; a.normal[3 * (size_t)i + 1] = b.n1; a.normal[3 * (size_t)i + 2] = b.n2; }
  }
}

}  // namespace

void cast_rays_device(hipStream_t s, int n_bodies, const double *pos, const double *R, const double *side,
                      const int32_t *shape, int n_rays, const int32_t *ray_ens, const int32_t *body_off, int n_ens,
                      const int32_t *ray_body, const double *origin, const double *dir, const double *tmax, int32_t *hit,
                      double *t, double *normal) {
  if (n_rays <= 0) return;
  const RayArgs a{n_bodies, n_rays, pos, R, side, shape, ray_ens, body_off, ray_body, origin, dir, tmax, hit, t, normal};
  const char *e = std::getenv("EGS_RAY_CULL");   // "0": every body of the ensemble takes the exact test; "1": the cull
  const bool cull = e ? std::atoi(e) != 0 : (long)n_bodies > (long)kRayChunk * (n_ens > 0 ? n_ens : 1);
  const dim3 grid((unsigned)((n_rays + kRayThreads - 1) / kRayThreads));
  if (cull) hipLaunchKernelGGL((raycast_kernel<true>), grid, dim3(kRayThreads), 0, s, a);
  else hipLaunchKernelGGL((raycast_kernel<false>), grid, dim3(kRayThreads), 0, s, a);
  HIPCHK(hipGetLastError());
}

}  // namespace egs
