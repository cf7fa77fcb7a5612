// collide.hip -- contact generation on the GPU: Ensemble::UpdateContacts
// (ensembles.cc:445-480) + the contact-vs-contact pruning of
// CheckAndCorrectEnsembleState (ensembles.cc:241-329), i.e. the step that feeds
// the constraint solve.
//
//   box-ground   collision.cc:408-436   (8 vertices, z < 0)
//   box-box      collision.cc:166-388   (15-axis SAT, face clipping, edge-edge)
//
// The contact LIST ORDER is part of the result (the solver sweeps in list
// order): all ground contacts by body, then body pairs i < j lexicographically,
// each pair's contacts in the order the reference emits them.  The GPU keeps it
// with counts + exclusive scans instead of push_back:
//   1. ground_count / cand_kernel     per body: ground contacts; candidate j > i
//      (bounding spheres overlap; ordered by wave ballot).  From 2048 bodies up
//      the candidates come from a hashed uniform grid instead of all pairs
//      (cand_grid_kernel; same sphere test, same ascending order)
//   2. flatten candidates (scan)      -> pair list in (i, j) order
//   3. narrow_kernel<false, .>        per pair: SAT + clipping, count kept contacts
//   4. scan, narrow_kernel<true, .> + ground emit  -> final arrays
// With a shape array (egs_shape per body) the same pipeline runs the SHAPES = 1 instantiations, which
// add sphere-ground, sphere-sphere and sphere-box beside the box code, or -- where the array holds a capsule --
// the SHAPES = 2 instantiations, which add the four capsule cases (collide.h has the geometry).
// Arithmetic follows oracle/collision.c operation by operation (fp64,
// -ffp-contract=off), so the contact set is bit-identical to the CPU oracle's.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "collide.h"
#include "runtime.h"

namespace egs {

namespace {

constexpr int KMAX = 64;      // candidate partners j > i per body
constexpr int MAXC = 16;      // contacts per pair before pruning

struct Box { double c[3]; double R[9]; double h[3]; };
struct V2 { double x, y; };

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *o) {
  double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}
__device__ __forceinline__ void mat3_vec(const double *A, const double *v, double *o) {
  double x = (A[0] * v[0] + A[1] * v[1]) + A[2] * v[2];
  double y = (A[3] * v[0] + A[4] * v[1]) + A[5] * v[2];
  double z = (A[6] * v[0] + A[7] * v[1]) + A[8] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}
__device__ __forceinline__ void mat3_mul(const double *A, const double *B, double *O) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) O[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void mat3_T(const double *A, double *O) {
  O[0] = A[0]; O[1] = A[3]; O[2] = A[6]; O[3] = A[1]; O[4] = A[4]; O[5] = A[7]; O[6] = A[2]; O[7] = A[5]; O[8] = A[8];
}
__device__ __forceinline__ void colv(const double *R, int j, double *o) { o[0] = R[j]; o[1] = R[3 + j]; o[2] = R[6 + j]; }
__device__ __forceinline__ double sgn(double a) { return (a >= 0) ? 1.0 : -1.0; }

// collision.cc:408-436; returns the count, optionally writes [<=8][7]
__device__ int ground_contacts(const double *c, const double *R, const double *side, double *out) {
  int n = 0;
  double c0[3], c1[3], c2[3];
  colv(R, 0, c0); colv(R, 1, c1); colv(R, 2, c2);
  for (int x = -1; x <= 1; x += 2)
    for (int y = -1; y <= 1; y += 2)
      for (int z = -1; z <= 1; z += 2) {
        double v[3];
        for (int k = 0; k < 3; ++k)
          v[k] = ((c[k] + c0[k] * side[0] * 0.5 * x) + c1[k] * side[1] * 0.5 * y) + c2[k] * side[2] * 0.5 * z;
        if (v[2] < 0) {
          if (out) {
            double *o = out + 7 * n;
            o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = 0; o[4] = 0; o[5] = 1; o[6] = -v[2];
          }
          ++n;
        }
      }
  return n;
}

__device__ void line_closest_approach(const double *pa, const double *ua, const double *pb, const double *ub,
                                      double *alpha, double *beta) {  // collision.cc:53-69
  double p[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
  double uaub = dot3(ua, ub), q1 = dot3(ua, p), q2 = -dot3(ub, p);
  double d = 1 - uaub * uaub;
  if (d == 0) { *alpha = 0; *beta = 0; }
  else { *alpha = (q1 + uaub * q2) / d; *beta = (uaub * q1 + q2) / d; }
}

__device__ int seg_line(V2 p1, V2 p2, V2 nrm, double d, V2 *p) {  // collision.cc:77-87
  double k1 = (nrm.x * p1.x + nrm.y * p1.y) + d;
  double k2 = (nrm.x * p2.x + nrm.y * p2.y) + d;
  if (k1 * k2 < 0) {
    double t = k1 / (k2 - k1);
    p->x = p1.x - t * (p2.x - p1.x);
    p->y = p1.y - t * (p2.y - p1.y);
    return 1;
  }
  return 0;
}

__device__ int clip_poly(const V2 *poly, int n, V2 nrm, double d, V2 *out) {  // collision.cc:91-106
  int k = 0;
  for (int i = 0; i < n; ++i) {
    if ((nrm.x * poly[i].x + nrm.y * poly[i].y) + d >= 0) out[k++] = poly[i];
    V2 np;
    if (seg_line(poly[i], poly[(i + 1) % n], nrm, d, &np)) out[k++] = np;
  }
  return k;
}

__device__ int box_rect(const Box *B, const Box *Rc, V2 *poly) {  // collision.cc:112-164
  const double kTol = 1e-9;
  double Bc[3] = {B->c[0] - Rc->c[0], B->c[1] - Rc->c[1], B->c[2] - Rc->c[2]};
  int n = 4;
  poly[0] = V2{-Rc->h[0], -Rc->h[1]};
  poly[1] = V2{-Rc->h[0], Rc->h[1]};
  poly[2] = V2{Rc->h[0], Rc->h[1]};
  poly[3] = V2{Rc->h[0], -Rc->h[1]};
  V2 tmp[24];
  double Rn[3], r0[3], r1[3];
  colv(Rc->R, 2, Rn); colv(Rc->R, 0, r0); colv(Rc->R, 1, r1);
  for (int i = 0; i < 3; ++i) {
    double Bn[3], cr[3];
    colv(B->R, i, Bn);
    double BnBc = dot3(Bn, Bc);
    cross3(Bn, Rn, cr);
    double crossn = sqrt(dot3(cr, cr));
    for (int j = -1; j <= 1; j += 2) {
      double Bd = -j * BnBc - B->h[i];
      if (crossn < kTol) {
        if (Bd <= 0) continue;
        return 0;
      }
      V2 H = {dot3(r0, Bn), dot3(r1, Bn)};
      V2 Hn = {-j * H.x, -j * H.y};
      int k = clip_poly(poly, n, Hn, -Bd, tmp);
      for (int q = 0; q < k; ++q) poly[q] = tmp[q];
      n = k;
      if (n == 0) return 0;
    }
  }
  return n;
}

// collision.cc:166-388.  contacts [<= MAXC][7]; returns the number generated.
__device__ int collide_boxes(const double *c1, const double *R1, const double *s1, const double *c2,
                             const double *R2, const double *s2, double *contacts) {
  const double kAlign = 0.9962, kTol = 1e-9;
  Box box1, box2;
  for (int k = 0; k < 3; ++k) { box1.c[k] = c1[k]; box2.c[k] = c2[k]; box1.h[k] = s1[k] * 0.5; box2.h[k] = s2[k] * 0.5; }
  for (int k = 0; k < 9; ++k) { box1.R[k] = R1[k]; box2.R[k] = R2[k]; }
  double R1t[9], R[9], Q[9], p[3], dc[3];
  mat3_T(R1, R1t);
  mat3_mul(R1t, R2, R);
  for (int k = 0; k < 3; ++k) dc[k] = c2[k] - c1[k];
  mat3_vec(R1t, dc, p);
  for (int k = 0; k < 9; ++k) Q[k] = fabs(R[k]);
  int aacount = 0;
  for (int j = 0; j < 3; ++j) {
    double mx = Q[j];
    if (Q[3 + j] > mx) mx = Q[3 + j];
    if (Q[6 + j] > mx) mx = Q[6 + j];
    aacount += (mx > kAlign);
  }
  const double *H1 = box1.h, *H2 = box2.h;
  double min_FN = -DBL_MAX, sep_FN[3] = {0, 0, 0};
  int code_FN = 0;
#define RR(i, j) R[3 * (i) + (j)]
#define QQ(i, j) Q[3 * (i) + (j)]
#define SEPF(e1expr, e2expr, Rsrc, col, thecode)                                  \
  {                                                                               \
    double e1 = (e1expr);                                                         \
    double separation = fabs(e1) - (e2expr);                                      \
    if (separation > 0) return 0;                                                 \
    if (separation > min_FN) {                                                    \
      min_FN = separation;                                                        \
      double nn[3]; colv(Rsrc, col, nn);                                          \
      double sg = sgn(e1);                                                        \
      sep_FN[0] = sg * nn[0]; sep_FN[1] = sg * nn[1]; sep_FN[2] = sg * nn[2];      \
      code_FN = (thecode);                                                        \
    }                                                                             \
  }
  SEPF(p[0], H1[0] + ((H2[0] * QQ(0, 0) + H2[1] * QQ(0, 1)) + H2[2] * QQ(0, 2)), R1, 0, 1)
  SEPF(p[1], H1[1] + ((H2[0] * QQ(1, 0) + H2[1] * QQ(1, 1)) + H2[2] * QQ(1, 2)), R1, 1, 2)
  SEPF(p[2], H1[2] + ((H2[0] * QQ(2, 0) + H2[1] * QQ(2, 1)) + H2[2] * QQ(2, 2)), R1, 2, 3)
  SEPF((RR(0, 0) * p[0] + RR(1, 0) * p[1]) + RR(2, 0) * p[2], ((H1[0] * QQ(0, 0) + H1[1] * QQ(1, 0)) + H1[2] * QQ(2, 0)) + H2[0], R2, 0, 4)
  SEPF((RR(0, 1) * p[0] + RR(1, 1) * p[1]) + RR(2, 1) * p[2], ((H1[0] * QQ(0, 1) + H1[1] * QQ(1, 1)) + H1[2] * QQ(2, 1)) + H2[1], R2, 1, 5)
  SEPF((RR(0, 2) * p[0] + RR(1, 2) * p[1]) + RR(2, 2) * p[2], ((H1[0] * QQ(0, 2) + H1[1] * QQ(1, 2)) + H1[2] * QQ(2, 2)) + H2[2], R2, 2, 6)
#undef SEPF
  double min_EE = -DBL_MAX, sep_EE[3] = {0, 0, 0};
  int code_EE = 0;
#define SEPE(e1expr, e2expr, n0, n1, n2, thecode)                                 \
  {                                                                               \
    double nv[3] = {(n0), (n1), (n2)};                                            \
    double len = sqrt(dot3(nv, nv));                                              \
    if (len > kTol) {                                                             \
      double e1 = (e1expr);                                                       \
      double separation = fabs(e1) - (e2expr);                                    \
      if (separation > 0) return 0;                                               \
      separation /= len;                                                          \
      if (separation > min_EE) {                                                  \
        min_EE = separation;                                                      \
        double dn = sgn(e1) * len;                                                \
        sep_EE[0] = nv[0] / dn; sep_EE[1] = nv[1] / dn; sep_EE[2] = nv[2] / dn;    \
        code_EE = (thecode);                                                      \
      }                                                                           \
    }                                                                             \
  }
  SEPE(p[2] * RR(1, 0) - p[1] * RR(2, 0), (H1[1] * QQ(2, 0) + H1[2] * QQ(1, 0) + H2[1] * QQ(0, 2) + H2[2] * QQ(0, 1)), 0, -RR(2, 0), RR(1, 0), 7)
  SEPE(p[2] * RR(1, 1) - p[1] * RR(2, 1), (H1[1] * QQ(2, 1) + H1[2] * QQ(1, 1) + H2[0] * QQ(0, 2) + H2[2] * QQ(0, 0)), 0, -RR(2, 1), RR(1, 1), 8)
  SEPE(p[2] * RR(1, 2) - p[1] * RR(2, 2), (H1[1] * QQ(2, 2) + H1[2] * QQ(1, 2) + H2[0] * QQ(0, 1) + H2[1] * QQ(0, 0)), 0, -RR(2, 2), RR(1, 2), 9)
  SEPE(p[0] * RR(2, 0) - p[2] * RR(0, 0), (H1[0] * QQ(2, 0) + H1[2] * QQ(0, 0) + H2[1] * QQ(1, 2) + H2[2] * QQ(1, 1)), RR(2, 0), 0, -RR(0, 0), 10)
  SEPE(p[0] * RR(2, 1) - p[2] * RR(0, 1), (H1[0] * QQ(2, 1) + H1[2] * QQ(0, 1) + H2[0] * QQ(1, 2) + H2[2] * QQ(1, 0)), RR(2, 1), 0, -RR(0, 1), 11)
  SEPE(p[0] * RR(2, 2) - p[2] * RR(0, 2), (H1[0] * QQ(2, 2) + H1[2] * QQ(0, 2) + H2[0] * QQ(1, 1) + H2[1] * QQ(1, 0)), RR(2, 2), 0, -RR(0, 2), 12)
  SEPE(p[1] * RR(0, 0) - p[0] * RR(1, 0), (H1[0] * QQ(1, 0) + H1[1] * QQ(0, 0) + H2[1] * QQ(2, 2) + H2[2] * QQ(2, 1)), -RR(1, 0), RR(0, 0), 0, 13)
  SEPE(p[1] * RR(0, 1) - p[0] * RR(1, 1), (H1[0] * QQ(1, 1) + H1[1] * QQ(0, 1) + H2[0] * QQ(2, 2) + H2[2] * QQ(2, 0)), -RR(1, 1), RR(0, 1), 0, 14)
  SEPE(p[1] * RR(0, 2) - p[0] * RR(1, 2), (H1[0] * QQ(1, 2) + H1[1] * QQ(0, 2) + H2[0] * QQ(2, 1) + H2[1] * QQ(2, 0)), -RR(1, 2), RR(0, 2), 0, 15)
#undef SEPE
#undef RR
#undef QQ
  {
    double t[3];
    mat3_vec(R1, sep_EE, t);
    sep_EE[0] = t[0]; sep_EE[1] = t[1]; sep_EE[2] = t[2];
  }
  const int best_FN = (code_EE == 0) ? 1 : (min_FN > min_EE);
  int n = 0;
  if (aacount == 0 && !best_FN) {  // edge-edge, collision.cc:278-301
    double pa[3], pb[3];
    for (int k = 0; k < 3; ++k) { pa[k] = c1[k]; pb[k] = c2[k]; }
    for (int j = 0; j < 3; ++j) {
      double a1[3], a2[3];
      colv(R1, j, a1); colv(R2, j, a2);
      double sa = sgn(dot3(sep_EE, a1)), sb = sgn(dot3(sep_EE, a2));
      for (int k = 0; k < 3; ++k) { pa[k] += sa * H1[j] * a1[k]; pb[k] -= sb * H2[j] * a2[k]; }
    }
    double ua[3], ub[3], alpha, beta;
    colv(R1, (code_EE - 7) / 3, ua);
    colv(R2, (code_EE - 7) % 3, ub);
    line_closest_approach(pa, ua, pb, ub, &alpha, &beta);
    for (int k = 0; k < 3; ++k) {
      contacts[k] = (pa[k] + ua[k] * alpha + pb[k] + ub[k] * beta) * 0.5;
      contacts[3 + k] = sep_EE[k];
    }
    contacts[6] = -min_EE;
    return 1;
  }
  const Box *A = (code_FN <= 3) ? &box1 : &box2;
  Box B = (code_FN <= 3) ? box2 : box1;
  const double sgnA = (code_FN <= 3) ? 1.0 : -1.0;
  double An[3] = {sep_FN[0] * sgnA, sep_FN[1] * sgnA, sep_FN[2] * sgnA};
  double BRt[9], nf[3];
  mat3_T(B.R, BRt);
  mat3_vec(BRt, An, nf);
  int nfi = 0;
  {
    double best = fabs(nf[0]);
    if (fabs(nf[1]) > best) { best = fabs(nf[1]); nfi = 1; }
    if (fabs(nf[2]) > best) { best = fabs(nf[2]); nfi = 2; }
  }
  double Bn[3], bcol[3];
  colv(B.R, nfi, bcol);
  for (int k = 0; k < 3; ++k) Bn[k] = -sgn(nf[nfi]) * bcol[k];
  {
    double BR[9], a0[3], a1[3], a2[3];
    for (int k = 0; k < 3; ++k) B.c[k] += Bn[k] * B.h[nfi];
    colv(B.R, (nfi + 1) % 3, a0); colv(B.R, (nfi + 2) % 3, a1); colv(B.R, nfi, a2);
    for (int k = 0; k < 3; ++k) { BR[3 * k] = a0[k]; BR[3 * k + 1] = a1[k]; BR[3 * k + 2] = a2[k]; }
    const double h0 = B.h[(nfi + 1) % 3], h1 = B.h[(nfi + 2) % 3];
    for (int k = 0; k < 9; ++k) B.R[k] = BR[k];
    B.h[0] = h0; B.h[1] = h1; B.h[2] = 0;
  }
  double Afc[3];
  for (int k = 0; k < 3; ++k) Afc[k] = A->c[k] + An[k] * A->h[(code_FN - 1) % 3];
  const double Ad = -dot3(An, Afc);
  V2 poly[24];
  const int np = box_rect(A, &B, poly);
  double b0[3], b1[3];
  colv(B.R, 0, b0); colv(B.R, 1, b1);
  for (int i = 0; i < np && n < MAXC; ++i) {
    double pos[3];
    for (int k = 0; k < 3; ++k) pos[k] = (B.c[k] + b0[k] * poly[i].x) + b1[k] * poly[i].y;
    const double depth = -(dot3(An, pos) + Ad);
    if (fabs(depth) > kTol || aacount >= 2) {
      double *o = contacts + 7 * n++;
      for (int k = 0; k < 3; ++k) { o[k] = pos[k]; o[3 + k] = sep_FN[k]; }
      o[6] = depth;
    }
  }
  if (n == 0) {  // collision.cc:378-386
    for (int k = 0; k < 3; ++k) { contacts[k] = c2[k]; contacts[3 + k] = sep_FN[k]; }
    contacts[6] = -min_FN;
    n = 1;
  }
  return n;
}

// ---- spheres (collide.h states the geometry) ---------------------------------
// A sphere is a body whose side row is (d, d, d), r = d / 2; its R is not read.  Each function has ONE
// operation order, written out below: fp64, one rounding per operation, sqrt and / only where the
// definition has them.  tests/sphere_twin.py restates it in numpy and is matched bit for bit.
constexpr int kShapeSphere = 1;   // EGS_SHAPE_SPHERE; every other value takes the box code (the ABI admits only 0)

// r = side[0] * 0.5;  qz = c[2] - r;  contact iff qz < 0:  (c[0], c[1], qz), (0, 0, 1), -qz
__device__ int ground_sphere(const double *c, const double *side, double *out) {
  const double r = side[0] * 0.5;
  const double qz = c[2] - r;
  if (!(qz < 0)) return 0;
  if (out) { out[0] = c[0]; out[1] = c[1]; out[2] = qz; out[3] = 0; out[4] = 0; out[5] = 1; out[6] = -qz; }
  return 1;
}

// d = cj - ci;  L = sqrt((d0 d0 + d1 d1) + d2 d2);  s = L - (ri + rj);  contact iff s <= 0
// n = d / L ((0, 0, 1) when L == 0);  t = ((ri + L) - rj) * 0.5;  position = ci + n * t;  depth = -s
__device__ int collide_spheres(const double *ci, const double *si, const double *cj, const double *sj, double *out) {
  const double ri = si[0] * 0.5, rj = sj[0] * 0.5;
  const double d[3] = {cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]};
  const double L = sqrt(dot3(d, d));
  const double s = L - (ri + rj);
  if (s > 0) return 0;
  double n[3] = {0, 0, 1};
  if (L != 0) { n[0] = d[0] / L; n[1] = d[1] / L; n[2] = d[2] / L; }
  const double t = ((ri + L) - rj) * 0.5;
  for (int k = 0; k < 3; ++k) { out[k] = ci[k] + n[k] * t; out[3 + k] = n[k]; }
  out[6] = -s;
  return 1;
}

// Sphere S against box B; flip = the sphere is body0, so the reported normal is -n_BS.
//   r = sideS[0] * 0.5;  dc = cS - cB;  p_k = (R[k] dc0 + R[3 + k] dc1) + R[6 + k] dc2  (R^T dc)
//   h_k = sideB[k] * 0.5;  q_k = min(max(p_k, -h_k), h_k);  e = p - q;  L = sqrt((e0 e0 + e1 e1) + e2 e2)
//   L > 0 (centre outside; an e too small for its squares to be normal numbers counts as inside):
//     contact iff L - r <= 0;  n = (R e) / L;  depth = r - L
//   L == 0 (centre inside or on the surface):
//     g_k = h_k - |p_k|;  k = argmin g (lowest k on a tie);  sg = sgn(p_k);  n = sg * column k of R
//     depth = g_k + r;  q_k = sg * h_k (the centre moved onto that face)
//   box point = R q + cB;  sphere point = cS - r * n;  position = (box point + sphere point) * 0.5
__device__ int collide_sphere_box(const double *cS, const double *sideS, const double *cB, const double *RB,
                                  const double *sideB, bool flip, double *out) {
  const double r = sideS[0] * 0.5;
  const double dc[3] = {cS[0] - cB[0], cS[1] - cB[1], cS[2] - cB[2]};
  double p[3], h[3], q[3], e[3], n[3], depth;
  for (int k = 0; k < 3; ++k) {
    p[k] = (RB[k] * dc[0] + RB[3 + k] * dc[1]) + RB[6 + k] * dc[2];
    h[k] = sideB[k] * 0.5;
    q[k] = fmin(fmax(p[k], -h[k]), h[k]);
    e[k] = p[k] - q[k];
  }
  const double L = sqrt(dot3(e, e));
  if (L > 0) {
    if (L - r > 0) return 0;
    double w[3];
    mat3_vec(RB, e, w);
    for (int k = 0; k < 3; ++k) n[k] = w[k] / L;
    depth = r - L;
  } else {
    const double g[3] = {h[0] - fabs(p[0]), h[1] - fabs(p[1]), h[2] - fabs(p[2])};
    int k = 0;
    if (g[1] < g[k]) k = 1;
    if (g[2] < g[k]) k = 2;
    const double sg = sgn(p[k]);
    double col[3];
    colv(RB, k, col);
    for (int a = 0; a < 3; ++a) n[a] = sg * col[a];
    depth = g[k] + r;
    q[k] = sg * h[k];
  }
  double bq[3];
  mat3_vec(RB, q, bq);
  const double fs = flip ? -1.0 : 1.0;
  for (int k = 0; k < 3; ++k) {
    const double boxpt = bq[k] + cB[k];
    const double sphpt = cS[k] - r * n[k];
    out[k] = (boxpt + sphpt) * 0.5;
    out[3 + k] = fs * n[k];
  }
  out[6] = depth;
  return 1;
}

// ---- capsules (collide.h states the geometry) ---------------------------------
// A capsule is a body whose side row is (d, d, l), l > d: r = side[0] * 0.5, e = (side[2] - side[0]) * 0.5, axis
// u = (R[2], R[5], R[8]); the ball at t is centred at c_k + t * u_k (one product, one sum).  Every contact is a sphere
// rule applied to such a ball, so the sphere functions above are called with the capsule's own side row (they read
// side[0] alone).  One operation order each, restated in numpy by tests/capsule_twin.py.
constexpr int kShapeCapsule = 2;   // EGS_SHAPE_CAPSULE
constexpr double kFlat = 1e-9;     // the flat rule: an interior candidate this close (centre distance) to an emitted end is dropped

struct Capsule { double e; double u[3]; };
__device__ __forceinline__ Capsule capsule_of(const double *R, const double *side) {
  return Capsule{(side[2] - side[0]) * 0.5, {R[2], R[5], R[8]}};
}
__device__ __forceinline__ void ball_at(const double *c, const double *u, double t, double *b) {
  b[0] = c[0] + t * u[0]; b[1] = c[1] + t * u[1]; b[2] = c[2] + t * u[2];
}

// collide_spheres with the centre distance L reported (written whether or not there is a contact)
__device__ int collide_balls(const double *ci, const double *si, const double *cj, const double *sj, double *out, double *Lout) {
  const double ri = si[0] * 0.5, rj = sj[0] * 0.5;
  const double d[3] = {cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]};
  const double L = sqrt(dot3(d, d));
  *Lout = L;
  const double s = L - (ri + rj);
  if (s > 0) return 0;
  double n[3] = {0, 0, 1};
  if (L != 0) { n[0] = d[0] / L; n[1] = d[1] / L; n[2] = d[2] / L; }
  const double t = ((ri + L) - rj) * 0.5;
  for (int k = 0; k < 3; ++k) { out[k] = ci[k] + n[k] * t; out[3 + k] = n[k]; }
  out[6] = -s;
  return 1;
}

// ground_sphere on the ball at -e, then on the ball at +e
__device__ int ground_capsule(const double *c, const double *R, const double *side, double *out) {
  const Capsule C = capsule_of(R, side);
  double b[3];
  ball_at(c, C.u, -C.e, b);
  int n = ground_sphere(b, side, out);
  ball_at(c, C.u, C.e, b);
  n += ground_sphere(b, side, out ? out + 7 * n : nullptr);
  return n;
}

// t = min(max(dot3(cS - cC, u), -e), e): the parameter of the capsule's ball nearest the point cS
__device__ __forceinline__ double capsule_nearest(const double *cC, const Capsule &C, const double *cS) {
  const double w[3] = {cS[0] - cC[0], cS[1] - cC[1], cS[2] - cC[2]};
  return fmin(fmax(dot3(w, C.u), -C.e), C.e);
}

// The capsule's ball nearest the sphere's centre against the sphere, in the pair's order (first = the capsule is body0).
__device__ int collide_capsule_sphere(const double *cC, const double *RC, const double *sideC, const double *cS,
                                      const double *sideS, bool first, double *out) {
  const Capsule C = capsule_of(RC, sideC);
  double b[3];
  ball_at(cC, C.u, capsule_nearest(cC, C, cS), b);
  return first ? collide_spheres(b, sideC, cS, sideS, out) : collide_spheres(cS, sideS, b, sideC, out);
}

// Capsules i < j.  Candidates in order: end 0 of i, end 1 of i (each against j's nearest ball), end 0 of j, end 1 of j
// (each against i's nearest ball), then the interior pair:
//   w = cj - ci;  A = ui.ui;  B = uj.uj;  a = ui.uj;  p = ui.w;  q = uj.w;  det = A * B - a * a
//   s = (p * B - a * q) / det;  t = (a * p - A * q) / det;  exists iff det != 0, -ei < s < ei and -ej < t < ej
// (two capsules with the same R bits have A = B = a, det = 0 exactly).  The interior pair is dropped if an emitted end
// candidate's centre distance L is within kFlat of its own.  Every candidate is collide_balls(ball of i, ball of j).
__device__ int collide_capsules(const double *ci, const double *Ri, const double *si, const double *cj, const double *Rj,
                                const double *sj, double *out) {
  const Capsule Ci = capsule_of(Ri, si), Cj = capsule_of(Rj, sj);
  int n = 0;
  double Lend[4], L, bi[3], bj[3];
  bool hit[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double te = (q & 1) ? 1.0 : -1.0;
    if (q < 2) { ball_at(ci, Ci.u, te * Ci.e, bi); ball_at(cj, Cj.u, capsule_nearest(cj, Cj, bi), bj); }
    else       { ball_at(cj, Cj.u, te * Cj.e, bj); ball_at(ci, Ci.u, capsule_nearest(ci, Ci, bj), bi); }
    const int c = collide_balls(bi, si, bj, sj, out + 7 * n, &L);
    hit[q] = c != 0; Lend[q] = L;
    n += c;
  }
  const double w[3] = {cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]};
  const double A = dot3(Ci.u, Ci.u), B = dot3(Cj.u, Cj.u), a = dot3(Ci.u, Cj.u), p = dot3(Ci.u, w), q = dot3(Cj.u, w);
  const double det = A * B - a * a;
  if (det != 0) {
    const double s = (p * B - a * q) / det, t = (a * p - A * q) / det;
    if (s > -Ci.e && s < Ci.e && t > -Cj.e && t < Cj.e) {
      double row[7];
      ball_at(ci, Ci.u, s, bi); ball_at(cj, Cj.u, t, bj);
      const int c = collide_balls(bi, si, bj, sj, row, &L);
      bool flat = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) flat |= hit[k] && fabs(Lend[k] - L) <= kFlat;
      if (c && !flat) { for (int k = 0; k < 7; ++k) out[7 * n + k] = row[k]; ++n; }
    }
  }
  return n;
}

// dist(t)^2 of the capsule axis in the box frame: p_k = p0_k + t * ub_k;  q_k = min(max(p_k, -h_k), h_k);  e = p - q;  e.e
__device__ __forceinline__ double axis_dist2(const double *p0, const double *ub, const double *h, double t) {
  double e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double p = p0[k] + t * ub[k];
    e[k] = p - fmin(fmax(p, -h[k]), h[k]);
  }
  return dot3(e, e);
}

#define EGS_CSWAP(a, b) { const double lo_ = fmin(a, b), hi_ = fmax(a, b); a = lo_; b = hi_; }

// Capsule C against box B; flip = the capsule is body0.  Candidates: the ball at -e, the ball at +e, the ball at t*,
// each through collide_sphere_box.  In the box frame the axis is p0 + t ub:
//   dc = cC - cB;  p0_k = (R[k] dc0 + R[3 + k] dc1) + R[6 + k] dc2;  ub_k = (R[k] u0 + R[3 + k] u1) + R[6 + k] u2;  h_k = sideB[k] * 0.5
//   breakpoints x_{2k} = (-h_k - p0_k) / ub_k, x_{2k+1} = (h_k - p0_k) / ub_k  (ub_k == 0: both +inf)
//   clip: lo = max(-e, min(x_{2k}, x_{2k+1}) over k), hi = min(e, max(x_{2k}, x_{2k+1}) over k); a k with ub_k == 0 and
//   |p0_k| > h_k empties it.  lo <= hi (the axis enters the box): t* = (lo + hi) * 0.5.
//   Otherwise tau_0 = -e, tau_1..6 = the breakpoints clamped to [-e, e] and sorted (a fixed network), tau_7 = e; for
//   piece i = 0..6: m = (tau_i + tau_{i+1}) * 0.5, sg_k = +1 if p_k(m) > h_k, -1 if p_k(m) < -h_k, else 0 (inactive),
//   num = sum over active k of ub_k * (p0_k - sg_k h_k), den = sum over active k of ub_k * ub_k (k ascending, from 0),
//   s_i = min(max(-num / den, tau_i), tau_{i+1}) if den > 0.  t* = the candidate with the lowest axis_dist2 among
//   tau_0, s_0, tau_1, s_1, ..., s_6, tau_7 in this order, the first on a tie.
//   t* counts iff -e < t* < e;  D(t) = sqrt(axis_dist2(t));  the interior candidate is dropped if an emitted end's D is
//   within kFlat of D(t*).
__device__ int collide_capsule_box(const double *cC, const double *RC, const double *sideC, const double *cB,
                                   const double *RB, const double *sideB, bool flip, double *out) {
  const Capsule C = capsule_of(RC, sideC);
  const double dc[3] = {cC[0] - cB[0], cC[1] - cB[1], cC[2] - cB[2]};
  double p0[3], ub[3], h[3], x0, x1, x2, x3, x4, x5;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p0[k] = (RB[k] * dc[0] + RB[3 + k] * dc[1]) + RB[6 + k] * dc[2];
    ub[k] = (RB[k] * C.u[0] + RB[3 + k] * C.u[1]) + RB[6 + k] * C.u[2];
    h[k] = sideB[k] * 0.5;
  }
  double lo = -C.e, hi = C.e;
#define EGS_SLAB(k, xa, xb)                                                      \
  if (ub[k] != 0) {                                                              \
    xa = (-h[k] - p0[k]) / ub[k]; xb = (h[k] - p0[k]) / ub[k];                   \
    lo = fmax(lo, fmin(xa, xb)); hi = fmin(hi, fmax(xa, xb));                    \
  } else {                                                                       \
    xa = INFINITY; xb = INFINITY;                                                \
    if (fabs(p0[k]) > h[k]) hi = -INFINITY;                                      \
  }
  EGS_SLAB(0, x0, x1) EGS_SLAB(1, x2, x3) EGS_SLAB(2, x4, x5)
#undef EGS_SLAB
  double ts;
  if (lo <= hi) {
    ts = (lo + hi) * 0.5;
  } else {
    x0 = fmin(fmax(x0, -C.e), C.e); x1 = fmin(fmax(x1, -C.e), C.e); x2 = fmin(fmax(x2, -C.e), C.e);
    x3 = fmin(fmax(x3, -C.e), C.e); x4 = fmin(fmax(x4, -C.e), C.e); x5 = fmin(fmax(x5, -C.e), C.e);
    EGS_CSWAP(x0, x5) EGS_CSWAP(x1, x3) EGS_CSWAP(x2, x4)
    EGS_CSWAP(x1, x2) EGS_CSWAP(x3, x4)
    EGS_CSWAP(x0, x3) EGS_CSWAP(x2, x5)
    EGS_CSWAP(x0, x1) EGS_CSWAP(x2, x3) EGS_CSWAP(x4, x5)
    EGS_CSWAP(x1, x2) EGS_CSWAP(x3, x4)
    const double tau[8] = {-C.e, x0, x1, x2, x3, x4, x5, C.e};
    ts = tau[0];
    double best = axis_dist2(p0, ub, h, ts);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const double m = (tau[i] + tau[i + 1]) * 0.5;
      double num = 0, den = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double p = p0[k] + m * ub[k];
        const double sg = p > h[k] ? 1.0 : (p < -h[k] ? -1.0 : 0.0);
        if (sg != 0) { num = num + ub[k] * (p0[k] - sg * h[k]); den = den + ub[k] * ub[k]; }
      }
      if (den > 0) {
        const double s = fmin(fmax(-num / den, tau[i]), tau[i + 1]);
        const double f = axis_dist2(p0, ub, h, s);
        if (f < best) { best = f; ts = s; }
      }
      const double f = axis_dist2(p0, ub, h, tau[i + 1]);
      if (f < best) { best = f; ts = tau[i + 1]; }
    }
  }
  int n = 0;
  double b[3];
  ball_at(cC, C.u, -C.e, b);
  const int n0 = collide_sphere_box(b, sideC, cB, RB, sideB, flip, out);
  n += n0;
  ball_at(cC, C.u, C.e, b);
  const int n1 = collide_sphere_box(b, sideC, cB, RB, sideB, flip, out + 7 * n);
  n += n1;
  if (ts > -C.e && ts < C.e) {
    const double Ds = sqrt(axis_dist2(p0, ub, h, ts));
    bool flat = false;
    if (n0) flat |= fabs(sqrt(axis_dist2(p0, ub, h, -C.e)) - Ds) <= kFlat;
    if (n1) flat |= fabs(sqrt(axis_dist2(p0, ub, h, C.e)) - Ds) <= kFlat;
    if (!flat) {
      ball_at(cC, C.u, ts, b);
      n += collide_sphere_box(b, sideC, cB, RB, sideB, flip, out + 7 * n);
    }
  }
  return n;
}
#undef EGS_CSWAP

// ---- kernels ---------------------------------------------------------------
// SHAPES = 0 is the all-box code, launched whenever no shape array is set; SHAPES = 1 reads shape [n] (egs_shape) and
// dispatches boxes and spheres per lane; SHAPES = 2 dispatches capsules as well and is launched only when the shape
// array holds one, so a scene without capsules runs the kernels it ran before there were any.  The broad phase below
// does not look at shapes: its bounding radius 0.5 |side| is (sqrt(3) / 2) d >= r for a (d, d, d) sphere and
// 0.5 sqrt(2 d^2 + l^2) >= l / 2 for a (d, d, l) capsule, so the candidate ball contains the body and the candidate
// order (ascending j) is the box scene's.
// Batched worlds (ens != NULL): body b's ground contacts follow the pair contacts of the ensembles before
// its own, ebase[2e] of them (ens_base_kernel).
template <int SHAPES>
__global__ void __launch_bounds__(256) ground_kernel(int n, const double *pos, const double *R, const double *side,
                                                     const int *off, int *count, int *b0, int *b1, double *data,
                                                     const int *ens = nullptr, const int *ebase = nullptr,
                                                     const int32_t *shape = nullptr) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  double buf[8 * 7];
  int c;
  if (SHAPES == 2 && shape[b] == kShapeCapsule)
    c = ground_capsule(pos + 3 * (size_t)b, R + 9 * (size_t)b, side + 3 * (size_t)b, off ? buf : nullptr);
  else if (SHAPES && shape[b] == kShapeSphere)
    c = ground_sphere(pos + 3 * (size_t)b, side + 3 * (size_t)b, off ? buf : nullptr);
  else
    c = ground_contacts(pos + 3 * (size_t)b, R + 9 * (size_t)b, side + 3 * (size_t)b, off ? buf : nullptr);
  if (!off) { count[b] = c; return; }
  const size_t shift = ens ? (size_t)ebase[2 * ens[b]] : 0;
  for (int k = 0; k < c; ++k) {
    const size_t o = (size_t)off[b] + shift + k;
    b0[o] = -1; b1[o] = b;  // contact.h:13-15: ground contacts are (null, body)
    for (int q = 0; q < 7; ++q) data[o * 7 + q] = buf[7 * k + q];
  }
}

// One wavefront per body i: candidates j > i whose bounding spheres overlap, in
// ascending j (ballot keeps the order).  In a batched world (ens != NULL) j stops at the end
// of body i's ensemble: no cross-ensemble pair, O(sum n_e^2) instead of O(n^2).
__global__ void __launch_bounds__(64) cand_kernel(int n, const double *pos, const double *side, int *cand, int *count,
                                                  int *overflow, const int *ens = nullptr, const int *eoff = nullptr) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const double ci[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
  const double ri = 0.5 * sqrt(dot3(side + 3 * (size_t)i, side + 3 * (size_t)i));
  if (ens) n = eoff[ens[i] + 1];
  int found = 0;
  for (int base = i + 1; base < n; base += 64) {
    const int j = base + lane;
    bool hit = false;
    if (j < n) {
      const double d[3] = {pos[3 * (size_t)j] - ci[0], pos[3 * (size_t)j + 1] - ci[1], pos[3 * (size_t)j + 2] - ci[2]};
      const double rj = 0.5 * sqrt(dot3(side + 3 * (size_t)j, side + 3 * (size_t)j));
      const double rr = (ri + rj) * 1.0000001 + 1e-12;  // conservative: never drops a touching pair
      hit = dot3(d, d) <= rr * rr;
    }
    const unsigned long long mask = __ballot(hit);
    if (hit) {
      const int k = found + __popcll(mask & ((1ull << lane) - 1ull));
      if (k < KMAX) cand[(size_t)i * KMAX + k] = j;
    }
    found += __popcll(mask);
  }
  if (lane == 0) {
    if (found > KMAX) { atomicOr(overflow, 1); found = KMAX; }
    count[i] = found;
  }
}

// The same test without the KMAX cap, for the rare scene in which some body has more than KMAX
// partners (a big plate under many small boxes): FILL = false counts, FILL = true writes the pairs of
// body i at off[i] in ascending j -- the order of the capped kernels, so the contact list is unchanged.
template <bool FILL>
__global__ void __launch_bounds__(64) cand_all_kernel(int n, const double *pos, const double *side, const int *off,
                                                      int *count, int *pi, int *pj, const int *ens = nullptr,
                                                      const int *eoff = nullptr) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const double ci[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
  const double ri = 0.5 * sqrt(dot3(side + 3 * (size_t)i, side + 3 * (size_t)i));
  if (ens) n = eoff[ens[i] + 1];
  int found = 0;
  for (int base = i + 1; base < n; base += 64) {
    const int j = base + lane;
    bool hit = false;
    if (j < n) {
      const double d[3] = {pos[3 * (size_t)j] - ci[0], pos[3 * (size_t)j + 1] - ci[1], pos[3 * (size_t)j + 2] - ci[2]};
      const double rj = 0.5 * sqrt(dot3(side + 3 * (size_t)j, side + 3 * (size_t)j));
      const double rr = (ri + rj) * 1.0000001 + 1e-12;
      hit = dot3(d, d) <= rr * rr;
    }
    const unsigned long long mask = __ballot(hit);
    if (FILL && hit) {
      const int k = off[i] + found + __popcll(mask & ((1ull << lane) - 1ull));
      pi[k] = i; pj[k] = j;
    }
    found += __popcll(mask);
  }
  if (!FILL && lane == 0) count[i] = found;
}

// ---- uniform-grid broad phase (large n) ---------------------------------------
// Cell edge >= the largest rr of the sphere test, so a touching pair is always in
// adjacent cells.  Bodies are binned into a hashed table (count -> scan -> fill);
// one wavefront per body i then visits its 27 neighbour cells, keeps j > i that
// pass the SAME sphere test as cand_kernel, and sorts the (<= 64) survivors
// ascending -- so the candidate list, hence the contact order, is identical to
// the all-pairs kernel's.
constexpr int kCellClamp = 1 << 20;

// e: the body's ensemble in a batched world (0 otherwise, which leaves the hash as it was): co-located
// ensembles never share a cell, so the KMAX limit and the spill path count same-ensemble candidates only
__device__ __forceinline__ unsigned cell_hash(int x, int y, int z, int e = 0) {
  return (unsigned)x * 73856093u ^ (unsigned)y * 19349663u ^ (unsigned)z * 83492791u ^ (unsigned)e * 2654435761u;
}

__global__ void __launch_bounds__(1024) cell_size_kernel(int n, const double *side, double *cell) {
  __shared__ double red[1024];
  double r = 0.0;
  for (int b = threadIdx.x; b < n; b += 1024) r = fmax(r, 0.5 * sqrt(dot3(side + 3 * (size_t)b, side + 3 * (size_t)b)));
  red[threadIdx.x] = r;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]); __syncthreads(); }
  if (threadIdx.x == 0) cell[0] = 2.0 * red[0] * 1.000001 + 1e-9;
}

__global__ void __launch_bounds__(256) cell_bin_kernel(int n, const double *pos, const double *cell, int table_mask,
                                                       int *coords, int *bucket_of, int *arrival, int *tcount,
                                                       const int *ens = nullptr) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  const double c = cell[0];
  int q[3];
  for (int k = 0; k < 3; ++k) {
    double f = floor(pos[3 * (size_t)b + k] / c);
    f = fmin(fmax(f, (double)-kCellClamp), (double)kCellClamp);   // monotone, so neighbours stay neighbours
    q[k] = (int)f;
    coords[3 * (size_t)b + k] = q[k];
  }
  const int bkt = (int)(cell_hash(q[0], q[1], q[2], ens ? ens[b] : 0) & (unsigned)table_mask);
  bucket_of[b] = bkt;
  arrival[b] = atomicAdd(&tcount[bkt], 1);   // order inside a bucket is irrelevant: candidates are sorted later
}

__global__ void __launch_bounds__(256) cell_fill_kernel(int n, const int *bucket_of, const int *arrival, const int *toff,
                                                        int *sorted) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < n) sorted[toff[bucket_of[b]] + arrival[b]] = b;
}

__global__ void __launch_bounds__(64) cand_grid_kernel(int n, const double *pos, const double *side, const int *coords,
                                                       int table_mask, const int *toff, const int *tcount,
                                                       const int *sorted, int *cand, int *count, int *overflow,
                                                       const int *ens = nullptr) {
  __shared__ int list[KMAX];
  const int i = blockIdx.x, lane = threadIdx.x;
  const int ei = ens ? ens[i] : 0;
  const double ci[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
  const double ri = 0.5 * sqrt(dot3(side + 3 * (size_t)i, side + 3 * (size_t)i));
  const int cx = coords[3 * (size_t)i], cy = coords[3 * (size_t)i + 1], cz = coords[3 * (size_t)i + 2];
  int found = 0;
  for (int nb = 0; nb < 27; ++nb) {
    const int x = cx + nb % 3 - 1, y = cy + (nb / 3) % 3 - 1, z = cz + nb / 9 - 1;
    const int bkt = (int)(cell_hash(x, y, z, ei) & (unsigned)table_mask);
    const int beg = toff[bkt], cnt = tcount[bkt];
    for (int base = 0; base < cnt; base += 64) {
      const int k = base + lane;
      bool hit = false;
      int j = -1;
      if (k < cnt) {
        j = sorted[beg + k];
        // exact cell match: a bucket shared by two cells (hash collision) is never counted twice
        if (j > i && coords[3 * (size_t)j] == x && coords[3 * (size_t)j + 1] == y && coords[3 * (size_t)j + 2] == z &&
            (!ens || ens[j] == ei)) {
          const double d[3] = {pos[3 * (size_t)j] - ci[0], pos[3 * (size_t)j + 1] - ci[1], pos[3 * (size_t)j + 2] - ci[2]};
          const double rj = 0.5 * sqrt(dot3(side + 3 * (size_t)j, side + 3 * (size_t)j));
          const double rr = (ri + rj) * 1.0000001 + 1e-12;
          hit = dot3(d, d) <= rr * rr;
        }
      }
      const unsigned long long mask = __ballot(hit);
      if (hit) {
        const int idx = found + __popcll(mask & ((1ull << lane) - 1ull));
        if (idx < KMAX) list[idx] = j;
      }
      found += __popcll(mask);
    }
  }
  __syncthreads();
  const int nf = found < KMAX ? found : KMAX;
  const int c = lane < nf ? list[lane] : 0x7fffffff;
  int rank = 0;
  for (int k = 0; k < nf; ++k) rank += (__shfl(c, k) < c) ? 1 : 0;   // candidates are distinct bodies
  if (lane < nf) cand[(size_t)i * KMAX + rank] = c;
  if (lane == 0) {
    if (found > KMAX) atomicOr(overflow, 1);
    count[i] = nf;
  }
}

__global__ void __launch_bounds__(256) flatten_kernel(int n, const int *cand, const int *count, const int *off, int *pi,
                                                      int *pj) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int k = 0; k < count[i]; ++k) { pi[off[i] + k] = i; pj[off[i] + k] = cand[(size_t)i * KMAX + k]; }
}

// Narrow phase + contact-vs-contact pruning within the pair
// (ensembles.cc:308-316, kMinConstraintDistance = 1e-6: a contact is deleted if
// ANY earlier contact of the same pair lies within 1e-6 of it).
// Joints between the same two bodies prune contacts within 1e-6 of the joint
// position (ensembles.cc:296-306; Joint::GetConstraintPosition, joints.cc:57-75).
struct JointList { int mj; const int *b0, *b1; const double *data; };

template <bool EMIT, int SHAPES>
__global__ void __launch_bounds__(64) narrow_kernel(int npairs, const int *pi, const int *pj, const double *pos,
                                                    const double *R, const double *side, const int *off, int base,
                                                    int *count, int *b0, int *b1, double *data, JointList jl,
                                                    const int *ens = nullptr, const int *ebase = nullptr,
                                                    const int32_t *shape = nullptr) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= npairs) return;
  const int i = pi[t], j = pj[t];
  double cs[MAXC * 7];
  int nc;
  const bool si = SHAPES && shape[i] == kShapeSphere, sj = SHAPES && shape[j] == kShapeSphere;
  const bool ki = SHAPES == 2 && shape[i] == kShapeCapsule, kj = SHAPES == 2 && shape[j] == kShapeCapsule;
  if (ki || kj) {   // the capsule's partner: a capsule, a sphere (si / sj) or a box
    const double *ci = pos + 3 * (size_t)i, *Ri = R + 9 * (size_t)i, *di = side + 3 * (size_t)i;
    const double *cj = pos + 3 * (size_t)j, *Rj = R + 9 * (size_t)j, *dj = side + 3 * (size_t)j;
    if (ki && kj) nc = collide_capsules(ci, Ri, di, cj, Rj, dj, cs);
    else if (ki && sj) nc = collide_capsule_sphere(ci, Ri, di, cj, dj, /*first=*/true, cs);
    else if (kj && si) nc = collide_capsule_sphere(cj, Rj, dj, ci, di, /*first=*/false, cs);
    else if (ki) nc = collide_capsule_box(ci, Ri, di, cj, Rj, dj, /*flip=*/true, cs);
    else nc = collide_capsule_box(cj, Rj, dj, ci, Ri, di, /*flip=*/false, cs);
  } else if (si && sj)   // a sphere pair or sphere-box pair has one contact: only the joint test below can drop it
    nc = collide_spheres(pos + 3 * (size_t)i, side + 3 * (size_t)i, pos + 3 * (size_t)j, side + 3 * (size_t)j, cs);
  else if (si)
    nc = collide_sphere_box(pos + 3 * (size_t)i, side + 3 * (size_t)i, pos + 3 * (size_t)j, R + 9 * (size_t)j,
                            side + 3 * (size_t)j, /*flip=*/true, cs);
  else if (sj)
    nc = collide_sphere_box(pos + 3 * (size_t)j, side + 3 * (size_t)j, pos + 3 * (size_t)i, R + 9 * (size_t)i,
                            side + 3 * (size_t)i, /*flip=*/false, cs);
  else
    nc = collide_boxes(pos + 3 * (size_t)i, R + 9 * (size_t)i, side + 3 * (size_t)i, pos + 3 * (size_t)j,
                       R + 9 * (size_t)j, side + 3 * (size_t)j, cs);
  int kept = 0;
  for (int a = 0; a < nc; ++a) {
    bool del = false;
    for (int q = 0; q < jl.mj; ++q) {
      const int a0 = jl.b0[q], a1 = jl.b1[q];
      if (!((a0 == i && a1 == j) || (a0 == j && a1 == i))) continue;
      double r0[3], r1[3];
      mat3_vec(R + 9 * (size_t)a0, jl.data + 7 * (size_t)q, r0);
      mat3_vec(R + 9 * (size_t)a1, jl.data + 7 * (size_t)q + 3, r1);
      double d[3];
      for (int k = 0; k < 3; ++k) {
        const double jp = ((pos[3 * (size_t)a0 + k] + r0[k]) + (pos[3 * (size_t)a1 + k] + r1[k])) / 2;
        d[k] = jp - cs[7 * a + k];
      }
      if (sqrt(dot3(d, d)) < 1e-6) del = true;
    }
    for (int b = 0; b < a; ++b) {
      const double d[3] = {cs[7 * b] - cs[7 * a], cs[7 * b + 1] - cs[7 * a + 1], cs[7 * b + 2] - cs[7 * a + 2]};
      if (sqrt(dot3(d, d)) < 1e-6) del = true;
    }
    if (del) continue;
    if (EMIT) {   // batched: after the ground contacts of ensembles 0..e, ebase[2e + 1] of them
      const size_t o = (size_t)(ens ? ebase[2 * ens[i] + 1] : base) + off[t] + kept;
      b0[o] = i; b1[o] = j;
      for (int q = 0; q < 7; ++q) data[o * 7 + q] = cs[7 * a + q];
    }
    ++kept;
  }
  if (!EMIT) count[t] = kept;
}

// Batched world: where each ensemble's contacts go.  The list is, ensemble by ensemble, its ground
// contacts then its pairs; goff / coff / poff are the exclusive scans over ALL bodies / pairs and
// totals = {-, G, C, P}.  ebase[2e] = pair contacts of the ensembles before e, ebase[2e + 1] = ground
// contacts of ensembles 0..e; contact_off[e] (e <= E) = first contact of ensemble e.
__global__ void __launch_bounds__(256) ens_base_kernel(int E, int n, const int *eoff, const int *goff, const int *coff,
                                                       const int *poff, const int *totals, int *ebase, int *contact_off) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e > E) return;
  const int G = totals[1], C = totals[2], P = totals[3];
  const int b = eoff[e];
  const int g_before = b < n ? goff[b] : G;
  const int c_first = b < n ? coff[b] : C;
  const int p_before = c_first < C ? poff[c_first] : P;
  contact_off[e] = g_before + p_before;
  if (e < E) {
    const int b1 = eoff[e + 1];
    ebase[2 * e] = p_before;
    ebase[2 * e + 1] = b1 < n ? goff[b1] : G;
  }
}

// Copies the contact topology into device-visible (page-locked host) memory: a
// small PCIe write by the GPU is far cheaper than two DMA-engine copies.
__global__ void __launch_bounds__(256) export_pairs_kernel(int m, const int *b0, const int *b1, int *o0, int *o1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) { o0[i] = b0[i]; o1[i] = b1[i]; }
}

// ---- exclusive scan (int32), three small kernels ----------------------------
constexpr int SCAN_CHUNK = 2048;  // elements per block (256 threads x 8)
__global__ void __launch_bounds__(256) scan_reduce_kernel(int n, const int *in, int *block_sums) {
  __shared__ int red[256];
  const int base = blockIdx.x * SCAN_CHUNK;
  int s = 0;
  for (int k = threadIdx.x; k < SCAN_CHUNK; k += 256) if (base + k < n) s += in[base + k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0];
}
__global__ void scan_blocks_kernel(int nblocks, int *block_sums, int *total) {  // one thread: nblocks is small
  int run = 0;
  for (int b = 0; b < nblocks; ++b) { const int v = block_sums[b]; block_sums[b] = run; run += v; }
  *total = run;
}
__global__ void __launch_bounds__(256) scan_apply_kernel(int n, const int *in, const int *block_sums, int *out) {
  __shared__ int part[256];
  const int base = blockIdx.x * SCAN_CHUNK + threadIdx.x * 8;
  int v[8], s = 0;
  for (int k = 0; k < 8; ++k) { v[k] = (base + k < n) ? in[base + k] : 0; s += v[k]; }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) { int run = block_sums[blockIdx.x]; for (int t = 0; t < 256; ++t) { const int x = part[t]; part[t] = run; run += x; } }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int k = 0; k < 8; ++k) { if (base + k < n) out[base + k] = run; run += v[k]; }
}

// n <= 16384: the whole scan in one 1024-thread workgroup (one launch instead of three)
constexpr int SCAN_SMALL = 16384;
__global__ void __launch_bounds__(1024) scan_small_kernel(int n, const int *in, int *out, int *total) {
  __shared__ int part[1024];
  const int per = (n + 1023) / 1024;            // contiguous elements per thread, <= 16
  const int base = threadIdx.x * per;
  int v[16], sum = 0;
  for (int k = 0; k < per; ++k) { v[k] = (base + k < n) ? in[base + k] : 0; sum += v[k]; }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {          // inclusive Hillis-Steele over the 1024 partial sums
    const int add = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  int run = part[threadIdx.x] - sum;            // exclusive prefix of this thread's chunk
  for (int k = 0; k < per; ++k) { if (base + k < n) out[base + k] = run; run += v[k]; }
  if (threadIdx.x == 1023) *total = part[1023];
}

void exclusive_scan_async(hipStream_t s, int n, const int *in, int *out, int *scratch_blocks, int *total_d) {
  const int nblocks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
  if (n <= 0) return;
  if (n <= SCAN_SMALL) {
    hipLaunchKernelGGL(scan_small_kernel, dim3(1), dim3(1024), 0, s, n, in, out, total_d);
    return;
  }
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(nblocks), dim3(256), 0, s, n, in, scratch_blocks);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1), 0, s, nblocks, scratch_blocks, total_d);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(nblocks), dim3(256), 0, s, n, in, scratch_blocks, out);
}

int exclusive_scan(hipStream_t s, int n, const int *in, int *out, int *scratch_blocks, int *total_d) {
  if (n <= 0) return 0;
  exclusive_scan_async(s, n, in, out, scratch_blocks, total_d);
  int total = 0;
  HIPCHK(hipMemcpyAsync(&total, total_d, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return total;
}

}  // namespace

// ---- device-resident collider ---------------------------------------------
namespace {
constexpr int kGridMinBodies = 2048;   // below this the all-pairs wave scan is a single cheap launch
bool use_grid(int n) {
  const char *e = std::getenv("EGS_BROADPHASE");   // "grid" / "pairs" force one broad phase (tests)
  if (e && !std::strcmp(e, "grid")) return true;
  if (e && !std::strcmp(e, "pairs")) return false;
  return n >= kGridMinBodies;
}
}  // namespace

struct Collider::Impl {
  // grow-only: a world runs the collider every step
  DevBuf<int> gcount, goff, ccount, coff, cand, flags, blocks, pi, pj, pcount, poff, blocks2, b0, b1;
  DevBuf<int> coords, bucket_of, arrival, tcount, toff, sorted, blocks3, scratch;   // uniform grid
  DevBuf<int> ebase;                                                                 // batched worlds
  DevBuf<double> data, cell;
};

Collider::Collider() : impl_(new Impl) {}
Collider::~Collider() { delete impl_; }
const int32_t *Collider::body0() const { return impl_->b0.p; }
const int32_t *Collider::body1() const { return impl_->b1.p; }
const double *Collider::data() const { return impl_->data.p; }
void Collider::set_ensembles(int n_ens, const int32_t *ens, const int32_t *eoff, int32_t *contact_off) {
  n_ens_ = n_ens; ens_ = ens; eoff_ = eoff; contact_off_ = contact_off;
}

int Collider::run(hipStream_t s, int n, const double *dpos, const double *dR, const double *dside, int mj,
                  const int32_t *djb0, const int32_t *djb1, const double *djdata, const int32_t *dshape, bool capsules) {
  const JointList jl{mj, djb0, djb1, djdata};
  Impl &I = *impl_;
  n_ground_ = 0; n_pairs_ = 0;
  const int *ens = n_ens_ > 0 ? ens_ : nullptr, *eoff = n_ens_ > 0 ? eoff_ : nullptr;
  if (n <= 0) {
    if (ens) HIPCHK(hipMemsetAsync(contact_off_, 0, (size_t)(n_ens_ + 1) * sizeof(int32_t), s));
    return 0;
  }
  const size_t nn = (size_t)n;
  I.gcount.alloc(nn); I.goff.alloc(nn); I.ccount.alloc(nn); I.coff.alloc(nn); I.cand.alloc(nn * KMAX); I.flags.alloc(4);
  I.blocks.alloc((nn + SCAN_CHUNK - 1) / SCAN_CHUNK + 8); I.blocks2.alloc((nn + SCAN_CHUNK - 1) / SCAN_CHUNK + 8);
  // flags: [0] candidate overflow, [1] ground contacts, [2] candidate pairs, [3] pair contacts
  HIPCHK(hipMemsetAsync(I.flags.p, 0, 4 * sizeof(int), s));
  const int gb = (n + 255) / 256;
  // dshape == NULL: every body a box, the SHAPES = 0 instantiations (the launches of a world without shapes)
  // the SHAPES = 2 forms only where the caller's shape array holds a capsule
  if (dshape && capsules)
    hipLaunchKernelGGL((ground_kernel<2>), dim3(gb), dim3(256), 0, s, n, dpos, dR, dside, (const int *)nullptr, I.gcount.p,
                       (int *)nullptr, (int *)nullptr, (double *)nullptr, (const int *)nullptr, (const int *)nullptr, dshape);
  else if (dshape)
    hipLaunchKernelGGL((ground_kernel<1>), dim3(gb), dim3(256), 0, s, n, dpos, dR, dside, (const int *)nullptr, I.gcount.p,
                       (int *)nullptr, (int *)nullptr, (double *)nullptr, (const int *)nullptr, (const int *)nullptr, dshape);
  else
  hipLaunchKernelGGL((ground_kernel<0>), dim3(gb), dim3(256), 0, s, n, dpos, dR, dside, (const int *)nullptr, I.gcount.p,
                     (int *)nullptr, (int *)nullptr, (double *)nullptr);
  exclusive_scan_async(s, n, I.gcount.p, I.goff.p, I.blocks.p, I.flags.p + 1);
  if (use_grid(n)) {
    int table = 1024;
    while (table < 2 * n) table <<= 1;
    I.cell.alloc(1); I.coords.alloc(nn * 3); I.bucket_of.alloc(nn); I.arrival.alloc(nn); I.sorted.alloc(nn);
    I.tcount.alloc((size_t)table); I.toff.alloc((size_t)table); I.blocks3.alloc((size_t)table / SCAN_CHUNK + 8);
    I.scratch.alloc(1);
    HIPCHK(hipMemsetAsync(I.tcount.p, 0, (size_t)table * sizeof(int), s));
    hipLaunchKernelGGL(cell_size_kernel, dim3(1), dim3(1024), 0, s, n, dside, I.cell.p);
    hipLaunchKernelGGL(cell_bin_kernel, dim3(gb), dim3(256), 0, s, n, dpos, I.cell.p, table - 1, I.coords.p, I.bucket_of.p,
                       I.arrival.p, I.tcount.p, ens);
    exclusive_scan_async(s, table, I.tcount.p, I.toff.p, I.blocks3.p, I.scratch.p);
    hipLaunchKernelGGL(cell_fill_kernel, dim3(gb), dim3(256), 0, s, n, I.bucket_of.p, I.arrival.p, I.toff.p, I.sorted.p);
    hipLaunchKernelGGL(cand_grid_kernel, dim3(n), dim3(64), 0, s, n, dpos, dside, I.coords.p, table - 1, I.toff.p,
                       I.tcount.p, I.sorted.p, I.cand.p, I.ccount.p, I.flags.p, ens);
  } else {
    hipLaunchKernelGGL(cand_kernel, dim3(n), dim3(64), 0, s, n, dpos, dside, I.cand.p, I.ccount.p, I.flags.p, ens, eoff);
  }
  exclusive_scan_async(s, n, I.ccount.p, I.coff.p, I.blocks2.p, I.flags.p + 2);
  int totals[4] = {0, 0, 0, 0};   // ONE read-back for overflow, G and C
  HIPCHK(hipMemcpyAsync(totals, I.flags.p, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const bool spill = totals[0] != 0;   // some body has more than KMAX partners: uncapped count -> scan -> fill
  if (spill) {
    hipLaunchKernelGGL((cand_all_kernel<false>), dim3(n), dim3(64), 0, s, n, dpos, dside, (const int *)nullptr, I.ccount.p,
                       (int *)nullptr, (int *)nullptr, ens, eoff);
    totals[2] = exclusive_scan(s, n, I.ccount.p, I.coff.p, I.blocks2.p, I.flags.p + 2);
  }
  const int G = totals[1], C = totals[2];
  int P = 0;
  if (C > 0) {
    I.pi.alloc(C); I.pj.alloc(C); I.pcount.alloc(C); I.poff.alloc(C); I.blocks2.alloc(((size_t)C + SCAN_CHUNK - 1) / SCAN_CHUNK + 8);
    if (spill) hipLaunchKernelGGL((cand_all_kernel<true>), dim3(n), dim3(64), 0, s, n, dpos, dside, I.coff.p, (int *)nullptr, I.pi.p, I.pj.p,
                                  ens, eoff);
    else
    hipLaunchKernelGGL(flatten_kernel, dim3(gb), dim3(256), 0, s, n, I.cand.p, I.ccount.p, I.coff.p, I.pi.p, I.pj.p);
    if (dshape && capsules)
      hipLaunchKernelGGL((narrow_kernel<false, 2>), dim3((C + 63) / 64), dim3(64), 0, s, C, I.pi.p, I.pj.p, dpos, dR, dside,
                         (const int *)nullptr, 0, I.pcount.p, (int *)nullptr, (int *)nullptr, (double *)nullptr, jl,
                         (const int *)nullptr, (const int *)nullptr, dshape);
    else if (dshape)
      hipLaunchKernelGGL((narrow_kernel<false, 1>), dim3((C + 63) / 64), dim3(64), 0, s, C, I.pi.p, I.pj.p, dpos, dR, dside,
                         (const int *)nullptr, 0, I.pcount.p, (int *)nullptr, (int *)nullptr, (double *)nullptr, jl,
                         (const int *)nullptr, (const int *)nullptr, dshape);
    else
    hipLaunchKernelGGL((narrow_kernel<false, 0>), dim3((C + 63) / 64), dim3(64), 0, s, C, I.pi.p, I.pj.p, dpos, dR, dside,
                       (const int *)nullptr, 0, I.pcount.p, (int *)nullptr, (int *)nullptr, (double *)nullptr, jl);
    P = exclusive_scan(s, C, I.pcount.p, I.poff.p, I.blocks2.p, I.flags.p + 3);
  }
  const int m = G + P;
  n_ground_ = G; n_pairs_ = C;
  if (ens) {   // per-ensemble order: ground contacts then pairs, ensemble by ensemble
    I.ebase.alloc((size_t)n_ens_ * 2);
    hipLaunchKernelGGL(ens_base_kernel, dim3(n_ens_ / 256 + 1), dim3(256), 0, s, n_ens_, n, eoff, I.goff.p, I.coff.p, I.poff.p,
                       I.flags.p, I.ebase.p, contact_off_);
  }
  if (m == 0) return 0;
  I.b0.alloc(m); I.b1.alloc(m); I.data.alloc((size_t)m * 7);
  if (dshape && capsules)
    hipLaunchKernelGGL((ground_kernel<2>), dim3(gb), dim3(256), 0, s, n, dpos, dR, dside, I.goff.p, (int *)nullptr, I.b0.p,
                       I.b1.p, I.data.p, ens, ens ? I.ebase.p : nullptr, dshape);
  else if (dshape)
    hipLaunchKernelGGL((ground_kernel<1>), dim3(gb), dim3(256), 0, s, n, dpos, dR, dside, I.goff.p, (int *)nullptr, I.b0.p,
                       I.b1.p, I.data.p, ens, ens ? I.ebase.p : nullptr, dshape);
  else
  hipLaunchKernelGGL((ground_kernel<0>), dim3(gb), dim3(256), 0, s, n, dpos, dR, dside, I.goff.p, (int *)nullptr, I.b0.p,
                     I.b1.p, I.data.p, ens, ens ? I.ebase.p : nullptr);
  if (C > 0 && dshape && capsules)
    hipLaunchKernelGGL((narrow_kernel<true, 2>), dim3((C + 63) / 64), dim3(64), 0, s, C, I.pi.p, I.pj.p, dpos, dR, dside,
                       I.poff.p, G, (int *)nullptr, I.b0.p, I.b1.p, I.data.p, jl, ens, ens ? I.ebase.p : nullptr, dshape);
  else if (C > 0 && dshape)
    hipLaunchKernelGGL((narrow_kernel<true, 1>), dim3((C + 63) / 64), dim3(64), 0, s, C, I.pi.p, I.pj.p, dpos, dR, dside,
                       I.poff.p, G, (int *)nullptr, I.b0.p, I.b1.p, I.data.p, jl, ens, ens ? I.ebase.p : nullptr, dshape);
  else if (C > 0)
    hipLaunchKernelGGL((narrow_kernel<true, 0>), dim3((C + 63) / 64), dim3(64), 0, s, C, I.pi.p, I.pj.p, dpos, dR, dside,
                       I.poff.p, G, (int *)nullptr, I.b0.p, I.b1.p, I.data.p, jl, ens, ens ? I.ebase.p : nullptr);
  HIPCHK(hipGetLastError());
  return m;
}

void Collider::export_topology(hipStream_t s, int m, int32_t *mapped_b0, int32_t *mapped_b1) const {
  if (m <= 0) return;
  hipLaunchKernelGGL(export_pairs_kernel, dim3((m + 255) / 256), dim3(256), 0, s, m, impl_->b0.p, impl_->b1.p, mapped_b0,
                     mapped_b1);
  HIPCHK(hipGetLastError());
}

int update_contacts(hipStream_t s, int n, const double *pos, const double *R, const double *side, int max_contacts,
                    int32_t *body0, int32_t *body1, double *data, int *n_ground, int *n_pairs, int mj,
                    const int32_t *jb0, const int32_t *jb1, const double *jdata, const int32_t *shape) {
  if (n_ground) *n_ground = 0;
  if (n_pairs) *n_pairs = 0;
  if (n <= 0) return 0;
  const size_t nn = (size_t)n;
  ScopedDevBuf<double> dpos(nn * 3), dR(nn * 9), dside(nn * 3);
  HIPCHK(hipMemcpyAsync(dpos.p, pos, nn * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dR.p, R, nn * 9 * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dside.p, side, nn * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  ScopedDevBuf<int> djb0((size_t)mj), djb1((size_t)mj);
  ScopedDevBuf<double> djdata((size_t)mj * 7);
  if (mj > 0) {
    HIPCHK(hipMemcpyAsync(djb0.p, jb0, (size_t)mj * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(djb1.p, jb1, (size_t)mj * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(djdata.p, jdata, (size_t)mj * 7 * sizeof(double), hipMemcpyHostToDevice, s));
  }
  ScopedDevBuf<int> dshape(shape ? nn : 0);
  if (shape) HIPCHK(hipMemcpyAsync(dshape.p, shape, nn * sizeof(int), hipMemcpyHostToDevice, s));
  bool capsules = false;
  for (size_t b = 0; shape && b < nn; ++b) capsules |= shape[b] == kShapeCapsule;
  Collider col;
  const int m = col.run(s, n, dpos.p, dR.p, dside.p, mj, djb0.p, djb1.p, djdata.p, shape ? dshape.p : nullptr, capsules);
  if (n_ground) *n_ground = col.n_ground();
  if (n_pairs) *n_pairs = col.n_pairs();
  if (m > max_contacts) throw std::invalid_argument("update_contacts: max_contacts too small (" + std::to_string(m) + " needed)");
  if (m == 0) return 0;
  HIPCHK(hipMemcpyAsync(body0, col.body0(), (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(body1, col.body1(), (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(data, col.data(), (size_t)m * 7 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return m;
}

}  // namespace egs
