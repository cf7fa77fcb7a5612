// collide.h -- contact generation on the GPU (see collide.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace egs {

// ---- shapes (egs_shape in eggshell_amd.h; shape == NULL everywhere below means every body is a box) -----------
// A SPHERE is a body whose side row is (d, d, d) with d > 0; r = d / 2 and its R is not read.  The conventions are
// the box code's: contacts are (body0, body1) with body0 < body1 or body0 = -1 (ground), the normal points from
// body0 towards body1, depth >= 0, an exactly touching pair (separation == 0) IS a contact, a ground contact needs
// z < 0 strictly.
//   sphere - ground   q = (c_x, c_y, c_z - r); contact iff q_z < 0: position q, normal (0, 0, 1), depth -q_z.
//   sphere i - j      d = c_j - c_i, L = |d|, s = L - (r_i + r_j); contact iff s <= 0; n = d / L ((0, 0, 1) when
//                     L == 0); depth = -s; position = c_i + n (r_i + L - r_j) / 2, the midpoint of the two surface
//                     points on the centre line.
//   sphere S - box B  p = R_B^T (c_S - c_B), h = side_B / 2, q_k = clamp(p_k, -h_k, h_k).
//                     Centre outside (q != p): e = p - q, L = |e|; contact iff L - r <= 0; n_BS = R_B e / L,
//                     depth = r - L; box point R_B q + c_B, sphere point c_S - r n_BS.
//                     Centre inside or on the surface (q == p): k = argmin_k (h_k - |p_k|), lowest k on a tie;
//                     n_BS = sgn(p_k) (column k of R_B), sgn(0) = +1; depth = (h_k - |p_k|) + r; box point = the
//                     centre moved onto that face, sphere point c_S - r n_BS.
//                     Position = the midpoint of the two points; the normal is n_BS if the box is body0, -n_BS if
//                     the sphere is.
// A pair with a sphere yields at most one contact, so only the joint-vs-contact pruning can remove it.  List order:
// per ensemble the ground contacts by body, then the pairs i < j; box-box pairs emit what they emit without shapes.
//
// A CAPSULE (EGS_SHAPE_CAPSULE = 2) is a body whose side row is (d, d, l) with d > 0 and l > d strictly, both finite
// (l == d is a sphere and is refused: use EGS_SHAPE_SPHERE).  r = d / 2, half axis e = (l - d) / 2 > 0, axis u =
// column 2 of R (R[2], R[5], R[8]); "the ball at t" is the sphere of diameter d centred at c + t u, t in [-e, e];
// end 0 is t = -e, end 1 is t = +e.  The conventions are the ones above, and every rule is one of the three sphere
// rules applied to balls of the capsule:
//   capsule - ground   the sphere - ground rule on the ball at end 0, then at end 1: at most 2 contacts, in that order.
//   capsule - sphere   t = clamp((c_S - c) . u, -e, e); the sphere - sphere rule between the ball at t and the sphere,
//                      in the pair's (i, j) order: at most 1 contact.
//   capsule i - j      candidates in this order: end 0 of i against capsule j, end 1 of i against j, end 0 of j against
//                      capsule i, end 1 of j against i (each by the capsule - sphere rule, normal always i -> j), then
//                      the interior pair: the balls at the axes' common-perpendicular parameters (s, t), which exists
//                      only where s and t lie strictly inside both segments and the 2 x 2 determinant
//                      (u_i.u_i)(u_j.u_j) - (u_i.u_j)^2 is non-zero in the device's arithmetic.  Whenever the closest
//                      pair of the two segments involves an end it is one of the four end candidates, so parallel axes
//                      need no special case.  At most 5 contacts.
//   capsule - box      dist(t) = the L of the sphere - box rule for a centre at c + t u (0 inside the box).  Candidates:
//                      end 0, end 1, then the interior point t*, each by the sphere - box rule.  t* is the lowest
//                      minimiser of dist on [-e, e] and counts only when strictly inside; if the axis enters the box
//                      (minimum 0) t* is the midpoint of the stretch of axis inside the box (the segment clipped
//                      against the three slabs).  dist^2 is a convex piecewise quadratic in t with at most 6
//                      breakpoints (a box-frame coordinate of the axis crossing +-h_k); the minimiser is found exactly
//                      up to rounding from the ends, the breakpoints and each piece's stationary point.  At most 3.
//   A candidate is emitted iff its sphere rule says contact.
//   Flat rule (capsule - capsule and capsule - box): the interior candidate is dropped if an EMITTED end candidate's
//   centre distance (for a box: its dist) is within 1e-9 of its own; 1e-9 is absolute, in metres, a constant of the
//   kind of the collider's 1e-6.  So a log flat on a plate and two logs side by side get 2 contacts, a capsule bridging
//   two boxes one per box; a crossed pair, a capsule see-sawing on a box edge and a capsule lying across a box narrower
//   than itself get 1.  In that last case dist is constant along the stretch above the box up to rounding, and the
//   contact's position ALONG that flat stretch is unspecified within the stretch.
// The kernel's same-pair 1e-6 pruning and the joint-vs-contact pruning then run unchanged.  List order and the output
// of box - box pairs and of spheres are unchanged.

// pos [n][3], R [n][9] row-major, side [n][3] on the host.  Writes the contact
// list in the reference's order (ground contacts by body, then pairs i < j):
// body0/body1 [m], data [m][7] = position, normal, depth.  Returns m.
// Throws std::invalid_argument if m > max_contacts or a body has more than 64
// overlapping partners.  shape [n] (host, egs_shape) or NULL; the caller has checked its values and the sides of the
// spheres and the capsules.
int update_contacts(hipStream_t s, int n, const double *pos, const double *R, const double *side, int max_contacts,
                    int32_t *body0, int32_t *body1, double *data, int *n_ground, int *n_pairs, int mj = 0,
                    const int32_t *jb0 = nullptr, const int32_t *jb1 = nullptr, const double *jdata = nullptr,
                    const int32_t *shape = nullptr);

// Device-resident form: body state already on the device, the contact list stays
// there (body0()/body1()/data() are device pointers valid until the next run()).
class Collider {
 public:
  Collider();
  ~Collider();
  Collider(const Collider &) = delete;
  Collider &operator=(const Collider &) = delete;
  // optional joints (device arrays, body-body only matter): contacts within 1e-6 of a
  // joint between the same two bodies are dropped (ensembles.cc:296-306).
  // dshape [n] (device, egs_shape) or NULL = all boxes, which takes the launches of a collider without shapes.
  int run(hipStream_t s, int n, const double *dpos, const double *dR, const double *dside, int mj = 0,
          const int32_t *djb0 = nullptr, const int32_t *djb1 = nullptr, const double *djdata = nullptr,
          const int32_t *dshape = nullptr, bool capsules = false);  // returns m
  // capsules: dshape holds an EGS_SHAPE_CAPSULE (the caller knows from its host copy); only then are the
  // capsule instantiations of the kernels launched -- false with a capsule in dshape collides it as a box.
  // body0()/body1() of the last run() written to device-visible host memory (hipHostMalloc)
  void export_topology(hipStream_t s, int m, int32_t *mapped_b0, int32_t *mapped_b1) const;
  const int32_t *body0() const;
  const int32_t *body1() const;
  const double *data() const;
  // Batched world (egs_world_create_batch): n_ens > 0 ensembles, ens [n] = each body's ensemble and
  // eoff [n_ens + 1] = body offsets, device arrays the caller keeps alive.  Pairs across ensembles are
  // never candidates; the list is, ensemble by ensemble, its ground contacts then its pairs i < j, and
  // run() writes each ensemble's first contact to contact_off [n_ens + 1] (device).  n_ens = 0: off.
  void set_ensembles(int n_ens, const int32_t *ens, const int32_t *eoff, int32_t *contact_off);
  int n_ground() const { return n_ground_; }
  int n_pairs() const { return n_pairs_; }

 private:
  struct Impl;
  Impl *impl_;
  int n_ground_ = 0, n_pairs_ = 0;
  int n_ens_ = 0;
  const int32_t *ens_ = nullptr, *eoff_ = nullptr;
  int32_t *contact_off_ = nullptr;
};

}  // namespace egs
