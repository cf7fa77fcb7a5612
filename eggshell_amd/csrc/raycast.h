// raycast.h -- ray casts against the world's solids on the GPU (see raycast.hip; the rules are stated above
// egs_cast_rays in eggshell_amd.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace egs {

// bodies staged into LDS per round of the kernel: the scan of a ray's ensemble goes chunk by chunk
constexpr int kRayChunk = 128;

// One launch, one ray per lane, every array on the device.  pos [n][3], R [n][9], side [n][3] are the fp64 arrays the
// collider reads, shape [n] (egs_shape) or NULL = boxes.  ray_ens [n_rays] non-decreasing with body_off [n_ens + 1], or
// both NULL: one ensemble, the bodies [0, n_bodies).  ray_body [n_rays] (global index, -1 = world frame) or NULL = all
// world frame: origin and dir are then in that body's frame and the body is not tested.  Writes hit [n_rays], t
// [n_rays], normal [n_rays][3] (may be NULL).  The caller has checked every index.  The bounding-sphere rejection is on
// where an ensemble holds more than one chunk of bodies on average (n_bodies / n_ens > kRayChunk; measured in DESIGN.md
// 4o: it costs a quarter on 64-body heaps and saves 2.4 x on a 4 096-body plate); EGS_RAY_CULL=0 / 1 (read here, per
// call) forces it off / on.  The results are the same either way.
void cast_rays_device(hipStream_t s, int n_bodies, const double *pos, const double *R, const double *side,
                      const int32_t *shape, int n_rays, const int32_t *ray_ens, const int32_t *body_off, int n_ens,
                      const int32_t *ray_body, const double *origin, const double *dir, const double *tmax, int32_t *hit,
                      double *t, double *normal);

}  // namespace egs
