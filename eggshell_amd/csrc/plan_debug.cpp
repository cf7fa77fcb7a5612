// plan_debug.cpp -- the plan-inspection entries of the C ABI (egs_debug_plan*, egs_debug_matvec_plan,
// egs_debug_choose_oversize_schedule, egs_debug_face_split, egs_debug_face_form): what the host planners (plan.h, matvec_plan.h) and the schedule policy
// (policy.h) decide for a constraint graph, per constraint.  Host code only: no HIP call, no context, no device.
#include <exception>

#include "../../include/eggshell_amd.h"
#include "matvec_plan.h"
#include "plan.h"
#include "policy.h"

using namespace egs;

namespace {

// the entries' argument check and error boundary: a planner that throws (std::exception) is an invalid graph
template <typename F>
egs_status plan_entry(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, F &&f) {
  if (n < 0 || m < 0 || (m > 0 && (!body0 || !body1))) return EGS_ERR_INVALID;
  try {
    return f();
  } catch (const std::exception &) {
    return EGS_ERR_INVALID;
  }
}

// f(lane, tile, lane index) for every lane of n_tiles tiles of `block` lanes that holds a constraint
template <typename LANE, typename F>
void for_each_constraint_lane(const std::vector<LANE> &lanes, int n_tiles, int block, F &&f) {
  for (int t = 0; t < n_tiles; ++t)
    for (int l = 0; l < block; ++l) {
      const LANE &d = lanes[(size_t)t * block + l];
      if (d.cidx >= 0) f(d, t, l);
    }
}

// out[0..m) = v where the caller asked for the table
inline void fill(int32_t *out, int32_t m, int32_t v) {
  if (out) std::fill(out, out + m, v);
}
inline void put(int32_t *out, int32_t i, int32_t v) {
  if (out) out[i] = v;
}

}  // namespace

extern "C" {

int32_t egs_debug_choose_oversize_schedule(int32_t n_patch_tiles, int32_t quad_per_cu, int32_t patch_per_cu,
                                           int32_t cu_count, int32_t patches_enabled, int32_t quad_patches_enabled) {
  return (int32_t)choose_oversize_schedule(n_patch_tiles, quad_per_cu, patch_per_cu, cu_count, patches_enabled != 0,
                                           quad_patches_enabled != 0);
}

egs_status egs_debug_matvec_plan(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, int32_t tile_size,
                                 int32_t *n_tiles, int32_t *n_islands, int32_t *n_shared_bodies, int32_t *n_boundary,
                                 int32_t *cons_tile, int32_t *cons_lane) {
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const MatvecPlan pl = build_matvec_plan(n, m, body0, body1, tile_size);
    if (n_tiles) *n_tiles = pl.n_tiles;
    if (n_islands) *n_islands = pl.n_islands;
    if (n_shared_bodies) *n_shared_bodies = pl.n_shared_bodies;
    if (n_boundary) *n_boundary = (int32_t)pl.boundary.size();
    for_each_constraint_lane(pl.lanes, pl.n_tiles, pl.block, [&](const MvLane &d, int t, int l) {
      put(cons_tile, d.cidx, t);
      put(cons_lane, d.cidx, l);
    });
    return EGS_OK;
  });
}

egs_status egs_debug_plan(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, int32_t tile_size,
                          int32_t *n_islands, int32_t *n_tiles, int32_t *n_global, int32_t *cons_tile,
                          int32_t *pos0, int32_t *cnt0, int32_t *pos1, int32_t *cnt1) {
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, tile_size);
    if (n_islands) *n_islands = pl.n_islands;
    if (n_tiles) *n_tiles = pl.n_tiles;
    if (n_global) *n_global = (int32_t)pl.global.size();
    fill(cons_tile, m, -1);
    auto tickets = [&](const auto &d) {   // LaneDesc and GlobalDesc name them alike
      put(pos0, d.cidx, d.pos0);
      put(cnt0, d.cidx, d.cnt0);
      put(pos1, d.cidx, d.pos1);
      put(cnt1, d.cidx, d.cnt1);
    };
    for_each_constraint_lane(pl.lanes, pl.n_tiles, pl.block, [&](const LaneDesc &d, int t, int) {
      put(cons_tile, d.cidx, t);
      tickets(d);
    });
    for (const GlobalDesc &g : pl.global) tickets(g);
    return EGS_OK;
  });
}

egs_status egs_debug_plan_patches(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, int32_t *n_patches,
                                  int32_t *cons_patch, int32_t *cons_lane, int32_t *remote0, int32_t *remote1) {
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, 256);
    if (n_patches) *n_patches = pl.n_patch_tiles;
    fill(cons_patch, m, -1);
    fill(cons_lane, m, -1);
    fill(remote0, m, 0);
    fill(remote1, m, 0);
    for_each_constraint_lane(pl.patch_lanes, pl.n_patch_tiles, pl.block, [&](const LaneDesc &d, int t, int l) {
      put(cons_patch, d.cidx, t);
      put(cons_lane, d.cidx, l);
      put(remote0, d.cidx, ((d.slot0 & kPrevRemote) ? 1 : 0) | ((d.slot0 & kNextRemote) ? 2 : 0));
      put(remote1, d.cidx, ((d.slot1 & kPrevRemote) ? 1 : 0) | ((d.slot1 & kNextRemote) ? 2 : 0));
    });
    return EGS_OK;
  });
}

egs_status egs_debug_plan_slots(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, int32_t tile_size,
                                int32_t *lane, int32_t *slot0, int32_t *slot1, int32_t *tile_nslots) {
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, tile_size);
    fill(lane, m, -1);
    fill(slot0, m, -1);
    fill(slot1, m, -1);
    fill(tile_nslots, m, -1);
    for_each_constraint_lane(pl.lanes, pl.n_tiles, pl.block, [&](const LaneDesc &d, int t, int l) {
      put(lane, d.cidx, l);
      put(slot0, d.cidx, d.slot0);
      put(slot1, d.cidx, d.slot1);
      put(tile_nslots, d.cidx, pl.tile_nslots[t]);
    });
    return EGS_OK;
  });
}

egs_status egs_debug_plan_timetable(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, int32_t tile_size,
                                    int32_t *level, int32_t *period, int32_t *depth, int32_t *runs) {
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, tile_size, nullptr, tile_size == 0 ? (1 << 30) : 0);
    if (!pl.levels_ok) return EGS_ERR_INVALID;
    if (runs) *runs = pl.runs ? 1 : 0;
    fill(level, m, -1);
    fill(period, m, -1);
    fill(depth, m, -1);
    for_each_constraint_lane(pl.lanes, pl.n_tiles, pl.block, [&](const LaneDesc &d, int t, int l) {
      put(level, d.cidx, pl.lane_level[(size_t)t * pl.block + l]);
      put(period, d.cidx, pl.tile_period[t]);
      put(depth, d.cidx, pl.tile_depth[t]);
    });
    return EGS_OK;
  });
}

egs_status egs_debug_plan_pairable(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, int32_t *pairable) {
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, 256);
    if (pairable) *pairable = pl.pairable ? 1 : 0;
    return EGS_OK;
  });
}

egs_status egs_debug_plan_chained(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, int32_t *chained) {
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, 256);
    if (chained) *chained = pl.chained ? 1 : 0;
    return EGS_OK;
  });
}

egs_status egs_debug_plan_share(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, const double *data,
                                int32_t *share) {
  if (m > 0 && !data) return EGS_ERR_INVALID;
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, 256);
    if (share) *share = plan_shares_normals(pl, data) ? 1 : 0;
    return EGS_OK;
  });
}

egs_status egs_debug_plan_faced(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, int32_t *faced) {
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, 256);
    if (faced) *faced = pl.faced ? 1 : 0;
    return EGS_OK;
  });
}

egs_status egs_debug_plan_face_normals(int32_t n, int32_t m, const int32_t *body0, const int32_t *body1, const double *data,
                                       int32_t *face) {
  if (m > 0 && !data) return EGS_ERR_INVALID;
  return plan_entry(n, m, body0, body1, [&]() -> egs_status {
    const Plan pl = build_plan(n, m, body0, body1, 256);
    if (face) *face = plan_faces_normals(pl, data) ? 1 : 0;
    return EGS_OK;
  });
}

egs_status egs_debug_face_split(int32_t n_tiles, int32_t slots, int32_t depth, int32_t period, int32_t sweeps,
                                int32_t force_tiles, int32_t force_s1, int32_t *split_tiles, int32_t *s1, int32_t *pieces,
                                int32_t *n_pieces) {
  if (n_tiles < 0 || slots <= 0 || sweeps < 0) return EGS_ERR_INVALID;
  try {
    const FaceSplit f = force_tiles >= 0 ? face_split_forced(n_tiles, force_tiles, force_s1, sweeps)
                                         : face_split_policy(n_tiles, slots, depth, period, sweeps);
    if (split_tiles) *split_tiles = f.tiles;
    if (s1) *s1 = f.s1;
    std::vector<FacePiece> list;
    face_piece_list(n_tiles, slots, f, sweeps, list);
    if (n_pieces) *n_pieces = (int32_t)list.size();
    if (pieces)
      for (size_t i = 0; i < list.size(); ++i) {
        pieces[4 * i] = list[i].tile; pieces[4 * i + 1] = list[i].resume;
        pieces[4 * i + 2] = list[i].sweeps; pieces[4 * i + 3] = list[i].kind;
      }
    return EGS_OK;
  } catch (const std::exception &) {
    return EGS_ERR_INVALID;
  }
}

egs_status egs_debug_face_form(int32_t n_tiles, int32_t cus, int32_t depth, int32_t period, int32_t sweeps,
                               int32_t max_slots, int32_t *lean, double *us, int32_t *split, int64_t *lds_bytes) {
  if (n_tiles < 0 || cus <= 0 || sweeps < 0) return EGS_ERR_INVALID;
  const FaceForm f = face_form_policy(n_tiles, cus, depth, period, sweeps);
  if (lean) *lean = f.lean ? 1 : 0;
  if (us) { us[0] = f.us[0]; us[1] = f.us[1]; }
  if (split)
    for (int k = 0; k < 2; ++k) { split[2 * k] = f.split[k].tiles; split[2 * k + 1] = f.split[k].s1; }
  if (lds_bytes) *lds_bytes = max_slots > 0 ? (int64_t)face_lds_bytes(max_slots, true, kFaceLeanTilesPerCu) : 0;
  return EGS_OK;
}

}  // extern "C"
