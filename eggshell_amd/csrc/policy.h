// policy.h -- the host-side schedule policy: which plan and which kernel family a problem of a given shape gets.
// Pure functions of sizes, plan figures and the precision; no HIP, so the plan-inspection entries (plan_debug.cpp)
// can use them without a device.  choose_sweep (solve.cpp) and ensure_tile_plan (problem.cpp) apply them.
#pragma once

#include <algorithm>

#include "../../include/eggshell_amd.h"
#include "plan.h"

namespace egs {

// The 4-lane schedule is the faster one while its tiles are all resident at once (one round): 5 x 64
// constraints per CU in fp64 (94 VGPRs), 8 x 64 in fp32 -- hipOccupancyMaxActiveBlocksPerMultiprocessor
// of the instantiation decides (C3 fp64: 4 piles 0.33 ms against 0.41 on the 1-lane schedule, 6 piles
// 0.53 against 0.45).  No 4-lane plan is built at all beyond the register file's 5 (fp64) / 8 (fp32)
// tiles per CU.
inline int quad_tiles_per_cu_max(int precision) { return precision == EGS_F32 ? 8 : 5; }
constexpr int kBigTileMinConstraints = 196608;   // 768 tiles of 256: from here 512-constraint tiles
// The tile plan's GS / SOR sweep on its static timetable (step_device.h) or on tickets
// (tile_solve_kernel)?  The timetable takes depth + P x sweeps barrier steps, P = the largest level
// span of a body in a tile; the ticket sweep follows the true dependency chains, about
// depth + (largest per-body count) x sweeps updates long.  Regular islands (piles of columns) have
// P = the per-body count and the timetable wins (every lane due at a step shares ONE pass); an
// irregular island can have spans far beyond its counts, then the tickets win.
inline bool timetable_pays(const Plan &pl, int sweeps) {
  const double grp = pl.runs ? 4.0 : 1.0;     // with runs the timetable counts groups of four updates (plan.h)
  const double fixed = grp * ((double)pl.max_depth + (double)pl.max_period * sweeps);
  const double ticket = grp * (double)pl.max_depth + (double)pl.max_cnt * sweeps;
  return fixed <= 1.15 * ticket;
}

// Which kernel takes the oversize islands of a GS / SOR solve.  Patches wait on each other, so
// all of a launch's patches must be co-resident: the limits are occupancy (workgroups per CU of
// the exact kernel instantiation, queried from the runtime) x CUs, never above what was
// measured on MI355X -- one 1024-thread patch (4 lanes per constraint) or two 256-thread
// patches (232 VGPRs) per CU.  A kernel change that lowers occupancy lowers the limit and the
// island falls through to the next schedule instead of stalling.
enum OversizeSchedule { kQuadPatches = 0, kLanePatches = 1, kAllGlobal = 2 };
inline OversizeSchedule choose_oversize_schedule(int n_patch_tiles, int quad_per_cu, int patch_per_cu, int cu_count,
                                                 bool patches_enabled, bool quad_patches_enabled) {
  if (n_patch_tiles <= 0 || !patches_enabled) return kAllGlobal;
  const long quad_cap = (long)std::min(quad_per_cu, 1) * cu_count, lane_cap = (long)std::min(patch_per_cu, 2) * cu_count;
  if (quad_patches_enabled && n_patch_tiles <= quad_cap) return kQuadPatches;
  if (n_patch_tiles <= lane_cap) return kLanePatches;
  return kAllGlobal;
}

// The FACE form of the fused step launch (step_face.hip) runs a 256-constraint tile on 128 threads at up to 256 VGPRs:
// four tiles fit a CU.  Resident tiles per CU it asks for, 3 or 4 (3: by a larger LDS request); measured on MI355X,
// 24 C3 piles (1 536 tiles on 256 CUs: 1 024 + 512 at four, 768 + 768 at three): DESIGN.md section 5.  Measured again
// with the launch split in time (below): at four the 512 are split and the step runs at 52 230 pile-steps/s, at three
// there is no remainder to split and it stays at 48 025.  Four.
constexpr int kFaceTilesPerCu = 4;

// The LEAN form of the same kernels holds the linear w J products alone (step_face.hip: kFaceLeanLin), fits 168 VGPRs and
// so three wavefronts per SIMD: six tiles per CU.  Six tiles share the CU's 160 KiB of LDS, so a tile may ask for 26 KiB
// at most.  A tile's request (bytes): the accumulators (max_slots x 6 doubles) and, lean, behind them the owner's scalars the loops would otherwise reload from
// scratch (kFaceLeanParked doubles per thread, element e of thread i at e x 128 + i); before either, the prologue keeps
// blocks of the first assembly there while the second runs: 27 doubles per thread, lean 26 (one stays in its
// register).  tiles_per_cu 3 / 4 below the form's own count: the request is padded past a quarter resp. a fifth of the
// CU's LDS.  0: a lean tile of that many slots does not fit six to a CU -- the launch keeps the present kernel.
constexpr int kFaceLeanTilesPerCu = 6;
constexpr int kFaceTileThreads = 128;
constexpr int kFaceStaged = 27, kFaceLeanStaged = 26, kFaceLeanParked = 18;
constexpr size_t kCuLdsBytes = 160 * 1024, kFaceLeanLdsMax = 26 * 1024;
inline size_t face_lds_bytes(int max_slots, bool lean, int tiles_per_cu) {
  const size_t acc = (size_t)max_slots * 6, th = kFaceTileThreads;
  size_t lds = (lean ? std::max(acc + kFaceLeanParked * th, kFaceLeanStaged * th) : std::max(acc, kFaceStaged * th)) * sizeof(double);
  if (lean && lds > kFaceLeanLdsMax) return 0;
  if (tiles_per_cu == 3) lds = std::max(lds, kCuLdsBytes / 4 + 1024);
  else if (lean && tiles_per_cu == 4) lds = std::max(lds, kCuLdsBytes / 5 + 1024);
  return lds;
}

// The FACE launch split in time (step_face.hip: pieces).  With n_tiles = k x slots + R, 0 < R <= slots / 2, the last
// round keeps half the resident slots empty or more.  R tiles are then cut after sweep s1: a slot runs
//     a first part (accumulation + sweeps 1 .. s1), then a whole tile        depth + P s1  +  depth + P S   steps
//     a whole tile, then a second part (sweeps s1 + 1 .. S, resumed)         depth + P S   +  depth + P (S - s1 - 1)
// where two rounds walk 2 (depth + P S).  s1 = S / 2 makes the two sequences equal to within one period.  Per slot the
// split saves P (S - s1) steps and adds a second fill (depth) and what a second prologue, the hand-over and tiles that
// no longer walk in step on a CU cost, kFaceSplitPrologueSteps.  Measured on MI355X, 24 C3 piles (depth 64, P 8; a
// block of 4 steps is about 1 us): a prologue and an epilogue take about 25 us (100 steps), and at 100 and at 50 sweeps
// the split launch came out 27 and 28 us (about 110 steps) behind what that alone predicts -- 0.442 against 0.475 ms at
// 100 sweeps, 0.294 against 0.275 at 50.  260 steps with a margin: the split starts at 81 sweeps on such a tile, where
// the saving is 328 steps against 324.  At the headline it is 400, half of P S, against 324.
constexpr int kFaceSplitPrologueSteps = 260;
struct FaceSplit {
  int tiles = 0;   // H: the LAST H tiles of the plan are split; 0: no split
  int s1 = 0;      // ... after this many sweeps, 1 .. S - 1
};
inline FaceSplit face_split_policy(long n_tiles, long slots, int depth, int P, int S) {
  FaceSplit f;
  if (slots <= 0 || n_tiles <= slots || S < 2 || P <= 0) return f;
  const long R = n_tiles % slots;
  if (R == 0 || 2 * R > slots) return f;
  const int s1 = S / 2;
  if ((long)P * (S - s1) <= (long)depth + kFaceSplitPrologueSteps) return f;
  f.tiles = (int)R;
  f.s1 = s1;
  return f;
}

// EGS_STEP_FACE_SPLIT_FORCE=h,s1: the last h tiles (clamped to the tile count) after s1 sweeps, whatever the policy says
inline FaceSplit face_split_forced(long n_tiles, long h, long s1, int S) {
  FaceSplit f;
  if (h <= 0 || s1 < 1 || s1 > S - 1) return f;
  f.tiles = (int)std::min(h, n_tiles);
  f.s1 = (int)s1;
  return f;
}

// One piece of work in the split FACE launch.  Workgroups take pieces in list order (by ticket), so a second part
// comes after its first part in the list.
struct FacePiece {
  int32_t tile, resume, sweeps, kind;   // kind: kFaceWhole, kFaceFirst (publishes the tile), kFaceSecond (waits for it)
};
enum { kFaceWhole = 0, kFaceFirst = 1, kFaceSecond = 2 };
// The list for n_tiles tiles of which the last f.tiles are split after f.s1 of S sweeps: the whole tiles of the full
// rounds; then the first parts spread evenly among the whole tiles that fill the resident slots with them; then the
// remaining whole tiles, which follow the first parts; then the second parts, which follow the first group's tiles.
template <typename VEC>
inline void face_piece_list(int n_tiles, long slots, FaceSplit f, int S, VEC &out) {
  out.clear();
  const int H = std::min(std::max(f.tiles, 0), n_tiles), whole = n_tiles - H;
  const bool split = H > 0 && f.s1 >= 1 && f.s1 < S;
  if (!split) {
    for (int t = 0; t < n_tiles; ++t) out.push_back(FacePiece{t, 0, S, kFaceWhole});
    return;
  }
  // whole tiles that run beside the first parts: what is left of the slots, as far as there are tiles; those before
  // them are the full rounds, those after them follow the first parts
  const long beside = std::min<long>(whole, std::max<long>(slots - H, 0));
  const long later = std::min<long>(whole - beside, H);
  const int lead = (int)(whole - beside - later);
  int t = 0;
  for (; t < lead; ++t) out.push_back(FacePiece{t, 0, S, kFaceWhole});
  // first parts and the `beside` whole tiles, interleaved evenly (whichever dispatch order the slots fill in, a CU gets
  // its share of both)
  long done_f = 0, done_w = 0;
  const long total = H + beside;
  for (long i = 0; i < total; ++i) {
    // first part number done_f is due once (done_f + 1) / H <= (i + 1) / total
    if (done_f < H && (done_w >= beside || done_f * total <= i * (long)H)) {
      out.push_back(FacePiece{whole + (int)done_f, 0, f.s1, kFaceFirst});
      ++done_f;
    } else {
      out.push_back(FacePiece{t++, 0, S, kFaceWhole});
      ++done_w;
    }
  }
  for (; t < whole; ++t) out.push_back(FacePiece{t, 0, S, kFaceWhole});
  for (int h = 0; h < H; ++h) out.push_back(FacePiece{whole + h, 1, S - f.s1, kFaceSecond});
}

// The persistent FACE launch without a split: wherever the tiles take more than one round of the resident slots.  With a
// workgroup per tile the hardware refills freed slots late (32 C3 piles: 0.600 ms where two rounds of 0.237 ms are
// 0.474); `slots` persistent workgroups on the whole-tile list refill themselves.
inline bool face_persist_pays(long n_tiles, long slots) { return slots > 0 && n_tiles > slots; }

// Which FACE form takes a launch: the present kernels on 4 x CUs resident slots or the lean ones on 6 x CUs, each with
// the split (face_split_policy) and the persistence rule applied to its own slot count.  A launch is predicted as the
// busiest slot's work: per piece a fixed part (prologue, epilogue, refill), per block of four steps the form's block
// time with every slot taken, and for a split its kFaceSplitPrologueSteps.  Six lean tiles keep a CU's SIMDs busier than
// four present ones, but not by half: a lean block takes 1.65 times a present one, so the lean form pays only where it
// saves a round (or the split's half round).  At and below 4 x CUs tiles the present form is kept without a prediction.
// The constants (microseconds; MI355X, C3 piles, depth 64, period 8: a tile walks 16 + 2 S blocks), from the `fixed_us`
// and `us_per_sweep` columns of profiles/lean/step1.json:
//   present, 16 piles (four tiles per CU): 1.875 per sweep, 43.1 fixed  ->  0.93 per block, 28 per piece;
//   lean, 24 piles (six tiles per CU):     3.059 per sweep, 71.7 fixed  ->  1.53 per block, 47 per piece.
// Checked against rows of that file it was not fitted to, at 100 sweeps: present, 32 piles (two rounds) 458 predicted,
// 468 .. 486 measured; present, 24 piles (split) 425 and 424 .. 432; lean, 24 piles 377 and 377 .. 393.
// Nobody has measured another depth, period or CU count: there the per-piece part (which holds the prologue's and the
// epilogue's share of a tile of THIS depth) and the block time are an extrapolation.  The guard on 4 x CUs tiles and the
// round arithmetic keep a wrong constant from doing more than choosing the slower of two correct launches.
constexpr double kFaceBlockUs = 0.93, kFacePieceUs = 28.0;
constexpr double kFaceLeanBlockUs = 1.53, kFaceLeanPieceUs = 47.0;
struct FaceForm {
  bool lean = false;
  double us[2] = {0.0, 0.0};   // the predicted launch, present and lean
  FaceSplit split[2];          // ... and the split each form would take
};
inline double face_launch_us(long n_tiles, long slots, int depth, int P, int S, double block_us, double piece_us, FaceSplit &f) {
  f = face_split_policy(n_tiles, slots, depth, P, S);
  if (n_tiles <= 0 || slots <= 0) return 0.0;
  const double tile = (double)depth + (double)P * S;
  const long full = n_tiles / slots, rest = n_tiles % slots;
  double steps = full * tile, pieces = (double)full;
  if (f.tiles > 0) {   // the remainder as half tiles on every slot: the longer half, a second fill and the hand-over
    steps += (double)depth + (double)P * std::max(f.s1, S - f.s1) + kFaceSplitPrologueSteps;
    pieces += 1;
  } else if (rest > 0) {
    steps += tile;
    pieces += 1;
  }
  return pieces * piece_us + steps / 4 * block_us;
}
inline FaceForm face_form_policy(long n_tiles, int cus, int depth, int P, int S) {
  FaceForm r;
  r.us[0] = face_launch_us(n_tiles, (long)cus * kFaceTilesPerCu, depth, P, S, kFaceBlockUs, kFacePieceUs, r.split[0]);
  r.us[1] = face_launch_us(n_tiles, (long)cus * kFaceLeanTilesPerCu, depth, P, S, kFaceLeanBlockUs, kFaceLeanPieceUs, r.split[1]);
  r.lean = n_tiles > (long)cus * kFaceTilesPerCu && r.us[1] < r.us[0];
  return r;
}

// Isotropic bodies, batched work: the register-light tile kernel (no stored B, three
// 256-constraint tiles per CU in fp64, four in fp32) against the regular one (fp64:
// 512-constraint tiles, one per CU; fp32: three 256-constraint tiles).
// Tiles are dispatched in rounds of 3C resp. C, so the better choice depends on how the
// tile count quantises; per-round times (ms, C3 columns, 100 sweeps) measured on MI355X.
inline bool iso_schedule_pays(long m, int cu, int precision) {
  const long t = (m + 255) / 256;                       // 256-constraint tiles
  if (precision == EGS_F32) return t > 3L * cu;         // fp32: 4 instead of 3 tiles per CU (C4: +7 %)
  if (t < 2L * cu) return false;                       // fewer than two tiles per CU: registers are not the limit
  const long full3 = t / (3L * cu), rem3 = t % (3L * cu);
  // (timetable kernels: one / two / three isotropic tiles per CU walk a launch in 0.435 / 0.462 / 0.50 ms, a round of
  //  512-constraint regular tiles in 0.415 ms; the ticket kernels' figures were 0.45 / 0.57 / 0.66 and 0.53 -- same choices)
  const double iso = 0.50 * full3 + (rem3 == 0 ? 0.0 : rem3 <= cu ? 0.435 : rem3 <= 2L * cu ? 0.462 : 0.50);
  const double regular = 0.415 * ((t / 2 + cu - 1) / cu);
  return iso < regular;
}

}  // namespace egs
