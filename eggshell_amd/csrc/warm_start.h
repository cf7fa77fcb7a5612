// warm_start.h -- carrying lambda across a contact list that changes (see warm_start.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace egs {

// The start of a solve from the previous step's lambda.  A constraint list is mj permanent joints followed by
// contacts; both contact lists are, ensemble by ensemble, in the collider's order (collide.h: ground contacts by body
// with b0 = -1, then pairs i < j), i.e. sorted by (b0, b1) within an ensemble, so a pair's old contacts are one
// contiguous run.  All device pointers; REAL is the precision lambda, rhs and x0 are held in.
//   old contacts: b0, b1 [m_old], pos (a contact's position, `old_stride` doubles apart), off [n_ens + 1], valid [n_ens]
//   new contacts: b0, b1 [m_new], pos (`new_stride` apart), off [n_ens + 1]
//   rows: old_lambda [mj + m_old][3], new_rhs, x0 [mj + m_new][3], source [mj + m_new]
//   n_ens == 1: the offset tables may be NULL (one ensemble owns everything)
// New contact c of ensemble e:
//   valid[e] == 0                                   x0 = its rhs rows (the default start, Q7), source -2
//   else, among e's old contacts of the same ordered pair (b0, b1), the one with the smallest squared distance
//   between the positions that is <= r2, a tie going to the lowest old index:
//                                                   x0 = its lambda rows, bit for bit, source = its old contact index
//   none                                            x0 = 0, source -1
// Two new contacts may take the same old one.  Joint j of ensemble e: its own previous rows and source j if valid[e],
// else its rhs rows and -2.
template <typename REAL>
struct MatchArgs {
  int32_t n_ens = 1, mj = 0, m_old = 0, m_new = 0;
  const int32_t *joint_off = nullptr, *old_off = nullptr, *new_off = nullptr;
  const uint8_t *valid = nullptr;
  const int32_t *old_b0 = nullptr, *old_b1 = nullptr;
  const double *old_pos = nullptr;
  const REAL *old_lambda = nullptr;
  const int32_t *new_b0 = nullptr, *new_b1 = nullptr;
  const double *new_pos = nullptr;
  const REAL *new_rhs = nullptr;
  int32_t old_stride = 3, new_stride = 3;
  double r2 = 0.0;
  REAL *x0 = nullptr;
  int32_t *source = nullptr;
  // what the solve itself starts from, if asked for: x0, but the rhs rows (exactly 0) for an ensemble that sits this
  // step out (dt[e] == 0, egs_world_step_each) -- its lambda stays 0 while x0 keeps what it holds
  const double *dt = nullptr;   // [n_ens] or NULL
  REAL *start = nullptr;        // [mj + m_new][3] or NULL
};
template <typename REAL>
void launch_match_contacts(const MatchArgs<REAL> &a, hipStream_t s);

// After a successful solve the current list becomes the history: contacts' b0, b1 and positions, every constraint's
// rows lambda[i] = (its ensemble sat the step out: dt[e] == 0) ? x0[i] : x[i], and valid[e] = 1 for every ensemble
// that stepped.  An ensemble that sat out keeps valid[e] and, through x0, the rows it held.  dt == NULL: all stepped.
template <typename REAL>
struct SnapshotArgs {
  int32_t n_ens = 1, mj = 0, mc = 0;
  const int32_t *joint_off = nullptr, *contact_off = nullptr;   // NULL with n_ens == 1
  const double *dt = nullptr;                                   // [n_ens] or NULL
  const int32_t *b0 = nullptr, *b1 = nullptr;                   // the contacts'
  const double *pos = nullptr;
  int32_t stride = 7;
  const REAL *x0 = nullptr, *x = nullptr;                       // [mj + mc][3]; x0 is read for ensembles sitting out only
  int32_t *h_b0 = nullptr, *h_b1 = nullptr;
  double *h_pos = nullptr;                                      // [mc][3]
  REAL *h_lambda = nullptr;                                     // [mj + mc][3]
  uint8_t *valid = nullptr;
};
template <typename REAL>
void launch_warm_snapshot(const SnapshotArgs<REAL> &a, hipStream_t s);

}  // namespace egs
