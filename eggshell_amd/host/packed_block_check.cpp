// packed_block_check.cpp -- csrc/packed_block.h on the CPU, under AddressSanitizer and UBSan: the section lists of its
// three users (mixed_batch.hip, dantzig.hip, dense_iter.hip) rebuilt from the same counts, with stand-ins of the same
// size and alignment for their structs.  For every list: each section inside its zone, aligned, overlapping no other;
// the download zone [0, download_bytes()); the upload zone one range behind it; and a round trip through a host block
// of exactly host_bytes() and a "device" block of exactly total_bytes(), so that one byte too many on either side is a
// sanitizer report.  The caller's batch has a decoy problem in front and one behind; sel takes the listed sizes in
// reverse, so it is neither the identity nor the whole batch.  The dense iteration takes every problem of its call in
// order and copies its vectors whole; here its block goes through the same gather and scatter as the other two.
// Built by `make packed_block_check`, run by tests/test_packed_block_cpu.py.  Needs no device and no library.
#include "../csrc/packed_block.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace egs;

namespace {

int g_checks = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    ++g_checks;                                                                            \
    if (!(cond)) { std::printf("%s:%d: FAILED %s  [%s]\n", __FILE__, __LINE__, #cond, g_what.c_str()); std::exit(1); } \
  } while (0)
std::string g_what;

// as MixedBatchProblem, MixedBatchOut, MixedFrictionOut (mixed_batch.hip), LcpResult (dantzig.hip), DenseIterOut and
// DenseIterProblem (dense_iter.hip)
struct MixedProblem { int64_t a_off, v_off, ws_off; int32_t n, pad; };
struct MixedOut { int32_t ok, pivots; };
struct FrictionOut { int32_t outer, pad; double change; };
struct LcpResult { int32_t ok, pivots, reason, pad; };
struct IterOut { double residual; int32_t iterations, pad; };
struct IterProblem { int64_t a_off, v_off; int32_t n, pad; };

// a PackedBlock that remembers what was asked of it
struct Recorded {
  struct Rec { Zone zone; size_t offset, bytes, align; };
  PackedBlock blk;
  std::vector<Rec> recs;
  template <class T>
  Section<T> add(Zone zone, size_t count, size_t align = alignof(T)) {
    const Section<T> s = blk.add<T>(zone, count, align);
    CHECK(s.count == count && s.end() == s.offset + count * sizeof(T));
    recs.push_back(Rec{zone, s.offset, count * sizeof(T), std::max(align, alignof(T))});
    return s;
  }
  void verify() const {     // (a), (b), (c)
    const size_t lo[3] = {0, blk.upload_begin(), blk.upload_end()};
    const size_t hi[3] = {blk.download_bytes(), blk.upload_end(), blk.total_bytes()};
    CHECK(blk.download_bytes() <= blk.upload_begin() && blk.upload_begin() <= blk.upload_end());
    CHECK(blk.host_bytes() == blk.upload_end() && blk.upload_end() <= blk.total_bytes());
    size_t zone_end[3] = {0, blk.upload_begin(), blk.upload_end()};
    bool first_download = true;
    for (size_t i = 0; i < recs.size(); ++i) {
      const Rec &r = recs[i];
      const int z = (int)r.zone;
      CHECK(r.offset % r.align == 0);
      CHECK(r.offset >= lo[z] && r.offset + r.bytes <= hi[z]);
      if (z == 0 && first_download) { CHECK(r.offset == 0); first_download = false; }
      zone_end[z] = std::max(zone_end[z], r.offset + r.bytes);
      for (size_t j = 0; j < i; ++j)
        CHECK(r.bytes == 0 || recs[j].bytes == 0 || r.offset >= recs[j].offset + recs[j].bytes || recs[j].offset >= r.offset + r.bytes);
    }
    CHECK(zone_end[0] == blk.download_bytes());      // the zones end with their last section: nothing else is copied
    CHECK(zone_end[1] == blk.upload_end() && zone_end[2] == blk.total_bytes());
  }
};

// the caller's packed batch: a decoy, the listed sizes, a decoy; the fused problems are the listed ones in reverse
struct Caller {
  std::vector<int32_t> n, sel;
  std::vector<int64_t> a_off, v_off;
  size_t at = 0, vt = 0;
  explicit Caller(const std::vector<int> &sizes) {
    n.push_back(2);
    n.insert(n.end(), sizes.begin(), sizes.end());
    n.push_back(3);
    for (const int32_t nk : n) { a_off.push_back((int64_t)at); v_off.push_back((int64_t)vt); at += (size_t)nk * nk; vt += nk; }
    for (size_t f = 0; f < sizes.size(); ++f) sel.push_back((int32_t)(sizes.size() - f));
  }
  int count() const { return (int)sel.size(); }
  bool selected(int k) const { return k >= 1 && k + 1 < (int)n.size(); }
};

template <class T>
std::vector<T> ramp(size_t count, int salt) {
  std::vector<T> v(count);
  for (size_t i = 0; i < count; ++i) v[i] = (T)((i * 7 + (size_t)salt) % 113);
  return v;
}
constexpr double kSentinel = -77.5;
constexpr int32_t kSentinelInt = -4242;

// the two blocks, of exactly the sizes the layout states
struct Blocks {
  char *host, *device;
  explicit Blocks(PackedBlock &blk)
      : host(static_cast<char *>(std::malloc(blk.host_bytes()))), device(static_cast<char *>(std::malloc(blk.total_bytes()))) {
    CHECK(host && device);
    std::memset(host, 0xA5, blk.host_bytes());
    std::memset(device, 0x5A, blk.total_bytes());
    blk.bind(host, device);
  }
  ~Blocks() { std::free(host); std::free(device); }
  void upload(size_t from, size_t to) { std::memcpy(device + from, host + from, to - from); }
  void download(size_t bytes) { std::memcpy(host, device, bytes); }
};

void mixed_layout(const std::vector<int> &sizes, bool pyramid, bool want_beta) {
  g_what = "mixed, " + std::to_string(sizes.size()) + " problems from n = " + std::to_string(sizes[0]) + (pyramid ? ", pyramid" : "") +
           (want_beta ? "" : ", beta NULL");
  const Caller c(sizes);
  const int count = c.count();
  const std::vector<double> A = ramp<double>(c.at, 1), b = ramp<double>(c.vt, 2), lo = ramp<double>(c.vt, 3), hi = ramp<double>(c.vt, 4),
                            mu = ramp<double>(c.vt, 5);
  const std::vector<uint8_t> C = ramp<uint8_t>(c.vt, 6);
  const std::vector<int32_t> nrow = ramp<int32_t>(c.vt, 7);
  std::vector<double> x(c.vt, kSentinel), w(c.vt, kSentinel), beta(c.vt, kSentinel), change(c.n.size(), kSentinel);
  std::vector<int32_t> ok(c.n.size(), kSentinelInt), pivots(c.n.size(), kSentinelInt), outer(c.n.size(), kSentinelInt);
  // the counts of mixed_constraints_fused
  std::vector<MixedProblem> prob((size_t)count);
  size_t at = 0, vt = 0, wt = 0;
  for (int f = 0; f < count; ++f) {
    const size_t nk = (size_t)c.n[c.sel[f]];
    prob[f] = MixedProblem{(int64_t)at, (int64_t)vt, (int64_t)wt, (int32_t)nk, 0};
    at += nk * nk; vt += nk;
    if (nk > 64) wt += nk * nk;
  }
  const size_t nc = (size_t)count, fv = pyramid ? vt : 0, fc = pyramid ? nc : 0;
  Recorded r;
  const auto s_x = r.add<double>(Zone::Download, vt), s_w = r.add<double>(Zone::Download, vt), s_beta = r.add<double>(Zone::Download, fv);
  const auto s_fout = r.add<FrictionOut>(Zone::Download, fc);
  const auto s_out = r.add<MixedOut>(Zone::Download, nc);
  const auto s_A = r.add<double>(Zone::Upload, at, 16), s_b = r.add<double>(Zone::Upload, vt), s_lo = r.add<double>(Zone::Upload, vt),
             s_hi = r.add<double>(Zone::Upload, vt), s_mu = r.add<double>(Zone::Upload, fv);
  const auto s_prob = r.add<MixedProblem>(Zone::Upload, nc);
  const auto s_list = r.add<int32_t>(Zone::Upload, nc), s_nrow = r.add<int32_t>(Zone::Upload, fv);
  const auto s_C = r.add<uint8_t>(Zone::Upload, vt);
  const auto s_ws = r.add<double>(Zone::Scratch, wt, 16);
  r.verify();
  CHECK(s_A.offset % 16 == 0 && s_ws.offset % 16 == 0);
  PackedBlock &blk = r.blk;
  Blocks mem(blk);
  const auto rows = [&](int f) { return (size_t)prob[f].n; };
  const auto entries = [&](int f) { return (size_t)prob[f].n * (size_t)prob[f].n; };
  const auto a_at = [&](int f) { return (size_t)prob[f].a_off; };
  const auto v_at = [&](int f) { return (size_t)prob[f].v_off; };
  gather_ragged(blk.host(s_A), A.data(), count, c.sel.data(), c.a_off.data(), entries, a_at);
  gather_ragged(blk.host(s_b), b.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  gather_ragged(blk.host(s_lo), lo.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  gather_ragged(blk.host(s_hi), hi.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  gather_ragged(blk.host(s_C), C.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  if (pyramid) {
    gather_ragged(blk.host(s_mu), mu.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
    gather_ragged(blk.host(s_nrow), nrow.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  }
  std::copy(prob.begin(), prob.end(), blk.host(s_prob));
  for (int f = 0; f < count; ++f) blk.host(s_list)[f] = count - 1 - f;
  mem.upload(blk.upload_begin(), blk.upload_end());
  // the kernel's stand-in: everything through the device pointers
  for (int g = 0; g < count; ++g) {
    const int p = blk.device(s_list)[g];
    const MixedProblem P = blk.device(s_prob)[p];
    const double *dA = blk.device(s_A) + P.a_off;
    double *ws = blk.device(s_ws) + P.ws_off;
    for (int i = 0; i < P.n; ++i) {
      const size_t v = (size_t)P.v_off + i;
      double row = 0.0;
      for (int j = 0; j < P.n; ++j) row += dA[(size_t)i * P.n + j];
      if (P.n > 64) for (int j = 0; j < P.n; ++j) ws[(size_t)i * P.n + j] = row;
      blk.device(s_x)[v] = row + blk.device(s_b)[v];
      blk.device(s_w)[v] = blk.device(s_lo)[v] * 2.0 + blk.device(s_hi)[v] + blk.device(s_C)[v];
      if (pyramid) blk.device(s_beta)[v] = blk.device(s_mu)[v] + blk.device(s_nrow)[v];
    }
    blk.device(s_out)[p] = MixedOut{P.n, 100 + p};
    if (pyramid) blk.device(s_fout)[p] = FrictionOut{200 + p, 0, 0.5 * p};
  }
  mem.download(blk.download_bytes());
  scatter_ragged(x.data(), blk.host(s_x), count, c.sel.data(), c.v_off.data(), rows, v_at);
  scatter_ragged(w.data(), blk.host(s_w), count, c.sel.data(), c.v_off.data(), rows, v_at);
  if (pyramid && want_beta) scatter_ragged(beta.data(), blk.host(s_beta), count, c.sel.data(), c.v_off.data(), rows, v_at);
  for (int f = 0; f < count; ++f) {
    const int k = c.sel[f];
    ok[k] = blk.host(s_out)[f].ok; pivots[k] = blk.host(s_out)[f].pivots;
    if (pyramid) { outer[k] = blk.host(s_fout)[f].outer; change[k] = blk.host(s_fout)[f].change; }
  }
  for (int k = 0; k < (int)c.n.size(); ++k) {
    const bool in = c.selected(k);
    const int f = (int)sizes.size() - k;     // sel[f] = k
    CHECK(ok[k] == (in ? c.n[k] : kSentinelInt) && pivots[k] == (in ? 100 + f : kSentinelInt));
    CHECK(outer[k] == (in && pyramid ? 200 + f : kSentinelInt) && change[k] == (in && pyramid ? 0.5 * f : kSentinel));
    for (int i = 0; i < c.n[k]; ++i) {
      const size_t v = (size_t)c.v_off[k] + i;
      double row = 0.0;
      for (int j = 0; j < c.n[k]; ++j) row += A[(size_t)c.a_off[k] + (size_t)i * c.n[k] + j];
      CHECK(x[v] == (in ? row + b[v] : kSentinel));
      CHECK(w[v] == (in ? lo[v] * 2.0 + hi[v] + C[v] : kSentinel));
      CHECK(beta[v] == (in && pyramid && want_beta ? mu[v] + nrow[v] : kSentinel));
    }
  }
}

void schur_layout(const std::vector<int> &sizes, bool have_nub, bool want_perm) {
  g_what = "Schur, " + std::to_string(sizes.size()) + " problems from n = " + std::to_string(sizes[0]) + (have_nub ? "" : ", nub NULL") +
           (want_perm ? "" : ", perm NULL");
  const Caller c(sizes);
  const int count = c.count();
  std::vector<double> A = ramp<double>(c.at, 1);
  const std::vector<double> A0 = A, b = ramp<double>(c.vt, 2), lo = ramp<double>(c.vt, 3), hi = ramp<double>(c.vt, 4);
  const std::vector<int32_t> nub = ramp<int32_t>(c.n.size(), 5);
  std::vector<double> x(c.vt, kSentinel), w(c.vt, kSentinel);
  std::vector<int32_t> perm(c.vt, kSentinelInt), ok(c.n.size(), kSentinelInt), nub_out(c.n.size(), kSentinelInt);
  size_t at = 0, vt = 0;
  for (int k = 0; k < count; ++k) { const size_t nk = (size_t)c.n[c.sel[k]]; at += nk * nk; vt += nk; }
  const size_t nc = (size_t)count;
  Recorded r;
  const auto s_x = r.add<double>(Zone::Download, vt), s_w = r.add<double>(Zone::Download, vt);
  const auto s_perm = r.add<int32_t>(Zone::Download, vt);
  const auto s_res = r.add<LcpResult>(Zone::Download, nc, 8);
  const auto s_A = r.add<double>(Zone::Download, at);
  const auto s_b = r.add<double>(Zone::Upload, vt), s_lo = r.add<double>(Zone::Upload, vt), s_hi = r.add<double>(Zone::Upload, vt);
  const auto s_aoff = r.add<int64_t>(Zone::Upload, nc), s_voff = r.add<int64_t>(Zone::Upload, nc);
  const auto s_n = r.add<int32_t>(Zone::Upload, nc), s_nub = r.add<int32_t>(Zone::Upload, nc);
  r.verify();
  PackedBlock &blk = r.blk;
  CHECK(s_A.end() == blk.download_bytes());     // A is read back and uploaded: the last section of the download zone
  CHECK(blk.total_bytes() == blk.host_bytes());
  Blocks mem(blk);
  int64_t *haoff = blk.host(s_aoff), *hvoff = blk.host(s_voff);
  size_t ap = 0, vp = 0;
  for (int k = 0; k < count; ++k) {
    const int j = c.sel[k], nk = c.n[j];
    haoff[k] = (int64_t)ap; hvoff[k] = (int64_t)vp; blk.host(s_n)[k] = nk; blk.host(s_nub)[k] = have_nub ? nub[j] : -1;
    ap += (size_t)nk * nk; vp += nk;
  }
  const auto rows = [&](int k) { return (size_t)c.n[c.sel[k]]; };
  const auto entries = [&](int k) { return (size_t)c.n[c.sel[k]] * (size_t)c.n[c.sel[k]]; };
  const auto a_at = [&](int k) { return (size_t)haoff[k]; };
  const auto v_at = [&](int k) { return (size_t)hvoff[k]; };
  gather_ragged(blk.host(s_A), A.data(), count, c.sel.data(), c.a_off.data(), entries, a_at);
  gather_ragged(blk.host(s_b), b.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  gather_ragged(blk.host(s_lo), lo.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  gather_ragged(blk.host(s_hi), hi.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  mem.upload(s_A.offset, blk.upload_end());
  for (int k = 0; k < count; ++k) {
    const int nk = blk.device(s_n)[k];
    double *dA = blk.device(s_A) + blk.device(s_aoff)[k];
    const size_t v0 = (size_t)blk.device(s_voff)[k];
    for (int i = 0; i < nk; ++i) {
      blk.device(s_x)[v0 + i] = dA[(size_t)i * nk + i] + blk.device(s_b)[v0 + i];
      blk.device(s_w)[v0 + i] = blk.device(s_lo)[v0 + i] - blk.device(s_hi)[v0 + i];
      blk.device(s_perm)[v0 + i] = nk - 1 - i;
      for (int j = 0; j < nk; ++j) dA[(size_t)i * nk + j] += 1000.0;     // "permuted in place"
    }
    blk.device(s_res)[k] = LcpResult{nk, 100 + k, 0, blk.device(s_nub)[k]};
  }
  mem.download(blk.download_bytes());
  scatter_ragged(x.data(), blk.host(s_x), count, c.sel.data(), c.v_off.data(), rows, v_at);
  scatter_ragged(w.data(), blk.host(s_w), count, c.sel.data(), c.v_off.data(), rows, v_at);
  if (want_perm) scatter_ragged(perm.data(), blk.host(s_perm), count, c.sel.data(), c.v_off.data(), rows, v_at);
  for (int k = 0; k < count; ++k) {
    const int j = c.sel[k], nk = c.n[j];
    double *Ak = A.data() + c.a_off[j];
    const double *Hk = blk.host(s_A) + haoff[k];
    for (int i = 0; i < nk; ++i) std::memcpy(Ak + (size_t)i * nk, Hk + (size_t)i * nk, (size_t)(i + 1) * sizeof(double));
    ok[j] = blk.host(s_res)[k].ok; nub_out[j] = blk.host(s_res)[k].pad;
  }
  for (int k = 0; k < (int)c.n.size(); ++k) {
    const bool in = c.selected(k);
    const int nk = c.n[k];
    CHECK(ok[k] == (in ? nk : kSentinelInt) && nub_out[k] == (in ? (have_nub ? nub[k] : -1) : kSentinelInt));
    for (int i = 0; i < nk; ++i) {
      const size_t v = (size_t)c.v_off[k] + i, a = (size_t)c.a_off[k] + (size_t)i * nk;
      CHECK(x[v] == (in ? A0[a + i] + b[v] : kSentinel) && w[v] == (in ? lo[v] - hi[v] : kSentinel));
      CHECK(perm[v] == (in && want_perm ? nk - 1 - i : kSentinelInt));
      for (int j = 0; j < nk; ++j) CHECK(A[a + j] == A0[a + j] + (in && j <= i ? 1000.0 : 0.0));     // the lower triangle only
    }
  }
}

void iterate_layout(const std::vector<int> &sizes, bool history, int max_iters) {
  g_what = "dense iteration, " + std::to_string(sizes.size()) + " problems from n = " + std::to_string(sizes[0]) + (history ? ", history" : "");
  const Caller c(sizes);
  const int count = c.count();
  const size_t hlen = (size_t)max_iters + 1;
  const std::vector<double> A = ramp<double>(c.at, 1), b = ramp<double>(c.vt, 2), lo = ramp<double>(c.vt, 3), hi = ramp<double>(c.vt, 4);
  const std::vector<uint8_t> C = ramp<uint8_t>(c.vt, 6);
  std::vector<double> x(c.vt, kSentinel), residual(c.n.size(), kSentinel), hist(c.n.size() * hlen, kSentinel);
  std::vector<int32_t> iterations(c.n.size(), kSentinelInt);
  // the counts of dense_iterate_batch: every matrix at an even offset, the problems with rows in the index list
  std::vector<IterProblem> prob((size_t)count);
  std::vector<int32_t> list;
  size_t vt = 0, dat = 0;
  for (int f = 0; f < count; ++f) {
    const size_t nk = (size_t)c.n[c.sel[f]];
    prob[f] = IterProblem{(int64_t)dat, (int64_t)vt, (int32_t)nk, 0};
    if (nk) list.push_back(f);
    vt += nk; dat += (nk * nk + 1) & ~size_t(1);
  }
  const size_t nc = (size_t)count;
  Recorded r;
  const auto s_x = r.add<double>(Zone::Download, vt);
  const auto s_out = r.add<IterOut>(Zone::Download, nc);
  const auto s_hist = r.add<double>(Zone::Download, history ? nc * hlen : 0);
  const auto s_A = r.add<double>(Zone::Upload, dat, 16), s_b = r.add<double>(Zone::Upload, vt), s_lo = r.add<double>(Zone::Upload, vt),
             s_hi = r.add<double>(Zone::Upload, vt);
  const auto s_prob = r.add<IterProblem>(Zone::Upload, nc);
  const auto s_sel = r.add<int32_t>(Zone::Upload, list.size());
  const auto s_C = r.add<uint8_t>(Zone::Upload, vt);
  r.verify();
  CHECK(s_A.offset % 16 == 0);
  PackedBlock &blk = r.blk;
  CHECK(blk.total_bytes() == blk.host_bytes());
  Blocks mem(blk);
  const auto rows = [&](int f) { return (size_t)prob[f].n; };
  const auto entries = [&](int f) { return (size_t)prob[f].n * (size_t)prob[f].n; };
  const auto a_at = [&](int f) { return (size_t)prob[f].a_off; };
  const auto v_at = [&](int f) { return (size_t)prob[f].v_off; };
  gather_ragged(blk.host(s_A), A.data(), count, c.sel.data(), c.a_off.data(), entries, a_at);
  for (int f = 0; f < count; ++f)
    if (entries(f) & 1) blk.host(s_A)[a_at(f) + entries(f)] = 0.0;
  gather_ragged(blk.host(s_b), b.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  gather_ragged(blk.host(s_lo), lo.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  gather_ragged(blk.host(s_hi), hi.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  gather_ragged(blk.host(s_C), C.data(), count, c.sel.data(), c.v_off.data(), rows, v_at);
  std::copy(prob.begin(), prob.end(), blk.host(s_prob));
  std::copy(list.begin(), list.end(), blk.host(s_sel));
  mem.upload(blk.upload_begin(), blk.upload_end());
  for (size_t g = 0; g < list.size(); ++g) {
    const int p = blk.device(s_sel)[g];
    const IterProblem P = blk.device(s_prob)[p];
    CHECK(P.a_off % 2 == 0);
    const double *dA = blk.device(s_A) + P.a_off;
    double sum = 0.0;
    for (int i = 0; i < P.n; ++i) {
      const size_t v = (size_t)P.v_off + i;
      blk.device(s_x)[v] = dA[(size_t)i * P.n + (P.n - 1)] + blk.device(s_b)[v] + blk.device(s_lo)[v] * 2.0 + blk.device(s_hi)[v] * 3.0 + blk.device(s_C)[v];
      sum += dA[(size_t)i * P.n];
    }
    if ((P.n * P.n) & 1) sum += dA[(size_t)P.n * P.n];     // the padding the small kernel's paired loads may touch
    blk.device(s_out)[p] = IterOut{sum, 100 + p, 0};
    if (history) for (size_t s = 0; s < hlen; ++s) blk.device(s_hist)[(size_t)p * hlen + s] = sum + (double)s;
  }
  mem.download(blk.download_bytes());
  scatter_ragged(x.data(), blk.host(s_x), count, c.sel.data(), c.v_off.data(), rows, v_at);
  for (int f = 0; f < count; ++f) {
    if (!prob[f].n) continue;          // not launched
    const int k = c.sel[f];
    iterations[k] = blk.host(s_out)[f].iterations; residual[k] = blk.host(s_out)[f].residual;
    if (history) std::memcpy(hist.data() + (size_t)k * hlen, blk.host(s_hist) + (size_t)f * hlen, hlen * sizeof(double));
  }
  for (int k = 0; k < (int)c.n.size(); ++k) {
    const int nk = c.n[k];
    const bool in = c.selected(k) && nk > 0;
    const int f = (int)sizes.size() - k;
    double sum = 0.0;
    for (int i = 0; i < nk; ++i) {
      const size_t v = (size_t)c.v_off[k] + i, a = (size_t)c.a_off[k] + (size_t)i * nk;
      CHECK(x[v] == (in ? A[a + nk - 1] + b[v] + lo[v] * 2.0 + hi[v] * 3.0 + C[v] : kSentinel));
      sum += A[a];
    }
    CHECK(iterations[k] == (in ? 100 + f : kSentinelInt) && residual[k] == (in ? sum : kSentinel));
    for (size_t s = 0; s < hlen; ++s) CHECK(hist[(size_t)k * hlen + s] == (in && history ? sum + (double)s : kSentinel));
  }
}

void out_of_order_add_throws() {     // (d)
  g_what = "order of the zones";
  const Zone zones[3] = {Zone::Download, Zone::Upload, Zone::Scratch};
  for (int later = 1; later < 3; ++later)
    for (int earlier = 0; earlier < later; ++earlier) {
      PackedBlock blk;
      blk.add<double>(zones[later], 3);
      bool threw = false;
      try { blk.add<int32_t>(zones[earlier], 1); } catch (const std::logic_error &) { threw = true; }
      CHECK(threw);
      const size_t before = blk.total_bytes();
      blk.add<double>(zones[later], 0);          // the refused call changed nothing; the same zone again is fine
      CHECK(blk.total_bytes() == before);
    }
  PackedBlock blk;                               // an upload zone without sections starts where the download zone ends
  blk.add<uint8_t>(Zone::Download, 5);
  CHECK(blk.upload_begin() == 5 && blk.upload_end() == 5 && blk.host_bytes() == 5);
  const auto s = blk.add<double>(Zone::Scratch, 2, 16);
  CHECK(s.offset == 16 && blk.total_bytes() == 32 && blk.host_bytes() == 5);
}

}  // namespace

int main() {
  out_of_order_add_throws();
  const std::vector<std::vector<int>> shared = {{1}, {3, 1, 2}};
  std::vector<std::vector<int>> mixed = shared, schur = shared, iterate = shared;
  mixed.push_back({1, 32, 33, 64, 65, 112});
  schur.push_back({1, 96});
  iterate.push_back({0, 1, 96, 97});
  for (const auto &sizes : mixed) {
    mixed_layout(sizes, false, true);
    mixed_layout(sizes, true, true);
    mixed_layout(sizes, true, false);
  }
  for (const auto &sizes : schur)
    for (int have_nub = 0; have_nub < 2; ++have_nub)
      for (int want_perm = 0; want_perm < 2; ++want_perm) schur_layout(sizes, have_nub != 0, want_perm != 0);
  for (const auto &sizes : iterate) {
    iterate_layout(sizes, false, 5);
    iterate_layout(sizes, true, 5);
    iterate_layout(sizes, true, 0);
  }
  std::printf("packed_block_check: ok (%d checks)\n", g_checks);
  return 0;
}
