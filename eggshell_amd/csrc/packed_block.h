// packed_block.h -- the one packed block of the fused batch pipelines (mixed_batch.hip, dantzig.hip, dense_iter.hip):
// the same byte layout in page-locked host memory and in one device allocation, so that a call is one upload, its
// launches and one read-back.  Host only and free of HIP: host/packed_block_check.cpp runs every user's section list
// on the CPU under the sanitizers.
//
// Three zones in this order, each one contiguous range:
//   download  written by the device and read back:    [0, download_bytes())
//   upload    written by the host, copied to the device: [upload_begin(), upload_end())
//   scratch   device only: up to total_bytes(); the host block ends at host_bytes() = upload_end()
// A section the device rewrites in place (the Schur matrix) goes LAST in the download zone and its user uploads from
// that section's offset: the one upload then still covers one range that ends at upload_end().
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>

namespace egs {

enum class Zone { Download = 0, Upload = 1, Scratch = 2 };

template <class T>
struct Section {
  size_t offset = 0, count = 0;      // bytes from the block's start, elements
  size_t end() const { return offset + count * sizeof(T); }
};

class PackedBlock {
 public:
  // appends `count` elements of T at the next offset that is a multiple of max(align, alignof(T)); a section of no
  // elements is legal.  A zone earlier than the last one added to: std::logic_error.
  template <class T>
  Section<T> add(Zone zone, size_t count, size_t align = alignof(T)) {
    if ((int)zone < (int)zone_) throw std::logic_error("PackedBlock: a section added to an earlier zone");
    zone_ = zone;
    const size_t a = std::max(align, alignof(T));
    const Section<T> s{(end_[2] + a - 1) / a * a, count};
    if (zone == Zone::Upload && !have_upload_) { upload_begin_ = s.offset; have_upload_ = true; }
    for (int z = (int)zone; z < 3; ++z) end_[z] = s.end();
    return s;
  }
  size_t download_bytes() const { return end_[0]; }
  size_t upload_begin() const { return have_upload_ ? upload_begin_ : end_[0]; }
  size_t upload_end() const { return end_[1]; }
  size_t host_bytes() const { return end_[1]; }
  size_t total_bytes() const { return end_[2]; }

  // host: host_bytes() of page-locked memory, device: total_bytes(), both aligned to the widest section
  void bind(char *host, char *device) { host_ = host; device_ = device; }
  template <class T> T *host(const Section<T> &s) const { return reinterpret_cast<T *>(host_ + s.offset); }
  template <class T> T *device(const Section<T> &s) const { return reinterpret_cast<T *>(device_ + s.offset); }

 private:
  Zone zone_ = Zone::Download;
  size_t end_[3] = {0, 0, 0};        // of each zone so far; a zone not reached yet ends where the one before it does
  size_t upload_begin_ = 0;
  bool have_upload_ = false;
  char *host_ = nullptr, *device_ = nullptr;
};

// The ragged gather of a batch: fused problem f is problem sel[f] of the caller's packed array `src`, its len(f)
// elements start at src + off[sel[f]] and go to block + at(f).  scatter_ragged is the inverse.
template <class T, class Len, class At>
void gather_ragged(T *block, const T *src, int count, const int32_t *sel, const int64_t *off, Len len, At at) {
  for (int f = 0; f < count; ++f)
    if (const size_t m = len(f)) std::memcpy(block + at(f), src + off[sel[f]], m * sizeof(T));
}
template <class T, class Len, class At>
void scatter_ragged(T *dst, const T *block, int count, const int32_t *sel, const int64_t *off, Len len, At at) {
  for (int f = 0; f < count; ++f)
    if (const size_t m = len(f)) std::memcpy(dst + off[sel[f]], block + at(f), m * sizeof(T));
}

}  // namespace egs
