// engine_lists.h -- the host plumbing every entry point shares, free of HIP: the checks of caller-owned lists (packed
// behind offsets, or strided with counts) and of dims, and the carving of one device block into arrays.  Only standard
// headers and the ABI's codes and records: a plain host compiler builds tests/cpp/engine_lists_check.cpp from it.
#ifndef VH_ENGINE_LISTS_H
#define VH_ENGINE_LISTS_H
#include "../../include/viso_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace vh_engine {

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// n lists packed behind offsets[n + 1]: list s is [offsets[s], offsets[s + 1])
struct ListSpan { int64_t first = 0, end = 0, total = 0, longest = 0; };  // offsets[0], offsets[n], their difference, the longest list
// refuses a null pointer, a negative offsets[0] and a decreasing pair; n = 0 judges offsets[0] alone
inline int32_t check_offsets(const int32_t *offsets, int32_t n, ListSpan &out) {
  out = ListSpan();
  if (!offsets || offsets[0] < 0) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n; s++) {
    if (offsets[s + 1] < offsets[s]) return VH_ERR_INVALID_ARG;
    out.longest = std::max<int64_t>(out.longest, (int64_t)offsets[s + 1] - offsets[s]);
  }
  out.first = offsets[0]; out.end = offsets[std::max(n, 0)]; out.total = out.end - out.first;
  return VH_OK;
}

// n strided lists, list l = counts[l] records at l * stride: refuses a null pointer and a count outside [0, stride]
inline int32_t check_counts(const int32_t *counts, int64_t n, int64_t stride, int32_t &longest) {
  longest = 0;
  if (!counts) return VH_ERR_INVALID_ARG;
  for (int64_t l = 0; l < n; l++) {
    if (counts[l] < 0 || counts[l] > stride) return VH_ERR_INVALID_ARG;
    longest = std::max(longest, counts[l]);
  }
  return VH_OK;
}

// {width, height, bytes per line}: positive sides of at most 16384; need_pitch: a line holds its width
inline int32_t check_dims(const int32_t *dims, bool need_pitch) {
  if (!dims || dims[0] <= 0 || dims[1] <= 0 || (need_pitch && dims[2] < dims[0])) return VH_ERR_INVALID_ARG;
  if (dims[0] > 16384 || dims[1] > 16384) return VH_ERR_UNSUPPORTED;
  return VH_OK;
}

// Cuts one block into arrays that each begin on a multiple of 256 bytes, in the order they are taken.  Without a base
// it only measures (ptr gives null), so the size is known before the allocation and the same calls give the pointers after it.
struct Carver {
  uint8_t *base = nullptr;
  size_t next = 0, end = 0;  // where the next array begins / where the last one ends
  explicit Carver(void *b = nullptr) : base((uint8_t *)b) {}
  template <class T> size_t take(size_t count) {  // -> the array's offset
    const size_t o = next;
    end = o + sizeof(T) * count; next = up256(end);
    return o;
  }
  template <class T> T *ptr(size_t count) {
    const size_t o = take<T>(count);
    return base ? (T *)(base + o) : nullptr;
  }
  size_t bytes() const { return next; }  // every array rounded up to 256
  size_t tight() const { return end; }   // the last array as long as it is
};

// The arrays of one classification inside one device block: flags | records | positions | tile counts | counts | ok | tr
struct InlierArrays {
  uint8_t *d_flags = nullptr;   // [slots]
  vh_p_match *d_out = nullptr;  // [slots] the inlier records of each list, in list order
  int32_t *d_src = nullptr;     // [slots] their positions in the list
  int32_t *d_tiles = nullptr;   // [lists][tiles]
  int32_t *d_ninl = nullptr, *d_ok = nullptr;  // [lists]
  double *d_tr = nullptr;       // [lists][6]
  // -> the carver behind them: bytes() is the block's size, further takes lie behind the arrays
  Carver carve(void *base, size_t lists, size_t slots, size_t tiles) {
    Carver c(base);
    d_flags = c.ptr<uint8_t>(slots); d_out = c.ptr<vh_p_match>(slots); d_src = c.ptr<int32_t>(slots);
    d_tiles = c.ptr<int32_t>(lists * tiles); d_ninl = c.ptr<int32_t>(lists); d_ok = c.ptr<int32_t>(lists);
    d_tr = c.ptr<double>(6 * lists);
    return c;
  }
};

}  // namespace vh_engine
#endif
