// vh_findmatch.h -- the pieces of Matcher::findMatch (reference src/matcher.cpp:216-272) and of the circle rules of
// Matcher::matching that more than one kernel needs, one definition each.  Device code only; included by
// kernels_match.hip (the tile searches), kernels_chain.hip (circles, ranged search, emission), kernels_prior.hip (the
// searches with the prior term) and kernels_refine.hip.  Everything is __forceinline__ and takes its operands as they
// are: a wave-uniform argument stays wave-uniform in the caller.
#ifndef VH_FINDMATCH_H
#define VH_FINDMATCH_H

#include "vh_dev.h"

// features of a set that are in its bin order (the set's true count, s.count, can be larger: capacity)
__device__ __forceinline__ int32_t indexed_count(const VhSets &s, int32_t set) { return s.bin_start[(int64_t)set * (s.nbins + 1) + s.nbins]; }

// ---- SAD of two 32-byte descriptors (matcher.cpp:251-255)
__device__ __forceinline__ uint32_t sad4(uint32_t a, uint32_t b, uint32_t acc) {
  return __builtin_amdgcn_sad_u8(a, b, acc);  // v_sad_u8: 4 byte-wise |a-b| summed into acc
}
__device__ __forceinline__ uint32_t sad4hi(uint32_t a, uint32_t b, uint32_t acc) {
  return __builtin_amdgcn_sad_hi_u8(a, b, acc);  // v_sad_hi_u8: the same sum added at bit 16 of acc
}
// seed + SAD (HI: seed + (SAD << 16)), a chain of eight
template <bool HI = false>
__device__ __forceinline__ uint32_t sad32(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1, uint32_t seed) {
  const auto f = [](uint32_t a, uint32_t b, uint32_t acc) { return HI ? sad4hi(a, b, acc) : sad4(a, b, acc); };
  uint32_t k = f(a0.x, b0.x, seed);
  k = f(a0.y, b0.y, k); k = f(a0.z, b0.z, k); k = f(a0.w, b0.w, k);
  k = f(a1.x, b1.x, k); k = f(a1.y, b1.y, k); k = f(a1.z, b1.z, k); k = f(a1.w, b1.w, k);
  return k;
}

// ---- search window and accept test (matcher.cpp:231-234, :249)
// Packed 16-bit form for a window of +-ru, +-rv around the query: with t = (u2, v2) - (u_lo, v_lo) (mod 2^16 per half),
// the candidate is inside the window iff t.u <= 2 * ru and t.v <= 2 * rv, i.e. iff min(t, span) == t.  Exact because
// coordinates are < 2^14 and radii <= 2^14 (|u2 - u1| + r < 2^15).  Coordinates travel as u | v << 16.
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ us2 as_us2(uint32_t x) { return __builtin_bit_cast(us2, x); }
__device__ __forceinline__ uint32_t as_u32(us2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ us2 window_lo2(uint32_t uv1, int32_t ru, int32_t rv) { return as_us2(uv1) - us2{(unsigned short)ru, (unsigned short)rv}; }
__device__ __forceinline__ us2 window_span2(int32_t ru, int32_t rv) { return us2{(unsigned short)(2 * ru), (unsigned short)(2 * rv)}; }
__device__ __forceinline__ bool outside_window(uint32_t uv2, us2 lo2, us2 span2) {
  const us2 t = as_us2(uv2) - lo2;
  return as_u32(t) != as_u32(__builtin_elementwise_min(t, span2));
}
// The literal form, for windows that are not symmetric around the query or may be empty (ranged search) and for the
// one-lane searches that mirror the reference line by line.
struct VhWindow { int32_t u_lo, u_hi, v_lo, v_hi; };
__device__ __forceinline__ bool outside_window(uint32_t uv2, const VhWindow &w) {
  const int32_t u2 = (int32_t)(uv2 & 0xFFFFu), v2 = (int32_t)(uv2 >> 16);
  return u2 < w.u_lo || u2 > w.u_hi || v2 < w.v_lo || v2 > w.v_hi;
}

// ---- bins of interest (matcher.cpp:237-240)
// For x < 0 the clamp to 0 makes the truncating division equivalent to the reference's floor.  __umulhi(x, inv_binsize)
// is x / binsize for 0 <= x < 2^18 and never below it for larger x, where both exceed every bin count: after the clamp
// the two are equal for any x.
__device__ __forceinline__ int32_t bin_of(const VhSets &s, int32_t x, int32_t nb) {
  const uint32_t xx = (uint32_t)max(x, 0);
  return min((int32_t)(s.binsize == 1 ? xx : __umulhi(xx, s.inv_binsize)), nb - 1);
}
// any window, an empty one included, gives 0 <= bin < bin count
struct VhBins { int32_t ub0, ub1, vb0, vb1; };
__device__ __forceinline__ VhBins bins_of_interest(const VhSets &s, const VhWindow &w) {
  return VhBins{bin_of(s, w.u_lo, s.ubn), bin_of(s, w.u_hi, s.ubn), bin_of(s, w.v_lo, s.vbn), bin_of(s, w.v_hi, s.vbn)};
}

// ---- first-writer pixel mask of the flow method (matcher.cpp:331-334)
// Every closing feature bids for its pixel with atomicMax(epoch << 24 | (2^24 - 1 - i1c)); the lowest i1c of this
// epoch wins, and no clearing between frames is needed.
__device__ __forceinline__ uint32_t mask_bid(uint32_t epoch, int32_t i) {
  return (epoch << VH_MASK_IDX_BITS) | (((1u << VH_MASK_IDX_BITS) - 1u) - (uint32_t)i);
}
template <class T>
__device__ __forceinline__ T *mask_cell(const VhSets &s, T *mask, int32_t stream, uint32_t uv) {
  return mask + ((int64_t)stream * s.W * s.H + (int64_t)(uv >> 16) * s.W + (uv & 0xFFFFu));
}

// Survivors per emission chunk: one atomic per wave (the lanes of a wave hold features of one 256-feature chunk), not
// one per lane -- 64 same-address atomics per wave made the chain kernel 8x slower.  `keep` carries whatever else
// decides that a lane counts (the ranged circle: one lane per driver).
__device__ __forceinline__ void count_chunk(bool keep, int32_t *counter) {
  const uint64_t bal = __ballot(keep);
  if (bal && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(bal)) atomicAdd(counter, (int32_t)__popcll(bal));
}

#endif
