// vh_wave.h -- the wave-level and workgroup-level building blocks of the kernels, once (device only).
//
// gfx950 runs 64-lane waves and every function here assumes that: the ladders step through 32 .. 1 (or 1 .. 32),
// a ballot is a uint64_t, lane numbers are threadIdx.x & 63 (all kernels are launched with one-dimensional
// workgroups).  A change to any of this is made here and nowhere else.
#ifndef VH_WAVE_H
#define VH_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ int32_t vh_wave_scan(int32_t v) {
  const int32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int32_t d = 1; d < 64; d <<= 1) {
    const int32_t o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// all-reduce sum (int32_t, double): every lane ends with the total.  The butterfly's order of additions is fixed, so
// a double total is the same on every lane and from run to run.
template <class T> __device__ __forceinline__ T vh_wave_sum(T v) {
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ int32_t vh_wave_min(int32_t v) {
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ int32_t vh_wave_max(int32_t v) {
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// 64-bit keys travel as two 32-bit shuffles
__device__ __forceinline__ uint64_t vh_shfl_xor_u64(uint64_t k, int32_t d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int32_t)(uint32_t)k, d), hi = (uint32_t)__shfl_xor((int32_t)(uint32_t)(k >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}
// all-reduce minimum / maximum over every aligned group of WIDTH lanes (a power of two; 64: the wave)
template <int WIDTH = 64> __device__ __forceinline__ uint64_t vh_wave_min_u64(uint64_t k) {
#pragma unroll
  for (int32_t d = WIDTH / 2; d >= 1; d >>= 1) { const uint64_t o = vh_shfl_xor_u64(k, d); k = o < k ? o : k; }
  return k;
}
template <int WIDTH = 64> __device__ __forceinline__ uint64_t vh_wave_max_u64(uint64_t k) {
#pragma unroll
  for (int32_t d = WIDTH / 2; d >= 1; d >>= 1) { const uint64_t o = vh_shfl_xor_u64(k, d); k = o > k ? o : k; }
  return k;
}

// rank of this lane in a ballot mask: the number of set bits below the lane's own (two v_mbcnt; the mask may differ
// from lane to lane, as the peer masks of the radix sort do)
__device__ __forceinline__ int32_t vh_wave_rank(uint64_t mask) {
  return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// One step of an ordered compaction across the four waves of a 256-thread workgroup: pos = kept threads before this
// one (in thread order), total = kept threads of the workgroup.  sWave: int32_t[4] of LDS; w, lane: threadIdx.x >> 6
// and & 63.  Holds ONE __syncthreads (after the wave counts are written): every thread of the workgroup calls it, and
// the caller puts a barrier between its last use of the result and the next call, which rewrites sWave.
struct VhCompact { int32_t pos, total; };
__device__ __forceinline__ VhCompact vh_compact4(bool keep, int32_t *sWave, int32_t w, int32_t lane) {
  const uint64_t bal = __ballot(keep);
  if (lane == 0) sWave[w] = __popcll(bal);
  __syncthreads();
  VhCompact c;
  c.pos = vh_wave_rank(bal);
  c.total = 0;
#pragma unroll
  for (int32_t k = 0; k < 4; k++) { const int32_t x = sWave[k]; c.pos += k < w ? x : 0; c.total += x; }
  return c;
}

#endif
