// kernels_stats.hip -- computePriorStatistics of multi-stage matching on the device (DESIGN.md section 6,
// "Statistics"; host form: engine.hip: prior_statistics, which this file restates value for value).
//
//   prior_stats   one workgroup of 256 lanes per list.  Minimum and maximum do not depend on the order of the
//                 records, so the lanes take them in any order: every float is mapped to a 32-bit key whose unsigned
//                 order is the float order, and the table [bins][4 stages][2 axes]{min, max} is kept with integer
//                 atomic min / max.  The keys of the two NaN patterns 0xffffffff / 0x00000000 never belong to a finite
//                 value and mark "no observation".  The table lives in LDS while bins * 64 bytes fit VH_STATS_LDS_MAX;
//                 beyond that the keys are kept in the output table itself (one list = one workgroup, so workgroup
//                 barriers order the three phases; the keys are read back with device-scope atomic loads).
//                 A finishing sweep over (bin, stage, axis) widens in float exactly as the host does and writes either
//                 the float table or the integer windows ceil(min) .. floor(max) that ranged_circle_kernel reads.
//
// Built with -ffp-contract=off (Makefile): hi - lo, (20 - d) / 2, lo - h, hi + h round one by one as on the host.
#include "vh_dev.h"
#include "../../include/viso_hip.h"
#include "vh_vote.h"

namespace {

// float -> key with the same order (unsigned compare), and back
__device__ __forceinline__ uint32_t key_of(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

constexpr uint32_t kNoMin = 0xffffffffu, kNoMax = 0u;

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// engine.hip: range_bound
__device__ __forceinline__ int32_t window_bound(float x, bool is_min) {
  const float r = is_min ? ceilf(x) : floorf(x);
  return (int32_t)fminf(fmaxf(r, -1048576.0f), 1048576.0f);
}

// GLOBAL: the keys live in the list's output table; otherwise in dynamic LDS.  WINDOWS: integer windows instead of floats.
template <bool GLOBAL, bool WINDOWS>
__global__ __launch_bounds__(256) void prior_stats_kernel(VhStatsArgs a) {
  extern __shared__ uint32_t lds_keys[];
  const int32_t l = blockIdx.x, tid = threadIdx.x;
  const int32_t nb = a.ubn * a.vbn, nst = a.method == VH_METHOD_QUAD ? 4 : 2;
  uint32_t *out = (uint32_t *)a.out + (int64_t)l * nb * 16;
  uint32_t *keys = GLOBAL ? out : lds_keys;
  int32_t n = a.counts[(int64_t)l * a.count_stride];
  n = n < 0 ? 0 : (n > a.count_cap ? a.count_cap : n);
  // a list the vote refused: no statistics, the full window in every bin (the ranged search is the unranged one then)
  if (a.status) {
    const int32_t st = a.status[(int64_t)l * a.count_stride];
    if (st == VH_VOTE_TRUNCATED || st == VH_VOTE_UNSUPPORTED || st == VH_VOTE_STACK) n = 0;
  }
  for (int32_t k = tid; k < nb * 16; k += 256) keys[k] = (k & 1) ? kNoMax : kNoMin;
  if (GLOBAL) __threadfence();
  __syncthreads();
  const vh_p_match *pm = a.pm + (int64_t)l * a.pm_stride;
  bool bad = false;
  for (int32_t i = tid; i < n; i += 256) {
    // {u1p v1p i1p u2p | v2p i2p u1c v1c | i1c u2c v2c i2c}
    const float4 *q = (const float4 *)(pm + i);
    const float4 w0 = q[0], w1 = q[1], w2 = q[2];
    const float u1p = w0.x, v1p = w0.y, u2p = w0.w, v2p = w1.x, u1c = w1.z, v1c = w1.w, u2c = w2.y, v2c = w2.z;
    float d[8] = {0, 0, 0, 0, 0, 0, 0, 0}, u, v;
    if (a.method == VH_METHOD_FLOW) {
      d[0] = u1p - u1c; d[1] = v1p - v1c; d[2] = u1c - u1p; d[3] = v1c - v1p;
      u = u1c; v = v1c;
    } else if (a.method == VH_METHOD_STEREO) {
      d[0] = u2c - u1c; d[2] = u1c - u2c;
      u = u1c; v = v1c;
    } else {
      d[0] = u2p - u1p; d[2] = u2c - u2p; d[3] = v2c - v2p; d[4] = u1c - u2c; d[6] = u1p - u1c; d[7] = v1p - v1c;
      u = u1p; v = v1p;
    }
    bool fin = finite_f(u) && finite_f(v);
#pragma unroll
    for (int32_t k = 0; k < 8; k++) fin = fin && finite_f(d[k]);  // (the stages a method lacks hold 0)
    if (!fin) { bad = true; continue; }
    const int32_t ub = (int32_t)fminf(fmaxf(floorf(u / a.bs), -1.0f), (float)a.ubn);
    const int32_t vb = (int32_t)fminf(fmaxf(floorf(v / a.bs), -1.0f), (float)a.vbn);
    const int32_t x0 = min(max(ub - 1, 0), a.ubn - 1), x1 = min(max(ub + 1, 0), a.ubn - 1);
    const int32_t y0 = min(max(vb - 1, 0), a.vbn - 1), y1 = min(max(vb + 1, 0), a.vbn - 1);
    uint32_t kd[8];
#pragma unroll
    for (int32_t k = 0; k < 8; k++) kd[k] = key_of(d[k] + 0.0f);  // (-0 -> +0: one key per value)
    for (int32_t y = y0; y <= y1; y++)
      for (int32_t x = x0; x <= x1; x++) {
        uint32_t *r = keys + ((int64_t)y * a.ubn + x) * 16;
#pragma unroll
        for (int32_t k = 0; k < 8; k++)
          if (k < 2 * nst) { atomicMin(r + 2 * k, kd[k]); atomicMax(r + 2 * k + 1, kd[k]); }
      }
  }
  if (bad && a.err) a.err[l] = 1;
  if (GLOBAL) __threadfence();
  __syncthreads();
  // (bin, stage, axis): the pair {min, max} at 2 * item.  The trip count is the same for every lane (barrier inside).
  for (int32_t it0 = 0; it0 < nb * 8; it0 += 256) {
    const int32_t it = it0 + tid;
    const bool live = it < nb * 8;
    const int32_t b = it >> 3, st = (it >> 1) & 3;
    uint32_t kmin = kNoMin, kmax = kNoMax, seen = kNoMin;
    if (live && GLOBAL) {
      seen = __hip_atomic_load(keys + (int64_t)b * 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      kmin = __hip_atomic_load(keys + 2 * (int64_t)it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      kmax = __hip_atomic_load(keys + 2 * (int64_t)it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (live) {
      seen = keys[b * 16]; kmin = keys[2 * it]; kmax = keys[2 * it + 1];
    }
    float lo = -a.R, hi = a.R;
    if (seen != kNoMin && st < nst) {  // (stage 0, axis 0 of a bin is written by every observation)
      lo = float_of(kmin); hi = float_of(kmax);
      const float dd = hi - lo;
      if (dd < 20.0f) { const float h = ceilf((20.0f - dd) / 2.0f); lo -= h; hi += h; }
    }
    if (GLOBAL) __syncthreads();  // an item's bin-mates have read `seen` before the bin's first key is overwritten
    if (!live) continue;
    if (WINDOWS) { ((int32_t *)out)[2 * (int64_t)it] = window_bound(lo, true); ((int32_t *)out)[2 * (int64_t)it + 1] = window_bound(hi, false); }
    else { ((float *)out)[2 * (int64_t)it] = lo; ((float *)out)[2 * (int64_t)it + 1] = hi; }
  }
}

}  // namespace

void vh_launch_prior_stats(const VhStatsArgs &a, int32_t windows, hipStream_t st) {
  if (a.n_lists < 1) return;
  const size_t bytes = sizeof(uint32_t) * 16 * (size_t)a.ubn * (size_t)a.vbn;
  const dim3 grid(a.n_lists), block(256);
  if (bytes <= VH_STATS_LDS_MAX) {
    if (windows) hipLaunchKernelGGL((prior_stats_kernel<false, true>), grid, block, bytes, st, a);
    else hipLaunchKernelGGL((prior_stats_kernel<false, false>), grid, block, bytes, st, a);
  } else {
    if (windows) hipLaunchKernelGGL((prior_stats_kernel<true, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((prior_stats_kernel<true, false>), grid, block, 0, st, a);
  }
}
