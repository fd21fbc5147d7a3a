// kernels_ranged.hip -- pass 2 of multi-stage matching: Matcher::matching with use_prior = true.
//
// Stock libviso2 matches a sparse feature set first, turns the surviving sparse matches into a search range per
// statistics bin and stage (engine.hip: prior_statistics), and searches the dense sets inside that range only
// [upstream-recollection; the reference tree keeps the arguments -- stat_bin, stage, use_prior of findMatch,
// src/matcher.cpp:216-218 -- and nothing behind them].  The range a stage searches belongs to the DRIVING feature of the
// circle (its statistics bin, src/matcher.cpp:314-317), not to the query of the stage, so a stage is a function of
// (driver, query) and cannot be one table over all queries as in match_kernel: the whole circle is walked per driver.
//
// Mapping: VH_RANGED_G lanes per driver, stages in sequence.  The lanes of a group share the query of the stage and
// split its candidates: the bins of interest are walked in the reference's order (u-bin outer; the v-bins of a u-bin
// are one contiguous run of bin-order positions), lane g takes positions start + g, start + g + G, ...  The winner is
// the minimum of SAD << 32 | position: ascending position IS the reference's visiting order, so the first strict
// minimum (src/matcher.cpp:264) comes out in any arrival order; no accepted candidate leaves min_ind = 0 (:221).
// The accept window is integer: query + range of the driver's bin, v replaced by +-disp_tolerance in a 1-d stage.
// The kernel writes what chain_kernel writes (index tuple, coordinate tuple, pixel-mask bid, survivors per emission
// chunk), so flow_keep, refine and emit_matches follow unchanged.
#include "vh_dev.h"
#include <algorithm>

#ifndef VH_RANGED_G
#define VH_RANGED_G 8  // lanes per driver (a power of two <= 64)
#endif

namespace {

__device__ __forceinline__ int32_t indexed_count(const VhSets &s, int32_t set) { return s.bin_start[(int64_t)set * (s.nbins + 1) + s.nbins]; }

// findMatch (src/matcher.cpp:216-272) of query `iq` of set `qset` in set `cset`, inside rg = {u_min, u_max, v_min, v_max}
// relative to the query; every lane of the group returns min_ind
__device__ __forceinline__ int32_t find_ranged(const VhSets &s, int32_t qset, int32_t iq, int32_t cset, const int4 rg, bool flow, int32_t disp_tol,
                                               int32_t g) {
  const int64_t cap = s.cap;
  const int32_t *__restrict__ q = s.feat + ((int64_t)qset * cap + iq) * 12;
  const int32_t u1 = q[0], v1 = q[1], c = q[3];
  const uint4 a0 = *(const uint4 *)(q + 4), a1 = *(const uint4 *)(q + 8);
  const int32_t u_lo = u1 + rg.x, u_hi = u1 + rg.y;
  const int32_t v_lo = flow ? v1 + rg.z : v1 - disp_tol, v_hi = flow ? v1 + rg.w : v1 + disp_tol;
  // bins of interest (:237-240); any window, an empty one included, gives 0 <= bin < bin count
  const int32_t ub0 = min(max(u_lo, 0) / s.binsize, s.ubn - 1), ub1 = min(max(u_hi, 0) / s.binsize, s.ubn - 1);
  const int32_t vb0 = min(max(v_lo, 0) / s.binsize, s.vbn - 1), vb1 = min(max(v_hi, 0) / s.binsize, s.vbn - 1);
  const int32_t *__restrict__ cbs = s.bin_start + (int64_t)cset * (s.nbins + 1);
  const uint32_t *__restrict__ cuv = s.s_uv + (int64_t)cset * cap;
  const uint4 *__restrict__ cdesc = (const uint4 *)(s.s_desc + (int64_t)cset * cap * 8);
  unsigned long long key = ~0ull;
  if (vb0 <= vb1) {
    for (int32_t ub = ub0; ub <= ub1; ub++) {
      const int32_t row = (c * s.ubn + ub) * s.vbn;
      const int32_t p1 = cbs[row + vb1 + 1];
      for (int32_t p = cbs[row + vb0] + g; p < p1; p += VH_RANGED_G) {
        const uint32_t uv2 = cuv[p];
        const int32_t u2 = (int32_t)(uv2 & 0xFFFFu), v2 = (int32_t)(uv2 >> 16);
        if (u2 < u_lo || u2 > u_hi || v2 < v_lo || v2 > v_hi) continue;
        const uint4 b0 = cdesc[2 * (int64_t)p], b1 = cdesc[2 * (int64_t)p + 1];
        uint32_t sad = __builtin_amdgcn_sad_u8(a0.x, b0.x, 0);
        sad = __builtin_amdgcn_sad_u8(a0.y, b0.y, sad); sad = __builtin_amdgcn_sad_u8(a0.z, b0.z, sad); sad = __builtin_amdgcn_sad_u8(a0.w, b0.w, sad);
        sad = __builtin_amdgcn_sad_u8(a1.x, b1.x, sad); sad = __builtin_amdgcn_sad_u8(a1.y, b1.y, sad);
        sad = __builtin_amdgcn_sad_u8(a1.z, b1.z, sad); sad = __builtin_amdgcn_sad_u8(a1.w, b1.w, sad);
        const unsigned long long k = ((unsigned long long)sad << 32) | (uint32_t)p;
        key = k < key ? k : key;
      }
    }
  }
#pragma unroll
  for (int32_t d = VH_RANGED_G / 2; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d);
    key = o < key ? o : key;
  }
  return key == ~0ull ? 0 : s.s_idx[(int64_t)cset * cap + (uint32_t)key];
}

// ranges: [row][ubn * vbn][4 stages]{u_min, u_max, v_min, v_max} int32
__global__ void __launch_bounds__(256) ranged_circle_kernel(VhSets s, VhMatchArgs a, int32_t method, const int4 *__restrict__ ranges,
                                                            int4 *__restrict__ chain, uint32_t *__restrict__ mask, uint32_t epoch,
                                                            int32_t *__restrict__ mchunk, int32_t nchm) {
  const int32_t stream = blockIdx.y;
  const int32_t set1p = vh_row_set(a, stream, 0), set2p = vh_row_set(a, stream, 1);
  const int32_t set1c = vh_row_set(a, stream, 2), set2c = vh_row_set(a, stream, 3);
  const int32_t n1p = indexed_count(s, set1p), n2p = indexed_count(s, set2p);
  const int32_t n1c = indexed_count(s, set1c), n2c = indexed_count(s, set2c);
  const int64_t cap = s.cap;
  const uint32_t *__restrict__ uv1p = s.f_uv + (int64_t)set1p * cap, *__restrict__ uv2p = s.f_uv + (int64_t)set2p * cap;
  const uint32_t *__restrict__ uv1c = s.f_uv + (int64_t)set1c * cap, *__restrict__ uv2c = s.f_uv + (int64_t)set2c * cap;
  const int4 *__restrict__ rrow = ranges + (int64_t)stream * (s.ubn * s.vbn) * 4;
  int4 *__restrict__ out = chain + 2 * (int64_t)stream * cap;
  const int32_t ndrive = (method == 2) ? n1p : n1c;
  const uint32_t *__restrict__ uvd = (method == 2) ? uv1p : uv1c;
  const int32_t per_wg = 256 / VH_RANGED_G, g = threadIdx.x % VH_RANGED_G;
  for (int32_t i = blockIdx.x * per_wg + threadIdx.x / VH_RANGED_G; i < ndrive; i += gridDim.x * per_wg) {
    int4 r = make_int4(-1, -1, -2, -1), c = make_int4(0, 0, 0, 0);
    // statistics bin of the driver (src/matcher.cpp:314-317): every stage of its circle searches this bin's ranges
    const uint32_t uvi = uvd[i];
    const int32_t sb = min((int32_t)(uvi >> 16) / s.binsize, s.vbn - 1) * s.ubn + min((int32_t)(uvi & 0xFFFFu) / s.binsize, s.ubn - 1);
    const int4 *__restrict__ rg = rrow + 4 * (int64_t)sb;
    if (method == 0) {
      if (n1p > 0) {
        const int32_t i1p = find_ranged(s, set1c, i, set1p, rg[0], true, a.disp_tol, g);
        const int32_t i1c2 = find_ranged(s, set1p, i1p, set1c, rg[1], true, a.disp_tol, g);
        if (i1c2 == i) {
          r = make_int4(i1p, -1, i, -1);
          c.x = (int32_t)uv1p[i1p]; c.z = (int32_t)uvi;
          if (g == 0)
            atomicMax(&mask[(int64_t)stream * s.W * s.H + (int64_t)(uvi >> 16) * s.W + (uvi & 0xFFFFu)],
                      (epoch << VH_MASK_IDX_BITS) | (((1u << VH_MASK_IDX_BITS) - 1u) - (uint32_t)i));
        }
      }
    } else if (method == 1) {
      if (n2c > 0) {
        const int32_t i2c = find_ranged(s, set1c, i, set2c, rg[0], false, a.disp_tol, g);
        const int32_t i1c2 = find_ranged(s, set2c, i2c, set1c, rg[1], false, a.disp_tol, g);
        c.z = (int32_t)uvi; c.w = (int32_t)uv2c[i2c];
        if (i1c2 == i && (uvi & 0xFFFFu) >= ((uint32_t)c.w & 0xFFFFu)) r = make_int4(-1, -1, i, i2c);
      }
    } else {
      if (n2p > 0 && n1c > 0 && n2c > 0) {
        const int32_t i2p = find_ranged(s, set1p, i, set2p, rg[0], false, a.disp_tol, g);
        const int32_t i2c = find_ranged(s, set2p, i2p, set2c, rg[1], true, a.disp_tol, g);
        const int32_t i1c = find_ranged(s, set2c, i2c, set1c, rg[2], false, a.disp_tol, g);
        const int32_t i1p2 = find_ranged(s, set1c, i1c, set1p, rg[3], true, a.disp_tol, g);
        c = make_int4((int32_t)uvi, (int32_t)uv2p[i2p], (int32_t)uv1c[i1c], (int32_t)uv2c[i2c]);
        const uint32_t u1p = uvi & 0xFFFFu, u2p = (uint32_t)c.y & 0xFFFFu, u1c = (uint32_t)c.z & 0xFFFFu, u2c = (uint32_t)c.w & 0xFFFFu;
        if (i1p2 == i && u1p >= u2p && u1c >= u2c) r = make_int4(i, i2p, i1c, i2c);
      }
    }
    if (g == 0) { out[2 * (int64_t)i] = r; out[2 * (int64_t)i + 1] = c; }
    if (method != 0) {
      // survivors per emission chunk of 256 drivers: the 64 / G drivers of a wave lie in one chunk, one atomic per wave
      const uint64_t bal = __ballot(g == 0 && r.z >= 0);
      if (bal && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(bal)) atomicAdd(mchunk + stream * nchm + (i >> 8), (int32_t)__popcll(bal));
    }
  }
}

}  // namespace

void vh_launch_ranged_circle(const VhSets &s, const VhMatchArgs &a, int32_t method, const int32_t *ranges, int4 *chain, uint32_t *mask,
                             uint32_t epoch, int32_t *mchunk, hipStream_t st) {
  static_assert((VH_RANGED_G & (VH_RANGED_G - 1)) == 0 && VH_RANGED_G >= 1 && VH_RANGED_G <= 64, "lanes per driver");
  const int32_t nchm = (s.cap + 255) / 256;
  const int32_t per_wg = 256 / VH_RANGED_G;
  dim3 grid(std::min(std::max((s.cap + per_wg - 1) / per_wg, 1), 2048), a.rows);
  hipLaunchKernelGGL(ranged_circle_kernel, grid, dim3(256), 0, st, s, a, method, (const int4 *)ranges, chain, mask, epoch, mchunk, nchm);
}
