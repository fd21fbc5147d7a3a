// kernels_chain.hip -- the circle-match compositions of Matcher::matching (reference src/matcher.cpp:274-344) and the
// emission of their results on gfx950.
//
// A circle is a sequence of findMatch hops that has to return to the driving feature.  What a hop IS differs:
//  * chain_kernel: a look-up in the tables that match_kernel (kernels_match.hip) filled for every query of a pass.
//  * ranged_circle_kernel: pass 2 of multi-stage matching, Matcher::matching with
//    use_prior = true.  Stock libviso2 matches a sparse feature set first, turns the surviving sparse matches into a
//    search range per statistics bin and stage (engine.hip: prior_statistics), and searches the dense sets inside that
//    range only [upstream-recollection; the reference tree keeps the arguments -- stat_bin, stage, use_prior of
//    findMatch, src/matcher.cpp:216-218 -- and nothing behind them].  The range a stage searches belongs to the DRIVING
//    feature of the circle (its statistics bin, src/matcher.cpp:314-317), not to the query of the stage, so a stage is
//    a function of (driver, query) and cannot be one table over all queries: every hop is a search (find_ranged).
// The rules around the hops (circle below) are the same, and both kernels write the same things: index tuple,
// coordinate tuple, pixel-mask bid, survivors per emission chunk.  flow_keep, refine and emit_matches follow either.
#include "vh_findmatch.h"
#include "vh_prior.h"
#include "vh_wave.h"
#include <algorithm>

#ifndef VH_RANGED_G
#define VH_RANGED_G 8  // ranged circle: lanes per driver (a power of two <= 64)
#endif

namespace {

// ---------------------------------------------------------------------- circle
// Follows the circle of driving feature i and records the index tuple (i1p,i2p,i1c,i2c), z = -2 when the circle does
// not close / the disparity test fails, and the coordinate tuple.
//   flow   (matcher.cpp:308-336): 1c ->1p ->1c
//   stereo (stock libviso2): 1c ->2c ->1c, u1c >= u2c
//   quad   (stock libviso2): 1p ->2p ->2c ->1c ->1p,
//                                             u1p >= u2p and u1c >= u2c
// For flow the reference additionally keeps only the FIRST match per pixel of the current image (mask M,
// matcher.cpp:331-334): every closing feature bids for its pixel (mask_bid; flow_keep_kernel reads the winners).
//   hop(stage, query role, query index, candidate role, flow) = min_ind of that findMatch; roles: 0=1p 1=2p 2=1c 3=2c
//   writer: this lane stores for driver i (all lanes of a driver compute the same circle)
struct CircleSets {
  int32_t set[4], n[4];     // per role: set id, indexed count
  const uint32_t *uv[4];    // coordinates in reference order, 4 B per feature (the 48-byte records would cost a 64-byte sector per look-up)
};
__device__ __forceinline__ CircleSets circle_sets(const VhSets &s, const VhMatchArgs &a, int32_t stream) {
  CircleSets cs;
#pragma unroll
  for (int32_t r = 0; r < 4; r++) {
    cs.set[r] = vh_row_set(a, stream, r);
    cs.n[r] = indexed_count(s, cs.set[r]);
    cs.uv[r] = s.f_uv + (int64_t)cs.set[r] * s.cap;
  }
  return cs;
}
template <class Hop>
__device__ __forceinline__ void circle(const VhSets &s, const CircleSets &cs, int32_t method, int32_t stream, int32_t i, bool writer, Hop hop,
                                       int4 *__restrict__ out, uint32_t *__restrict__ mask, uint32_t epoch, int32_t *__restrict__ mchunk) {
  int4 r = make_int4(-1, -1, -2, -1), c = make_int4(0, 0, 0, 0);
  if (method == 0) {
    if (cs.n[0] > 0) {
      const int32_t i1p = hop(0, 2, i, 0, true);
      const int32_t i1c2 = hop(1, 0, i1p, 2, true);
      if (i1c2 == i) {
        r = make_int4(i1p, -1, i, -1);
        c.x = (int32_t)cs.uv[0][i1p]; c.z = (int32_t)cs.uv[2][i];
        if (writer) atomicMax(mask_cell(s, mask, stream, (uint32_t)c.z), mask_bid(epoch, i));
      }
    }
  } else if (method == 1) {
    if (cs.n[3] > 0) {
      const int32_t i2c = hop(0, 2, i, 3, false);
      const int32_t i1c2 = hop(1, 3, i2c, 2, false);
      c.z = (int32_t)cs.uv[2][i]; c.w = (int32_t)cs.uv[3][i2c];
      if (i1c2 == i && ((uint32_t)c.z & 0xFFFFu) >= ((uint32_t)c.w & 0xFFFFu)) r = make_int4(-1, -1, i, i2c);
    }
  } else {
    if (cs.n[1] > 0 && cs.n[2] > 0 && cs.n[3] > 0) {
      const int32_t i2p = hop(0, 0, i, 1, false);
      const int32_t i2c = hop(1, 1, i2p, 3, true);
      const int32_t i1c = hop(2, 3, i2c, 2, false);
      const int32_t i1p2 = hop(3, 2, i1c, 0, true);
      c = make_int4((int32_t)cs.uv[0][i], (int32_t)cs.uv[1][i2p], (int32_t)cs.uv[2][i1c], (int32_t)cs.uv[3][i2c]);
      const uint32_t u1p = (uint32_t)c.x & 0xFFFFu, u2p = (uint32_t)c.y & 0xFFFFu, u1c = (uint32_t)c.z & 0xFFFFu, u2c = (uint32_t)c.w & 0xFFFFu;
      if (i1p2 == i && u1p >= u2p && u1c >= u2c) r = make_int4(i, i2p, i1c, i2c);
    }
  }
  if (writer) { out[2 * (int64_t)i] = r; out[2 * (int64_t)i + 1] = c; }
  if (method != 0) count_chunk(writer && r.z >= 0, mchunk + (i >> 8));
}

// The hops are look-ups in the per-pass tables.  (Quad with a motion prior: table 1 is indexed by the DRIVING feature,
// kernels_prior.hip.)
__global__ void chain_kernel(VhSets s, VhMatchArgs a, int32_t method, const int32_t *__restrict__ best,
                             int4 *__restrict__ chain, uint32_t *__restrict__ mask, uint32_t epoch,
                             int32_t *__restrict__ mchunk, int32_t nchm) {
  const int32_t stream = blockIdx.y;
  const CircleSets cs = circle_sets(s, a, stream);
  const int64_t cap = s.cap;
  const int32_t *__restrict__ T = best + (int64_t)stream * 4 * cap;
  const int32_t ndrive = (method == 2) ? cs.n[0] : cs.n[2];
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ndrive; i += gridDim.x * blockDim.x)
    circle(s, cs, method, stream, i, true,
           [&](int32_t stage, int32_t, int32_t iq, int32_t, bool) __attribute__((always_inline)) { return T[stage * cap + (method == 2 && stage == 1 && a.prior ? i : iq)]; },
           chain + 2 * (int64_t)stream * cap, mask, epoch, mchunk + stream * nchm);
}

// --------------------------------------------------------------- ranged circle
// Mapping: VH_RANGED_G lanes per driver, stages in sequence.  The lanes of a group share the query of the stage and
// split its candidates: the bins of interest are walked in the reference's order (u-bin outer; the v-bins of a u-bin
// are one contiguous run of bin-order positions), lane g takes positions start + g, start + g + G, ...  The winner is
// the minimum of SAD << 32 | position: ascending position IS the reference's visiting order, so the first strict
// minimum (src/matcher.cpp:264) comes out in any arrival order; no accepted candidate leaves min_ind = 0 (:221).
// The accept window is integer: query + range of the driver's bin, v replaced by +-disp_tolerance in a 1-d stage.
//
// findMatch (src/matcher.cpp:216-272) of query `iq` of set `qset` in set `cset`, inside rg = {u_min, u_max, v_min, v_max}
// relative to the query; every lane of the group returns min_ind
__device__ __forceinline__ int32_t find_ranged(const VhSets &s, int32_t qset, int32_t iq, int32_t cset, const int4 rg, bool flow, int32_t disp_tol,
                                               int32_t g) {
  const int64_t cap = s.cap;
  const int32_t *__restrict__ q = s.feat + ((int64_t)qset * cap + iq) * 12;
  const int32_t u1 = q[0], v1 = q[1], c = q[3];
  const uint4 a0 = *(const uint4 *)(q + 4), a1 = *(const uint4 *)(q + 8);
  const VhWindow w = {u1 + rg.x, u1 + rg.y, flow ? v1 + rg.z : v1 - disp_tol, flow ? v1 + rg.w : v1 + disp_tol};
  const VhBins b = bins_of_interest(s, w);
  const int32_t *__restrict__ cbs = s.bin_start + (int64_t)cset * (s.nbins + 1);
  const uint32_t *__restrict__ cuv = s.s_uv + (int64_t)cset * cap;
  const uint4 *__restrict__ cdesc = (const uint4 *)(s.s_desc + (int64_t)cset * cap * 8);
  unsigned long long key = ~0ull;
  if (b.vb0 <= b.vb1) {
    for (int32_t ub = b.ub0; ub <= b.ub1; ub++) {
      const int32_t row = (c * s.ubn + ub) * s.vbn;
      const int32_t p1 = cbs[row + b.vb1 + 1];
      for (int32_t p = cbs[row + b.vb0] + g; p < p1; p += VH_RANGED_G) {
        if (outside_window(cuv[p], w)) continue;
        const unsigned long long k = ((unsigned long long)sad32(a0, a1, cdesc[2 * (int64_t)p], cdesc[2 * (int64_t)p + 1], 0) << 32) | (uint32_t)p;
        key = k < key ? k : key;
      }
    }
  }
  key = vh_wave_min_u64<VH_RANGED_G>(key);
  return key == ~0ull ? 0 : s.s_idx[(int64_t)cset * cap + (uint32_t)key];
}

// The same findMatch with the motion prior's distance term (vh_prior.h; src/matcher.cpp:257-264) for the prediction
// (u_, v_): the cost is a double, so the key trick does not apply.  Every lane keeps the first strict minimum below
// 10000000 (:222) of the candidates it visits, in ascending position; the group reduces lexicographically on (cost,
// position), which is the first strict minimum of the reference's visiting order in any arrival order.  A cost that is
// not below 10000000 (an infinite prediction) or does not compare (NaN) is never accepted: min_ind = 0 (:221).
__device__ __forceinline__ int32_t find_ranged_prior(const VhSets &s, int32_t qset, int32_t iq, int32_t cset, const int4 rg, int32_t g, double u_,
                                                     double v_) {
  const int64_t cap = s.cap;
  const int32_t *__restrict__ q = s.feat + ((int64_t)qset * cap + iq) * 12;
  const int32_t u1 = q[0], v1 = q[1], c = q[3];
  const uint4 a0 = *(const uint4 *)(q + 4), a1 = *(const uint4 *)(q + 8);
  const VhWindow w = {u1 + rg.x, u1 + rg.y, v1 + rg.z, v1 + rg.w};  // (the hop is a flow stage)
  const VhBins b = bins_of_interest(s, w);
  const int32_t *__restrict__ cbs = s.bin_start + (int64_t)cset * (s.nbins + 1);
  const uint32_t *__restrict__ cuv = s.s_uv + (int64_t)cset * cap;
  const uint4 *__restrict__ cdesc = (const uint4 *)(s.s_desc + (int64_t)cset * cap * 8);
  double min_cost = 10000000;
  int32_t min_pos = INT32_MAX;
  if (b.vb0 <= b.vb1) {
    for (int32_t ub = b.ub0; ub <= b.ub1; ub++) {
      const int32_t row = (c * s.ubn + ub) * s.vbn;
      const int32_t p1 = cbs[row + b.vb1 + 1];
      for (int32_t p = cbs[row + b.vb0] + g; p < p1; p += VH_RANGED_G) {
        const uint32_t uv2 = cuv[p];
        if (outside_window(uv2, w)) continue;
        const double cost = vh_prior_cost(sad32(a0, a1, cdesc[2 * (int64_t)p], cdesc[2 * (int64_t)p + 1], 0), uv2, u_, v_);
        if (cost < min_cost) { min_cost = cost; min_pos = p; }
      }
    }
  }
#pragma unroll
  for (int32_t d = VH_RANGED_G / 2; d >= 1; d >>= 1) {
    const double oc = __longlong_as_double((long long)vh_shfl_xor_u64((uint64_t)__double_as_longlong(min_cost), d));
    const int32_t op = __shfl_xor(min_pos, d);
    if (oc < min_cost || (oc == min_cost && op < min_pos)) { min_cost = oc; min_pos = op; }
  }
  return min_pos == INT32_MAX ? 0 : s.s_idx[(int64_t)cset * cap + min_pos];
}

// The hops are searches inside the ranges of the driver's statistics bin; lane g == 0 of a driver's group writes.
// ranges: [row][ubn * vbn][4 stages]{u_min, u_max, v_min, v_max} int32
// PRIOR (quad only): stage 1, previous right -> current right, carries the distance term for the driver's prediction
// under pa.tr[row]; its accept window stays query + range[stage 1], the other three stages keep the integer key.
template <bool PRIOR>
__device__ __forceinline__ void ranged_circle(const VhSets &s, const VhMatchArgs &a, int32_t method, const int4 *__restrict__ ranges,
                                              int4 *__restrict__ chain, uint32_t *__restrict__ mask, uint32_t epoch,
                                              int32_t *__restrict__ mchunk, int32_t nchm, const VhPriorArgs &pa) {
  const int32_t stream = blockIdx.y;
  const CircleSets cs = circle_sets(s, a, stream);
  const int4 *__restrict__ rrow = ranges + (int64_t)stream * (s.ubn * s.vbn) * 4;
  const int32_t ndrive = (method == 2) ? cs.n[0] : cs.n[2];
  const uint32_t *__restrict__ uvd = (method == 2) ? cs.uv[0] : cs.uv[2];
  const int32_t per_wg = 256 / VH_RANGED_G, g = threadIdx.x % VH_RANGED_G;
  for (int32_t i = blockIdx.x * per_wg + threadIdx.x / VH_RANGED_G; i < ndrive; i += gridDim.x * per_wg) {
    // statistics bin of the driver (src/matcher.cpp:314-317): every stage of its circle searches this bin's ranges
    const uint32_t uvi = uvd[i];
    const int32_t sb = bin_of(s, (int32_t)(uvi >> 16), s.vbn) * s.ubn + bin_of(s, (int32_t)(uvi & 0xFFFFu), s.ubn);
    const int4 *__restrict__ rg = rrow + 4 * (int64_t)sb;
    // (the 64 / G drivers of a wave lie in one emission chunk of 256 drivers)
    circle(s, cs, method, stream, i, g == 0,
           [&](int32_t stage, int32_t qrole, int32_t iq, int32_t crole, bool flow) __attribute__((always_inline)) {
             if (PRIOR && stage == 1) {
               const int32_t u2p = s.feat[((int64_t)cs.set[qrole] * s.cap + iq) * 12];  // the query of this hop: previous right feature i2p
               const VhPrediction pr = vh_prior_predict(pa.tr + 16 * (int64_t)stream, pa.f, pa.cu, pa.cv, pa.base, (int32_t)(uvi & 0xFFFFu),
                                                        (int32_t)(uvi >> 16), u2p);
               return find_ranged_prior(s, cs.set[qrole], iq, cs.set[crole], rg[stage], g, pr.u, pr.v);
             }
             return find_ranged(s, cs.set[qrole], iq, cs.set[crole], rg[stage], flow, a.disp_tol, g);
           },
           chain + 2 * (int64_t)stream * s.cap, mask, epoch, mchunk + stream * nchm);
  }
}
__global__ void __launch_bounds__(256) ranged_circle_kernel(VhSets s, VhMatchArgs a, int32_t method, const int4 *__restrict__ ranges,
                                                            int4 *__restrict__ chain, uint32_t *__restrict__ mask, uint32_t epoch,
                                                            int32_t *__restrict__ mchunk, int32_t nchm) {
  ranged_circle<false>(s, a, method, ranges, chain, mask, epoch, mchunk, nchm, VhPriorArgs{});
}
__global__ void __launch_bounds__(256) ranged_circle_prior_kernel(VhSets s, VhMatchArgs a, const int4 *__restrict__ ranges, int4 *__restrict__ chain,
                                                                  int32_t *__restrict__ mchunk, int32_t nchm, VhPriorArgs pa) {
  ranged_circle<true>(s, a, 2, ranges, chain, nullptr, 0u, mchunk, nchm, pa);
}

// ------------------------------------------------------------------ flow_keep
// Flow only: after every closing feature has bid for its pixel, keep the winner
// (the reference's first writer, matcher.cpp:331-334), drop the others, and
// count the survivors per emission chunk.
__global__ void flow_keep_kernel(VhSets s, VhMatchArgs a, int4 *__restrict__ chain,
                                 const uint32_t *__restrict__ mask, uint32_t epoch,
                                 int32_t *__restrict__ mchunk, int32_t nchm) {
  const int32_t stream = blockIdx.y;
  const int32_t set1c = vh_row_set(a, stream, 2);
  const int32_t n1c = indexed_count(s, set1c);
  int4 *__restrict__ ch = chain + 2 * (int64_t)stream * s.cap;
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n1c; i += gridDim.x * blockDim.x) {
    const int4 r = ch[2 * (int64_t)i];
    const uint32_t uv = (uint32_t)ch[2 * (int64_t)i + 1].z;
    const bool win = r.z >= 0 && *mask_cell(s, mask, stream, uv) == mask_bid(epoch, i);
    if (r.z >= 0 && !win) ch[2 * (int64_t)i].z = -2;
    count_chunk(win, mchunk + stream * nchm + (i >> 8));
  }
}

// --------------------------------------------------------------- emit_matches
// One 256-thread workgroup per 256 driving features: ordered compaction of the closed
// circles into p_match records (48 B, src/matcher.h:89-104), in ascending order
// of the driving feature index as the reference's loops emit them.  The offset of
// a chunk is the sum of the survivor counts of the chunks before it.
// REFINED (refinement > 0): the coordinates of a kept entry come from ref (kernels_refine.hip) instead of the chain.
template <bool REFINED>
__global__ void __launch_bounds__(256)
emit_matches_kernel(VhSets s, VhMatchArgs a, int32_t method, const int4 *__restrict__ chain,
                    float *__restrict__ matches, int32_t mcap, int32_t *__restrict__ match_count,
                    int32_t *__restrict__ overflow, const int32_t *__restrict__ mchunk, int32_t nchm,
                    int32_t *__restrict__ redo, int32_t *__restrict__ mchunk_next, int4 *__restrict__ host_out,
                    float *__restrict__ host_matches, const float4 *__restrict__ ref) {
  __shared__ int32_t sWave[4];
  __shared__ int32_t sBase;
  const int32_t chunk = blockIdx.x, stream = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // the chunk counters of the NEXT launch (the other buffer; its last reader, the emission before this one, is done)
  // are zeroed here instead of by a memset of their own: two fill kernels and a launch gap per step
  if (tid == 0) mchunk_next[stream * nchm + chunk] = 0;
  int32_t sets[4];
#pragma unroll
  for (int32_t r = 0; r < 4; r++) sets[r] = vh_row_set(a, stream, r);
  const int32_t drive = (method == 2) ? sets[0] : sets[2];
  const int32_t n = indexed_count(s, drive);
  if (chunk * 256 >= n && chunk != nchm - 1) return;
  const int4 *__restrict__ ch = chain + 2 * (int64_t)stream * s.cap;
  float *__restrict__ out = matches + (int64_t)stream * mcap * 12;
  // matches emitted by earlier chunks
  int32_t part = 0;
  for (int32_t k = tid; k < chunk; k += 256) part += mchunk[stream * nchm + k];
  part = vh_wave_sum(part);
  if (lane == 0) sWave[w] = part;
  __syncthreads();
  if (tid == 0) { int32_t t = 0; for (int32_t k = 0; k < 4; k++) t += sWave[k]; sBase = t; }
  __syncthreads();
  const int32_t base = sBase;
  __syncthreads();

  const int32_t i = chunk * 256 + tid;
  int4 r = make_int4(-1, -1, -2, -1), c = make_int4(0, 0, 0, 0);
  if (i < n) { r = ch[2 * (int64_t)i]; c = ch[2 * (int64_t)i + 1]; }
  const bool keep = r.z >= 0;
  uint32_t rec[12];
#pragma unroll
  for (int32_t k = 0; k < 12; k++) rec[k] = (k % 3 == 2) ? 0xFFFFFFFFu : __float_as_uint(-1.0f);
  if (keep) {
    const int32_t idx[4] = {r.x, r.y, r.z, r.w};
    const uint32_t uv[4] = {(uint32_t)c.x, (uint32_t)c.y, (uint32_t)c.z, (uint32_t)c.w};
    float q[8];
    if (REFINED) {
      const float4 q0 = ref[2 * ((int64_t)stream * s.cap + i)], q1 = ref[2 * ((int64_t)stream * s.cap + i) + 1];
      q[0] = q0.x; q[1] = q0.y; q[2] = q0.z; q[3] = q0.w; q[4] = q1.x; q[5] = q1.y; q[6] = q1.z; q[7] = q1.w;
    }
#pragma unroll
    for (int32_t k = 0; k < 4; k++) {
      if (idx[k] >= 0) {
        rec[3 * k + 0] = __float_as_uint(REFINED ? q[2 * k] : (float)(uv[k] & 0xFFFFu));
        rec[3 * k + 1] = __float_as_uint(REFINED ? q[2 * k + 1] : (float)(uv[k] >> 16));
      }
      rec[3 * k + 2] = (uint32_t)idx[k];
    }
  }
  const VhCompact cp = vh_compact4(keep, sWave, w, lane);
  const int32_t pos = base + cp.pos, tot = cp.total;
  if (keep && pos < mcap) {
    uint4 *o = (uint4 *)(out + (int64_t)pos * 12);
    o[0] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
    o[1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
    o[2] = make_uint4(rec[8], rec[9], rec[10], rec[11]);
    if (host_matches) {  // small groups: the records also go straight to host-mapped memory (no download before getMatches)
      uint4 *h = (uint4 *)(host_matches + ((int64_t)stream * mcap + pos) * 12);
      h[0] = o[0]; h[1] = o[1]; h[2] = o[2];
    }
  }
  if (chunk == nchm - 1 && tid == 0) {
    match_count[stream] = base + tot;
    // a set this method read held more features than the capacity: the matching ran on
    // its first `cap` records only, which the host reports as VH_ERR_CAPACITY
    int32_t ov = 0;
#pragma unroll
    for (int32_t r = 0; r < 4; r++) {
      const bool used = method == 2 || r == 2 || (method == 0 && r == 0) || (method == 1 && r == 3);
      if (used && s.count[sets[r]] > s.cap) ov = 1;
    }
    overflow[stream] = ov;
    // statistics of this launch for the host's loop policy: queries searched again / queries searched
    int32_t nq = 0;
#pragma unroll
    for (int32_t k = 0; k < 4; k++) if (k < a.npass) nq += indexed_count(s, vh_row_set(a, stream, a.pass[k].qset));
    // count, overflow flag and the launch's statistics also go straight to host-mapped memory: the host reads
    // them after the launch's event instead of through small device->host copies (each a blit kernel + a round trip)
    host_out[stream] = make_int4(base + tot, ov, redo[stream], nq);
    redo[stream] = 0;
  }
}

}  // namespace

void vh_launch_chain(const VhSets &s, const VhMatchArgs &a, int32_t method, const int32_t *best,
                     int4 *chain, uint32_t *mask, uint32_t epoch, int32_t *mchunk, hipStream_t st) {
  const int32_t nchm = (s.cap + 255) / 256;
  dim3 grid(std::min(std::max(s.cap / 1024, 8), 256), a.rows);
  hipLaunchKernelGGL(chain_kernel, grid, dim3(256), 0, st, s, a, method, best, chain, mask, epoch, mchunk, nchm);
  if (method == 0) vh_launch_flow_keep(s, a, chain, mask, epoch, mchunk, st);
}
void vh_launch_flow_keep(const VhSets &s, const VhMatchArgs &a, int4 *chain, const uint32_t *mask, uint32_t epoch, int32_t *mchunk,
                         hipStream_t st) {
  const int32_t nchm = (s.cap + 255) / 256;
  dim3 grid(std::min(std::max(s.cap / 1024, 8), 256), a.rows);
  hipLaunchKernelGGL(flow_keep_kernel, grid, dim3(256), 0, st, s, a, chain, mask, epoch, mchunk, nchm);
}
void vh_launch_emit_matches(const VhSets &s, const VhMatchArgs &a, int32_t method, const int4 *chain,
                            void *matches, int32_t mcap, int32_t *match_count, int32_t *overflow,
                            const int32_t *mchunk, int32_t *redo, int32_t *mchunk_next, void *host_out, void *host_matches,
                            const float4 *ref, hipStream_t st) {
  const int32_t nchm = (s.cap + 255) / 256;
  // every row of the handle, a.rows or not: the rows a sequence chunk leaves empty read the empty set here and report 0
  // matches (their chain tables were not written, their chunk counters are zero), and their counters are reset
  if (ref)
    hipLaunchKernelGGL(emit_matches_kernel<true>, dim3(nchm, a.S), dim3(256), 0, st, s, a, method, chain,
                       (float *)matches, mcap, match_count, overflow, mchunk, nchm, redo, mchunk_next, (int4 *)host_out, (float *)host_matches, ref);
  else
    hipLaunchKernelGGL(emit_matches_kernel<false>, dim3(nchm, a.S), dim3(256), 0, st, s, a, method, chain,
                       (float *)matches, mcap, match_count, overflow, mchunk, nchm, redo, mchunk_next, (int4 *)host_out, (float *)host_matches, ref);
}
void vh_launch_ranged_circle(const VhSets &s, const VhMatchArgs &a, int32_t method, const int32_t *ranges, int4 *chain, uint32_t *mask,
                             uint32_t epoch, int32_t *mchunk, hipStream_t st) {
  static_assert((VH_RANGED_G & (VH_RANGED_G - 1)) == 0 && VH_RANGED_G >= 1 && VH_RANGED_G <= 64, "lanes per driver");
  const int32_t nchm = (s.cap + 255) / 256;
  const int32_t per_wg = 256 / VH_RANGED_G;
  dim3 grid(std::min(std::max((s.cap + per_wg - 1) / per_wg, 1), 2048), a.rows);
  hipLaunchKernelGGL(ranged_circle_kernel, grid, dim3(256), 0, st, s, a, method, (const int4 *)ranges, chain, mask, epoch, mchunk, nchm);
}
void vh_launch_ranged_circle_prior(const VhSets &s, const VhMatchArgs &a, const int32_t *ranges, const VhPriorArgs &pa, int4 *chain, int32_t *mchunk,
                                   hipStream_t st) {
  const int32_t nchm = (s.cap + 255) / 256;
  const int32_t per_wg = 256 / VH_RANGED_G;
  dim3 grid(std::min(std::max((s.cap + per_wg - 1) / per_wg, 1), 2048), a.rows);
  hipLaunchKernelGGL(ranged_circle_prior_kernel, grid, dim3(256), 0, st, s, a, (const int4 *)ranges, chain, mchunk, nchm, pa);
}
