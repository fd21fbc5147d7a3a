// kernels_prior.hip -- quad matching with the motion prior of stock libviso2 on gfx950.
//
// The reference tree accepts Tr_delta in Matcher::matchFeatures and ignores it (src/matcher.cpp:93-111); what it does
// pin is the cost term findMatch adds when a predicted position (u_, v_) is given (src/matcher.cpp:257-262):
// cost = SAD + 4 * ||(u2, v2) - (u_, v_)|| in double, first strict minimum in visiting order.  Stock libviso2 uses it on
// ONE hop of the quad circle, previous right -> current right [upstream-recollection]: the 3-d point of the (1p, 2p)
// pair is moved by Tr_delta and projected into the current right image.  The prediction belongs to the DRIVING feature
// i1p, not to the query i2p, so this hop cannot be a table over the features of set 2p like the other three: it is
// evaluated per driving feature, after the 1p -> 2p table exists, one lane per circle, walking the query's bins in the
// reference's order (u-bin, v-bin, list position = ascending bin-order position) with the literal accept test and a
// double-precision compare.  Built with -ffp-contract=off: du * du + dv * dv rounds twice, as on the reference's x86 build.
#include "vh_findmatch.h"
#include "vh_prior.h"

namespace {

// findMatch (src/matcher.cpp:216-272) of query `iq` of set `qset` in set `cset` by ONE lane, window +-ru, +-rv, with
// the distance term when a prediction (u_, v_) is given (both >= 0, :257): the cost is not an integer then, so the
// key trick of the tile searches does not apply.  The lane walks the bins of interest in the reference's order (u-bin,
// v-bin, list position = ascending bin-order position) with the literal accept test and keeps the first strict minimum
// of the double cost (:264); returns min_ind (0 when nothing was accepted, :221).  sqrt is the correctly rounded one.
__device__ __forceinline__ int32_t find_match_prior(const VhSets &s, int32_t qset, int32_t iq, int32_t cset, int32_t ru, int32_t rv, double u_,
                                                    double v_) {
  const int32_t *q = s.feat + ((int64_t)qset * s.cap + iq) * 12;
  const int32_t u1 = q[0], v1 = q[1], c = q[3];
  const uint4 a0 = *(const uint4 *)(q + 4), a1 = *(const uint4 *)(q + 8);
  const VhWindow w = {u1 - ru, u1 + ru, v1 - rv, v1 + rv};
  const VhBins b = bins_of_interest(s, w);
  const int32_t *__restrict__ cbs = s.bin_start + (int64_t)cset * (s.nbins + 1);
  const uint32_t *__restrict__ cuv = s.s_uv + (int64_t)cset * s.cap;
  const uint4 *__restrict__ cdesc = (const uint4 *)(s.s_desc + (int64_t)cset * s.cap * 8);
  double min_cost = 10000000;  // matcher.cpp:222
  int32_t min_pos = -1;
  for (int32_t ub = b.ub0; ub <= b.ub1; ub++) {
    const int32_t row = (c * s.ubn + ub) * s.vbn;
    for (int32_t p = cbs[row + b.vb0]; p < cbs[row + b.vb1 + 1]; p++) {
      const uint32_t uv2 = cuv[p];
      if (outside_window(uv2, w)) continue;
      const double cost = vh_prior_cost(sad32(a0, a1, cdesc[2 * (int64_t)p], cdesc[2 * (int64_t)p + 1], 0), uv2, u_, v_);
      if (cost < min_cost) { min_cost = cost; min_pos = p; }
    }
  }
  return min_pos >= 0 ? s.s_idx[(int64_t)cset * s.cap + min_pos] : 0;
}

// findMatch with one prediction for every query of pass 0 (a parity entry point: vh_match_all_prior)
__global__ void match_prior_kernel(VhSets s, VhMatchArgs a, double u_, double v_, int32_t *__restrict__ best) {
  const int32_t qset = vh_row_set(a, 0, a.pass[0].qset);
  const int32_t cset = vh_row_set(a, 0, a.pass[0].cset);
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= indexed_count(s, qset)) return;
  best[i] = find_match_prior(s, qset, i, cset, a.radius, a.pass[0].flow ? a.radius : a.disp_tol, u_, v_);
}

// tr: [S][16] row-major 4x4 per stream
__global__ void __launch_bounds__(128) quad_prior_kernel(VhSets s, VhMatchArgs a, const double *__restrict__ tr, double f, double cu, double cv,
                                                         double base, int32_t *__restrict__ best) {
  const int32_t stream = blockIdx.y;
  const int32_t set1p = vh_row_set(a, stream, 0), set2p = vh_row_set(a, stream, 1);
  const int32_t set2c = vh_row_set(a, stream, 3);
  const int64_t cap = s.cap;
  const int32_t n1p = indexed_count(s, set1p), n2p = indexed_count(s, set2p), n2c = indexed_count(s, set2c);
  int32_t *__restrict__ T = best + (int64_t)stream * 4 * cap;
  const double *__restrict__ t = tr + 16 * (int64_t)stream;
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n1p; i += gridDim.x * blockDim.x) {
    if (n2p <= 0 || n2c <= 0) { T[1 * cap + i] = 0; continue; }
    const int32_t i2p = T[0 * cap + i];
    const uint32_t uv1 = s.f_uv[(int64_t)set1p * cap + i];
    const int32_t u2p = s.feat[((int64_t)set2p * cap + i2p) * 12];  // the query of this hop: previous right feature i2p
    const int32_t u1p = (int32_t)(uv1 & 0xFFFFu), v1p = (int32_t)(uv1 >> 16);
    const VhPrediction pr = vh_prior_predict(t, f, cu, cv, base, u1p, v1p, u2p);
    // flow search window; table slot 1 is indexed by the DRIVING feature here (kernels_chain.hip: chain_kernel, a.prior)
    T[1 * cap + i] = find_match_prior(s, set2p, i2p, set2c, a.radius, a.radius, pr.u, pr.v);
  }
}

}  // namespace

void vh_launch_match_prior(const VhSets &s, const VhMatchArgs &a, double u_, double v_, int32_t *best,
                           hipStream_t st) {
  hipLaunchKernelGGL(match_prior_kernel, dim3((s.cap + 127) / 128), dim3(128), 0, st, s, a, u_, v_, best);
}
void vh_launch_quad_prior(const VhSets &s, const VhMatchArgs &a, const double *tr, double f, double cu, double cv, double base, int32_t *best,
                          hipStream_t st) {
  dim3 grid((uint32_t)((s.cap + 127) / 128 < 256 ? (s.cap + 127) / 128 : 256), a.rows);
  hipLaunchKernelGGL(quad_prior_kernel, grid, dim3(128), 0, st, s, a, tr, f, cu, cv, base, best);
}
