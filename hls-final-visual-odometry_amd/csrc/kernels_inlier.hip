// kernels_inlier.hip -- which records of whole match lists agree with a given motion, and those records compacted in
// list order, on gfx950.
//
// Replaces, for every list of a call in one launch sequence:
//   VisualOdometryStereo::getInlier                   (reference src/viso_stereo.cpp:159-177)
// for any quad list and any tr[6]: the 3-d point of the previous pair (:80-86), the rotation (:244-250, ego_rot), the
// prediction (:274-276, :317-321, ego_predict) and the strict compare of the squared reprojection error with
// inlier_threshold^2 (:171-174, ego_is_inlier) -- vh_ego.h, the estimator's own device functions.  Double precision,
// built with -ffp-contract=off; only sin / cos come from the device library.  `reweighting` is not read.
//
// A list is cut into tiles of INL_TILE records; a 256-lane workgroup takes one tile, one record per lane and trip:
//   inlier_flag     the flag of every record (one byte) and the number of inliers of the tile.  A record is read as
//                   three 16-byte loads, all trips of a lane in flight at once; wave 0 builds the rotation meanwhile.
//   inlier_scan     one workgroup per list: the tile counts become the tiles' first output positions, their sum the
//                   list's inlier count.
//   inlier_compact  a tile's inliers go to their positions (vh_compact4 per trip: thread order is list order), with
//                   the position each came from.
// Every output position is a function of the flags alone: no atomics, the same bytes from run to run.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_ego.h"

namespace {

#define INL_T 256
#define INL_R 4  // trips: records per lane
static_assert(INL_T * INL_R == VH_INLIER_TILE, "tile");

struct InlList {
  const vh_p_match *pm;
  int32_t n;
  int64_t out0;  // first element of this list in flags / out / src_pos
};
__device__ __forceinline__ InlList inl_list(const VhInlierArgs &a, int32_t s) {
  const VhList L = vh_list(s, a.pm, a.pm_stride, a.offsets, a.counts, a.count_cap);
  InlList r;
  r.pm = L.pm; r.n = L.n;
  r.out0 = a.offsets ? (int64_t)a.offsets[s] : (int64_t)s * a.out_stride;
  return r;
}

__global__ void __launch_bounds__(INL_T)
inlier_flag_kernel(VhInlierArgs a) {
  __shared__ double sR[9], sTr[6];
  __shared__ int32_t sWave[INL_T / 64];
  const int32_t s = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const InlList L = inl_list(a, s);
  const int32_t i0 = tile * VH_INLIER_TILE;
  if (i0 >= L.n) return;  // (an empty list reads neither ok nor tr)
  uint8_t *fl = a.flags + L.out0;
  int32_t cnt = 0;
  if (a.ok[s]) {
    float4 q[INL_R][3];
#pragma unroll
    for (int32_t k = 0; k < INL_R; k++) {
      const int32_t i = i0 + k * INL_T + tid;
      if (i < L.n) {
        const float4 *p = (const float4 *)(L.pm + i);
        q[k][0] = p[0]; q[k][1] = p[1]; q[k][2] = p[2];
      } else {
        q[k][0] = q[k][1] = q[k][2] = make_float4(0, 0, 0, 0);
      }
    }
    if (w == 0) {  // the rotation, once per workgroup
      double t6[6];
      for (int32_t m = 0; m < 6; m++) t6[m] = a.tr[6 * (int64_t)s + m];
      EgoRot R0;
      ego_rot(t6, R0);
      if (lane == 0) {
        for (int32_t m = 0; m < 9; m++) sR[m] = R0.r[m];
        for (int32_t m = 0; m < 6; m++) sTr[m] = t6[m];
      }
    }
    __syncthreads();
    EgoRot R;
    double tr[6];
    for (int32_t m = 0; m < 9; m++) R.r[m] = sR[m];
    for (int32_t m = 0; m < 6; m++) tr[m] = sTr[m];
#pragma unroll
    for (int32_t k = 0; k < INL_R; k++) {
      const int32_t i = i0 + k * INL_T + tid;
      bool in_ = false;
      if (i < L.n) {
        // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c} {i1c, u2c, v2c, i2c}
        const EgoObs o = ego_observe(a.e, q[k][0].x, q[k][0].y, q[k][0].w, q[k][1].z, q[k][1].w, q[k][2].y, q[k][2].z);
        in_ = ego_is_inlier(a.e, R, tr, o);  // (a NaN or infinite sum compares false)
        fl[i] = in_ ? 1 : 0;
      }
      cnt += __popcll(__ballot(in_));
    }
  } else {
#pragma unroll
    for (int32_t k = 0; k < INL_R; k++) {
      const int32_t i = i0 + k * INL_T + tid;
      if (i < L.n) fl[i] = 0;
    }
  }
  if (lane == 0) sWave[w] = cnt;
  __syncthreads();
  if (tid == 0) a.tile_cnt[(int64_t)s * a.tiles_per_list + tile] = (sWave[0] + sWave[1]) + (sWave[2] + sWave[3]);
}

__global__ void __launch_bounds__(INL_T)
inlier_scan_kernel(VhInlierArgs a) {
  __shared__ int32_t sWave[INL_T / 64];
  const int32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const InlList L = inl_list(a, s);
  const int32_t ntiles = (L.n + VH_INLIER_TILE - 1) / VH_INLIER_TILE;  // <= tiles_per_list: n <= the capacity the grid was sized for
  int32_t *tc = a.tile_cnt + (int64_t)s * a.tiles_per_list;
  int32_t base = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += INL_T) {
    const int32_t t = t0 + tid;
    const int32_t v = t < ntiles ? tc[t] : 0;
    const int32_t incl = vh_wave_scan(v);
    if (lane == 63) sWave[w] = incl;
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t k = 0; k < INL_T / 64; k++) { const int32_t x = sWave[k]; before += k < w ? x : 0; total += x; }
    if (t < ntiles) tc[t] = base + before + incl - v;
    base += total;
    __syncthreads();
  }
  if (tid == 0) a.n_inl[s] = base;
}

__global__ void __launch_bounds__(INL_T)
inlier_compact_kernel(VhInlierArgs a) {
  __shared__ int32_t sWave[INL_T / 64];
  const int32_t s = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const InlList L = inl_list(a, s);
  const int32_t i0 = tile * VH_INLIER_TILE;
  if (i0 >= L.n) return;
  const uint8_t *fl = a.flags + L.out0;
  int64_t dst0 = L.out0 + a.tile_cnt[(int64_t)s * a.tiles_per_list + tile];
#pragma unroll
  for (int32_t k = 0; k < INL_R; k++) {
    const int32_t i = i0 + k * INL_T + tid;
    const bool keep = i < L.n && fl[i] != 0;
    const VhCompact c = vh_compact4(keep, sWave, w, lane);
    if (keep) {  // dst0 + c.pos < out0 + (inliers of the list) <= out0 + n
      const float4 *p = (const float4 *)(L.pm + i);
      float4 *o = (float4 *)(a.out + dst0 + c.pos);
      const float4 q0 = p[0], q1 = p[1], q2 = p[2];
      o[0] = q0; o[1] = q1; o[2] = q2;
      a.src_pos[dst0 + c.pos] = i;
    }
    dst0 += c.total;
    __syncthreads();
  }
}

}  // namespace

// grid: a.n_lists x a.tiles_per_list workgroups (the caller keeps the product below 2^24 and tiles_per_list <= 65535)
void vh_launch_inlier_flag(const VhInlierArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(inlier_flag_kernel, dim3(a.n_lists, a.tiles_per_list), dim3(INL_T), 0, st, a);
}
void vh_launch_inlier_compact(const VhInlierArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(inlier_scan_kernel, dim3(a.n_lists), dim3(INL_T), 0, st, a);
  hipLaunchKernelGGL(inlier_compact_kernel, dim3(a.n_lists, a.tiles_per_list), dim3(INL_T), 0, st, a);
}
