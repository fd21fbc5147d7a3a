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
//   inlier_flag_mono  the same tiles under VisualOdometryMono::getInlier (src/viso_mono.cpp:268-315) and a vh_mono_model
//                   per list (vh_mono.h: the estimator's normalisation and Sampson test): two 16-byte loads per record,
//                   the model by uniform loads, pure double arithmetic and one division.
//   inlier_scan     one workgroup per list: the tile counts become the tiles' first output positions, their sum the
//                   list's inlier count.
//   inlier_compact  a tile's inliers go to their positions (vh_compact4 per trip: thread order is list order), with
//                   the position each came from.
// Every output position is a function of the flags alone: no atomics, the same bytes from run to run.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_ego.h"
#include "vh_mono.h"

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
  const VhList L = vh_list(a.lists, s);
  InlList r;
  r.pm = L.pm; r.n = L.n;
  r.out0 = a.lists.offsets ? (int64_t)a.lists.offsets[s] : (int64_t)s * a.out_stride;
  return r;
}

// The per-record test of a flag kernel: what a lane keeps of a record (Rec, from 16-byte loads), what the workgroup
// prepares once between the loads and the first use (setup), and the test itself.
// VisualOdometryStereo::getInlier under tr[6] (vh_ego.h): three loads; wave 0 builds the rotation while they are in
// flight and hands it over through LDS.
struct InlStereo {
  struct Rec { float4 q[3]; };
  EgoRot R;
  double tr[6];
  static __device__ __forceinline__ Rec load(const vh_p_match *m) {
    const float4 *p = (const float4 *)m;
    Rec r; r.q[0] = p[0]; r.q[1] = p[1]; r.q[2] = p[2];
    return r;
  }
  static __device__ __forceinline__ Rec none() { Rec r; r.q[0] = r.q[1] = r.q[2] = make_float4(0, 0, 0, 0); return r; }
  __device__ __forceinline__ void setup(const VhInlierArgs &a, int32_t s, int32_t w, int32_t lane) {
    __shared__ double sR[9], sTr[6];
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
    for (int32_t m = 0; m < 9; m++) R.r[m] = sR[m];
    for (int32_t m = 0; m < 6; m++) tr[m] = sTr[m];
  }
  __device__ __forceinline__ bool inlier(const VhInlierArgs &a, const Rec &r) const {
    // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c} {i1c, u2c, v2c, i2c}
    const EgoObs o = ego_observe(a.e, r.q[0].x, r.q[0].y, r.q[0].w, r.q[1].z, r.q[1].w, r.q[2].y, r.q[2].z);
    return ego_is_inlier(a.e, R, tr, o);  // (a NaN or infinite sum compares false)
  }
};
// VisualOdometryMono::getInlier under a vh_mono_model (vh_mono.h): two loads (the last third of a record is not
// fetched); the model is the same for the whole workgroup -- 16 doubles at a uniform address, no LDS, no barrier.
struct InlMono {
  struct Rec { float4 q[2]; };
  vh_mono_model m;
  static __device__ __forceinline__ Rec load(const vh_p_match *pm) {
    const float4 *p = (const float4 *)pm;
    Rec r; r.q[0] = p[0]; r.q[1] = p[1];
    return r;
  }
  static __device__ __forceinline__ Rec none() { Rec r; r.q[0] = r.q[1] = make_float4(0, 0, 0, 0); return r; }
  __device__ __forceinline__ void setup(const VhInlierArgs &a, int32_t s, int32_t, int32_t) { m = a.model[s]; }
  __device__ __forceinline__ bool inlier(const VhInlierArgs &a, const Rec &r) const {
    // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c}
    return mono_is_inlier(m, r.q[0].x, r.q[0].y, r.q[1].z, r.q[1].w, a.mono_threshold);  // (a NaN or infinite quotient compares false)
  }
};

// One tile of one list: the flag of every record and the tile's inlier count -- the skeleton of both flag kernels.
template <class Test>
__device__ __forceinline__ void inlier_flag_tile(const VhInlierArgs &a) {
  __shared__ int32_t sWave[INL_T / 64];
  const int32_t s = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const InlList L = inl_list(a, s);
  const int32_t i0 = tile * VH_INLIER_TILE;
  if (i0 >= L.n) return;  // (an empty list reads neither ok nor its motion / model)
  uint8_t *fl = a.flags + L.out0;
  int32_t cnt = 0;
  if (a.ok[s]) {
    typename Test::Rec q[INL_R];
#pragma unroll
    for (int32_t k = 0; k < INL_R; k++) {
      const int32_t i = i0 + k * INL_T + tid;
      q[k] = i < L.n ? Test::load(L.pm + i) : Test::none();
    }
    Test t;
    t.setup(a, s, w, lane);
#pragma unroll
    for (int32_t k = 0; k < INL_R; k++) {
      const int32_t i = i0 + k * INL_T + tid;
      bool in_ = false;
      if (i < L.n) {
        in_ = t.inlier(a, q[k]);
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
inlier_flag_kernel(VhInlierArgs a) { inlier_flag_tile<InlStereo>(a); }

__global__ void __launch_bounds__(INL_T)
inlier_flag_mono_kernel(VhInlierArgs a) { inlier_flag_tile<InlMono>(a); }

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

// grid: a.lists.n_lists x a.tiles_per_list workgroups (the caller keeps the product below 2^24 and tiles_per_list <= 65535)
void vh_launch_inlier_flag(const VhInlierArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(inlier_flag_kernel, dim3(a.lists.n_lists, a.tiles_per_list), dim3(INL_T), 0, st, a);
}
void vh_launch_inlier_flag_mono(const VhInlierArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(inlier_flag_mono_kernel, dim3(a.lists.n_lists, a.tiles_per_list), dim3(INL_T), 0, st, a);
}
void vh_launch_inlier_compact(const VhInlierArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(inlier_scan_kernel, dim3(a.lists.n_lists), dim3(INL_T), 0, st, a);
  hipLaunchKernelGGL(inlier_compact_kernel, dim3(a.lists.n_lists, a.tiles_per_list), dim3(INL_T), 0, st, a);
}
