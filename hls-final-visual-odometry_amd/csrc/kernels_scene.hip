// kernels_scene.hip -- the 3-d point of every record of whole match lists, stereo and mono, compacted in list order, on
// gfx950.
//
// For every list of a call, under the motion (stereo: tr[6]) or the pose (mono: vh_mono_pose) the list comes with:
//   stereo  the point of the previous pair as getInlier forms it (ego_observe: float df = max(u1p - u2p, 0.0001f)), moved
//           into the current frame by ego_predict where that frame is asked for; err = the square root of the four-term
//           sum ego_is_inlier compares; sigma_z = z * z / (f * base) -- vh_ego.h, the estimator's own device functions;
//   mono    P1 = K [I | 0], P2 = K [R | t] by the statements of mono_pose_candidates, the record triangulated as
//           triangulateChieral does (mono_pose_triangulate: a 4x4 decomposition in registers), the point as
//           mono_pose_point forms it, times the pose's scale; err from the two reprojections -- vh_mono_pose.h.
// Double precision, built with -ffp-contract=off; the six sin / cos of the stereo rotation are the device library's, the
// mono path calls nothing of it but sqrt.  A value is rounded to float once, at the store.
//
// A list is cut into tiles of SCN_T records and a 256-lane workgroup takes one tile, one record per lane, so that a lone
// list of 100 000 records is 391 workgroups:
//   scene_flag_*   the keep decision of every record and the number of survivors of the tile;
//   scene_scan     one workgroup per list: the tile counts become the tiles' first output positions, their sum the
//                  list's count (0 for a list with ok = 0, whose motion / pose is not read);
//   scene_store_*  the point computed again by the same function (the same instructions on the same inputs: the same
//                  bits) and each survivor's 32-byte record written once, as two 16-byte stores, at the tile's position
//                  + vh_compact4's rank: thread order is list order.
// Every output position is a function of the keep decisions alone: no atomics, the same bytes from run to run, whatever
// else the launch holds.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_ego.h"
#include "vh_mono_pose.h"

namespace {

#define SCN_T VH_SCENE_TILE
static_assert(SCN_T == 256, "vh_compact4 joins four waves");

struct ScnList {
  const vh_p_match *pm;
  int32_t n;
  int64_t out0;  // first element of this list in out / src
};
__device__ __forceinline__ ScnList scn_list(const VhSceneArgs &a, int32_t s) {
  const VhList L = vh_list(a.lists, s);
  ScnList r;
  r.pm = L.pm; r.n = L.n;
  r.out0 = a.lists.offsets ? (int64_t)a.lists.offsets[s] : (int64_t)s * a.out_stride;
  return r;
}

// what a lane knows of its record once it is evaluated: the point in the frame asked for (before Tw) and the decision
struct ScnPoint {
  double x, y, z, sigma_z, err;
  bool keep;
};

// The filters both kinds share, on the camera-frame values (strict compares in double; a NaN compares false, so the
// finiteness test comes first), then Tw (the top three rows, added left to right) and the last test: what is stored is finite.
__device__ __forceinline__ void scn_finish(const VhSceneArgs &a, const double *Tw, ScnPoint &p) {
  bool keep = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.err) && p.z > 0.0;
  if (a.sp.max_depth > 0.0 && p.z > a.sp.max_depth) keep = false;
  if (a.sp.max_err > 0.0 && p.err > a.sp.max_err) keep = false;
  if (Tw) {
    const double x = Tw[0] * p.x + Tw[1] * p.y + Tw[2] * p.z + Tw[3];
    const double y = Tw[4] * p.x + Tw[5] * p.y + Tw[6] * p.z + Tw[7];
    const double z = Tw[8] * p.x + Tw[9] * p.y + Tw[10] * p.z + Tw[11];
    p.x = x; p.y = y; p.z = z;
  }
  p.keep = keep && isfinite((float)p.x) && isfinite((float)p.y) && isfinite((float)p.z) && isfinite((float)p.sigma_z) && isfinite((float)p.err);
}

// Stereo: three 16-byte loads per record; wave 0 builds the rotation while they are in flight and hands it over through LDS.
struct ScnStereo {
  struct Rec { float4 q[3]; };
  double r[9], tr[6];
  const double *Tw;
  static __device__ __forceinline__ Rec load(const vh_p_match *m) {
    const float4 *p = (const float4 *)m;
    Rec v; v.q[0] = p[0]; v.q[1] = p[1]; v.q[2] = p[2];
    return v;
  }
  static __device__ __forceinline__ Rec none() { Rec v; v.q[0] = v.q[1] = v.q[2] = make_float4(0, 0, 0, 0); return v; }
  static __device__ __forceinline__ int32_t i1p(const Rec &v) { return __float_as_int(v.q[0].z); }
  static __device__ __forceinline__ int32_t i1c(const Rec &v) { return __float_as_int(v.q[2].x); }
  __device__ __forceinline__ void setup(const VhSceneArgs &a, int32_t s, int32_t w, int32_t lane) {
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
    for (int32_t m = 0; m < 9; m++) r[m] = sR[m];
    for (int32_t m = 0; m < 6; m++) tr[m] = sTr[m];
    Tw = a.Tw ? a.Tw + 16 * (int64_t)s : nullptr;
  }
  __device__ __forceinline__ ScnPoint eval(const VhSceneArgs &a, const Rec &v) const {
    // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c} {i1c, u2c, v2c, i2c}
    const EgoObs o = ego_observe(a.e, v.q[0].x, v.q[0].y, v.q[0].w, v.q[1].z, v.q[1].w, v.q[2].y, v.q[2].z);
    EgoRot R;  // (ego_predict reads r alone)
#pragma unroll
    for (int32_t m = 0; m < 9; m++) R.r[m] = r[m];
    double p[4], X1c, Y1c, Z1c;
    ego_predict(a.e, R, tr, o, p, X1c, Y1c, Z1c);
    const double d0 = o.u1c - p[0], d1 = o.v1c - p[1], d2 = o.u2c - p[2], d3 = o.v2c - p[3];
    ScnPoint q;
    q.err = sqrt(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3);
    if (a.sp.frame == 0) { q.x = o.X; q.y = o.Y; q.z = o.Z; }
    else { q.x = X1c; q.y = Y1c; q.z = Z1c; }
    q.sigma_z = q.z * q.z / (a.e.f * a.e.base);
    scn_finish(a, Tw, q);
    // (the float difference ego_observe clamps; a NaN difference compares false and ends at the finiteness test)
    if (a.sp.min_disp > 0.0f && (double)(v.q[0].x - v.q[0].w) < (double)a.sp.min_disp) q.keep = false;
    return q;
  }
};

// Mono: two 16-byte loads (the last third of a record holds i1c alone of what is needed: one 4-byte load); thread 0
// builds the projection matrices in LDS, every lane reads them at uniform addresses.
struct ScnMono {
  struct Rec { float4 q[2]; int32_t i1c; };
  const double *P1, *P2, *R, *t;
  double scale;
  const double *Tw;
  static __device__ __forceinline__ Rec load(const vh_p_match *m) {
    const float4 *p = (const float4 *)m;
    Rec v; v.q[0] = p[0]; v.q[1] = p[1]; v.i1c = m->i1c;
    return v;
  }
  static __device__ __forceinline__ Rec none() { Rec v; v.q[0] = v.q[1] = make_float4(0, 0, 0, 0); v.i1c = 0; return v; }
  static __device__ __forceinline__ int32_t i1p(const Rec &v) { return __float_as_int(v.q[0].z); }
  static __device__ __forceinline__ int32_t i1c(const Rec &v) { return v.i1c; }
  __device__ __forceinline__ void setup(const VhSceneArgs &a, int32_t s, int32_t, int32_t) {
    __shared__ double sP[24 + 12 + 1];  // P1[12] P2[12] | R[9] t[3] | scale
    if (threadIdx.x == 0) {
      const vh_mono_pose &ps = a.pose[s];
      const double K[9] = {a.m.f, 0, a.m.cu, 0, a.m.f, a.m.cv, 0, 0, 1};
      // the statements of mono_pose_candidates for the one candidate that won
      for (int32_t i = 0; i < 3; i++) for (int32_t j = 0; j < 4; j++) sP[i * 4 + j] = j < 3 ? K[i * 3 + j] : 0.0;
      double Rt[12];
      for (int32_t i = 0; i < 3; i++) { for (int32_t j = 0; j < 3; j++) Rt[i * 4 + j] = ps.R[i * 3 + j]; Rt[i * 4 + 3] = ps.t[i]; }
      matmul(K, 3, 3, Rt, 4, sP + 12);
      for (int32_t q = 0; q < 9; q++) sP[24 + q] = ps.R[q];
      for (int32_t q = 0; q < 3; q++) sP[33 + q] = ps.t[q];
      sP[36] = ps.scale;
    }
    __syncthreads();
    P1 = sP; P2 = sP + 12; R = sP + 24; t = sP + 33; scale = sP[36];
    Tw = a.Tw ? a.Tw + 16 * (int64_t)s : nullptr;
  }
  __device__ __forceinline__ ScnPoint eval(const VhSceneArgs &a, const Rec &v) const {
    // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c}
    const float u1p = v.q[0].x, v1p = v.q[0].y, u1c = v.q[1].z, v1c = v.q[1].w;
    double X[4], x, y, z;
    mono_pose_triangulate(P1, P2, u1p, v1p, u1c, v1c, X);
    mono_pose_point(X[0], X[1], X[2], X[3], x, y, z);
    // both reprojections of (x, y, z, 1): sums from zero, left to right, as mono_pose_in_front_of_both adds
    const double h[4] = {x, y, z, 1.0};
    double pa[3], pb[3];
#pragma unroll
    for (int32_t i = 0; i < 3; i++) {
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int32_t j = 0; j < 4; j++) sa += P1[i * 4 + j] * h[j];
#pragma unroll
      for (int32_t j = 0; j < 4; j++) sb += P2[i * 4 + j] * h[j];
      pa[i] = sa; pb[i] = sb;
    }
    const double d0 = u1p - pa[0] / pa[2], d1 = v1p - pa[1] / pa[2], d2 = u1c - pb[0] / pb[2], d3 = v1c - pb[1] / pb[2];
    ScnPoint q;
    q.err = sqrt(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3);
    if (a.sp.frame == 0) { q.x = x * scale; q.y = y * scale; q.z = z * scale; }
    else {
      const double xc = R[0] * x + R[1] * y + R[2] * z + t[0];
      const double yc = R[3] * x + R[4] * y + R[5] * z + t[1];
      const double zc = R[6] * x + R[7] * y + R[8] * z + t[2];
      q.x = xc * scale; q.y = yc * scale; q.z = zc * scale;
    }
    q.sigma_z = 0.0;
    scn_finish(a, Tw, q);
    return q;
  }
};

// grid: n_lists * tiles_per_list workgroups, list-major
template <class Kind>
__device__ __forceinline__ void scene_flag_tile(const VhSceneArgs &a) {
  __shared__ int32_t sWave[SCN_T / 64];
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const ScnList L = scn_list(a, s);
  const int64_t i = (int64_t)tile * SCN_T + tid;
  if ((int64_t)tile * SCN_T >= L.n) return;  // (an empty list reads neither ok nor its motion / pose)
  if (!a.ok[s]) return;                      // (scene_scan gives such a list the count 0 without reading the tile counts)
  const typename Kind::Rec v = i < L.n ? Kind::load(L.pm + i) : Kind::none();
  Kind k;
  k.setup(a, s, w, lane);
  bool keep = false;
  if (i < L.n) keep = k.eval(a, v).keep;
  const int32_t cnt = __popcll(__ballot(keep));
  if (lane == 0) sWave[w] = cnt;
  __syncthreads();
  if (tid == 0) a.tile_cnt[(int64_t)s * a.tiles_per_list + tile] = (sWave[0] + sWave[1]) + (sWave[2] + sWave[3]);
}

template <class Kind>
__device__ __forceinline__ void scene_store_tile(const VhSceneArgs &a) {
  __shared__ int32_t sWave[SCN_T / 64];
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const ScnList L = scn_list(a, s);
  const int64_t i = (int64_t)tile * SCN_T + tid;
  if ((int64_t)tile * SCN_T >= L.n) return;
  if (!a.ok[s]) return;
  const typename Kind::Rec v = i < L.n ? Kind::load(L.pm + i) : Kind::none();
  const int32_t src = i < L.n ? (a.src ? a.src[L.out0 + i] : (int32_t)i) : 0;
  Kind k;
  k.setup(a, s, w, lane);
  ScnPoint p;
  p.keep = false;
  if (i < L.n) p = k.eval(a, v);
  const VhCompact c = vh_compact4(p.keep, sWave, w, lane);
  if (p.keep) {  // out0 + (survivors before the tile) + c.pos < out0 + (survivors of the list) <= out0 + n
    const int64_t dst = L.out0 + a.tile_cnt[(int64_t)s * a.tiles_per_list + tile] + c.pos;
    float4 *o = (float4 *)(a.out + dst);
    o[0] = make_float4((float)p.x, (float)p.y, (float)p.z, (float)p.sigma_z);
    o[1] = make_float4((float)p.err, __int_as_float(src), __int_as_float(Kind::i1p(v)), __int_as_float(Kind::i1c(v)));
  }
}

__global__ void __launch_bounds__(SCN_T)
scene_flag_stereo_kernel(VhSceneArgs a) { scene_flag_tile<ScnStereo>(a); }
__global__ void __launch_bounds__(SCN_T)
scene_store_stereo_kernel(VhSceneArgs a) { scene_store_tile<ScnStereo>(a); }
__global__ void __launch_bounds__(SCN_T)
scene_flag_mono_kernel(VhSceneArgs a) { scene_flag_tile<ScnMono>(a); }
__global__ void __launch_bounds__(SCN_T)
scene_store_mono_kernel(VhSceneArgs a) { scene_store_tile<ScnMono>(a); }

// one workgroup per list: exclusive scan of its tile counts in place, the total to n_out
__global__ void __launch_bounds__(SCN_T)
scene_scan_kernel(VhSceneArgs a) {
  __shared__ int32_t sWave[SCN_T / 64];
  const int32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const ScnList L = scn_list(a, s);
  if (L.n <= 0 || !a.ok[s]) {  // (uniform: no barrier has been passed)
    if (tid == 0) a.n_out[s] = 0;
    return;
  }
  const int32_t ntiles = (int32_t)(((int64_t)L.n + SCN_T - 1) / SCN_T);  // <= tiles_per_list: n <= the capacity the grid was sized for
  int32_t *tc = a.tile_cnt + (int64_t)s * a.tiles_per_list;
  int32_t base = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += SCN_T) {
    const int32_t t = t0 + tid;
    const int32_t v = t < ntiles ? tc[t] : 0;
    const int32_t incl = vh_wave_scan(v);
    if (lane == 63) sWave[w] = incl;
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t k = 0; k < SCN_T / 64; k++) { const int32_t x = sWave[k]; before += k < w ? x : 0; total += x; }
    if (t < ntiles) tc[t] = base + before + incl - v;
    base += total;
    __syncthreads();
  }
  if (tid == 0) a.n_out[s] = base;
}

}  // namespace

// The three launches on one stream.  The caller keeps n_lists * tiles_per_list below 2^30 and tiles_per_list >=
// ceil(longest list / VH_SCENE_TILE).
void vh_launch_scene_points(const VhSceneArgs &a, bool mono, hipStream_t st) {
  const dim3 grid((uint32_t)a.lists.n_lists * (uint32_t)a.tiles_per_list), block(SCN_T);
  if (mono) hipLaunchKernelGGL(scene_flag_mono_kernel, grid, block, 0, st, a);
  else hipLaunchKernelGGL(scene_flag_stereo_kernel, grid, block, 0, st, a);
  vh_launch_scene_scan(a, st);
  if (mono) hipLaunchKernelGGL(scene_store_mono_kernel, grid, block, 0, st, a);
  else hipLaunchKernelGGL(scene_store_stereo_kernel, grid, block, 0, st, a);
}

// The scan alone, for every stage that compacts tiles of VH_SCENE_TILE records in list order (kernels_landmark.hip): it
// reads the lists' lengths (never a record), ok, tile_cnt and tiles_per_list, and writes tile_cnt and n_out.
void vh_launch_scene_scan(const VhSceneArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(scene_scan_kernel, dim3(a.lists.n_lists), dim3(SCN_T), 0, st, a);
}
