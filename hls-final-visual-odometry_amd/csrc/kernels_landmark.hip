// kernels_landmark.hip -- the scene points of a step fused along the feature tracks, on gfx950.
//
// For every record j of every tracked list of a call: the state of the record it continues in the predecessor list
// (vh_track.prev: a gather, never dereferenced outside that list), this step's scene point of the record if it has one
// (vh_scene_point.src_pos == j), and the rule of include/viso_hip.h -- carry, gap count, gate, accumulate -- in double,
// built with -ffp-contract=off: every product and sum rounds on its own, sums are added left to right.  The chain of sums
// of one track is sequential over the steps and independent of every other record, so the bytes are those of a plain
// host loop.
//
// A list is cut into tiles of LMK_T records and a 256-lane workgroup takes one tile, one record (or point) per lane:
//   landmark_index  one lane per scene point: obs[src_pos] = the point's position (obs was filled with -1 before);
//   landmark_fuse   one lane per record: the rule; the 48-byte state written as three 16-byte stores; obs[j] is put back
//                   to -1 where the record emits nothing, so that obs >= 0 is the keep flag; the tile's survivor count;
//   scene_scan      kernels_scene.hip's own kernel through vh_launch_scene_scan, one workgroup per list: the tile counts
//                   become the tiles' first output positions, their sum the list's count (0 for a list without points);
//   landmark_store  state_out[j] and trk[j] read again, three divisions and one sqrt, the 48-byte landmark written once,
//                   as three 16-byte stores, at the tile's position + vh_compact4's rank: thread order is list order.
// Every output position is a function of the keep decisions alone: no atomics, the same bytes from run to run, whatever
// else the launch holds.
#include "vh_dev.h"
#include "vh_wave.h"

namespace {

#define LMK_T VH_SCENE_TILE
static_assert(LMK_T == 256, "vh_compact4 joins four waves; the tiles are scene_scan's");
static_assert(sizeof(vh_landmark_state) == 48 && sizeof(vh_landmark) == 48 && sizeof(vh_scene_point) == 32 && sizeof(vh_track) == 24,
              "the vector loads and stores below");

struct LmkList {
  int64_t rec0, pt0, prev0;    // first element of the list in trk / state_out / out / obs, in pts, in prev
  int32_t n, n_pt, n_prev;
};
__device__ __forceinline__ int32_t lmk_count(const int32_t *counts, int32_t s, int64_t stride) {
  return (int32_t)min((int64_t)max(counts[s], 0), stride);
}
__device__ __forceinline__ LmkList lmk_list(const VhLandmarkArgs &a, int32_t s) {
  LmkList L;
  if (a.rec_offsets) { L.rec0 = a.rec_offsets[s]; L.n = a.rec_offsets[s + 1] - a.rec_offsets[s]; }
  else { L.rec0 = (int64_t)s * a.rec_stride; L.n = lmk_count(a.rec_counts, s, a.rec_stride); }
  if (a.pt_offsets) { L.pt0 = a.pt_offsets[s]; L.n_pt = a.pt_offsets[s + 1] - a.pt_offsets[s]; }
  else { L.pt0 = (int64_t)s * a.pt_stride; L.n_pt = lmk_count(a.pt_counts, s, a.pt_stride); }
  L.prev0 = 0; L.n_prev = 0;
  if (a.prev) {
    if (a.prev_offsets) { L.prev0 = a.prev_offsets[s]; L.n_prev = a.prev_offsets[s + 1] - a.prev_offsets[s]; }
    else { L.prev0 = (int64_t)s * a.prev_stride; L.n_prev = lmk_count(a.prev_counts, s, a.prev_stride); }
  }
  return L;
}

struct LmkState {
  double sw, swx, swy, swz;
  int32_t n_obs, n_missed;
};
__device__ __forceinline__ LmkState lmk_zero() { LmkState st; st.sw = st.swx = st.swy = st.swz = 0.0; st.n_obs = st.n_missed = 0; return st; }
__device__ __forceinline__ LmkState lmk_load(const vh_landmark_state *p) {
  const double2 a = ((const double2 *)p)[0], b = ((const double2 *)p)[1];
  const int2 c = ((const int2 *)p)[4];
  LmkState st;
  st.sw = a.x; st.swx = a.y; st.swy = b.x; st.swz = b.y; st.n_obs = c.x; st.n_missed = c.y;
  return st;
}

// grid: n_lists * tiles_per_list workgroups, list-major (a list holds no more points than records)
__global__ void __launch_bounds__(LMK_T)
landmark_index_kernel(VhLandmarkArgs a) {
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  const LmkList L = lmk_list(a, s);
  const int64_t k = (int64_t)tile * LMK_T + threadIdx.x;
  if (k >= L.n_pt) return;
  const int32_t j = a.pts[L.pt0 + k].src_pos;
  if (j >= 0 && j < L.n) a.obs[L.rec0 + j] = (int32_t)k;  // (the entries refuse other lists; a handle's hold none)
}

__global__ void __launch_bounds__(LMK_T)
landmark_fuse_kernel(VhLandmarkArgs a) {
  __shared__ int32_t sWave[LMK_T / 64];
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const LmkList L = lmk_list(a, s);
  if ((int64_t)tile * LMK_T >= L.n) return;  // (uniform)
  const int64_t j = (int64_t)tile * LMK_T + tid;
  bool keep = false;
  if (j < L.n) {
    const int64_t r = L.rec0 + j;
    const int32_t q = a.trk[r].prev, k = a.obs[r];
    LmkState st = lmk_zero();
    if (q >= 0 && q < L.n_prev) st = lmk_load(a.prev + L.prev0 + q);  // 1. carry
    if (k < 0 || k >= L.n_pt) {                                        // 2. no observation
      if (st.n_obs > 0) {
        st.n_missed += 1;
        if (a.lp.max_missed >= 0 && st.n_missed > a.lp.max_missed) st = lmk_zero();
      }
    } else {                                                           // 3. the observation
      const float4 p = *(const float4 *)(a.pts + L.pt0 + k);
      const double x = p.x, y = p.y, z = p.z, sg = p.w;
      const double wt = sg > 0.0 ? 1.0 / (sg * sg) : 1.0;
      if (st.n_obs > 0) {
        const double T = a.lp.max_dist + a.lp.gate_sigma * sg;
        if (T > 0.0) {
          const double dx = x - st.swx / st.sw, dy = y - st.swy / st.sw, dz = z - st.swz / st.sw;
          if (dx * dx + dy * dy + dz * dz > T * T) st = lmk_zero();
        }
      }
      st.sw += wt; st.swx += wt * x; st.swy += wt * y; st.swz += wt * z;
      st.n_obs += 1; st.n_missed = 0;
      if (!(isfinite(st.sw) && isfinite(st.swx) && isfinite(st.swy) && isfinite(st.swz))) st = lmk_zero();
      else keep = st.n_obs >= a.lp.min_obs;                            // 5.
      if (!keep) a.obs[r] = -1;
    }
    double2 *o = (double2 *)(a.state_out + r);                         // 4.
    o[0] = make_double2(st.sw, st.swx);
    o[1] = make_double2(st.swy, st.swz);
    ((int4 *)o)[2] = make_int4(st.n_obs, st.n_missed, 0, 0);
  }
  const VhCompact c = vh_compact4(keep, sWave, w, lane);
  if (tid == 0) a.tile_cnt[(int64_t)s * a.tiles_per_list + tile] = c.total;
}

__global__ void __launch_bounds__(LMK_T)
landmark_store_kernel(VhLandmarkArgs a) {
  __shared__ int32_t sWave[LMK_T / 64];
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const LmkList L = lmk_list(a, s);
  if ((int64_t)tile * LMK_T >= L.n) return;
  const int64_t j = (int64_t)tile * LMK_T + tid;
  const int32_t k = j < L.n ? a.obs[L.rec0 + j] : -1;
  const bool keep = k >= 0 && k < L.n_pt;
  const VhCompact c = vh_compact4(keep, sWave, w, lane);
  if (keep) {  // rec0 + (survivors before the tile) + c.pos < rec0 + (survivors of the list) <= rec0 + n
    const int64_t r = L.rec0 + j;
    const LmkState st = lmk_load(a.state_out + r);
    const int2 *t = (const int2 *)(a.trk + r);  // {birth_frame} {birth_pos, age} {prev, reserved}
    const int2 t0 = t[0], t1 = t[1];
    const int32_t i1c = a.pts[L.pt0 + k].i1c;
    const float x = (float)(st.swx / st.sw), y = (float)(st.swy / st.sw), z = (float)(st.swz / st.sw);
    const float sigma = (float)sqrt(1.0 / st.sw);
    const int64_t dst = L.rec0 + a.tile_cnt[(int64_t)s * a.tiles_per_list + tile] + c.pos;
    float4 *o = (float4 *)(a.out + dst);
    o[0] = make_float4(x, y, z, sigma);
    o[1] = make_float4(__int_as_float(st.n_obs), __int_as_float(t1.y), __int_as_float(t0.x), __int_as_float(t0.y));
    o[2] = make_float4(__int_as_float(t1.x), __int_as_float((int32_t)j), __int_as_float(i1c), __int_as_float(k));
  }
}

}  // namespace

hipError_t vh_launch_landmarks(const VhLandmarkArgs &a, int64_t obs_elems, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(a.obs, 0xFF, sizeof(int32_t) * (size_t)obs_elems, st);
  if (e != hipSuccess) return e;
  const dim3 grid((uint32_t)a.n_lists * (uint32_t)a.tiles_per_list), block(LMK_T);
  hipLaunchKernelGGL(landmark_index_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(landmark_fuse_kernel, grid, block, 0, st, a);
  VhSceneArgs sc{};  // what scene_scan reads: the record lists' lengths, ok, the tile counts
  sc.lists = a.rec_offsets ? VhLists::packed(nullptr, a.rec_offsets, a.n_lists)
                           : VhLists::slots(nullptr, a.rec_stride, a.rec_counts, (int32_t)a.rec_stride, a.n_lists);
  sc.tiles_per_list = a.tiles_per_list; sc.ok = a.ok; sc.out_stride = a.rec_stride; sc.tile_cnt = a.tile_cnt; sc.n_out = a.n_out;
  vh_launch_scene_scan(sc, st);
  hipLaunchKernelGGL(landmark_store_kernel, grid, block, 0, st, a);
  return hipSuccess;
}
