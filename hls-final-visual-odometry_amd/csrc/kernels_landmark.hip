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
#include "vh_landmark.h"
#include "vh_wave.h"

namespace {

#define LMK_T VH_SCENE_TILE
static_assert(LMK_T == 256, "vh_compact4 joins four waves; the tiles are scene_scan's");
static_assert(sizeof(vh_landmark) == 48 && sizeof(vh_track) == 24, "the vector loads and stores below");

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
    const bool seen = k >= 0 && k < L.n_pt;
    keep = lmk_step(st, a.lp, seen ? a.pts + L.pt0 + k : nullptr);     // 2., 3., 5. (vh_landmark.h)
    if (seen && !keep) a.obs[r] = -1;
    lmk_store(a.state_out + r, st);                                    // 4.
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

static dim3 landmark_grid(const VhLandmarkArgs &a) { return dim3((uint32_t)a.n_lists * (uint32_t)a.tiles_per_list); }

// the pieces the chain form shares (kernels_landmark_chain.hip)
void vh_launch_landmark_index(const VhLandmarkArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(landmark_index_kernel, landmark_grid(a), dim3(LMK_T), 0, st, a);
}
void vh_launch_landmark_scan(const VhLandmarkArgs &a, hipStream_t st) {
  VhSceneArgs sc{};  // what scene_scan reads: the record lists' lengths, ok, the tile counts
  sc.lists = a.rec_offsets ? VhLists::packed(nullptr, a.rec_offsets, a.n_lists)
                           : VhLists::slots(nullptr, a.rec_stride, a.rec_counts, (int32_t)a.rec_stride, a.n_lists);
  sc.tiles_per_list = a.tiles_per_list; sc.ok = a.ok; sc.out_stride = a.rec_stride; sc.tile_cnt = a.tile_cnt; sc.n_out = a.n_out;
  vh_launch_scene_scan(sc, st);
}
void vh_launch_landmark_store(const VhLandmarkArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(landmark_store_kernel, landmark_grid(a), dim3(LMK_T), 0, st, a);
}

hipError_t vh_launch_landmarks(const VhLandmarkArgs &a, int64_t obs_elems, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(a.obs, 0xFF, sizeof(int32_t) * (size_t)obs_elems, st);
  if (e != hipSuccess) return e;
  vh_launch_landmark_index(a, st);
  hipLaunchKernelGGL(landmark_fuse_kernel, landmark_grid(a), dim3(LMK_T), 0, st, a);
  vh_launch_landmark_scan(a, st);
  vh_launch_landmark_store(a, st);
  return hipSuccess;
}
