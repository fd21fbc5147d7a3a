// kernels_landmark_chain.hip -- the landmarks of lists that are the rows of one chain, on gfx950.
//
// The lists of a call are rows 0 .. n - 1: list s's predecessor is list s - 1 of the same call (the rows of a sequence
// handle's chunk; the lists vh_link_tracks linked), list 0's a carry state array or none.  The state a record continues
// is then computed by the same call, so the gather of kernels_landmark.hip becomes a walk along the track chains that
// carries the 48-byte state in registers from row to row -- track_rank's shape (kernels_track.hip) with the rule of
// vh_landmark.h at every hop.  A list is cut into tiles of LMK_T records, a 256-lane workgroup per tile:
//   landmark_index  kernels_landmark.hip's own kernel: obs[src_pos] = the point's position (obs and next were filled with -1);
//   landmark_link   one lane per record of the rows >= 1: next[row - 1][prev] = j where 0 <= prev < n[row - 1].  A
//                   predecessor record is continued by at most one record (the link rule of section 4.6; the stateless
//                   entry refuses lists that break it), so there is no contest and no atomic;
//   landmark_chain  one lane per head -- a record of list 0, or one whose prev lies outside its predecessor list: zeros, or
//                   carry[prev] in list 0; then row by row: the record's link and observation index, the rule, the state
//                   as three 16-byte stores, obs put back to -1 where the record emits nothing.  The next row's link and
//                   index are loaded before this row's point, so the dependent hop runs under the point load and the
//                   divisions.  Every record lies on exactly one chain: every state is written once, no atomics;
//   landmark_count  one lane per record: obs >= 0 into the tile's survivor count;
//   scene_scan and landmark_store as in kernels_landmark.hip, unchanged.
// No workgroup waits for another one: the order is that of the launches on one stream.
#include "vh_landmark.h"
#include "vh_wave.h"

namespace {

#define LMK_T VH_SCENE_TILE
static_assert(LMK_T == 256, "vh_compact4 joins four waves; the tiles are scene_scan's");

__global__ void __launch_bounds__(LMK_T)
landmark_link_kernel(VhLandmarkChainArgs c) {
  const VhLandmarkArgs &a = c.a;
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  if (s == 0) return;
  const LmkList L = lmk_list(a, s);
  const int64_t j = (int64_t)tile * LMK_T + threadIdx.x;
  if (j >= L.n) return;
  const LmkList P = lmk_list(a, s - 1);
  const int32_t q = a.trk[L.rec0 + j].prev;
  if (q >= 0 && q < P.n) c.next[P.rec0 + q] = (int32_t)j;
}

__global__ void __launch_bounds__(LMK_T)
landmark_chain_kernel(VhLandmarkChainArgs c) {
  const VhLandmarkArgs &a = c.a;
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  LmkList L = lmk_list(a, s);
  const int64_t j0 = (int64_t)tile * LMK_T + threadIdx.x;
  if (j0 >= L.n) return;  // (no barrier below)
  int64_t r = L.rec0 + j0;
  const int32_t q = a.trk[r].prev;
  LmkState st = lmk_zero();
  if (s > 0) {
    // Not a head: the head of this chain comes through here and writes the record
    if (q >= 0 && q < lmk_list(a, s - 1).n) return;
  } else if (c.carry) {
    const int32_t nc = c.carry_count ? min(max(*c.carry_count, 0), c.carry_cap) : c.n_carry;
    if (q >= 0 && q < nc) st = lmk_load(c.carry + q);                // 1. carry
  }
  int32_t nx = c.next[r], k = a.obs[r];
  asm volatile("" : "+v"(nx), "+v"(k));  // (both have arrived before the loop: no load is pending across its head, see below)
  for (int32_t row = s;; row++) {
    // the next row's record first: its link and index do not wait for this row's point
    const bool more = nx >= 0 && row + 1 < a.n_lists;
    LmkList Ln = L;
    int64_t rn = r;
    int32_t nxn = -1, kn = -1;
    if (more) {
      // (every lane of the workgroup began in row s and has made the same number of hops: the row is uniform, its
      //  offsets and counts are scalar loads)
      Ln = lmk_list(a, __builtin_amdgcn_readfirstlane(row + 1));
      VH_CHECK_RANGE(c, 15, nx, 0, Ln.n);
      rn = Ln.rec0 + nx;
      nxn = c.next[rn]; kn = a.obs[rn];
    }
    const bool seen = k >= 0 && k < L.n_pt;
    const bool keep = lmk_step(st, a.lp, seen ? a.pts + L.pt0 + k : nullptr);
    lmk_store(a.state_out + r, st);                                  // 4.
    if (seen && !keep) a.obs[r] = -1;
    // (the first use of the next row's two loads: without it the compiler copies them into the loop's registers, and
    //  waits for them, in front of this row's point load)
    asm volatile("" : "+v"(nxn), "+v"(kn));
    if (!more) break;
    L = Ln; r = rn; nx = nxn; k = kn;
  }
}

__global__ void __launch_bounds__(LMK_T)
landmark_count_kernel(VhLandmarkChainArgs c) {
  __shared__ int32_t sWave[LMK_T / 64];
  const VhLandmarkArgs &a = c.a;
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  const int32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const LmkList L = lmk_list(a, s);
  if ((int64_t)tile * LMK_T >= L.n) return;  // (uniform)
  const int64_t j = (int64_t)tile * LMK_T + tid;
  const int32_t k = j < L.n ? a.obs[L.rec0 + j] : -1;
  const VhCompact cp = vh_compact4(k >= 0 && k < L.n_pt, sWave, w, lane);
  if (tid == 0) a.tile_cnt[(int64_t)s * a.tiles_per_list + tile] = cp.total;
}

}  // namespace

const char *vh_landmark_chain_scope(int32_t k) {
  static const char *const names[VH_LANDMARK_CHAIN_STAGES] = {"landmark_index", "landmark_link", "landmark_chain", "landmark_count",
                                                               "landmark_scan", "landmark_store"};
  return names[k];
}

hipError_t vh_launch_landmarks_chain_clear(const VhLandmarkChainArgs &c, int64_t obs_elems, hipStream_t st) {
  // obs and next are the halves of one array: one memset puts both to -1
  return hipMemsetAsync(c.a.obs, 0xFF, sizeof(int32_t) * 2 * (size_t)obs_elems, st);
}

void vh_launch_landmarks_chain_stage(const VhLandmarkChainArgs &c, int32_t k, hipStream_t st) {
  const dim3 grid((uint32_t)c.a.n_lists * (uint32_t)c.a.tiles_per_list), block(LMK_T);
  switch (k) {
    case 0: vh_launch_landmark_index(c.a, st); break;
    case 1: if (c.a.n_lists > 1) hipLaunchKernelGGL(landmark_link_kernel, grid, block, 0, st, c); break;
    case 2: hipLaunchKernelGGL(landmark_chain_kernel, grid, block, 0, st, c); break;
    case 3: hipLaunchKernelGGL(landmark_count_kernel, grid, block, 0, st, c); break;
    case 4: vh_launch_landmark_scan(c.a, st); break;
    default: vh_launch_landmark_store(c.a, st); break;
  }
}
