// kernels_track.hip -- feature tracks: link the match lists of consecutive frame pairs (include/viso_hip.h: vh_track,
// DESIGN.md section 4.6).
//
// Record j of a list (A -> B) continues record q of its predecessor list (Z -> A) iff i1c(q) == i1p(j): the same left
// feature of frame A.  Three kernels per match call, whatever the number of rows, on the stream that emitted the lists:
//   track_scatter  per record, two first-writer bids by feature index: tab_c[slot][i1c] (who holds this feature as its
//                  current one: what the NEXT list looks up) and tab_p[row][i1p] (who continues this feature: the
//                  lowest j wins, so that a predecessor record is continued at most once).
//   track_link     per record, prev = the predecessor list's tab_c at i1p, if the record won its own bid in tab_p; where
//                  the predecessor is a row of the same launch (sequence handles, vh_link_tracks) the forward link is
//                  left in the predecessor's record.
//   track_rank     one lane per track head (a record without prev, or whose predecessor list is final already: the
//                  carry, or the previous step of a group) walks its chain forward through the rows of the launch and
//                  writes birth and age.  Every record lies on exactly one chain, chains run strictly from row to
//                  row + 1, so every record is written once.
// The tables hold epoch << 24 | (2^24 - 1 - position) and are bid for with atomicMax: a newer epoch beats whatever an
// earlier match call left there (no reset per step; the pixel mask of the flow method works the same way), the lowest
// position wins inside an epoch.  These are gather / scatter kernels bound by random 64-byte sectors, not by issue.
#include "vh_dev.h"
#include "../../include/viso_hip.h"

#include <algorithm>

static_assert(sizeof(vh_track) == 24, "vh_track layout");

namespace {

__device__ inline int32_t track_count(const VhTrackArgs &t, int32_t row) {
  const int32_t n = t.counts[row];
  return n < 0 ? 0 : (n < t.count_cap ? n : t.count_cap);
}
__device__ inline uint32_t track_key(uint32_t epoch, int32_t pos) { return (epoch << VH_TRACK_POS_BITS) | (VH_TRACK_POS_MASK - (uint32_t)pos); }
__device__ inline int32_t track_pos(uint32_t key, uint32_t epoch) {
  return (epoch != 0u && (key >> VH_TRACK_POS_BITS) == epoch) ? (int32_t)(VH_TRACK_POS_MASK - (key & VH_TRACK_POS_MASK)) : -1;
}

__global__ void __launch_bounds__(256) track_scatter_kernel(VhTrackArgs t) {
  const int32_t row = blockIdx.y, slot = t.slot0 + row, n = track_count(t, row);
  if (blockIdx.x == 0 && threadIdx.x == 0) t.slot_count[slot] = n;
  const int32_t *__restrict__ pm = (const int32_t *)t.pm + (int64_t)row * t.pm_stride * 12;
  uint32_t *__restrict__ tc = t.tab_c + (int64_t)slot * t.n_index;
  uint32_t *__restrict__ tp = t.tab_p + (int64_t)row * t.n_index;
  vh_track *__restrict__ trk = t.trk + (int64_t)slot * t.trk_stride;
  for (int32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
    const int32_t i1p = pm[12 * (int64_t)j + 2], i1c = pm[12 * (int64_t)j + 8];
    const uint32_t key = track_key(t.epoch, j);
    if (i1c >= 0 && i1c < t.n_index) atomicMax(tc + i1c, key);
    if (i1p >= 0 && i1p < t.n_index) atomicMax(tp + i1p, key);
    trk[j].reserved = -1;  // (the forward link until track_rank has passed)
  }
}

__global__ void __launch_bounds__(256) track_link_kernel(VhTrackArgs t) {
  const int32_t row = blockIdx.y, slot = t.slot0 + row, n = track_count(t, row);
  bool inl = false;
  const int32_t pred = vh_track_pred(t, row, &inl);
  const uint32_t pe = inl ? t.epoch : t.pred_epoch;
  const int32_t *__restrict__ pm = (const int32_t *)t.pm + (int64_t)row * t.pm_stride * 12;
  const uint32_t *__restrict__ tp = t.tab_p + (int64_t)row * t.n_index;
  vh_track *__restrict__ trk = t.trk + (int64_t)slot * t.trk_stride;
  for (int32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
    const int32_t i1p = pm[12 * (int64_t)j + 2];
    int32_t prev = -1;
    if (pred >= 0 && i1p >= 0 && i1p < t.n_index && track_pos(tp[i1p], t.epoch) == j) {
      prev = track_pos(t.tab_c[(int64_t)pred * t.n_index + i1p], pe);
      if (prev >= 0) VH_CHECK_RANGE(t, 8, prev, 0, t.slot_count[pred]);
    }
    trk[j].prev = prev;
    if (prev >= 0 && inl) t.trk[(int64_t)pred * t.trk_stride + prev].reserved = j;
  }
}

// (Whole-record store.  A lane of the record's own row may be reading o->prev at the same time to decide that it is no
//  head: the value stored is the one already there and the field is an aligned dword of its own, so that read sees it
//  either way.  Packing prev with another field, or storing a different prev here, would break that.)
__device__ inline void track_store(vh_track *o, int64_t bf, int32_t bp, int32_t age, int32_t prev) {
  vh_track r;
  r.birth_frame = bf; r.birth_pos = bp; r.age = age; r.prev = prev; r.reserved = 0;
  *o = r;
}

__global__ void __launch_bounds__(256) track_rank_kernel(VhTrackArgs t) {
  const int32_t row = blockIdx.y, slot = t.slot0 + row, n = track_count(t, row);
  bool inl = false;
  const int32_t pred = vh_track_pred(t, row, &inl);
  for (int32_t j0 = blockIdx.x * 256 + threadIdx.x; j0 < n; j0 += gridDim.x * 256) {
    vh_track *rec = t.trk + (int64_t)slot * t.trk_stride + j0;
    const int32_t prev = rec->prev;
    // Not a head: the head of this chain comes through here and writes the record.  Only `prev` is read on this path, and
    // a walker never changes it (track_store); a head's own `reserved` is written by track_link alone, never by a walker,
    // because no chain enters a head.
    if (prev >= 0 && inl) continue;
    int64_t bf = t.serial0 + (t.chain ? row : 0);
    int32_t bp = j0, age = 1;
    if (prev >= 0) {  // continues a list that is final: the carry, or the previous step of a group
      const vh_track p = t.trk[(int64_t)pred * t.trk_stride + prev];
      bf = p.birth_frame; bp = p.birth_pos; age = p.age + 1;
    }
    int32_t nxt = rec->reserved;
    track_store(rec, bf, bp, age, prev);
    for (int32_t r = row + 1; nxt >= 0 && r < t.rows; r++) {
      VH_CHECK_RANGE(t, 9, nxt, 0, t.slot_count[t.slot0 + r]);
      rec = t.trk + (int64_t)(t.slot0 + r) * t.trk_stride + nxt;
      const int32_t pv = rec->prev;
      nxt = rec->reserved;
      track_store(rec, bf, bp, ++age, pv);
    }
  }
}

// slot src -> slot dst: table, records and count (the carry of a sequence handle)
__global__ void __launch_bounds__(256) track_copy_kernel(VhTrackArgs t, int32_t src, int32_t dst) {
  const int32_t n = t.slot_count[src], step = gridDim.x * 256, i0 = blockIdx.x * 256 + threadIdx.x;
  if (i0 == 0) t.slot_count[dst] = n;
  for (int32_t i = i0; i < t.n_index; i += step) t.tab_c[(int64_t)dst * t.n_index + i] = t.tab_c[(int64_t)src * t.n_index + i];
  for (int32_t i = i0; i < n; i += step) t.trk[(int64_t)dst * t.trk_stride + i] = t.trk[(int64_t)src * t.trk_stride + i];
}

// the epoch counter has come round: the entries of epoch `live` in the slots [keep0, keep1) become epoch 1, all others empty
__global__ void __launch_bounds__(256) track_retag_kernel(uint32_t *tab, int64_t n_index, int64_t n_slots, int64_t keep0, int64_t keep1,
                                                          uint32_t live) {
  const int64_t total = n_index * n_slots;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t slot = i / n_index;
    const uint32_t k = tab[i];
    tab[i] = (slot >= keep0 && slot < keep1 && live != 0u && (k >> VH_TRACK_POS_BITS) == live) ? ((1u << VH_TRACK_POS_BITS) | (k & VH_TRACK_POS_MASK)) : 0u;
  }
}

dim3 track_grid(const VhTrackArgs &t) { return dim3((unsigned)std::min(std::max((t.count_cap + 1023) / 1024, 1), 64), (unsigned)t.rows); }

}  // namespace

void vh_launch_track_scatter(const VhTrackArgs &t, hipStream_t st) {
  if (t.rows > 0) hipLaunchKernelGGL(track_scatter_kernel, track_grid(t), dim3(256), 0, st, t);
}
void vh_launch_track_link(const VhTrackArgs &t, hipStream_t st) {
  if (t.rows > 0) hipLaunchKernelGGL(track_link_kernel, track_grid(t), dim3(256), 0, st, t);
}
void vh_launch_track_rank(const VhTrackArgs &t, hipStream_t st) {
  if (t.rows > 0) hipLaunchKernelGGL(track_rank_kernel, track_grid(t), dim3(256), 0, st, t);
}
void vh_launch_track_copy(const VhTrackArgs &t, int32_t src, int32_t dst, hipStream_t st) {
  const int32_t work = std::max(t.n_index, t.count_cap);
  hipLaunchKernelGGL(track_copy_kernel, dim3((unsigned)std::min(std::max((work + 1023) / 1024, 1), 256)), dim3(256), 0, st, t, src, dst);
}
void vh_launch_track_retag(uint32_t *tab, int64_t n_index, int64_t n_slots, int64_t keep0, int64_t keep1, uint32_t live, hipStream_t st) {
  const int64_t total = n_index * n_slots;
  hipLaunchKernelGGL(track_retag_kernel, dim3((unsigned)std::min<int64_t>(std::max<int64_t>((total + 1023) / 1024, 1), 4096)), dim3(256), 0, st,
                     tab, n_index, n_slots, keep0, keep1, live);
}
