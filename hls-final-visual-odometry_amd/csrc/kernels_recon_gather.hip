// kernels_recon_gather.hip -- from tracked match lists to the arrays recon_kernel reads, on gfx950.
//
// A lost track is a record that no record of the next list continues.  Its pixels lie along its `prev` chain, one record
// per list, back through the lists of earlier frames; the ring (VhReconRec, vh_dev.h) keeps what that walk needs of the
// last `ring_slots` lists.  Per reconstruct call, on the stream that linked the lists:
//   recon_store   two launches.  The first copies every record's four left-camera floats and its vh_track prev / age /
//                 birth_pos into the slot of its list and clears the record's continued mark; the second marks, for every
//                 record with prev >= 0, the continued record in the slot of the list before.  A slot is cleared by the
//                 first launch only and marked by the second only, so no mark is ever cleared after it was set.
//   recon_tails   over the lists that have a successor now: every unmarked record ends a lost track.  The counting mode
//                 adds up tracks and pixels (frames = age + 1; a track with age > history takes no pixels), the host sizes
//                 the gather buffers, the appending mode writes one VhReconTail per track.  One atomic per wave hands out
//                 the track indices AND the pixel offsets (tracks << 40 | pixels), so that track t's pixels end where
//                 track t + 1's begin -- offsets[] as recon_kernel reads it.
//   recon_gather  one lane per solved track walks prev from the last record to the first and writes the pixels back to
//                 front, ending with the head's (u1p, v1p); fills first_frame, offsets and the identity order.
// The list axis: a frame holds lists_per_frame lists, one per camera stream -- 1 on a sequence
// handle, S on a group.  blockIdx.y of the store, mark and tails launches runs over (frame, stream); a record's
// predecessor, and every step of the gather's walk, stays in the slots of its own stream.
// Gather / scatter kernels bound by random sectors (as kernels_track.hip): a walk step is one dependent 32-byte record.
// Every store is a plain vector store.  Indices that address a STORE are bounded in the shipped build too.
#include "vh_dev.h"
#include "vh_wave.h"
#include "../../include/viso_hip.h"

#include <algorithm>

static_assert(sizeof(VhReconRec) == 32 && sizeof(VhReconTail) == 32 && sizeof(vh_p_match) == 48, "record layouts");

namespace {

__device__ inline int32_t rg_count(const VhReconGatherArgs &a, int64_t list) {
  const int32_t n = a.counts[list], cap = a.count_cap < a.ring_cap ? a.count_cap : a.ring_cap;
  return n < 0 ? 0 : (n < cap ? n : cap);
}
__device__ inline int32_t rg_slot(const VhReconGatherArgs &a, int64_t frame, int32_t stream) {  // (frames are >= 0)
  return (int32_t)(frame % a.ring_slots) * a.lists_per_frame + stream;
}
// blockIdx.y of a launch over the lists of some frames -> (frame index in the launch, stream)
__device__ inline int32_t rg_split(const VhReconGatherArgs &a, int32_t *stream) {
  const int32_t y = (int32_t)blockIdx.y, f = y / a.lists_per_frame;
  *stream = y - f * a.lists_per_frame;
  return f;
}

__global__ void __launch_bounds__(256) recon_store_kernel(VhReconGatherArgs a) {
  int32_t stream;
  const int32_t row = a.row_lo + rg_split(a, &stream), slot = rg_slot(a, a.frame0 + row, stream);
  const int64_t list = row + (int64_t)stream * a.stream_stride;
  const int32_t n = rg_count(a, list);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.ring_count[slot] = n;
  const float4 *__restrict__ pm = (const float4 *)(a.pm + list * a.pm_stride);  // 3 per record: {u1p v1p i1p u2p} {v2p i2p u1c v1c} {..}
  const vh_track *__restrict__ trk = a.trk + list * a.trk_stride;
  float4 *__restrict__ out = (float4 *)(a.ring + (int64_t)slot * a.ring_cap);
  const bool heads = row == a.row_lo && !a.pred_valid;
  for (int32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
    const float4 q0 = pm[3 * (int64_t)j], q1 = pm[3 * (int64_t)j + 1];
    const vh_track t = trk[j];
    int4 h;
    h.x = heads ? -1 : t.prev; h.y = heads ? 1 : t.age; h.z = heads ? j : t.birth_pos; h.w = 0;
    out[2 * (int64_t)j] = make_float4(q0.x, q0.y, q1.z, q1.w);
    ((int4 *)out)[2 * (int64_t)j + 1] = h;
  }
}

__global__ void __launch_bounds__(256) recon_mark_kernel(VhReconGatherArgs a) {
  int32_t stream;
  const int32_t row = a.row_lo + rg_split(a, &stream);
  if (row == a.row_lo && !a.pred_valid) return;
  const int32_t slot = rg_slot(a, a.frame0 + row, stream), pslot = rg_slot(a, a.frame0 + row - 1, stream);  // the same stream, one frame back
  const int32_t n = a.ring_count[slot], pn = a.ring_count[pslot];
  const VhReconRec *__restrict__ rec = a.ring + (int64_t)slot * a.ring_cap;
  VhReconRec *__restrict__ pred = a.ring + (int64_t)pslot * a.ring_cap;
  for (int32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
    int32_t prev = rec[j].prev;
    if (prev < 0) continue;
    VH_CHECK_RANGE(a, 10, prev, 0, pn);
    if (prev < pn) pred[prev].cont = 1;
  }
}

template <int APPEND> __global__ void __launch_bounds__(256) recon_tails_kernel(VhReconGatherArgs a) {
  int32_t stream;
  const int64_t frame = a.tail_lo + rg_split(a, &stream);
  const int32_t slot = rg_slot(a, frame, stream), n = a.ring_count[slot], lane = threadIdx.x & 63;
  const int4 *__restrict__ half = (const int4 *)(a.ring + (int64_t)slot * a.ring_cap);
  for (int32_t base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {  // (uniform per workgroup: the waves vote)
    const int32_t j = base + threadIdx.x;
    int4 h = make_int4(-1, 0, 0, 1);
    if (j < n) h = half[2 * (int64_t)j + 1];
    const bool lost = h.w == 0, old = lost && h.y > a.history, solved = lost && !old;
    const uint64_t m_solved = __ballot(solved), m_old = __ballot(old);
    if ((m_solved | m_old) == 0) continue;
    const int32_t frames = h.y + 1, incl = vh_wave_scan(solved ? frames : 0), px = __shfl(incl, 63, 64);
    const int32_t ns = __popcll(m_solved), no = __popcll(m_old);
    if (!APPEND) {
      if (lane == 0) {
        if (ns) { atomicAdd(a.totals + 0, (unsigned long long)ns); atomicAdd(a.totals + 1, (unsigned long long)px); }
        if (no) atomicAdd(a.totals + 2, (unsigned long long)no);
      }
      continue;
    }
    uint32_t lo = 0, hi = 0, ob = 0;
    if (lane == 0) {
      if (ns) { const unsigned long long b = atomicAdd(a.totals + 3, ((unsigned long long)ns << 40) | (unsigned long long)px); lo = (uint32_t)b; hi = (uint32_t)(b >> 32); }
      if (no) ob = (uint32_t)atomicAdd(a.totals + 4, (unsigned long long)no);
    }
    lo = __shfl(lo, 0, 64); hi = __shfl(hi, 0, 64); ob = __shfl(ob, 0, 64);
    const uint64_t b = ((uint64_t)hi << 32) | lo;
    VhReconTail t;
    t.lost_off = (int32_t)(frame + 1 - a.window0); t.birth_off = (int32_t)(frame - h.y + 1 - a.window0);
    t.birth_pos = h.z; t.frames = frames; t.pos = j; t.stream = stream; t.reserved = 0;
    if (solved) {
      const int64_t idx = (int64_t)(b >> 40) + vh_wave_rank(m_solved), off = (int64_t)(b & ((1ull << 40) - 1)) + incl - frames;
      t.px_off = (int32_t)off;
      if (idx < a.n_solved && off + frames <= a.n_pixels) a.tails[idx] = t;
    } else if (old) {
      const int64_t idx = (int64_t)a.n_tails - 1 - ((int64_t)ob + vh_wave_rank(m_old));
      t.px_off = -1;
      if (idx >= a.n_solved && idx < a.n_tails) a.tails[idx] = t;
    }
  }
}

__global__ void __launch_bounds__(256) recon_gather_kernel(VhReconGatherArgs a) {
  const int32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_solved) return;
  const VhReconTail tail = a.tails[t];
  const int32_t frames = tail.frames, off = tail.px_off;
  a.first_frame[t] = tail.stream * a.window + tail.birth_off - 1;  // (one concatenated table: a window per stream)
  a.offsets[t] = off;
  a.order[t] = t;
  if (t == a.n_solved - 1) a.offsets[t + 1] = off + frames;
  if (off < 0 || (int64_t)off + frames > a.n_pixels) return;  // (never: recon_tails appended inside the totals it counted)
  float2 *__restrict__ px = (float2 *)a.pixels + off;
  int32_t fslot = (int32_t)((a.window0 + tail.lost_off - 1) % a.ring_slots), pos = tail.pos;
  for (int32_t k = frames - 1; k >= 1; k--) {
    const int32_t slot = fslot * a.lists_per_frame + tail.stream;
    VH_CHECK_RANGE(a, 11, pos, 0, a.ring_count[slot]);
    pos = pos < 0 ? 0 : (pos < a.ring_cap ? pos : a.ring_cap - 1);  // (a load only, but never outside the ring)
    const float4 *rec = (const float4 *)(a.ring + (int64_t)slot * a.ring_cap + pos);
    const int32_t prev = ((const int4 *)rec)[1].x;  // the walk's dependent load; the pixels are off its path
    const float4 q = rec[0];
    px[k] = make_float2(q.z, q.w);
    if (k == 1) px[0] = make_float2(q.x, q.y);
    pos = prev;
    fslot = fslot ? fslot - 1 : a.ring_slots - 1;
  }
}

// (lists <= 65 535: the hosts' limits on rows and streams)
dim3 list_grid(int32_t cap, int64_t lists) { return dim3((unsigned)std::min(std::max((cap + 1023) / 1024, 1), 64), (unsigned)lists); }

}  // namespace

void vh_launch_recon_store(const VhReconGatherArgs &a, hipStream_t st) {
  if (a.rows <= a.row_lo) return;
  hipLaunchKernelGGL(recon_store_kernel, list_grid(a.ring_cap, (int64_t)(a.rows - a.row_lo) * a.lists_per_frame), dim3(256), 0, st, a);
  hipLaunchKernelGGL(recon_mark_kernel, list_grid(a.ring_cap, (int64_t)(a.rows - a.row_lo) * a.lists_per_frame), dim3(256), 0, st, a);
}
void vh_launch_recon_tails(const VhReconGatherArgs &a, int32_t append, hipStream_t st) {
  if (a.tail_hi <= a.tail_lo) return;
  if (append) hipLaunchKernelGGL(recon_tails_kernel<1>, list_grid(a.ring_cap, (a.tail_hi - a.tail_lo) * a.lists_per_frame), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(recon_tails_kernel<0>, list_grid(a.ring_cap, (a.tail_hi - a.tail_lo) * a.lists_per_frame), dim3(256), 0, st, a);
}
void vh_launch_recon_gather(const VhReconGatherArgs &a, hipStream_t st) {
  if (a.n_solved < 1) return;
  hipLaunchKernelGGL(recon_gather_kernel, dim3((unsigned)((a.n_solved + 255) / 256)), dim3(256), 0, st, a);
}
