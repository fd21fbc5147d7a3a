// engine_landmark.hip -- landmarks: the scene points of a step fused along the feature tracks (kernels_landmark.hip): on a
// handle's current tracked lists and the scene points of its last scene_points call, the state kept beside the track
// buffers; on caller-owned lists; along the rows of one chain (kernels_landmark_chain.hip): a sequence handle's chunk,
// caller-owned linked lists; and their part of the ABI.
#include "engine.h"

namespace vh_engine {

static bool landmark_params_ok(const vh_landmark_params *lp) { return lp && lp->min_obs >= 1; }

// The tracked lists of the current pair (tk.d_trk, buffer trk_cur) and the points scn.d_out / scn.d_n; the predecessor
// state: buffer trk_cur ^ 1, where it was computed for the very list that buffer holds.  Nothing goes up but the params.
int32_t Group::landmarks(const vh_landmark_params *lp, int32_t *counts) {
  if (!landmark_params_ok(lp) || !counts) return VH_ERR_INVALID_ARG;
  if (seq) return lmk_chain ? landmarks_chain(lp, counts) : VH_ERR_UNSUPPORTED;
  if (!trk_on || !allocated || last_method < 0 || !trk_cur_valid || !scene_current()) return VH_ERR_STATE;
  if (!inliers_current() || inl.from_host) return VH_ERR_STATE;  // (src_pos numbers the list the classification read: it must be the tracked one)
  const int32_t tiles = (mcap + VH_SCENE_TILE - 1) / VH_SCENE_TILE;
  if (!lmk.d_out) {  // one block, before any launch: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(static_cast<LandmarkArrays &>(lmk), nullptr, false, (size_t)S, (size_t)S * mcap, (size_t)tiles);
    if (rc) return rc;
    lmk.tiles = tiles;
    lmk.state_seq[0] = lmk.state_seq[1] = -1;
  }
  const int32_t cur = trk_cur, pred = trk_cur ^ 1;
  const bool has_prev = trk_pred_valid && lmk.state_seq[pred] >= 0 && lmk.state_seq[pred] == trk_fill_seq[pred];
  lmk.valid = false;
  lmk.state_seq[cur] = -1;  // (until the launches below have run)
  lmk.n.assign((size_t)S, 0);
  VhLandmarkArgs a{};
  a.lp = *lp;
  a.n_lists = S; a.tiles_per_list = lmk.tiles;
  a.trk = tk.d_trk + (size_t)cur * S * mcap; a.rec_counts = tk.d_tcount + (size_t)cur * S; a.rec_stride = mcap;
  a.pts = scn.d_out; a.pt_counts = scn.d_n; a.pt_stride = mcap; a.ok = scn.d_n;
  if (has_prev) { a.prev = lmk.d_state[pred]; a.prev_counts = tk.d_tcount + (size_t)pred * S; a.prev_stride = mcap; }
  a.state_out = lmk.d_state[cur]; a.out = lmk.d_out; a.obs = lmk.d_obs; a.tile_cnt = lmk.d_tiles; a.n_out = lmk.d_n;
  // (the tracks were linked on the post stream, the points were computed on it: the same stream orders this behind both)
  { Scope sc(this, "landmarks", post_stream); VH_HIP(vh_launch_landmarks(a, (int64_t)S * mcap, post_stream)); }
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(lmk.n.data(), lmk.d_n, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  for (int32_t s = 0; s < S; s++) counts[s] = lmk.n[s];
  lmk.valid = true; lmk.seq = match_seq; lmk.state_seq[cur] = trk_fill_seq[cur];
  return VH_OK;
}

// A push of a sequence handle has succeeded: the states of the chunk that ends become the next chunk's carry iff the
// last landmarks call came after the last match call (lmk.seq) and that match call was on this very chunk (trk_cur_valid,
// which every push resets): a chunk without a call, or matched again after it, breaks the chain of states.
void Group::lmk_pushed(bool first, int32_t prev_chunk_rows) {
  if (!lmk_chain) return;
  const bool carries = !first && trk_on && trk_cur_valid && lmk.d_out && lmk.valid && lmk.seq == match_seq && prev_chunk_rows > 0;
  lmk.carry_valid = false;  // (the carry buffer holds an older chunk's states until the copy below is queued)
  lmk.carry_src = carries ? prev_chunk_rows - 1 : -1;
}

// The chain form over the rows of the chunk (kernels_landmark_chain.hip): row r's predecessor is row r - 1, row 0's the
// track carry slot with the states in lmk.d_state[1].  Rows >= the chunk's hold no list: count 0, nothing launched for them.
int32_t Group::landmarks_chain(const vh_landmark_params *lp, int32_t *counts) {
  if (!trk_on || !allocated || last_method < 0 || !trk_cur_valid || !scene_current()) return VH_ERR_STATE;
  if (!inliers_current() || inl.from_host) return VH_ERR_STATE;
  const int32_t tiles = (mcap + VH_SCENE_TILE - 1) / VH_SCENE_TILE;
  if (!lmk.d_out) {  // one block, before any launch: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(static_cast<LandmarkArrays &>(lmk), nullptr, false, (size_t)S, (size_t)S * mcap, (size_t)tiles, (size_t)mcap);
    if (rc) return rc;
    lmk.tiles = tiles;
  }
  const int32_t rows = std::min(std::max(seq_n, 0), S);
  lmk.valid = false;
  lmk.n.assign((size_t)S, 0);
  Scope sc(this, "landmarks", post_stream);
  if (lmk.carry_src >= 0) {  // the first call of this chunk: the previous chunk's last row, before its states are overwritten
    const int32_t src = lmk.carry_src;
    lmk.carry_src = -1;
    VH_HIP(hipMemcpyAsync(lmk.d_state[1], lmk.d_state[0] + (size_t)src * mcap, sizeof(vh_landmark_state) * (size_t)mcap, hipMemcpyDeviceToDevice,
                          post_stream));
    lmk.carry_valid = true;
  }
  VhLandmarkChainArgs c{};
  VhLandmarkArgs &a = c.a;
  a.lp = *lp;
  a.n_lists = rows; a.tiles_per_list = lmk.tiles;
  a.trk = tk.d_trk; a.rec_counts = tk.d_tcount; a.rec_stride = mcap;
  a.pts = scn.d_out; a.pt_counts = scn.d_n; a.pt_stride = mcap; a.ok = scn.d_n;
  a.state_out = lmk.d_state[0]; a.out = lmk.d_out; a.obs = lmk.d_obs; a.tile_cnt = lmk.d_tiles; a.n_out = lmk.d_n;
  c.next = lmk.d_next;
  if (lmk.carry_valid && trk_pred_valid) { c.carry = lmk.d_state[1]; c.carry_count = tk.d_tcount + S; c.carry_cap = mcap; }
  c.check = sets.check;
  // (the tracks were linked on the post stream, the points were computed on it: the same stream orders this behind both)
  VH_HIP(hipMemsetAsync(lmk.d_n, 0, sizeof(int32_t) * (size_t)S, post_stream));
  if (rows > 0) {
    VH_HIP(vh_launch_landmarks_chain_clear(c, (int64_t)S * mcap, post_stream));
    for (int32_t k = 0; k < VH_LANDMARK_CHAIN_STAGES; k++) {
      Scope sk(this, vh_landmark_chain_scope(k), post_stream);
      vh_launch_landmarks_chain_stage(c, k, post_stream);
    }
  }
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(lmk.n.data(), lmk.d_n, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  for (int32_t s = 0; s < S; s++) counts[s] = lmk.n[s];
  lmk.valid = true; lmk.seq = match_seq;
  return VH_OK;
}

int32_t Group::get_landmarks(int32_t s, vh_landmark *out, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || capo < 0 || (capo > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!landmarks_current()) return VH_ERR_STATE;
  *n = lmk.n[s];
  bool over = false;
  const int32_t rc = get_slot(out, lmk.d_out, s, *n, capo, false, over);
  return rc ? rc : over ? VH_ERR_CAPACITY : VH_OK;
}

int32_t Group::get_landmarks_all(vh_landmark *out, int32_t cap_per_stream, int32_t *counts) {
  if (!out || !counts || cap_per_stream < 0) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < S; s++) counts[s] = 0;
  if (!landmarks_current()) return VH_ERR_STATE;
  bool over = false;
  for (int32_t s = 0; s < S; s++) {
    counts[s] = lmk.n[s];
    const int32_t rc = get_slot(out + (size_t)s * cap_per_stream, lmk.d_out, s, counts[s], cap_per_stream, true, over);
    if (rc) return rc;
  }
  VH_HIP(hipStreamSynchronize(post_stream));
  return over ? VH_ERR_CAPACITY : VH_OK;
}

}  // namespace vh_engine

using namespace vh_engine;

extern "C" {

void vh_default_landmark_params(vh_landmark_params *lp) {
  if (!lp) return;
  lp->min_obs = 2; lp->max_missed = 3; lp->max_dist = 0.0; lp->gate_sigma = 0.0;
}

// One device block (tracks | points | predecessor states, each with its offsets; points per list | states | landmarks | observation index |
// tile counts | counts), one memset and four launches.  Every refusal for an argument comes before anything is written.
int32_t vh_landmarks_update(const vh_landmark_params *lp, int32_t device, int32_t n_sets, const vh_track *trk, const int32_t *rec_offsets,
                            const vh_scene_point *pts, const int32_t *pt_offsets, const vh_landmark_state *prev, const int32_t *prev_offsets,
                            vh_landmark_state *state_out, vh_landmark *out, int32_t *counts) {
  if (!landmark_params_ok(lp) || n_sets < 0 || (prev != nullptr) != (prev_offsets != nullptr)) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan rec, pt, pv;
  if (!counts || packed_args(rec_offsets, n_sets, trk, rec) || packed_args(pt_offsets, n_sets, pts, pt)) return VH_ERR_INVALID_ARG;
  if (prev_offsets && check_offsets(prev_offsets, n_sets, pv)) return VH_ERR_INVALID_ARG;
  if (rec.total > 0 && (!state_out || !out)) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) {  // the points of a list name its records, each at most once, in list order
    const int64_t n_rec = (int64_t)rec_offsets[s + 1] - rec_offsets[s], n_pt = (int64_t)pt_offsets[s + 1] - pt_offsets[s];
    if (n_pt > n_rec) return VH_ERR_INVALID_ARG;
    int64_t last = -1;
    for (int64_t k = 0; k < n_pt; k++) {
      const int64_t j = pts[pt_offsets[s] + k].src_pos;
      if (j <= last || j >= n_rec) return VH_ERR_INVALID_ARG;
      last = j;
    }
  }
  for (int32_t s = 0; s < n_sets; s++) counts[s] = 0;
  if (rec.total == 0) return VH_OK;
  if (packed_limit(rec, n_sets) || pv.longest > kListMax) return VH_ERR_UNSUPPORTED;
  const size_t lists = (size_t)n_sets, tiles = (size_t)((rec.longest + VH_SCENE_TILE - 1) / VH_SCENE_TILE);  // (lists * tiles < 2^26 under the limits above)
  const int32_t rc = select_device(device);
  if (rc) return rc;
  vh_track *d_trk = nullptr; vh_scene_point *d_pts = nullptr; vh_landmark_state *d_prev = nullptr, *d_state = nullptr;
  vh_landmark *d_out = nullptr;
  int32_t *d_roff = nullptr, *d_poff = nullptr, *d_voff = nullptr, *d_ok = nullptr, *d_obs = nullptr, *d_tiles = nullptr, *d_n = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    d_trk = c.ptr<vh_track>((size_t)rec.end); d_roff = c.ptr<int32_t>(lists + 1);
    d_pts = c.ptr<vh_scene_point>((size_t)pt.end); d_poff = c.ptr<int32_t>(lists + 1); d_ok = c.ptr<int32_t>(lists);
    d_prev = c.ptr<vh_landmark_state>(prev ? (size_t)pv.end : 0); d_voff = c.ptr<int32_t>(prev ? lists + 1 : 0);
    d_state = c.ptr<vh_landmark_state>((size_t)rec.end); d_out = c.ptr<vh_landmark>((size_t)rec.end); d_obs = c.ptr<int32_t>((size_t)rec.end);
    d_tiles = c.ptr<int32_t>(lists * tiles); d_n = c.ptr<int32_t>(lists);
  }));
  VH_HIP(blk.up(d_trk + rec.first, trk + rec.first, (size_t)rec.total));
  VH_HIP(blk.up(d_roff, rec_offsets, lists + 1));
  if (pt.total > 0) VH_HIP(blk.up(d_pts + pt.first, pts + pt.first, (size_t)pt.total));
  VH_HIP(blk.up(d_poff, pt_offsets, lists + 1));
  std::vector<int32_t> has_points(lists);  // the scan's ok
  for (size_t s = 0; s < lists; s++) has_points[s] = pt_offsets[s + 1] - pt_offsets[s];
  VH_HIP(blk.up(d_ok, has_points.data(), lists));
  if (prev) {
    if (pv.total > 0) VH_HIP(blk.up(d_prev + pv.first, prev + pv.first, (size_t)pv.total));
    VH_HIP(blk.up(d_voff, prev_offsets, lists + 1));
  }
  VhLandmarkArgs a{};
  a.lp = *lp;
  a.n_lists = n_sets; a.tiles_per_list = (int32_t)tiles;
  a.trk = d_trk; a.rec_offsets = d_roff;
  a.pts = d_pts; a.pt_offsets = d_poff; a.ok = d_ok;
  if (prev) { a.prev = d_prev; a.prev_offsets = d_voff; }
  a.state_out = d_state; a.out = d_out; a.obs = d_obs; a.tile_cnt = d_tiles; a.n_out = d_n;
  VH_HIP(vh_launch_landmarks(a, rec.end, nullptr));
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(counts, d_n, lists));
  VH_HIP(blk.down(state_out + rec.first, d_state + rec.first, (size_t)rec.total));
  // (list s's counts[s] landmarks at rec_offsets[s]; what lies behind them in its slice is not written)
  for (int32_t s = 0; s < n_sets; s++) {
    const size_t o = (size_t)rec_offsets[s], k = (size_t)counts[s];
    if (k) VH_HIP(blk.down(out + o, d_out + o, k));
  }
  return VH_OK;
}

// The lists as the rows of one chain: vh_landmarks_update's block with the carry in the place of the predecessor states
// and the forward links behind the observation index, one memset and six launches.
int32_t vh_landmarks_chain(const vh_landmark_params *lp, int32_t device, int32_t n_sets, const vh_track *trk, const int32_t *rec_offsets,
                           const vh_scene_point *pts, const int32_t *pt_offsets, const vh_landmark_state *carry, int32_t n_carry,
                           vh_landmark_state *state_out, vh_landmark *out, int32_t *counts) {
  if (!landmark_params_ok(lp) || n_sets < 0 || n_carry < 0 || (n_carry > 0 && !carry)) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan rec, pt;
  if (!counts || packed_args(rec_offsets, n_sets, trk, rec) || packed_args(pt_offsets, n_sets, pts, pt)) return VH_ERR_INVALID_ARG;
  if (rec.total > 0 && (!state_out || !out)) return VH_ERR_INVALID_ARG;
  std::vector<uint8_t> mark;  // the link rule's uniqueness: a predecessor record is continued at most once
  for (int32_t s = 0; s < n_sets; s++) {
    const int64_t n_rec = (int64_t)rec_offsets[s + 1] - rec_offsets[s], n_pt = (int64_t)pt_offsets[s + 1] - pt_offsets[s];
    if (n_pt > n_rec) return VH_ERR_INVALID_ARG;
    int64_t last = -1;
    for (int64_t k = 0; k < n_pt; k++) {
      const int64_t j = pts[pt_offsets[s] + k].src_pos;
      if (j <= last || j >= n_rec) return VH_ERR_INVALID_ARG;
      last = j;
    }
    const int64_t n_pred = s ? (int64_t)rec_offsets[s] - rec_offsets[s - 1] : (carry ? n_carry : 0);
    mark.assign((size_t)n_pred, 0);
    for (int64_t j = 0; j < n_rec; j++) {
      const int64_t q = trk[rec_offsets[s] + j].prev;
      if (q < 0 || q >= n_pred) continue;
      if (mark[(size_t)q]) return VH_ERR_INVALID_ARG;
      mark[(size_t)q] = 1;
    }
  }
  for (int32_t s = 0; s < n_sets; s++) counts[s] = 0;
  if (rec.total == 0) return VH_OK;
  if (packed_limit(rec, n_sets) || n_carry > kListMax) return VH_ERR_UNSUPPORTED;
  const size_t lists = (size_t)n_sets, tiles = (size_t)((rec.longest + VH_SCENE_TILE - 1) / VH_SCENE_TILE);  // (lists * tiles < 2^26 under the limits above)
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t nc = carry ? (size_t)n_carry : 0;
  vh_track *d_trk = nullptr; vh_scene_point *d_pts = nullptr; vh_landmark_state *d_carry = nullptr, *d_state = nullptr;
  vh_landmark *d_out = nullptr;
  int32_t *d_roff = nullptr, *d_poff = nullptr, *d_ok = nullptr, *d_link = nullptr, *d_tiles = nullptr, *d_n = nullptr;
  uint32_t *d_check = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    d_trk = c.ptr<vh_track>((size_t)rec.end); d_roff = c.ptr<int32_t>(lists + 1);
    d_pts = c.ptr<vh_scene_point>((size_t)pt.end); d_poff = c.ptr<int32_t>(lists + 1); d_ok = c.ptr<int32_t>(lists);
    d_carry = c.ptr<vh_landmark_state>(nc);
    d_state = c.ptr<vh_landmark_state>((size_t)rec.end); d_out = c.ptr<vh_landmark>((size_t)rec.end);
    d_link = c.ptr<int32_t>(2 * (size_t)rec.end);  // the observation index | the forward links
    d_tiles = c.ptr<int32_t>(lists * tiles); d_n = c.ptr<int32_t>(lists); d_check = c.ptr<uint32_t>(64);
  }));
  VH_HIP(hipMemset(d_check, 0, 256));
  VH_HIP(blk.up(d_trk + rec.first, trk + rec.first, (size_t)rec.total));
  VH_HIP(blk.up(d_roff, rec_offsets, lists + 1));
  if (pt.total > 0) VH_HIP(blk.up(d_pts + pt.first, pts + pt.first, (size_t)pt.total));
  VH_HIP(blk.up(d_poff, pt_offsets, lists + 1));
  std::vector<int32_t> has_points(lists);  // the scan's ok
  for (size_t s = 0; s < lists; s++) has_points[s] = pt_offsets[s + 1] - pt_offsets[s];
  VH_HIP(blk.up(d_ok, has_points.data(), lists));
  if (nc) VH_HIP(blk.up(d_carry, carry, nc));
  VhLandmarkChainArgs c{};
  VhLandmarkArgs &a = c.a;
  a.lp = *lp;
  a.n_lists = n_sets; a.tiles_per_list = (int32_t)tiles;
  a.trk = d_trk; a.rec_offsets = d_roff;
  a.pts = d_pts; a.pt_offsets = d_poff; a.ok = d_ok;
  a.state_out = d_state; a.out = d_out; a.obs = d_link; a.tile_cnt = d_tiles; a.n_out = d_n;
  c.next = d_link + rec.end;
  if (nc) { c.carry = d_carry; c.n_carry = n_carry; }
  c.check = d_check;
  VH_HIP(vh_launch_landmarks_chain_clear(c, rec.end, nullptr));
  for (int32_t k = 0; k < VH_LANDMARK_CHAIN_STAGES; k++) vh_launch_landmarks_chain_stage(c, k, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  { const int32_t rv = report_violation(d_check); if (rv) return rv; }
  VH_HIP(blk.down(counts, d_n, lists));
  VH_HIP(blk.down(state_out + rec.first, d_state + rec.first, (size_t)rec.total));
  for (int32_t s = 0; s < n_sets; s++) {
    const size_t o = (size_t)rec_offsets[s], k = (size_t)counts[s];
    if (k) VH_HIP(blk.down(out + o, d_out + o, k));
  }
  return VH_OK;
}

int32_t vh_sequence_set_landmarks(vh_group *g, int32_t on) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (!gq->seq) return VH_ERR_UNSUPPORTED;  // a group or a lone matcher needs no switch
  if (gq->allocated) return VH_ERR_STATE;   // before the first push only
  gq->lmk_chain = on != 0;
  return VH_OK;
}

int32_t vh_group_landmarks(vh_group *g, const vh_landmark_params *lp, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->landmarks(lp, counts);
}
int32_t vh_match_landmarks(vh_matcher *m, const vh_landmark_params *lp, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->landmarks(lp, count);
}
int32_t vh_group_get_landmarks(vh_group *g, int32_t stream, vh_landmark *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_landmarks(stream, out, cap, n);
}
int32_t vh_group_get_landmarks_all(vh_group *g, vh_landmark *out, int32_t cap_per_stream, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_landmarks_all(out, cap_per_stream, counts);
}
int32_t vh_get_landmarks(vh_matcher *m, vh_landmark *out, int32_t cap, int32_t *n) {
  return vh_group_get_landmarks((vh_group *)m, 0, out, cap, n);
}
int32_t vh_group_landmarks_device(vh_group *g, const vh_landmark **d_out, int64_t *stride) {
  Group *gq = (Group *)g;
  if (!gq || !d_out || !stride) return VH_ERR_INVALID_ARG;
  if (!gq->landmarks_current()) return VH_ERR_STATE;
  *d_out = gq->lmk.d_out; *stride = gq->mcap;
  return VH_OK;
}

}  // extern "C"
