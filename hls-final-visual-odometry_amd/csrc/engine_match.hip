// engine_match.hip -- a match call: loop policy, the searches on tables or inside ranges, the motion prior,
// multi-stage ranges on host and device, feature tracks, caller-supplied features (engine.h).
#include "engine.h"

#include <thread>

namespace vh_engine {

// the integer accept window of a float range: ceil(min) .. floor(max), clamped so that coordinate + bound cannot overflow
static int32_t range_bound(float x, bool is_min) {
  const float r = is_min ? ceilf(x) : floorf(x);
  return (int32_t)std::min(std::max(r, -1048576.0f), 1048576.0f);
}

VhMatchArgs Group::match_args(int32_t method) const {
  VhMatchArgs a = role_args();
  a.radius = p.match_radius; a.disp_tol = p.match_disp_tolerance;
  if (method == VH_METHOD_FLOW) {  // matcher.cpp:320-321
    a.npass = 2; a.pass[0] = {VH_SET_1C, VH_SET_1P, 1, 0}; a.pass[1] = {VH_SET_1P, VH_SET_1C, 1, 1};
  } else if (method == VH_METHOD_STEREO) {
    a.npass = 2; a.pass[0] = {VH_SET_1C, VH_SET_2C, 0, 0}; a.pass[1] = {VH_SET_2C, VH_SET_1C, 0, 1};
  } else {
    a.npass = 4;
    a.pass[0] = {VH_SET_1P, VH_SET_2P, 0, 0}; a.pass[1] = {VH_SET_2P, VH_SET_2C, 1, 1};
    a.pass[2] = {VH_SET_2C, VH_SET_1C, 0, 2}; a.pass[3] = {VH_SET_1C, VH_SET_1P, 1, 3};
  }
  return a;
}

// speculative or tested search loops for the next launch (see the members above)
bool Group::choose_loop() {
  for (int sl = 0; sl < 2; sl++) {
    if (!mt.stats_pending[sl] || hipEventQuery(ev_post[sl]) != hipSuccess) continue;
    mt.stats_pending[sl] = false;
    int64_t again = 0, searched = 0;
    int32_t nq_max = 0;
    for (int32_t s = 0; s < S; s++) { again += mt.h_out[sl][s].z; searched += mt.h_out[sl][s].w; nq_max = std::max(nq_max, mt.h_out[sl][s].w); }
    // query tiles the fullest stream's sets held, per pass (the searches' grid is sized by it: vh_launch_match)
    if (mt.stats_npass[sl] > 0) mt.tiles_hint = nq_max / mt.stats_npass[sl] / VH_TILE_Q + 4;
    if (!mt.stats_was_spec[sl] || searched <= 0) continue;  // the tested loop reports nothing
    last_redo_rate = (double)again / (double)searched;
    if (spec_mode && last_redo_rate > 0.065) { spec_mode = false; probe_countdown = 16; }
    else if (!spec_mode && last_redo_rate < 0.055) spec_mode = true;
  }
  if (force_mode >= 0) return force_mode == 1;
  if (spec_mode) return true;
  if (--probe_countdown <= 0) { probe_countdown = 16; return true; }  // probe
  return false;
}

int32_t Group::match_recover() {
  VH_HIP(hipStreamSynchronize(match_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  for (int k = 0; k < 2; k++) VH_HIP(hipMemset(mt.d_mchunk2[k], 0, sizeof(int32_t) * (size_t)S * ((cap + 255) / 256)));
  VH_HIP(hipMemset(mt.d_redo, 0, sizeof(int32_t) * 2 * (size_t)S));
  mt.stats_pending[0] = mt.stats_pending[1] = false; mt.tiles_hint = 0;
  last_method = -1;
  // tracks: the failed call's lists are void (match()); a carry copy it may have left half done is void as well, so the
  // next lists of a sequence start new tracks instead of following a table in an unknown state
  if (trk_on && seq) { trk_pred_valid = false; trk_carry_src = -1; lmk.carry_valid = false; lmk.carry_src = -1; }  // (the landmark states go with the lists they belong to)
  match_dirty = false;
  return VH_OK;
}

int32_t Group::ensure_ranges(bool staging) {
  if (!rg.d_ranges) { const int32_t rc = dmalloc(&rg.d_ranges, n_ranges(), false); if (rc) return rc; }
  if (staging && !rg.h_ranges) VH_HIP(rg.h_ranges.alloc(n_ranges(), hipHostMallocDefault));
  return VH_OK;
}

// Pass 1 of multi-stage matching and the statistics: the method's matching on the sparse sets, the vote on the host
// (flow and quad lists), one range table per stream into rg.h_ranges, queued for the match stream.
int32_t Group::multi_stage_ranges(int32_t method, const double *tr16) {
  sparse->vote_rule = vote_rule;  // (pass 1 is voted under this handle's rule, with the sparse list's method)
  int32_t rc = sparse->match(method, tr16);
  if (rc) return rc;
  auto t0 = std::chrono::steady_clock::now();
  // a sequence handle: the rows of the chunk only -- the others hold no pair, their sparse lists are empty and their ranges +-R
  const int32_t rows = seq ? seq_n : S;
  for (int32_t s = 0; s < rows; s++) if ((rc = sparse->fetch_matches(s))) return rc;
  const int32_t threads = (int32_t)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  if ((rc = sparse->remove_outliers(0, rows, threads))) return rc;
  prof_host("sparse_vote_host", t0);
  // (the table the previous match's pass 2 read has gone up: the copy below is the next thing on the match stream)
  VH_HIP(hipStreamSynchronize(match_stream));
  t0 = std::chrono::steady_clock::now();
  const size_t per = (size_t)sets.ubn * sets.vbn * 16;
  std::vector<float> fr(per);
  for (int32_t s = 0; s < S; s++) {
    const std::vector<vh_p_match> &pm = sparse->host_matches[s];
    if ((rc = prior_statistics(p, dims, method, pm.data(), s < rows ? (int32_t)pm.size() : 0, fr.data()))) return rc;
    for (size_t k = 0; k < per; k++) rg.h_ranges[s * per + k] = range_bound(fr[k], (k & 1) == 0);
  }
  prof_host("statistics_host", t0);
  VH_HIP(hipMemcpyAsync(rg.d_ranges, rg.h_ranges, sizeof(int32_t) * n_ranges(), hipMemcpyHostToDevice, match_stream));
  return VH_OK;
}

// The same on the device (vh_group_set_multi_stage_device): nothing here waits for the GPU or moves a list.  Pass 1, the
// vote (kernels_vote.hip, the vote only: the lists are compacted in place in ms_vb) and the statistics (kernels_stats.hip,
// straight into rg.d_ranges) follow each other on the sparse group's post stream; the match stream waits for the statistics.
// The statistics of this step overwrite the table the previous step's pass 2 read: they wait for that launch
// (ev_tables of the previous buffer is recorded right behind it), the vote before them does not.
int32_t Group::ensure_ms_vote() {
  VH_HIP(ev_stats.create());
  if (ms_vb.block) return VH_OK;
  if (alloc_refused()) return VH_ERR_HIP;
  // (a sparse list beyond the vote's list length is refused by vote_prep: VH_VOTE_TRUNCATED)
  VH_HIP(ms_vb.alloc(S, std::min(sparse->mcap, VH_VOTE_LIST_MAX), 1, 1));
  return VH_OK;
}

int32_t Group::multi_stage_ranges_device(int32_t method, const double *tr16) {
  sparse->vote_rule = vote_rule;
  int32_t rc = sparse->match(method, tr16);
  if (rc) return rc;
  hipStream_t vs = sparse->post_stream;
  {
    Scope sc(this, "sparse_vote", vs);
    vh_launch_vote_prep(ms_vb.v, 0, S, (const vh_p_match *)sparse->mt.d_matches, sparse->mcap, sparse->mt.d_match_count, sparse->mcap, sparse->mt.d_overflow,
                        votes_on(method) ? 1 : 0, vs);
    vote_run(ms_vb.v, method, kMsVoteLanes, 0, 0.0f, 0.0f, ms_vb, vs);
  }
  VH_HIP(hipGetLastError());
  VH_HIP(hipStreamWaitEvent(vs, ev_tables[(match_seq + 1) & 1], 0));  // (never recorded: no wait)
  VhStatsArgs sa{};
  sa.pm = ms_vb.v.pm; sa.pm_stride = ms_vb.v.cap;
  sa.counts = &ms_vb.v.meta->kept; sa.status = &ms_vb.v.meta->status;
  sa.count_stride = (int32_t)(sizeof(VhVoteMeta) / sizeof(int32_t)); sa.count_cap = ms_vb.v.cap;
  sa.n_lists = S; sa.method = method; sa.ubn = sets.ubn; sa.vbn = sets.vbn;
  sa.bs = (float)p.match_binsize; sa.R = (float)p.match_radius;
  sa.out = rg.d_ranges; sa.err = nullptr;
  { Scope sc(this, "prior_stats", vs); vh_launch_prior_stats(sa, 1, vs); }
  VH_HIP(hipGetLastError());
  VH_HIP(hipEventRecord(ev_stats, vs));
  VH_HIP(hipStreamWaitEvent(match_stream, ev_stats, 0));
  return VH_OK;
}

// Caller-supplied ranges (vh_match_ranged): [ubn * vbn][4][4] float for every stream of the group
int32_t Group::load_ranges(const float *ranges) {
  int32_t rc = ensure_ranges();
  if (rc) return rc;
  const size_t per = (size_t)sets.ubn * sets.vbn * 16;
  for (size_t k = 0; k < per; k++) if (!std::isfinite(ranges[k])) return VH_ERR_INVALID_ARG;
  VH_HIP(hipStreamSynchronize(match_stream));
  for (int32_t s = 0; s < S; s++)
    for (size_t k = 0; k < per; k++) rg.h_ranges[s * per + k] = range_bound(ranges[k], (k & 1) == 0);
  VH_HIP(hipMemcpyAsync(rg.d_ranges, rg.h_ranges, sizeof(int32_t) * n_ranges(), hipMemcpyHostToDevice, match_stream));
  return VH_OK;
}

// ranged: search inside the ranges load_ranges() queued (vh_match_ranged); a handle with multi-stage matching on
// produces its own (multi_stage_ranges)
int32_t Group::match(int32_t method, const double *tr16, bool ranged) {
  const int32_t rc = match_call(method, tr16, ranged);
  if (rc && rh.on) recon_match_failed();  // (reconstruction: every failed match call is a break)
  return rc;
}

int32_t Group::match_call(int32_t method, const double *tr16, bool ranged) {
  if (method < 0 || method > 2) return VH_ERR_INVALID_ARG;
  if (!allocated || failed) return VH_ERR_STATE;
  if (sparse && tr16 && !ms_prior) return VH_ERR_UNSUPPORTED;  // the motion prior combines with multi-stage matching by its own switch only
  if (tr16 && method != VH_METHOD_QUAD) tr16 = nullptr;  // (stock libviso2 uses the prediction in the quad circle only)
  if (tr16 && !(p.f > 0 && p.base > 0)) return VH_ERR_STATE;  // setIntrinsics first
  if (sparse && tr16) { sparse->p.f = p.f; sparse->p.cu = p.cu; sparse->p.cv = p.cv; sparse->p.base = p.base; }  // (pass 1 predicts with the same camera)
  if (match_dirty) { const int32_t rr = match_recover(); if (rr) return rr; }
  if (tr16 && !pri.d_prior_tr) { const int32_t rt = dmalloc(&pri.d_prior_tr, 16 * (size_t)S, false); if (rt) return rt; }
  if (tr16 && !pri.h_prior_tr) VH_HIP(pri.h_prior_tr.alloc(2 * 16 * (size_t)S, hipHostMallocDefault));
  // everything that can fail without a kernel of the step in flight comes first
  if (method == VH_METHOD_FLOW && !mt.d_mask) {
    const int32_t rc = dmalloc(&mt.d_mask, (size_t)S * dims[0] * dims[1], false); if (rc) return rc;
    mt.mask_fresh = true;
  }
  if (trk_on) { const int32_t rt = trk_ensure(); if (rt) return rt; }
  if (sparse && ms_device) {
    int32_t rr = ensure_ranges(false);
    if (rr) return rr;
    if ((rr = ensure_ms_vote())) return rr;
    if ((rr = multi_stage_ranges_device(method, tr16))) { match_dirty = true; return rr; }
  } else if (sparse) {
    int32_t rr = ensure_ranges();
    if (rr) return rr;
    if ((rr = multi_stage_ranges(method, tr16))) return rr;
  }
  const int32_t rc = match_queued(method, tr16, (sparse || ranged) ? rg.d_ranges : nullptr);
  if (rc) { match_dirty = true; trk_cur_valid = false; }
  return rc;
}

int32_t Group::match_queued(int32_t method, const double *tr16, const int32_t *ranges) {
  VhMatchArgs a = match_args(method);
  a.prior = tr16 ? 1 : 0;
  hipStream_t ms = match_stream;
  const int32_t buf = (int32_t)(match_seq++ & 1);
  // the current slot's detection+indexing must be complete (the previous
  // slot's finished earlier on the same stream), and the post-processing that
  // last read this table buffer (two matches ago) must be done with it
  VH_HIP(hipStreamWaitEvent(ms, ev_det[pair_cur], 0));
  VH_HIP(hipStreamWaitEvent(ms, ev_det[pair_prev], 0));
  if (ev_post_valid[buf]) VH_HIP(hipStreamWaitEvent(ms, ev_post[buf], 0));
  if (ranges) {
    // Pass 2 of multi-stage matching: no tables -- kernels_ranged.hip walks every driver's circle inside the ranges of its
    // statistics bin and writes the chain entries itself, on the match stream (it is the step's search); the flow method's
    // keep step, the refinement and the emission follow on the post stream (match_post).  The kernel adds to the
    // chunk counters the previous emission zeroed and bids into the pixel mask the previous keep step read, so the match
    // stream also waits for the previous step's post-processing -- and the mask's epoch advances on the match stream.
    if (ev_post_valid[buf ^ 1]) VH_HIP(hipStreamWaitEvent(ms, ev_post[buf ^ 1], 0));
    if (method == VH_METHOD_FLOW) { const int32_t re = mask_epoch(ms); if (re) return re; }
    if (tr16) {  // (quad: pass 2 hands the estimate to its second hop, as pass 1 did on the sparse sets)
      const int32_t rp = stage_prior(tr16, buf, a.rows, ms);
      if (rp) return rp;
      const VhPriorArgs pa{pri.d_prior_tr, p.f, p.cu, p.cv, p.base};
      Scope sc(this, "ranged", ms);
      vh_launch_ranged_circle_prior(sets, a, ranges, pa, mt.d_chain2[buf], mt.d_mchunk2[buf], ms);
    } else {
      Scope sc(this, "ranged", ms);
      vh_launch_ranged_circle(sets, a, method, ranges, mt.d_chain2[buf], mt.d_mask, mt.epoch, mt.d_mchunk2[buf], ms);
    }
    VH_HIP(hipGetLastError());
    VH_HIP(hipEventRecord(ev_tables[buf], ms));
    return match_post(method, a, buf, true, false);
  }
  const bool spec = choose_loop();
  // A stepped group shares the chip with its own detection chain: a grid as tight as the tiles the sets really hold, and
  // the searches' workgroups padded to an LDS footprint that leaves the chain room on every CU (vh_launch_match has the
  // measurements).  How many LDS allocation units (1 280 bytes) is a property of what runs beside the searches: with
  // detect_nms<1|2> (14 units) and emit_features (21) six search workgroups of 21 units per CU are best (KITTI 107.5 ->
  // 111.5 k, 1080p 18.5 -> 19.2 k; 20 or 22-25 units lose 2-3 % against no hint at all); with detect_nms<3> (22 units,
  // 69 registers then, 79 since its 16-byte staging: the 4K configuration) five workgroups of 23-25 units (3.68 -> 4.08 k;
  // 21 units: 3.67; re-swept at 79 registers: 21 / 23 / 24 / 25 units = 3.65 / 4.08 / 4.07 / 4.09 k).  KITTI frames at
  // nms_n = 1 / 4 (detect_nms<1> 9 units, <4> 33 units): 21 units 86.0 -> 89.2 k / 106.1 -> 108.9 k, 24 units 87.7 / 105.6.
  // The generic detector (nms_n >= 5, unaligned strides) was not measured: no hint.  VH_MATCH_LDS_UNITS overrides (0: none).
  static const int units_env = [] { const char *ev = getenv("VH_MATCH_LDS_UNITS"); return ev ? atoi(ev) : -1; }();
  const int32_t units = units_env >= 0 ? units_env : (g.n == 3 ? 24 : (g.n <= 4 ? 21 : 0));
  const int32_t gx_hint = (!serial && units > 0 && mt.tiles_hint > 0) ? (mt.tiles_hint + 3) / 4 : 0;
  { Scope sc(this, "match", ms); vh_launch_match(sets, a, mt.d_best2[buf], mt.d_redo + (size_t)buf * S, spec ? 1 : 0, gx_hint, units * 1280, ms); }
  VH_HIP(hipGetLastError());
  if (tr16) {  // hop 2 of the circle, per driving feature, behind the 1p -> 2p table of the launch above
    const int32_t rp = stage_prior(tr16, buf, a.rows, ms);
    if (rp) return rp;
    { Scope sc(this, "quad_prior", ms); vh_launch_quad_prior(sets, a, pri.d_prior_tr, p.f, p.cu, p.cv, p.base, mt.d_best2[buf], ms); }
    VH_HIP(hipGetLastError());
  }
  VH_HIP(hipEventRecord(ev_tables[buf], ms));
  return match_post(method, a, buf, false, spec);
}

// the caller's motion estimates, one per row, to pri.d_prior_tr on `ms` through the page-locked slot of table buffer buf
int32_t Group::stage_prior(const double *tr16, int32_t buf, int32_t rows, hipStream_t ms) {
  double *ht = pri.h_prior_tr + (size_t)buf * 16 * S;
  VH_HIP(hipEventSynchronize(ev_tables[buf]));  // (recorded behind the copy that last read this slot, two matches ago; at once if never recorded)
  memcpy(ht, tr16, sizeof(double) * 16 * (size_t)rows);  // (a sequence chunk: one per frame pair)
  VH_HIP(hipMemcpyAsync(pri.d_prior_tr, ht, sizeof(double) * 16 * (size_t)rows, hipMemcpyHostToDevice, ms));
  return VH_OK;
}

// The flow method's pixel mask holds (epoch, feature index) per pixel: a new epoch per match call, the mask cleared on
// `st` when it is fresh from the allocation or the epochs have come round.
int32_t Group::mask_epoch(hipStream_t st) {
  if (mt.mask_fresh || mt.epoch + 1 >= (1u << (32 - VH_MASK_IDX_BITS)) - 1) {
    VH_HIP(hipMemsetAsync(mt.d_mask, 0, sizeof(uint32_t) * (size_t)S * dims[0] * dims[1], st));
    mt.epoch = 0; mt.mask_fresh = false;
  }
  mt.epoch++;
  return VH_OK;
}

// The post stream's share of a match call, behind the search recorded in ev_tables[buf]: the chain entries (from the tables
// of buffer buf; ranged: written by the search already, the flow method keeps the mask's winners), the refinement, the
// emission, the tracks, and the bookkeeping of the call.
int32_t Group::match_post(int32_t method, const VhMatchArgs &a, int32_t buf, bool ranged, bool spec) {
  hipStream_t ps = post_stream;
  VH_HIP(hipStreamWaitEvent(ps, ev_tables[buf], 0));
  int32_t *d_mchunk = mt.d_mchunk2[buf];  // zeroed by the previous launch's emission (at allocation for the first two)
  if (!ranged) {
    if (method == VH_METHOD_FLOW) { const int32_t re = mask_epoch(ps); if (re) return re; }
    Scope sc(this, "chain", ps);
    vh_launch_chain(sets, a, method, mt.d_best2[buf], mt.d_chain2[buf], mt.d_mask, mt.epoch, d_mchunk, ps);
  } else if (method == VH_METHOD_FLOW) {
    Scope sc(this, "chain", ps);
    vh_launch_flow_keep(sets, a, mt.d_chain2[buf], mt.d_mask, mt.epoch, d_mchunk, ps);
  }
  float4 *ref = p.refinement > 0 ? mt.d_ref2[buf] : nullptr;  // (before the emission: every reader of the list sees the refined one)
  if (ref) { Scope sc(this, "refine", ps); vh_launch_refine(sets, a, method, rf, mt.d_chain2[buf], ref, d_mchunk, ps); }
  // a download of the previous step's lists may still be reading mt.d_matches
  if (mt.ev_down_valid) VH_HIP(hipStreamWaitEvent(ps, ev_down, 0));
  {
    Scope sc(this, "emit_matches", ps);
    vh_launch_emit_matches(sets, a, method, mt.d_chain2[buf], mt.d_matches, mcap, mt.d_match_count, mt.d_overflow, d_mchunk, mt.d_redo + (size_t)buf * S,
                           mt.d_mchunk2[buf ^ 1], (int4 *)mt.h_out[buf].dev, mt.h_matches.dev, ref, ps);
  }
  VH_HIP(hipGetLastError());
  recon_before_link();
  if (trk_on) { const int32_t rt = trk_queue(a, ps); if (rt) return rt; }
  recon_matched(a);
  // (re-searched, searched) of this launch are read from mt.h_out[buf] by a later choose_loop(); the ranged search reports nothing
  mt.stats_pending[buf] = true; mt.stats_was_spec[buf] = spec; mt.stats_npass[buf] = a.npass;
  VH_HIP(hipEventRecord(ev_post[buf], ps)); ev_post_valid[buf] = true;
  // both slots stay in use until this point of the post stream
  VH_HIP(hipEventRecord(ev_read[pair_cur], ps)); ev_read_valid[pair_cur] = true;
  VH_HIP(hipEventRecord(ev_read[pair_prev], ps)); ev_read_valid[pair_prev] = true;
  last_method = method; drop_host_matches(); last_buf = buf;
  return VH_OK;
}

// a push has succeeded: which list is whose predecessor now
void Group::trk_pushed(bool shifted, bool first, int32_t prev_chunk_rows) {
  if (!trk_on) return;
  if (seq) {
    lmk_pushed(first, prev_chunk_rows);  // (before the flags of the chunk that ends are reset)
    if (first) { trk_pred_valid = false; trk_carry_src = -1; }
    else if (trk_cur_valid) trk_carry_src = prev_chunk_rows - 1;        // (supersedes a carry that was never needed)
    else { trk_pred_valid = false; trk_carry_src = -1; }                  // the previous chunk was never matched
    trk_cur_valid = false;
    return;
  }
  if (first) { trk_serial = 0; trk_cur_valid = trk_pred_valid = false; return; }
  if (!shifted) { trk_cur_valid = false; return; }  // replace: the pair's list is void, its predecessor stays
  trk_serial++;
  trk_pred_valid = trk_cur_valid; trk_pred_epoch = trk_cur_epoch;
  if (trk_cur_valid) trk_cur ^= 1;
  trk_cur_valid = false;
}

// before a match call queues anything: the buffers (the first call allocates them)
int32_t Group::trk_ensure() {
  int32_t rc;
  if (mcap > (int32_t)VH_TRACK_POS_MASK) return VH_ERR_UNSUPPORTED;  // a table entry has VH_TRACK_POS_BITS bits for the position
  const size_t slots = (size_t)trk_slots();
  if (!tk.d_ttab) { if ((rc = dmalloc(&tk.d_ttab, slots * cap, false))) return rc; tk.trk_fresh = true; }
  if (!tk.d_ttabp) { if ((rc = dmalloc(&tk.d_ttabp, (size_t)S * cap, false))) return rc; tk.trk_fresh = true; }
  if (!tk.d_trk) { if ((rc = dmalloc((uint8_t **)&tk.d_trk, slots * mcap * sizeof(vh_track), false))) return rc; tk.trk_fresh = true; }
  if (!tk.d_tcount) { if ((rc = dmalloc(&tk.d_tcount, slots, false))) return rc; tk.trk_fresh = true; }
  return VH_OK;
}

VhTrackArgs Group::trk_args(int32_t rows) const {
  VhTrackArgs t{};
  t.pm = (const vh_p_match *)mt.d_matches; t.pm_stride = mcap; t.counts = mt.d_match_count; t.count_cap = mcap;
  t.rows = rows; t.n_index = cap;
  t.tab_c = tk.d_ttab; t.tab_p = tk.d_ttabp; t.trk = tk.d_trk; t.trk_stride = mcap; t.slot_count = tk.d_tcount;
  t.chain = seq ? 1 : 0;
  t.slot0 = seq ? 0 : trk_cur * S;
  t.pred0 = trk_pred_valid ? (seq ? S : (trk_cur ^ 1) * S) : -1;
  t.epoch = trk_epoch; t.pred_epoch = trk_pred_epoch;
  t.serial0 = seq ? seq_first : trk_serial;
  t.check = sets.check;
  return t;
}

// behind emit_matches on the post stream: the lists of this match call are linked to their predecessors
int32_t Group::trk_queue(const VhMatchArgs &a, hipStream_t ps) {
  const size_t slots = (size_t)trk_slots();
  if (tk.trk_fresh) {
    VH_HIP(hipMemsetAsync(tk.d_ttab, 0, sizeof(uint32_t) * slots * cap, ps));
    VH_HIP(hipMemsetAsync(tk.d_ttabp, 0, sizeof(uint32_t) * (size_t)S * cap, ps));
    VH_HIP(hipMemsetAsync(tk.d_tcount, 0, sizeof(int32_t) * slots, ps));
    trk_reset_lists();
    tk.trk_fresh = false;
  }
  trk_cur_valid = false;  // (until everything below is queued)
  if (seq && trk_carry_src >= 0) {
    const int32_t src = trk_carry_src;
    trk_carry_src = -1; trk_pred_valid = false;
    { Scope sc(this, "track_carry", ps); vh_launch_track_copy(trk_args(0), src, S, ps); }
    VH_HIP(hipGetLastError());
    trk_pred_valid = true; trk_pred_epoch = trk_cur_epoch;
  }
  if (trk_epoch >= VH_TRACK_EPOCH_MAX) {  // the epochs have come round: the predecessors' bids become epoch 1, everything else empty
    const int64_t keep0 = seq ? S : (int64_t)(trk_cur ^ 1) * S, keep1 = seq ? S + 1 : keep0 + S;
    vh_launch_track_retag(tk.d_ttab, cap, (int64_t)slots, keep0, keep1, trk_pred_valid ? trk_pred_epoch : 0u, ps);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemsetAsync(tk.d_ttabp, 0, sizeof(uint32_t) * (size_t)S * cap, ps));
    trk_pred_epoch = 1; trk_epoch = 1;
  }
  trk_epoch++;
  const VhTrackArgs t = trk_args(a.rows);
  { Scope sc(this, "track_scatter", ps); vh_launch_track_scatter(t, ps); }
  { Scope sc(this, "track_link", ps); vh_launch_track_link(t, ps); }
  { Scope sc(this, "track_rank", ps); vh_launch_track_rank(t, ps); }
  VH_HIP(hipGetLastError());
  trk_cur_valid = true; trk_cur_epoch = trk_epoch;
  if (!seq) trk_fill_seq[trk_cur] = match_seq;  // (a state computed for the buffer's earlier list is stale now)
  return VH_OK;
}

int32_t Group::get_tracks(int32_t s, vh_track *out, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || capo < 0 || (capo > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!trk_on || !allocated || last_method < 0 || !trk_cur_valid) return VH_ERR_STATE;
  VH_HIP(hipEventSynchronize(ev_post[last_buf]));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  const int32_t cnt = mt.h_out[last_buf][s].x, ov = mt.h_out[last_buf][s].y;
  *n = cnt;
  const int32_t k = std::min(std::min(cnt, mcap), capo);
  if (k > 0) {
    VH_HIP(hipMemcpyAsync(out, tk.d_trk + ((size_t)(seq ? 0 : trk_cur * S) + s) * mcap, sizeof(vh_track) * (size_t)k, hipMemcpyDeviceToHost, post_stream));
    VH_HIP(hipStreamSynchronize(post_stream));
  }
  return (cnt > capo || cnt > mcap || ov) ? VH_ERR_CAPACITY : VH_OK;
}

int32_t Group::get_tracks_all(vh_track *out, int32_t cap_per_stream, int32_t *counts) {
  if (!out || !counts || cap_per_stream < 0) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < S; s++) counts[s] = 0;
  if (!trk_on || !allocated || last_method < 0 || !trk_cur_valid) return VH_ERR_STATE;
  VH_HIP(hipEventSynchronize(ev_post[last_buf]));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  bool over = false;
  for (int32_t s = 0; s < S; s++) {
    counts[s] = mt.h_out[last_buf][s].x;
    over = over || mt.h_out[last_buf][s].y != 0 || counts[s] > cap_per_stream || counts[s] > mcap;
    const int32_t k = std::min(std::min(counts[s], mcap), cap_per_stream);
    if (k > 0)
      VH_HIP(hipMemcpyAsync(out + (size_t)s * cap_per_stream, tk.d_trk + ((size_t)(seq ? 0 : trk_cur * S) + s) * mcap, sizeof(vh_track) * (size_t)k,
                            hipMemcpyDeviceToHost, post_stream));
  }
  VH_HIP(hipStreamSynchronize(post_stream));
  return over ? VH_ERR_CAPACITY : VH_OK;
}

// Load caller-supplied feature records into a role's set and index it.
int32_t Group::load_features(int32_t role, const int32_t *m, int32_t n) {
  if (n < 0 || (n > 0 && !m)) return VH_ERR_INVALID_ARG;
  if (n > cap) return VH_ERR_CAPACITY;
  for (int32_t i = 0; i < n; i++) {
    const int32_t *f = m + 12 * (size_t)i;
    if (f[0] < 0 || f[0] >= dims[0] || f[1] < 0 || f[1] >= dims[1] || f[3] < 0 || f[3] > 3) return VH_ERR_INVALID_ARG;
  }
  const int32_t set = vh_row_set(role_args(), 0, role);
  const int32_t slot = (role >= 2) ? pair_cur : pair_prev;
  if (ev_read_valid[slot]) VH_HIP(hipStreamWaitEvent(stream, ev_read[slot], 0));
  { int32_t rz = zero_bin_counters(set, 1); if (rz) return rz; }  // also clears the count, set right below
  if (n) VH_HIP(hipMemcpyAsync(sets.feat + (size_t)set * cap * 12, m, sizeof(int32_t) * 12 * (size_t)n, hipMemcpyHostToDevice, stream));
  VH_HIP(hipMemcpyAsync(sets.count + set, &n, sizeof(int32_t), hipMemcpyHostToDevice, stream));
  VH_HIP(hipStreamSynchronize(stream));
  int32_t rc = bin_sets(set, 1, false);
  if (rc) return rc;
  VH_HIP(hipEventRecord(ev_det[slot], stream));
  return VH_OK;
}

}  // namespace vh_engine
