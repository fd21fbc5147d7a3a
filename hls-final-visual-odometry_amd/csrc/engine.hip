// engine.hip -- host side of libviso_hip.so: device memory, geometry, the ring and its push paths
// (engine.h lists the other units).
//
// A vh_group owns S independent camera streams that are stepped together; a
// vh_matcher is a group of one.  The reference's Matcher state (ring buffer of
// two feature-set pairs, src/matcher.h:245-259) lives in HBM and rotates by
// moving the current/previous roles between the slots of a ring; nothing is copied on pushBack.
#include "engine.h"

namespace vh_engine {

thread_local std::string t_last_error;

// the role -> set mapping of the current step (vh_row_set), without the passes of a method
VhMatchArgs Group::role_args() const {
  VhMatchArgs a{};
  a.S = S; a.pair_cur = pairs(); a.rows = S;
  if (seq) {
    a.rows = seq_n;
    a.seq_prev_last = std::max(seq_n_prev - 1, 0);
    a.seq_lo = seq_first == 0 ? 1 : 0;
    a.seq_void = 2 * VH_RING * S;
  }
  return a;
}

int32_t Group::sync_all() {
  VH_HIP(hipStreamSynchronize(stream));
  VH_HIP(hipStreamSynchronize(match_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  VH_HIP(hipStreamSynchronize(down_stream));
  for (int k = 0; k < kVoteStreams; k++) if (vote_stream[k]) VH_HIP(hipStreamSynchronize(vote_stream[k]));
  if (sparse) { const int32_t rs = sparse->sync_all(); if (rs) return rs; }
  return check_violation();
}

// -DVH_CHECK builds: the kernels verify the index invariants they otherwise trust (vh_dev.h,
// VH_CHECK_RANGE) and record the first violation; the host aborts at the next point where it
// waits for the device anyway.  The shipped build compiles this to nothing.
int32_t Group::check_violation() {
#ifdef VH_CHECK
  if (allocated && sets.check) {
    VH_HIP(hipDeviceSynchronize());
    return report_violation(sets.check);
  }
#endif
  return VH_OK;
}

int32_t report_violation(const uint32_t *d_check) {
#ifdef VH_CHECK
  uint32_t c[4] = {0, 0, 0, 0};
  if (d_check) VH_HIP(hipMemcpy(c, d_check, sizeof(c), hipMemcpyDeviceToHost));
  if (c[0]) {
    fprintf(stderr, "VH_CHECK: %u index violations; first: code %u, value %d, bound %d (codes: vh_dev.h)\n", c[0], c[1], (int)c[2], (int)c[3]);
    fflush(stderr);
    abort();
  }
#endif
  return VH_OK;
}

int32_t upload_strided_lists(vh_p_match *dst, int64_t cap, const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t n) {
  for (int32_t l = 0; l < n; l++)
    if (counts[l]) VH_HIP(hipMemcpy(dst + (size_t)l * cap, pm + (size_t)l * stride, sizeof(vh_p_match) * (size_t)counts[l], hipMemcpyHostToDevice));
  return VH_OK;
}

// The lists a classification or a gain reads, on `st` behind the emission: the emission's own, or -- once the getters serve
// a host-side list for some stream -- all of them staged in `h`: the untouched streams' device lists and the replaced ones
// (each a subset of the device list it came from: it fits the slot).
int32_t Group::stage_host_lists(HostLists &h, hipStream_t st, bool &replaced, const vh_p_match *&pm, const int32_t *&counts) {
  pm = (const vh_p_match *)mt.d_matches; counts = mt.d_match_count;
  replaced = false;
  for (int32_t s = 0; s < S; s++) replaced = replaced || host_filtered[s] != 0;
  if (!replaced) return VH_OK;
  if (!h.d_pm) {  // one block: a refused allocation leaves nothing behind
    Carver c;
    const size_t o_pm = c.take<vh_p_match>((size_t)S * mcap), o_cnt = c.take<int32_t>((size_t)S);
    uint8_t *d = nullptr;
    const int32_t rc = dmalloc(&d, c.tight(), false);
    if (rc) return rc;
    h.d_pm = (vh_p_match *)(d + o_pm); h.d_cnt = (int32_t *)(d + o_cnt);
  }
  h.h_cnt.assign((size_t)S, 0);
  VH_HIP(hipMemcpyAsync(h.d_cnt, counts, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToDevice, st));
  for (int32_t s = 0; s < S; s++) {
    vh_p_match *dst = h.d_pm + (size_t)s * mcap;
    if (!host_filtered[s]) {
      VH_HIP(hipMemcpyAsync(dst, pm + (size_t)s * mcap, sizeof(vh_p_match) * (size_t)mcap, hipMemcpyDeviceToDevice, st));
      continue;
    }
    h.h_cnt[s] = (int32_t)std::min<size_t>(host_matches[s].size(), (size_t)mcap);
    if (h.h_cnt[s]) VH_HIP(hipMemcpyAsync(dst, host_matches[s].data(), sizeof(vh_p_match) * (size_t)h.h_cnt[s], hipMemcpyHostToDevice, st));
    VH_HIP(hipMemcpyAsync(h.d_cnt + s, &h.h_cnt[s], sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  pm = h.d_pm; counts = h.d_cnt;
  return VH_OK;
}

// everything allocate() and the calls after it made, so that the next ensure() starts from nothing (the work using it must have completed)
void Group::release() {
  vote_release();
  rh.release_device();
  allocs.clear(); device_bytes = 0;
  sets = {}; rf = {}; det = {}; mt = {}; stg = {}; pri = {}; tk = {}; ego = {}; post = {}; rg = {}; ms_vb = {}; inl = {}; rft = {}; cv = {}; mrf = {}; mps = {}; scn = {}; lmk = {}; lrf = {}; trj = {}; tcv = {}; gn = {};
  allocated = false;
}

// test hook (vh_group_debug_fail_next_alloc / _fail_alloc_after): true when the allocation about to be made is the one to fail
bool Group::alloc_refused() {
  if (!fail_next_alloc) return false;
  if (fail_alloc_skip > 0) { fail_alloc_skip--; return false; }
  fail_next_alloc = false;
  t_last_error = "allocation failure requested by vh_group_debug_fail_next_alloc";
  return true;
}

// release one block of `allocs` early (the work that used it must have completed)
void Group::dfree(void *q) {
  if (!q) return;
  auto it = std::find_if(allocs.begin(), allocs.end(), [q](const DeviceBlock &b) { return b.p == q; });
  if (it == allocs.end()) return;
  (void)hipStreamSynchronize(down_stream);
  allocs.erase(it);
}

// ---- geometry ----------------------------------------------------------
int32_t Group::block_count(int32_t extent, int32_t n) {
  // for (i=n+margin; i<extent-n-margin; i+=n+1)   (matcher.cpp:381-382)
  const int32_t lo = n + VH_MARGIN, hi = extent - n - VH_MARGIN;
  return hi > lo ? (hi - lo + n) / (n + 1) : 0;
}

int32_t Group::setup_geometry(const int32_t d[3]) {
  g = VhGeom{};
  g.W = d[0]; g.H = d[1]; g.bpl = d[2];
  if (p.half_resolution) {  // getHalfResolutionDimensions, matcher.cpp:566-570
    g.Wm = d[0] / 2; g.Hm = d[1] / 2;
    g.bplm = g.Wm > 0 ? g.Wm + 15 - (g.Wm - 1) % 16 : 16;
    g.scale = 2;
  } else {
    g.Wm = d[0]; g.Hm = d[1]; g.bplm = d[2]; g.scale = 1;
  }
  g.n = p.nms_n; g.tau = p.nms_tau;
  g.nbx = block_count(g.Wm, g.n); g.nby = block_count(g.Hm, g.n);
  if (g.nbx == 0 || g.nby == 0) g.nbx = g.nby = 0;
  g.nblocks = g.nbx * g.nby;
  g.nchunks = std::max(1, (g.nblocks + VH_CHUNK - 1) / VH_CHUNK);
  static const int32_t cand[][2] = {{32, 8}, {16, 8}, {16, 4}, {8, 4}, {4, 4}, {4, 2}, {2, 2}, {2, 1}, {1, 1}};
  for (auto &c : cand) {
    g.tbx = c[0]; g.tby = c[1];
    g.FW = g.tbx * (g.n + 1) + 2 * g.n; g.FH = g.tby * (g.n + 1) + 2 * g.n;
    g.IW = g.FW + 4; g.IH = g.FH + 4;
    g.IWp = round_up(g.IW, 4); g.FWp = g.FW;
    const size_t lds = (size_t)g.IH * g.IWp + 4 * (size_t)g.FH * g.FWp + 4 + 24 * (size_t)g.tbx * g.tby;
    if (lds <= 60 * 1024) return VH_OK;
  }
  return VH_ERR_UNSUPPORTED;
}

int32_t Group::ensure(const int32_t d[3]) {
  if (allocated && d[0] == dims[0] && d[1] == dims[1] && d[2] == dims[2]) return VH_OK;
  if (allocated) { int32_t rs = sync_all(); if (rs) return rs; release(); }
  const int32_t rc = allocate(d);
  // a failure half way leaves nothing behind: the next push starts from a clean slate (the memsets queued so far first)
  if (rc) { (void)hipStreamSynchronize(stream); release(); }
  return rc;
}

int32_t Group::allocate(const int32_t d[3]) {
  int32_t rc = check_dims(d, true);
  if (rc) return rc;
  // emit_features addresses its patch rows with 24 x 24 -> 32-bit byte offsets from the image base
  if (d[2] >= (1 << 24) || (int64_t)d[2] * d[1] > (1ll << 28)) return VH_ERR_UNSUPPORTED;
  if ((rc = setup_geometry(d))) return rc;
  dims[0] = d[0]; dims[1] = d[1]; dims[2] = d[2];
  int64_t c = req_features > 0 ? req_features : std::max<int64_t>(4 * (int64_t)g.nblocks, 64);
  if (c > (1 << VH_MASK_IDX_BITS) - 1) c = (1 << VH_MASK_IDX_BITS) - 1;  // feature indices are packed into VH_MASK_IDX_BITS bits (flow pixel mask)
  cap = (int32_t)c;
  mcap = req_matches > 0 ? req_matches : cap;

  sets = VhSets{};
  sets.cap = cap;
  sets.binsize = p.match_binsize;
  // exact for 0 <= x <= 32768 (every coordinate +- radius) when binsize <= 32768; a larger bin holds every x: quotient 0
  sets.inv_binsize = p.match_binsize > 32768 ? 0u : (uint32_t)(((1ull << 32) + p.match_binsize - 1) / p.match_binsize);
  sets.ubn = (dims[0] + p.match_binsize - 1) / p.match_binsize;  // ceil(W/binsize), matcher.cpp:282-283
  sets.vbn = (dims[1] + p.match_binsize - 1) / p.match_binsize;
  sets.nbins = 4 * sets.ubn * sets.vbn;
  sets.max_tiles = cap / VH_TILE_Q + 5;  // full tiles + one partial tile per class
  sets.W = dims[0]; sets.H = dims[1];
  {  // a bin of binsize px meets at most ceil(binsize/block)+1 NMS blocks per axis, one feature per class each
    const int32_t blk = g.scale * (g.n + 1);
    const int64_t per_axis = (p.match_binsize + blk - 1) / blk + 1;
    sets.stage_cap = (int32_t)std::min<int64_t>(per_axis * per_axis, cap);
  }
  const size_t ns = n_sets();
  if ((rc = dmalloc(&sets.feat, ns * cap * 12, false))) return rc;
  if ((rc = dmalloc(&sets.f_uv, ns * cap, false))) return rc;
  if ((rc = dmalloc(&sets.s_uv, ns * cap, false))) return rc;
  if ((rc = dmalloc(&sets.s_idx, ns * cap, false))) return rc;
  if ((rc = dmalloc(&sets.s_desc, ns * cap * 8, false))) return rc;
  if ((rc = dmalloc(&sets.bin_start, ns * (sets.nbins + 1), true))) return rc;
  if ((rc = dmalloc(&sets.hist, ns * sets.nbins, true))) return rc;
  if ((rc = dmalloc(&sets.cursor, ns * sets.nbins, true))) return rc;
  if ((rc = dmalloc(&sets.tmp_idx, ns * cap, false))) return rc;
  if ((rc = dmalloc(&sets.stage, ns * (size_t)sets.nbins * sets.stage_cap, false))) return rc;  // (per-bin staging lists: 2 MB per set at KITTI size)
  if ((rc = dmalloc(&sets.count, ns, true))) return rc;
  const size_t nrow = 4 * (size_t)dims[1];
  if ((rc = dmalloc(&sets.row_start, ns * (nrow + 1), true))) return rc;
  if ((rc = dmalloc(&sets.row_hist, ns * nrow, true))) return rc;
  if ((rc = dmalloc(&sets.row_cursor, ns * nrow, true))) return rc;
  if ((rc = dmalloc(&sets.r_pos, ns * cap, false))) return rc;
  if ((rc = dmalloc(&sets.tiles, ns * sets.max_tiles, false))) return rc;
  if ((rc = dmalloc(&sets.tile_cnt, ns, true))) return rc;
  if ((rc = dmalloc(&sets.snake_pos, ns * cap, false))) return rc;
  if ((rc = dmalloc(&sets.check, 4, true))) return rc;
  if ((rc = dmalloc(&det.d_rec, 2 * (size_t)S * std::max(g.nblocks, 1), false))) return rc;
  if ((rc = dmalloc(&det.d_chunk_count, 2 * (size_t)S * g.nchunks, true))) return rc;
  for (int k = 0; k < 2; k++) {
    if ((rc = dmalloc(&mt.d_best2[k], 4 * (size_t)S * cap, false))) return rc;
    if ((rc = dmalloc(&mt.d_chain2[k], 2 * (size_t)S * cap, false))) return rc;  // index tuple + coordinate tuple per driving feature
  }
  mt.d_best = mt.d_best2[0]; mt.d_chain = mt.d_chain2[0];
  for (int k = 0; k < 2; k++) {
    if ((rc = dmalloc(&mt.d_mchunk2[k], (size_t)S * ((cap + 255) / 256), true))) return rc;
    VH_HIP(mt.h_out[k].alloc((size_t)S, hipHostMallocMapped));
    memset(mt.h_out[k], 0, sizeof(int4) * (size_t)S);
  }
  if ((rc = dmalloc(&mt.d_redo, 2 * (size_t)S, true))) return rc;  // one set of counters per match-table buffer: the search of match n+1 runs beside the emission of match n
  if ((rc = dmalloc((uint8_t **)&mt.d_matches, (size_t)S * mcap * sizeof(vh_p_match), false))) return rc;
  if ((rc = dmalloc(&mt.d_match_count, (size_t)S, true))) return rc;
  if (serial && (size_t)S * mcap * sizeof(vh_p_match) <= (64u << 20)) {
    VH_HIP(mt.h_matches.alloc((size_t)S * mcap, hipHostMallocMapped));
  }
  if ((rc = dmalloc(&mt.d_overflow, (size_t)S, true))) return rc;
  VH_HIP(mt.h_overflow.alloc((size_t)S, hipHostMallocDefault));
  memset(mt.h_overflow, 0, sizeof(int32_t) * (size_t)S);
  if (p.half_resolution)
    if ((rc = dmalloc(&det.d_half, 2 * (size_t)S * g.bplm * g.Hm, false))) return rc;
  if (p.refinement > 0) {  // (a sequence handle's empty sets hold no features: they need no planes)
    vh_refine_setup(rf);
    rf.W = dims[0]; rf.H = dims[1]; rf.bpl = dims[2];
    rf.pitch = round_up(dims[0], 16);
    rf.plane = (int64_t)rf.pitch * dims[1];
    rf.mode = p.refinement == 2 ? 2 : 1;
    const size_t nplanes = 2 * VH_RING * (size_t)S;
    if ((rc = dmalloc(&rf.du, nplanes * rf.plane, false))) return rc;
    if ((rc = dmalloc(&rf.dv, nplanes * rf.plane, false))) return rc;
    for (int k = 0; k < 2; k++)
      if ((rc = dmalloc(&mt.d_ref2[k], 2 * (size_t)S * cap, false))) return rc;
  }
  if (gain_on) {  // the left images of the ring (a sequence handle's empty sets hold no image)
    gn.pitch = round_up(dims[0], 16);
    gn.plane = (int64_t)gn.pitch * dims[1];
    if ((rc = dmalloc(&gn.d_planes, VH_RING * (size_t)S * gn.plane, false))) return rc;
  }
  allocated = true;
  pair_cur = 0; pair_prev = 1; frames = 0; mt.epoch = 0; last_method = -1; failed = false;
  seq_n = seq_n_prev = 0; seq_first = seq_total = 0; trk_reset();
  host_matches.assign((size_t)S, {}); host_filtered.assign((size_t)S, 0);
  for (int k = 0; k < VH_RING; k++) ev_read_valid[k] = false;
  ev_post_valid[0] = ev_post_valid[1] = false; match_seq = 0;
  // every slot starts "detected" (empty): matches may wait on any of them
  for (int k = 0; k < VH_RING; k++) VH_HIP(hipEventRecord(ev_det[k], stream));
  return VH_OK;
}

void Group::prof_collect() {
  for (auto &kv : prof_entries) {
    for (auto &pr : kv.second.pending) {
      float ms = 0;
      (void)hipEventSynchronize(pr.second);
      (void)hipEventElapsedTime(&ms, pr.first, pr.second);
      kv.second.ms += ms; kv.second.launches++;
    }
    kv.second.pending.clear();
  }
}

void Group::prof_host(const char *name, std::chrono::steady_clock::time_point t0) {
  if (!prof) return;
  ProfEntry &e = prof_entries[name];
  e.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); e.launches++;
}

// ---- detect + bin ------------------------------------------------------
int32_t Group::zero_bin_counters(int32_t set0, int32_t nsets, int32_t *extra, int64_t n_extra) {
  // one launch instead of a memset per array
  vh_launch_zero_counters(sets, set0, nsets, extra, n_extra, stream);
  VH_HIP(hipGetLastError());
  return VH_OK;
}

// staged: the histograms and per-bin member lists were already produced by
// emit_features; otherwise (caller-supplied features) build them here.
int32_t Group::bin_sets(int32_t set0, int32_t nsets, bool staged) {
  if (!staged) { Scope sc(this, "bin_hist", stream); vh_launch_bin_hist(sets, set0, nsets, stream); }
  { Scope sc(this, "bin_scan", stream); vh_launch_bin_scan(sets, set0, nsets, stream); }
  if (!staged) { Scope sc(this, "bin_fill", stream); vh_launch_bin_fill(sets, set0, nsets, stream); }
  { Scope sc(this, "bin_sort", stream); vh_launch_bin_sort(sets, set0, nsets, staged ? 1 : 0, stream); }
  VH_HIP(hipGetLastError());
  return VH_OK;
}

// pushBack: a failure after the ring has rotated leaves the new slot half written;
// the roles are put back and the handle refuses to match (VH_ERR_STATE) until a
// later push has succeeded.
// rows: streams whose images are pushed (a sequence chunk: its frames; the counters of the other rows of the slot
// read 0); < 0: all S
int32_t Group::push_device(const void *dI1, const void *dI2, int64_t stride, const int32_t d[3], int32_t replace, int32_t rows) {
  if (!dI1 || !d) return VH_ERR_INVALID_ARG;
  if (rows < 0) rows = S;
  int32_t rc = ensure(d);
  if (rc != VH_OK) return rc;
  const int32_t old_cur = pair_cur, old_prev = pair_prev;
  const int64_t old_frames = frames;
  rc = push_device_queued(dI1, dI2, stride, d, replace, rows);
  if (rc == VH_OK && sparse) {
    // the sparse sets of the same images, behind the dense ones on the same stream; the images stay in use until then
    rc = sparse->push_device(dI1, dI2, stride, d, replace, rows);
    if (rc == VH_OK && hipEventRecord(ev_det[pair_cur], stream) != hipSuccess) rc = VH_ERR_HIP;
  }
  if (rc != VH_OK) { pair_cur = old_cur; pair_prev = old_prev; frames = old_frames; failed = true; }
  else {
    failed = false;
    trk_pushed(pair_cur != old_cur, old_frames == 0, seq_n);
    recon_pushed(old_frames == 0, pair_cur != old_cur);
    traj_pushed(pair_cur != old_cur || old_frames == 0);
    if (seq) { seq_n_prev = seq_n; seq_n = rows; seq_first = seq_total; seq_total += rows; }
  }
  return rc;
}

int32_t Group::push_device_queued(const void *dI1, const void *dI2, int64_t stride, const int32_t d[3], int32_t replace, int32_t rows) {
  int32_t rc = VH_OK;
  if (!replace && frames > 0) {  // ring buffer shift (matcher.cpp:64-79): prev <- cur, cur <- the slot used longest ago
    const int32_t fresh = (pair_cur + 1) % VH_RING;
    pair_prev = pair_cur;
    pair_cur = fresh;
  }
  frames++;
  drop_host_matches(); last_method = -1;
  const int32_t set0 = pair_cur * 2 * S, nsets = 2 * S;
  // order after the caller's stream (image producers) and after the last match
  // that still reads the slot we are about to overwrite
  if (user_stream_set) {
    VH_HIP(hipEventRecord(ev_user, user_stream));
    VH_HIP(hipStreamWaitEvent(stream, ev_user, 0));
  }
  if (ev_read_valid[pair_cur]) VH_HIP(hipStreamWaitEvent(stream, ev_read[pair_cur], 0));
  if ((rc = zero_bin_counters(set0, nsets, det.d_chunk_count, 2 * (int64_t)S * g.nchunks))) return rc;
  // The group is detected in up to four sub-batches of streams, one after the other on this
  // stream: the latency-bound kernels of a sub-batch (emit_features, bin_scan, bin_sort: < 45 %
  // of the VALU issue slots) then run beside the issue-bound ones of its neighbours and of the
  // previous frame's search instead of all at once.  Measured on MI355X, KITTI, S = 256 (with
  // the post stream): 1 / 2 / 4 / 8 / 16 sub-batches = 94.9 / 95.9 / 97.1 / 92.1 / 82.0 k pairs/s
  // -- below ~12 k detection workgroups per launch the launches themselves cost more.  (Round 1
  // measured the opposite, -9 % at n = 2: its kernels were not yet issue-bound.)  Sub-batches on
  // two alternating streams lose 8 %.  VH_SUBBATCH=n overrides.
  const int32_t ncam = dI2 ? 2 : 1;
  static const int subbatch_env = [] { const char *ev = getenv("VH_SUBBATCH"); return ev ? atoi(ev) : 0; }();
  const int64_t det_wgs = (int64_t)rows * ncam * ((g.nblocks + 255) / 256);
  // (a mono push is half the detection work of a stereo one: 4 sub-batches of 64 KITTI images leave emit_features with two
  //  rounds of workgroups per launch -- mono flow, S = 256: 1 / 2 / 4 / 8 sub-batches = 118 / 115 / 109 / 101 k frames/s)
  const int32_t subbatch = subbatch_env > 0 ? subbatch_env : (serial ? 1 : (int32_t)std::min<int64_t>(4, det_wgs / (ncam == 2 ? 12000 : 40000)));
  const int32_t nsub = std::max(1, std::min(subbatch, rows));
  const int32_t ssub = (rows + nsub - 1) / nsub;
  for (int32_t s0 = 0; s0 < rows; s0 += ssub) {
    const int32_t sn = std::min(ssub, rows - s0);
    VhImages im{};
    im.base[0] = (const uint8_t *)dI1 + (int64_t)s0 * stride;
    im.base[1] = dI2 ? (const uint8_t *)dI2 + (int64_t)s0 * stride : nullptr;
    im.stride = stride; im.ncam = ncam; im.S = sn; im.S_total = S; im.s0 = s0; im.pair_cur = pair_cur;
    uint64_t *rec = det.d_rec + (size_t)s0 * ncam * std::max(g.nblocks, 1);
    // the refinement's planes come from the pushed full-resolution images, inside the window they are borrowed for
    if (p.refinement > 0) { Scope sc(this, "refine_planes", stream); vh_launch_refine_planes(im, rf, stream); }
    if (gain_on && (rc = gain_copy(im))) return rc;  // (likewise: the full-resolution left images, before `im` turns to the half ones)
    int32_t *chunks = det.d_chunk_count + (size_t)s0 * ncam * g.nchunks;
    if (p.half_resolution) {
      const int64_t isz = (int64_t)g.bplm * g.Hm;
      uint8_t *half = det.d_half + (int64_t)s0 * ncam * isz;
      { Scope sc(this, "half_res", stream); vh_launch_half_res(im, half, g, stream); }
      // half images are stored by image id; present them as cameras with stride ncam*isz
      im.base[0] = half; im.base[1] = half + isz; im.stride = isz * ncam;
    }
    { Scope sc(this, "detect_nms", stream); vh_launch_detect_nms(im, g, rec, chunks, stream); }
    { Scope sc(this, "emit_features", stream); vh_launch_emit_features(im, g, rec, chunks, sets, stream); }
    VH_HIP(hipGetLastError());
    if ((rc = bin_sets(set0 + 2 * s0, 2 * sn, true))) return rc;
  }
  VH_HIP(hipEventRecord(ev_det[pair_cur], stream));
  return VH_OK;
}

int32_t Group::push_host(const uint8_t *I1, const uint8_t *I2, int64_t stride, const int32_t d[3], int32_t replace, int32_t rows) {
  if (!I1 || !d) return VH_ERR_INVALID_ARG;
  if (rows < 0) rows = S;
  int32_t rc = ensure(d);
  if (rc != VH_OK) return rc;
  const size_t isz = (size_t)d[2] * d[1];
  if (stg.stage_bytes < isz * S) {  // (once per allocation: a failure here releases the handle as a failed ensure() does)
    VH_HIP(hipStreamSynchronize(stream));
    for (int sl = 0; sl < 2 && !rc; sl++)
      for (int k = 0; k < 2 && !rc; k++) rc = dmalloc(&stg.d_stage_buf[sl][k], isz * S, false);
    if (rc) { (void)sync_all(); release(); return rc; }
    stg.stage_bytes = isz * S;
    stg.ev_stage_valid[0] = stg.ev_stage_valid[1] = false;
  }
  const int32_t sl = stage_slot;
  stage_slot ^= 1;
  // the detection that last read this staging slot (two pushes ago) must be done
  hipStream_t cs = serial ? stream : copy_stream;  // (a small group runs everything on one stream: no hand-over between streams)
  if (stg.ev_stage_valid[sl] && !serial) VH_HIP(hipStreamWaitEvent(cs, ev_stage[sl], 0));
  for (int k = 0; k < 2; k++) {
    const uint8_t *src = k ? I2 : I1;
    stg.d_stage[k] = stg.d_stage_buf[sl][k];
    if (!src) continue;
    if (stride == (int64_t)isz) {  // one transfer for all the images
      VH_HIP(hipMemcpyAsync(stg.d_stage[k], src, isz * rows, hipMemcpyHostToDevice, cs));
    } else {
      for (int32_t s = 0; s < rows; s++)
        VH_HIP(hipMemcpyAsync(stg.d_stage[k] + isz * s, src + stride * s, isz, hipMemcpyHostToDevice, cs));
    }
  }
  // The images are only borrowed for the duration of the call (demo.cpp:250-251): the host waits for the
  // copies -- but only after the detection has been queued behind them, so the first kernel starts
  // when the last byte lands instead of a host round trip later.
  VH_HIP(ev_h2d.create());
  VH_HIP(hipEventRecord(ev_h2d, cs));
  if (!serial) VH_HIP(hipStreamWaitEvent(stream, ev_h2d, 0));
  rc = push_device(stg.d_stage[0], I2 ? stg.d_stage[1] : nullptr, (int64_t)isz, d, replace, rows);
  VH_HIP(hipEventSynchronize(ev_h2d));
  if (rc == VH_OK) {
    VH_HIP(hipEventRecord(ev_stage[sl], stream));
    stg.ev_stage_valid[sl] = true;
  }
  return rc;
}

int32_t check_params(const vh_params *p) {
  if (!p) return VH_ERR_INVALID_ARG;
  if (p->nms_n < 1 || p->nms_n > 32 || p->match_binsize < 1 || p->match_radius < 0 || p->match_disp_tolerance < 0 ||
      p->match_radius > 16384 || p->match_disp_tolerance > 16384 || p->nms_tau < 0)  // the accept test packs 2*tolerance into 16 bits
    return VH_ERR_UNSUPPORTED;
  return VH_OK;
}

int32_t select_device(int32_t device) {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) { t_last_error = "no HIP device visible"; return VH_ERR_NO_DEVICE; }
  if (device < 0 || device >= cnt) return VH_ERR_INVALID_ARG;
  VH_HIP(hipSetDevice(device));
  return VH_OK;
}

int32_t group_new(const vh_params *p, int32_t device, int32_t S, int32_t mf, int32_t mm, Group **out) {
  if (!out) return VH_ERR_INVALID_ARG;
  *out = nullptr;
  int32_t rc = check_params(p);
  if (rc) return rc;
  if (S < 1 || S > 65535 / 4 || mf < 0 || mm < 0) return VH_ERR_INVALID_ARG;
  if ((rc = select_device(device))) return rc;
  Group *gq = new Group();
  gq->p = *p; gq->device = device; gq->S = S; gq->req_features = mf; gq->req_matches = mm;
  // Both streams at the default priority: raising the detect stream's priority
  // (so that detection finishes inside the shadow of the flow search) was
  // measured and lost ~3 % -- the single-workgroup-per-set kernels then wait for
  // the starved low-priority stream instead (profiles/, round 1).
  int prio_lo = 0, prio_hi = 0;
  if (getenv("VH_DET_PRIORITY")) (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (gq->own_stream.create(prio_hi) != hipSuccess) {
    t_last_error = "hipStreamCreateWithFlags failed";
    gq->own_stream.alias(nullptr); delete gq;
    return VH_ERR_HIP;
  }
  gq->stream = gq->own_stream;
  // VH_SERIAL=1 (profiling aid): run matching on the detect stream, i.e. no
  // overlap, so that per-kernel timings are exclusive
  // A small group (one or two cameras: the drop-in Matcher) also runs on one stream: it fills a few percent of
  // the chip, detection of frame t+1 has nothing to hide behind, and every hand-over between streams is a
  // ~14 us bubble on the path pushBack -> matchFeatures -> getMatches (VH_SERIAL=0 keeps the three streams).
  const char *serial = getenv("VH_SERIAL");
  bool ok = true;
  if (serial ? serial[0] == '1' : S <= 2) gq->match_stream.alias(gq->own_stream), gq->post_stream.alias(gq->own_stream), gq->serial = true;
  else {
    ok = gq->match_stream.create(prio_lo) == hipSuccess;
    // The chain/emission step runs on a stream of its own so that consecutive searches run back
    // to back and the two short, latency-bound kernels hide beside the next search: +2.8 % on
    // MI355X (KITTI, S = 256).  (Round 1 measured -17 % for the same switch, when the searches
    // did not yet fill the chip's issue slots.)  VH_POST_STREAM=0: same stream as the search.
    const char *pse = getenv("VH_POST_STREAM");
    if (ok && !(pse && pse[0] == '0')) ok = gq->post_stream.create(prio_lo) == hipSuccess;
    else gq->post_stream.alias(gq->match_stream);
  }
  for (int k = 0; k < 2 && ok; k++) ok = gq->ev_tables[k].create() == hipSuccess && gq->ev_post[k].create() == hipSuccess;
  for (int k = 0; k < VH_RING && ok; k++) ok = gq->ev_det[k].create() == hipSuccess && gq->ev_read[k].create() == hipSuccess;
  ok = ok && gq->ev_user.create() == hipSuccess;
  // VH_FLOW_TESTED=1 / =0: always the tested / always the speculative loops (default: adaptive)
  if (const char *ft = getenv("VH_FLOW_TESTED")) gq->force_mode = atoi(ft) ? 0 : 1;
  for (int k = 0; k < 2 && ok; k++) ok = gq->ev_stage[k].create() == hipSuccess;
  ok = ok && gq->copy_stream.create() == hipSuccess;
  ok = ok && gq->down_stream.create() == hipSuccess;
  ok = ok && gq->ev_down.create() == hipSuccess;
  if (!ok) { t_last_error = "stream/event creation failed"; delete gq; return VH_ERR_HIP; }
  *out = gq;
  return VH_OK;
}

}  // namespace vh_engine
