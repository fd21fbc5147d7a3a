// engine_post.hip -- what follows a match call: downloads and getters, outlier removal, the group estimators, the
// post pipelines on the host and on the device, bucketing and the host form of the prior statistics (engine.h).
#include "engine.h"

#include <atomic>
#include <thread>

namespace vh_engine {

// fn(s) for every stream s of [lo, hi), on up to `threads` host threads (the caller's is one of them), one stream per task
template <class Fn> static void for_each_stream(int32_t lo, int32_t hi, int32_t threads, Fn fn) {
  std::atomic<int32_t> next(lo);
  const auto work = [&]() { for (int32_t s = next++; s < hi; s = next++) fn(s); };
  std::vector<std::thread> pool;
  for (int32_t w = 1; w < std::min(threads, hi - lo); w++) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
}

// The voted sparse list of stream s in device mode: from the vote buffer (waits for the vote)
int32_t Group::get_sparse_device(int32_t s, vh_p_match *out, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || capo < 0 || (capo > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!allocated || !ms_vb.block || sparse->last_method < 0) return VH_OK;
  VH_HIP(hipStreamSynchronize(sparse->post_stream));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  VhVoteMeta m{};
  VH_HIP(hipMemcpy(&m, ms_vb.v.meta + s, sizeof(m), hipMemcpyDeviceToHost));
  if (m.status == VH_VOTE_TRUNCATED) return VH_ERR_CAPACITY;
  if (m.status != VH_VOTE_OK && m.status != VH_VOTE_SKIP) return VH_ERR_UNSUPPORTED;
  *n = m.kept;
  const int32_t k = std::min(m.kept, capo);
  if (k > 0) VH_HIP(hipMemcpy(out, ms_vb.v.pm + (size_t)s * ms_vb.v.cap, sizeof(vh_p_match) * (size_t)k, hipMemcpyDeviceToHost));
  return m.kept > capo ? VH_ERR_CAPACITY : VH_OK;
}

// Start the device->host copy of every stream's first cap_per_stream match
// records and of the S counts, ordered after the emission of the last step,
// and return at once.  One strided transfer: the copy engine moves it while
// the next step computes (its emit_matches waits for the download, above).
int32_t Group::download_async(vh_p_match *out, int32_t cap_per_stream, int32_t *counts) {
  if (!out || !counts || cap_per_stream < 1) return VH_ERR_INVALID_ARG;
  if (!allocated || last_method < 0) return VH_ERR_STATE;
  VH_HIP(hipStreamWaitEvent(down_stream, ev_post[last_buf], 0));
  const size_t width = sizeof(vh_p_match) * (size_t)std::min(cap_per_stream, mcap);
  VH_HIP(hipMemcpy2DAsync(out, sizeof(vh_p_match) * (size_t)cap_per_stream, mt.d_matches, sizeof(vh_p_match) * (size_t)mcap,
                          width, (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipMemcpyAsync(counts, mt.d_match_count, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipMemcpyAsync(mt.h_overflow, mt.d_overflow, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipEventRecord(ev_down, down_stream));
  mt.ev_down_valid = true;
  return VH_OK;
}

int32_t Group::wait_download() {
  if (!mt.ev_down_valid) return VH_OK;
  VH_HIP(hipEventSynchronize(ev_down));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  for (int32_t s = 0; s < S; s++) if (mt.h_overflow[s]) return VH_ERR_CAPACITY;
  return VH_OK;
}

int32_t Group::get_matches(int32_t s, vh_p_match *out, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || capo < 0 || (capo > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!allocated || last_method < 0) return VH_OK;
  if (host_filtered[s]) {
    *n = (int32_t)host_matches[s].size();
    const int32_t k = std::min(*n, capo);
    if (k) memcpy(out, host_matches[s].data(), sizeof(vh_p_match) * (size_t)k);
    return *n > capo ? VH_ERR_CAPACITY : VH_OK;
  }
  // count and overflow flag of the last launch: host-mapped memory, valid once its emission has run
  VH_HIP(hipEventSynchronize(ev_post[last_buf]));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  const int32_t cnt = mt.h_out[last_buf][s].x, ov = mt.h_out[last_buf][s].y;
  *n = cnt;
  const int32_t k = std::min(std::min(cnt, mcap), capo);
  if (k > 0 && mt.h_matches) {
    memcpy(out, mt.h_matches + (size_t)s * mcap, sizeof(vh_p_match) * (size_t)k);
  } else if (k > 0) {
    VH_HIP(hipMemcpyAsync(out, (const uint8_t *)mt.d_matches + (size_t)s * mcap * sizeof(vh_p_match),
                          sizeof(vh_p_match) * (size_t)k, hipMemcpyDeviceToHost, post_stream));
    VH_HIP(hipStreamSynchronize(post_stream));
  }
  // ov: a feature set of this match exceeded the feature capacity (the records beyond
  // it were dropped, so the list above comes from a truncated set)
  return (cnt > capo || cnt > mcap || ov) ? VH_ERR_CAPACITY : VH_OK;
}

int32_t Group::get_features(int32_t s, int32_t which, int32_t *out12, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || which < 0 || which > 3 || capo < 0 || (capo > 0 && !out12)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!allocated) return VH_OK;
  const int32_t set = vh_row_set(role_args(), s, which);
  int32_t cnt = 0;
  VH_HIP(hipMemcpyAsync(&cnt, sets.count + set, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  VH_HIP(hipStreamSynchronize(stream));
  *n = cnt;
  const int32_t k = std::min(std::min(cnt, cap), capo);
  if (k > 0) {
    VH_HIP(hipMemcpyAsync(out12, sets.feat + (size_t)set * cap * 12, sizeof(int32_t) * 12 * (size_t)k,
                          hipMemcpyDeviceToHost, stream));
    VH_HIP(hipStreamSynchronize(stream));
  }
  return (cnt > capo || cnt > cap) ? VH_ERR_CAPACITY : VH_OK;
}

int32_t Group::get_counts(int32_t *nf, int32_t *nm) {
  if (!allocated) return VH_ERR_STATE;
  if (nf) {
    std::vector<int32_t> all(n_sets());
    VH_HIP(hipMemcpyAsync(all.data(), sets.count, sizeof(int32_t) * all.size(), hipMemcpyDeviceToHost, stream));
    VH_HIP(hipStreamSynchronize(stream));
    const VhMatchArgs a = role_args();
    for (int32_t s = 0; s < S; s++)
      for (int32_t r = 0; r < 4; r++) nf[4 * s + r] = all[vh_row_set(a, s, r)];
  }
  if (nm) {
    VH_HIP(hipMemcpyAsync(nm, mt.d_match_count, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
    VH_HIP(hipStreamSynchronize(post_stream));
    for (int32_t s = 0; s < S; s++)
      if (host_filtered[s]) nm[s] = (int32_t)host_matches[s].size();
  }
  return VH_OK;
}

// All streams' matches in one go: counts first, then one transfer per stream
// into out[s * cap_per_stream ...], a single wait at the end.
int32_t Group::get_matches_all(vh_p_match *out, int32_t cap_per_stream, int32_t *counts) {
  if (!out || !counts || cap_per_stream < 0) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < S; s++) counts[s] = 0;
  if (!allocated || last_method < 0) return VH_OK;
  VH_HIP(hipMemcpyAsync(counts, mt.d_match_count, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(mt.h_overflow, mt.d_overflow, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  bool over = false;
  for (int32_t s = 0; s < S; s++) over = over || mt.h_overflow[s] != 0;
  for (int32_t s = 0; s < S; s++) {
    if (host_filtered[s]) {
      counts[s] = (int32_t)host_matches[s].size();
      const int32_t k = std::min(counts[s], cap_per_stream);
      if (k) memcpy(out + (size_t)s * cap_per_stream, host_matches[s].data(), sizeof(vh_p_match) * (size_t)k);
      over = over || counts[s] > cap_per_stream;
      continue;
    }
    const int32_t k = std::min(std::min(counts[s], mcap), cap_per_stream);
    over = over || counts[s] > cap_per_stream || counts[s] > mcap;
    if (k > 0)
      VH_HIP(hipMemcpyAsync(out + (size_t)s * cap_per_stream, (const uint8_t *)mt.d_matches + (size_t)s * mcap * sizeof(vh_p_match),
                            sizeof(vh_p_match) * (size_t)k, hipMemcpyDeviceToHost, post_stream));
  }
  VH_HIP(hipStreamSynchronize(post_stream));
  return over ? VH_ERR_CAPACITY : VH_OK;
}

// Bring stream s's current matches to the host (no-op if already there).
int32_t Group::fetch_matches(int32_t s) {
  if (s < 0 || s >= S) return VH_ERR_INVALID_ARG;
  if (!allocated || last_method < 0) return VH_ERR_STATE;
  if (host_filtered[s]) return VH_OK;
  int32_t n = 0;
  int32_t rc = get_matches(s, nullptr, 0, &n);
  if (rc != VH_OK && rc != VH_ERR_CAPACITY) return rc;
  if (n > mcap) return VH_ERR_CAPACITY;
  std::vector<vh_p_match> pm((size_t)n);
  if ((rc = get_matches(s, n ? pm.data() : nullptr, n, &n))) return rc;  // VH_ERR_CAPACITY: a feature set overflowed
  host_matches[s].swap(pm);
  host_filtered[s] = 1;
  return VH_OK;
}

// removeOutliers (remove_outliers.cpp:4-94) on streams [0, S): host work, one
// stream per task, `threads` workers.  Stereo records carry no previous-frame
// position (u1p = -1), so the reference's flow vote only applies to flow and quad
// matches; under the stock rule (vh_group_set_vote_rule) a stereo list is voted on its disparities.
int32_t Group::remove_outliers(int32_t s_lo, int32_t s_hi, int32_t threads) {
  if (!allocated || last_method < 0) return VH_ERR_STATE;
  if (!votes_on(last_method)) return VH_OK;
  const vh_vote_rule rule = rule_for(last_method);
  for (int32_t s = s_lo; s < s_hi; s++) {
    const int32_t rc = fetch_matches(s);
    if (rc) return rc;
  }
  std::atomic<int32_t> failed(0);
  for_each_stream(s_lo, s_hi, threads, [&](int32_t s) {
    std::vector<vh_p_match> &pm = host_matches[s];
    int32_t kept = 0;
    if (vh_remove_outliers_pm_rule(pm.data(), (int32_t)pm.size(), &rule, &kept) != VH_OK) { failed = 1; return; }
    pm.resize((size_t)kept);
  });
  return failed ? VH_ERR_INVALID_ARG : VH_OK;
}

// The shared end of the group estimators, on the post stream behind the kernels: the results, and the verdict on the
// lists they came from -- a truncated match list or feature set yields a pose of the truncated data: say so, as every
// get_matches path does.
int32_t Group::estimate_results(double *tr, int32_t *ok, int32_t *ninl) {
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(tr, ego.d_ego_tr, sizeof(double) * 6 * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ok, ego.d_ego_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ninl, ego.d_ego_ok + S, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  std::vector<int32_t> cnt((size_t)S);
  VH_HIP(hipMemcpyAsync(cnt.data(), mt.d_match_count, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(mt.h_overflow, mt.d_overflow, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  for (int32_t s = 0; s < S; s++) if (cnt[s] > mcap || mt.h_overflow[s]) return VH_ERR_CAPACITY;
  return VH_OK;
}

// VisualOdometryStereo::estimateMotion on the device-resident quad match lists of every stream (scratch: EgoScratch)
int32_t Group::estimate_motion(const vh_ego_params *e, const int32_t *rand3, double *tr, int32_t *ok, int32_t *ninl) {
  if (!e || !rand3 || !tr || !ok || !ninl || e->ransac_iters < 1) return VH_ERR_INVALID_ARG;
  if (!allocated || last_method != VH_METHOD_QUAD) return VH_ERR_STATE;
  const size_t nr = (size_t)S * e->ransac_iters * 3;
  int32_t rc;
  if (!ego.d_ego_xyz) {
    if ((rc = dmalloc(&ego.d_ego_xyz, (size_t)S * mcap * 4, false))) return rc;
    if (!ego.d_ego_tr) {
      if ((rc = dmalloc(&ego.d_ego_tr, 6 * (size_t)S, false))) return rc;
      if ((rc = dmalloc(&ego.d_ego_ok, 2 * (size_t)S, false))) return rc;
    }
  }
  if (ego.ego_rand_n < nr) {  // (the old block stays in `allocs` until the group is released: a few KB per change of ransac_iters)
    if ((rc = dmalloc(&ego.d_ego_rand, nr, false))) return rc;
    ego.ego_rand_n = nr;
  }
  VH_HIP(hipMemcpyAsync(ego.d_ego_rand, rand3, sizeof(int32_t) * nr, hipMemcpyHostToDevice, post_stream));
  {
    Scope sc(this, "ego_kernel", post_stream);
    vh_launch_ego(*e, VhLists::slots((const vh_p_match *)mt.d_matches, mcap, mt.d_match_count, mcap, S), ego.d_ego_rand, ego.d_ego_xyz, mcap, ego.d_ego_tr, ego.d_ego_ok,
                  ego.d_ego_ok + S, nullptr, 0, post_stream);
  }
  return estimate_results(tr, ok, ninl);
}

// VisualOdometryMono::estimateMotion on the device-resident match lists of every stream
// (model, nullable: [S] the lists' models come back too, through a device block of 128 bytes per stream allocated on first need)
int32_t Group::estimate_motion_mono(const vh_mono_params *e, const int32_t *rand8, double *tr, int32_t *ok, int32_t *ninl, vh_mono_model *model) {
  if (!e || !rand8 || !tr || !ok || !ninl || e->ransac_iters < 1) return VH_ERR_INVALID_ARG;
  if (!allocated || (last_method != VH_METHOD_FLOW && last_method != VH_METHOD_QUAD)) return VH_ERR_STATE;
  const size_t nr = (size_t)S * e->ransac_iters * 8;
  int32_t rc;
  if ((int64_t)S * e->ransac_iters > (int64_t)1 << 31) return VH_ERR_UNSUPPORTED;
  if (!ego.d_mono_scratch || ego.mono_scratch_iters < e->ransac_iters) {
    if ((rc = dmalloc(&ego.d_mono_scratch, (size_t)vh_mono_scratch_bytes(S, mcap, e->ransac_iters), false))) return rc;
    ego.mono_scratch_iters = e->ransac_iters;
    if (!ego.d_ego_tr) {
      if ((rc = dmalloc(&ego.d_ego_tr, 6 * (size_t)S, false))) return rc;
      if ((rc = dmalloc(&ego.d_ego_ok, 2 * (size_t)S, false))) return rc;
    }
  }
  if (ego.mono_rand_n < nr) {
    if ((rc = dmalloc(&ego.d_mono_rand, nr, false))) return rc;
    ego.mono_rand_n = nr;
  }
  if (model && !ego.d_mono_model && (rc = dmalloc(&ego.d_mono_model, (size_t)S, false))) return rc;
  VH_HIP(hipMemcpyAsync(ego.d_mono_rand, rand8, sizeof(int32_t) * nr, hipMemcpyHostToDevice, post_stream));
  vh_launch_mono(*e, VhLists::slots((const vh_p_match *)mt.d_matches, mcap, mt.d_match_count, mcap, S), ego.d_mono_rand, ego.d_mono_scratch, mcap, ego.d_ego_tr,
                 ego.d_ego_ok, ego.d_ego_ok + S, nullptr, 0, model ? ego.d_mono_model : nullptr, post_stream);
  if (model) VH_HIP(hipMemcpyAsync(model, ego.d_mono_model, sizeof(vh_mono_model) * (size_t)S, hipMemcpyDeviceToHost, post_stream));  // (estimate_results waits for the stream)
  return estimate_results(tr, ok, ninl);
}

// ---- the steps after matching, pipelined -----------------------------------
// What the reference's loop does after Matcher::matching -- removeOutliers (src/matcher.cpp:108),
// bucketFeatures (src/viso_stereo.cpp:41-43 -> matcher.cpp:140-187), estimateMotion
// (src/viso_stereo.cpp:49-51) -- for every stream of the group: post_begin() starts the download of the
// step's match lists into one of two page-locked slots and returns; post_finish() runs the Delaunay
// vote and the bucketing of a begun step on `threads` host threads (one stream per task), uploads the
// bucketed lists (a few hundred records per stream) and runs the batched egomotion kernel on them.
// A caller that issues step t+1 before finishing step t has the host work of t running beside the
// GPU work of t+1.

int32_t Group::post_begin(int32_t cap_ps) {
  if (cap_ps < 1) return VH_ERR_INVALID_ARG;
  if (!allocated || last_method < 0) return VH_ERR_STATE;
  PostSlot &sl = post.slot[post_seq & 1];
  cap_ps = std::min(cap_ps, mcap);
  if (sl.cap_ps < cap_ps) {
    VH_HIP(sl.h_pm.alloc((size_t)S * cap_ps, hipHostMallocDefault));
    sl.cap_ps = cap_ps;
  }
  if (!sl.h_cnt) VH_HIP(sl.h_cnt.alloc(2 * (size_t)S, hipHostMallocDefault));
  VH_HIP(sl.ev.create());
  VH_HIP(hipStreamWaitEvent(down_stream, ev_post[last_buf], 0));
  sl.width = cap_ps;
  VH_HIP(hipMemcpy2DAsync(sl.h_pm, sizeof(vh_p_match) * (size_t)sl.cap_ps, mt.d_matches, sizeof(vh_p_match) * (size_t)mcap,
                          sizeof(vh_p_match) * (size_t)cap_ps, (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipMemcpyAsync(sl.h_cnt, mt.d_match_count, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipMemcpyAsync(sl.h_cnt + S, mt.d_overflow, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipEventRecord(sl.ev, down_stream));
  // the next step's emission must not overwrite the lists before they have left (as vh_group_download_matches_async)
  VH_HIP(hipEventRecord(ev_down, down_stream)); mt.ev_down_valid = true;
  sl.pending = true; sl.method = last_method;
  post_seq++;
  return VH_OK;
}

// (e: the stereo estimator with rand3, or mono: the monocular one with rand8 -- at most one of them)
int32_t Group::post_finish(int32_t age, int32_t max_features, float bw, float bh, int32_t threads, const vh_ego_params *e, const int32_t *rand3,
                    const vh_mono_params *mono, const int32_t *rand8,
                    double *tr, int32_t *ok, int32_t *ninl, vh_p_match *out, int32_t out_cap, int32_t *out_counts, double *host_ms) {
  if (age < 0 || age > 1 || max_features < 1 || !(bw > 0) || !(bh > 0) || threads < 1 || (e && mono)) return VH_ERR_INVALID_ARG;
  if (e && (!rand3 || !tr || !ok || !ninl || e->ransac_iters < 1)) return VH_ERR_INVALID_ARG;
  if (mono && (!rand8 || !tr || !ok || !ninl || mono->ransac_iters < 1 || (int64_t)S * mono->ransac_iters > (int64_t)1 << 31)) return VH_ERR_INVALID_ARG;
  if (post_seq - 1 - age < 0) return VH_ERR_STATE;
  PostSlot &sl = post.slot[(post_seq - 1 - age) & 1];
  if (!sl.pending) return VH_ERR_STATE;
  if (e && sl.method != VH_METHOD_QUAD) return VH_ERR_STATE;       // the stereo estimator needs both cameras of both frames
  if (mono && sl.method == VH_METHOD_STEREO) return VH_ERR_STATE;  // the monocular one the left camera of both frames
  int64_t need = 0;
  { const int32_t rb = bucket_need(max_features, bw, bh, &need); if (rb) return rb; }  // (a bucket below one pixel is refused: the grid would not fit any index type)
  VH_HIP(hipEventSynchronize(sl.ev));
  sl.pending = false;
  for (int32_t s = 0; s < S; s++)
    if (sl.h_cnt[s] > sl.width || sl.h_cnt[S + s]) return VH_ERR_CAPACITY;  // a list longer than what was downloaded / a truncated feature set
  if (post.bcap < need) {
    for (void *old : {(void *)post.d_bucket, (void *)post.d_post_xyz}) dfree(old);  // (the superseded blocks: a caller raising max_features step by step must not pile them up)
    post.d_bucket = nullptr; post.d_post_xyz = nullptr;
    VH_HIP(post.h_bucket.alloc((size_t)S * need, hipHostMallocDefault));
    if (!post.h_bcnt) VH_HIP(post.h_bcnt.alloc((size_t)S, hipHostMallocDefault));
    int32_t rc;
    if ((rc = dmalloc((uint8_t **)&post.d_bucket, sizeof(vh_p_match) * (size_t)S * need, false))) return rc;
    if (!post.d_bcnt && (rc = dmalloc(&post.d_bcnt, (size_t)S, false))) return rc;
    if ((rc = dmalloc(&post.d_post_xyz, (size_t)S * need * 4, false))) return rc;
    if (!post.d_post_tr) { if ((rc = dmalloc(&post.d_post_tr, 6 * (size_t)S, false))) return rc; if ((rc = dmalloc(&post.d_post_ok, 2 * (size_t)S, false))) return rc; }
    post.bcap = (int32_t)need;
    post.post_mono_iters = 0;  // (the monocular scratch is sized by post.bcap as well)
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::atomic<int32_t> failed(0);
  const bool vote = votes_on(sl.method);  // stereo records carry no previous-frame position (as remove_outliers())
  const vh_vote_rule rule = rule_for(sl.method);
  for_each_stream(0, S, threads, [&](int32_t s) {
    thread_local std::vector<int32_t> scratch;
    vh_p_match *pm = sl.h_pm + (size_t)s * sl.cap_ps;
    int32_t n = sl.h_cnt[s];
    if (vote && vh_remove_outliers_pm_rule(pm, n, &rule, &n) != VH_OK) { failed = 1; return; }
    post.h_bcnt[s] = bucket_records(pm, n, max_features, bw, bh, post.h_bucket + (size_t)s * post.bcap, post.bcap, scratch);
  });
  if (host_ms) *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (failed) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < S; s++) if (post.h_bcnt[s] > post.bcap) return VH_ERR_CAPACITY;
  if (out_counts) for (int32_t s = 0; s < S; s++) out_counts[s] = post.h_bcnt[s];
  if (out) {
    for (int32_t s = 0; s < S; s++) {
      if (post.h_bcnt[s] > out_cap) return VH_ERR_CAPACITY;
      memcpy(out + (size_t)s * out_cap, post.h_bucket + (size_t)s * post.bcap, sizeof(vh_p_match) * (size_t)post.h_bcnt[s]);
    }
  }
  if (!e && !mono) return VH_OK;
  const size_t nr = e ? (size_t)S * e->ransac_iters * 3 : (size_t)S * mono->ransac_iters * 8;
  if (post.post_rand_n < nr) { int32_t rc = dmalloc(&post.d_post_rand, nr, false); if (rc) return rc; post.post_rand_n = nr; }
  if (mono && post.post_mono_iters < mono->ransac_iters) {
    int32_t rc = dmalloc(&post.d_post_mono, (size_t)vh_mono_scratch_bytes(S, post.bcap, mono->ransac_iters), false);
    if (rc) return rc;
    post.post_mono_iters = mono->ransac_iters;
  }
  // the bucketed lists go up as one block; everything on the download stream, beside the next step's kernels
  VH_HIP(hipMemcpyAsync(post.d_bucket, post.h_bucket, sizeof(vh_p_match) * (size_t)S * post.bcap, hipMemcpyHostToDevice, down_stream));
  VH_HIP(hipMemcpyAsync(post.d_bcnt, post.h_bcnt, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, down_stream));
  VH_HIP(hipMemcpyAsync(post.d_post_rand, e ? rand3 : rand8, sizeof(int32_t) * nr, hipMemcpyHostToDevice, down_stream));
  const VhLists bucketed = VhLists::slots(post.d_bucket, post.bcap, post.d_bcnt, post.bcap, S);
  if (e) vh_launch_ego(*e, bucketed, post.d_post_rand, post.d_post_xyz, post.bcap, post.d_post_tr, post.d_post_ok, post.d_post_ok + S, nullptr, 0, down_stream);
  else vh_launch_mono(*mono, bucketed, post.d_post_rand, post.d_post_mono, post.bcap, post.d_post_tr, post.d_post_ok, post.d_post_ok + S, nullptr, 0, nullptr, down_stream);
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(tr, post.d_post_tr, sizeof(double) * 6 * (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipMemcpyAsync(ok, post.d_post_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipMemcpyAsync(ninl, post.d_post_ok + S, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, down_stream));
  VH_HIP(hipStreamSynchronize(down_stream));
  static const bool timing = [] { const char *ev_ = getenv("VH_POST_TIMING"); return ev_ && ev_[0] == '1'; }();
  if (timing) fprintf(stderr, "post_finish: host %.2f ms, upload + ego + results %.2f ms\n",
                      host_ms ? *host_ms : -1.0, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - (host_ms ? *host_ms : 0.0));
  return VH_OK;
}

// ---- the steps after matching ON THE DEVICE ---------------------------------
// removeOutliers -> bucketFeatures -> estimateMotion without the host: kernels_vote.hip.  The triangulation
// under the vote is a sequential chain per list that takes tens of milliseconds as a GPU lane, so the
// throughput comes from lists in flight: post_begin_device() moves the step's S lists into the current
// BATCH (the matcher's buffer is free again at once); a batch of `vote_steps` steps is launched as one
// kernel sequence over vote_steps * S lists on one of a few low-priority streams (their own hardware
// queues: the long sweep kernel never stands in front of the matcher's kernels), and up to
// `vote_batches` batches are in flight.  post_finish_device(age) hands out the results of the step begun
// `age` begins ago, waiting for its batch if it has to -- a caller that stays vote_steps * (vote_batches - 1)
// steps ahead never waits.

int32_t Group::post_device_config(int32_t steps_per_batch, int32_t batches, int32_t lanes) {
  if (steps_per_batch < 1 || steps_per_batch > 256 || batches < 1 || batches > 64 || lanes < 1 || lanes > 64) return VH_ERR_INVALID_ARG;
  for (auto &b : vbatch) if (b.busy) return VH_ERR_STATE;  // steps begun whose results have not been handed out
  vote_release();
  vote_steps = steps_per_batch; vote_batches = batches; vote_lanes = lanes;
  return VH_OK;
}

// The dense stages of the batches (include/viso_hip.h: vh_group_post_device_dense).  A change of mode changes what a batch
// holds, so the ring is released and the next begin call sizes it again -- against the free memory, with the new mode's blocks.
int32_t Group::post_device_dense(int32_t mode) {
  if (mode < 0 || mode > 3) return VH_ERR_INVALID_ARG;
  for (auto &b : vbatch) if (b.busy) return VH_ERR_STATE;
  if (mode == vote_dense) return VH_OK;
  vote_release();
  vote_dense = mode;
  return VH_OK;
}

// The tail stages of the batches (include/viso_hip.h: vh_group_post_device_tail), under the rules of the dense mode: a
// change of the mask changes what a batch holds, so the ring is released and the next begin call sizes it again.
int32_t Group::post_device_tail(uint32_t stages) {
  for (auto &b : vbatch) if (b.busy) return VH_ERR_STATE;  // (the mask itself is judged by the ABI entry, before the handle)
  if (stages == vote_tail) return VH_OK;
  vote_release();
  vote_tail = stages;
  return VH_OK;
}

// The ring's shape in effect: the first begin call of a ring may have halved the configured steps per batch
int32_t Group::post_device_shape(int32_t *steps_per_batch, int32_t *batches) const {
  if (!steps_per_batch || !batches) return VH_ERR_INVALID_ARG;
  *steps_per_batch = vote_steps; *batches = vote_batches;
  return VH_OK;
}

// The tail block of batch b and its page-locked mirror, as vote_dense_alloc: before the batch's first launch; a refusal
// leaves the batch without one.
int32_t Group::vote_tail_alloc(VoteBatch &b, int32_t lists, uint32_t mask) {
  VoteTail &q = b.tl;
  const int32_t cap = b.vb.v.cap;
  // (the mirror too: a page-locked allocation that failed after the device block's must not pass for a finished one)
  if (q.block.p && q.lists >= lists && q.cap == cap && q.mask == mask && q.h_block.p && q.h_lists >= q.lists && q.h_mask == mask) return VH_OK;
  q.block = DeviceBlock(); q.bytes = 0; q.lists = 0; q.h = TailLists();
  if (alloc_refused()) return VH_ERR_HIP;
  const size_t total = VoteTail::bytes_for((size_t)lists, (size_t)cap, mask);
  VH_HIP(q.block.alloc(total));
  q.carve(q.block.p, (size_t)lists, (size_t)cap, mask);
  q.bytes = total; q.lists = lists; q.cap = cap; q.mask = mask;
  if (q.h_lists < lists || q.h_mask != mask) {
    q.h_lists = 0;
    Carver measure;
    TailLists().carve(measure, (size_t)lists, mask);
    VH_HIP(q.h_block.alloc(measure.bytes(), hipHostMallocDefault));
    q.h_lists = lists; q.h_mask = mask;
  }
  Carver c(q.h_block.p);
  q.h.carve(c, (size_t)q.h_lists, mask);
  return VH_OK;
}

// the compacted inlier lists of a batch's classification: what the refit and every tail stage read
static VhLists dense_lists(const VoteDense &q, const VhVote &v) { return VhLists::slots(q.d_out, v.cap, q.d_ninl, v.cap, v.P); }

// The tail stages of batch b, queued behind its dense stages (a: the classification's arguments as they stand, t: its test).
// Stereo: the covariance over the final inlier lists under the motion they belong to.  Mono: the model refitted on the
// inliers -> the classification again under it (a pointer switch, as mode 3) -> the pose over the final inlier lists
// under the model they were classified under, refined between its launches 1 and 2 -> the small downloads.  The kernels
// are the stateless entries' over the batch's fixed-stride slots; a list the gate closed has no records and ok = 0.
int32_t Group::vote_tail_launch(VoteBatch &b, const VhVote &v, const InlierTest &t, VhInlierArgs &a, hipStream_t vs) {
  VoteDense &q = b.dn;
  const VhLists inliers = dense_lists(q, v);
  VoteTail &tl = b.tl;
  const size_t P = (size_t)v.P;
  if (b.tail & VH_POST_TAIL_COV) {
    VhCovArgs c{};
    c.e = b.ego;
    c.lists = inliers;
    c.tr = b.dense_mode >= 2 ? q.d_tr_refit : b.d_tr; c.ok = b.dense_mode >= 2 ? q.d_ok_refit : q.d_ok;
    c.cov = tl.d.cov; c.ssr = tl.d.ssr; c.ok_out = tl.d.ok_cov;
    { Scope sc(this, "motion_cov", vs); vh_launch_motion_cov(c, vs); }
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(tl.h.cov, tl.d.cov, sizeof(double) * 36 * P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(tl.h.ssr, tl.d.ssr, sizeof(double) * P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(tl.h.ok_cov, tl.d.ok_cov, sizeof(int32_t) * P, hipMemcpyDeviceToHost, vs));
  }
  if (b.tail & VH_POST_TAIL_MONO_REFIT) {
    VhMonoRefitArgs r{};
    r.lists = inliers;
    r.model_in = q.d_model; r.ok_in = q.d_ok;
    r.model_out = tl.d.model; r.ok_out = tl.d.ok_model; r.w_out = tl.d.w;
    { Scope sc(this, "mono_refit", vs); vh_launch_mono_refit(r, vs); }
    VH_HIP(hipGetLastError());
    a.model = tl.d.model; a.ok = tl.d.ok_model;  // (the estimator's model stays where it is: vh_post_dense::model)
    launch_inliers(t, a, vs, this);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(tl.h.model, tl.d.model, sizeof(vh_mono_model) * P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(tl.h.w, tl.d.w, sizeof(double) * 2 * P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(tl.h.ok_model, tl.d.ok_model, sizeof(int32_t) * P, hipMemcpyDeviceToHost, vs));
  }
  if (b.tail & VH_POST_TAIL_MONO_POSE) {
    const bool refined = (b.tail & VH_POST_TAIL_MONO_REFINE) != 0;
    VhMonoPoseArgs m{};
    m.e = b.mono;
    m.lists = inliers;
    m.cap = v.cap; m.slot_stride = v.cap;
    m.model = a.model; m.ok_in = a.ok;
    m.hdr = tl.d_hdr; m.dist = tl.d_dist; m.d = tl.d_d; m.tr = tl.d.tr; m.ok = tl.d.ok_pose; m.pose = tl.d.pose;
    launch_mono_pose(m, refined, tl.d.refine, vs, this);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(tl.h.tr, tl.d.tr, sizeof(double) * 6 * P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(tl.h.ok_pose, tl.d.ok_pose, sizeof(int32_t) * P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(tl.h.pose, tl.d.pose, sizeof(vh_mono_pose) * P, hipMemcpyDeviceToHost, vs));
    if (refined) VH_HIP(hipMemcpyAsync(tl.h.refine, tl.d.refine, sizeof(vh_mono_refine) * P, hipMemcpyDeviceToHost, vs));
  }
  return VH_OK;
}

// The dense block of batch b for `lists` lists of the batch's record slots: allocated (or grown) before the batch's first
// launch; a refusal leaves the batch without one.
int32_t Group::vote_dense_alloc(VoteBatch &b, int32_t lists, bool model) {
  VoteDense &q = b.dn;
  const int32_t cap = b.vb.v.cap;
  if (q.block.p && q.lists >= lists && q.cap == cap && (q.with_model || !model)) return VH_OK;
  q.block = DeviceBlock(); q.bytes = 0; q.lists = 0;
  if (alloc_refused()) return VH_ERR_HIP;
  const size_t L = (size_t)lists, tiles = ((size_t)cap + VH_INLIER_TILE - 1) / VH_INLIER_TILE;
  const size_t total = VoteDense::bytes_for(L, (size_t)cap, model);
  VH_HIP(q.block.alloc(total));
  q.carve(q.block.p, L, (size_t)cap, model);
  q.bytes = total; q.lists = lists; q.cap = cap; q.tiles = (int32_t)tiles; q.with_model = model;
  if (q.h_lists < lists || (model && !q.h_with_model)) {
    q.h_lists = 0;
    VH_HIP(q.h_int.alloc(4 * L, hipHostMallocDefault));
    VH_HIP(q.h_tr.alloc(6 * L, hipHostMallocDefault));
    if (model) VH_HIP(q.h_model.alloc(L, hipHostMallocDefault));
    q.h_lists = lists; q.h_with_model = model;
  }
  return VH_OK;
}

// The dense stages of batch b, queued on its vote stream behind the estimator: gate -> flag -> scan + compact -> (mode >= 2)
// refit -> (mode 3) the classification again, the refit's tr / ok in the place of the estimator's -> the small downloads.
// The kernels are the stateless entries' (launch_inliers, vh_launch_refit) over the batch's fixed-stride slots.
int32_t Group::vote_dense_launch(VoteBatch &b, const VhVote &v, hipStream_t vs) {
  VoteDense &q = b.dn;
  {
    Scope sc(this, "post_dense_gate", vs);
    vh_launch_vote_gate(v, b.d_ok, q.d_cnt, q.d_ok, q.d_voted, vs);
  }
  VhInlierArgs a{};
  a.lists = VhLists::slots(v.pm, v.cap, q.d_cnt, v.cap, v.P);  // the voted lists, the gate's counts
  a.tiles_per_list = q.tiles;
  a.tr = b.has_mono ? nullptr : b.d_tr; a.model = b.has_mono ? q.d_model : nullptr; a.ok = q.d_ok; a.out_stride = v.cap;
  a.flags = q.d_flags; a.tile_cnt = q.d_tiles; a.n_inl = q.d_ninl; a.out = q.d_out; a.src_pos = q.d_src;
  const InlierTest t = b.has_mono ? InlierTest::monocular(&b.mono, nullptr) : InlierTest::stereo(&b.ego, nullptr);
  launch_inliers(t, a, vs, this);
  VH_HIP(hipGetLastError());
  const size_t P = (size_t)v.P, L = (size_t)q.h_lists;
  if (b.dense_mode >= 2) {
    VhRefitArgs r{};
    r.e = b.ego;
    r.lists = dense_lists(q, v);
    r.tr_in = b.d_tr; r.ok_in = q.d_ok;
    r.tr_out = q.d_tr_refit; r.ok_out = q.d_ok_refit; r.n_updates = q.d_nupd;
    { Scope sc(this, "motion_refit", vs); vh_launch_refit(r, vs); }
    VH_HIP(hipGetLastError());
    if (b.dense_mode == 3) {  // (a pointer switch: the refit's results stay where they are)
      a.tr = q.d_tr_refit; a.ok = q.d_ok_refit;
      launch_inliers(t, a, vs, this);
      VH_HIP(hipGetLastError());
    }
    VH_HIP(hipMemcpyAsync(q.h_int + 2 * L, q.d_ok_refit, sizeof(int32_t) * P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(q.h_int + 3 * L, q.d_nupd, sizeof(int32_t) * P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(q.h_tr, q.d_tr_refit, sizeof(double) * 6 * P, hipMemcpyDeviceToHost, vs));
  }
  if (b.tail) { const int32_t rc = vote_tail_launch(b, v, t, a, vs); if (rc) return rc; }  // (before the counts come down: the mono refit classifies again)
  VH_HIP(hipMemcpyAsync(q.h_int, q.d_voted, sizeof(int32_t) * P, hipMemcpyDeviceToHost, vs));
  VH_HIP(hipMemcpyAsync(q.h_int + L, q.d_ninl, sizeof(int32_t) * P, hipMemcpyDeviceToHost, vs));
  if (b.has_mono) VH_HIP(hipMemcpyAsync(q.h_model, q.d_model, sizeof(vh_mono_model) * P, hipMemcpyDeviceToHost, vs));
  return VH_OK;
}

// bucket grid of Matcher::bucketFeatures on this group's images: floor(u_max / bw) + 1 columns, floor(v_max / bh) + 1 rows (matcher.cpp:150-151)
int32_t Group::bucket_need(int32_t max_features, float bw, float bh, int64_t *need, int64_t *grid) const {
  if (max_features < 1 || !(bw >= 1) || !(bh >= 1)) return VH_ERR_INVALID_ARG;
  const int64_t cols = (int64_t)floorf((float)(dims[0] - 1) / bw) + 1, rows = (int64_t)floorf((float)(dims[1] - 1) / bh) + 1;
  if (cols * rows > (1 << 20)) return VH_ERR_UNSUPPORTED;
  *need = std::min<int64_t>(cols * rows * max_features, mcap);
  if (grid) *grid = cols * rows;
  return VH_OK;
}

void Group::vote_run(const VhVote &v, int32_t method, int32_t lanes, int32_t max_features, float bw, float bh, const VhVoteBuffers &vb, hipStream_t st) {
  const vh_vote_rule r = rule_for(method);
  const VhVoteRule rule = VhVoteRule::of(&r);
  Event e0, e1;
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool timed = prof && e0.create(hipEventDefault) == hipSuccess && e1.create(hipEventDefault) == hipSuccess;
  if (timed) { ev[0] = e0; ev[1] = e1; }
  vh_launch_vote(v, rule, lanes, max_features, bw, bh, vb.lfsr, vb.lfsr_n, vb.out, vb.out_cap, vb.out_count, nullptr, timed ? ev : nullptr, st);
  static const char *const names[4] = {"vote_tally", "vote_tally_flow", "vote_tally_disp", "vote_tally_quad"};
  if (timed) prof_entries[names[rule.test]].pending.emplace_back(std::move(e0), std::move(e1));
}

int32_t Group::vote_launch(VoteBatch &b, int32_t index) {
  if (b.launched || b.steps == 0) return VH_OK;
  hipStream_t vs = vote_stream[index % kVoteStreams];
  VhVote v = b.vb.v;
  v.P = b.steps * S;
  VH_HIP(hipStreamWaitEvent(vs, b.ev_prep, 0));
  vote_run(v, b.method, vote_lanes, b.max_features, b.bw, b.bh, b.vb, vs);
  VH_HIP(hipGetLastError());
  const VhLists voted = VhLists::slots(b.vb.out, b.vb.out_cap, b.vb.out_count, b.vb.out_cap, v.P);
  if (b.has_ego) vh_launch_ego(b.ego, voted, b.d_rand, b.d_xyz, b.vb.out_cap, b.d_tr, b.d_ok, b.d_ok + v.P, nullptr, 0, vs);
  else if (b.has_mono) vh_launch_mono(b.mono, voted, b.d_rand, b.d_mono, b.vb.out_cap, b.d_tr, b.d_ok, b.d_ok + v.P, nullptr, 0,
                                       b.dense_mode ? b.dn.d_model : nullptr, vs);
  VH_HIP(hipGetLastError());
  if (b.dense_mode) { const int32_t rc = vote_dense_launch(b, v, vs); if (rc) return rc; }
  if (b.has_ego || b.has_mono) {
    VH_HIP(hipMemcpyAsync(b.h_tr, b.d_tr, sizeof(double) * 6 * (size_t)v.P, hipMemcpyDeviceToHost, vs));
    VH_HIP(hipMemcpyAsync(b.h_ok, b.d_ok, sizeof(int32_t) * 2 * (size_t)v.P, hipMemcpyDeviceToHost, vs));
  }
  VH_HIP(hipMemcpyAsync(b.h_cnt, b.vb.out_count, sizeof(int32_t) * (size_t)v.P, hipMemcpyDeviceToHost, vs));
  VH_HIP(hipMemcpyAsync(b.h_meta, b.vb.v.meta, sizeof(VhVoteMeta) * (size_t)v.P, hipMemcpyDeviceToHost, vs));
  if (b.want_lists) VH_HIP(hipMemcpyAsync(b.h_out, b.vb.out, sizeof(vh_p_match) * (size_t)v.P * b.vb.out_cap, hipMemcpyDeviceToHost, vs));
  VH_HIP(hipEventRecord(b.ev_done, vs));
  static const bool serial_vote = [] { const char *ev = getenv("VH_VOTE_SERIAL"); return ev && ev[0] == '1'; }();
  if (serial_vote) VH_HIP(hipStreamWaitEvent(stream, b.ev_done, 0));  // experiment: the matcher's next step waits for this batch
  b.launched = true;
  return VH_OK;
}

int32_t Group::post_begin_device(int32_t cap_ps, int32_t max_features, float bw, float bh, const vh_ego_params *e, const int32_t *rand3,
                          const vh_mono_params *mono, const int32_t *rand8, int32_t want_lists) {
  if (cap_ps < 1 || (e && mono)) return VH_ERR_INVALID_ARG;
  if (e && (!rand3 || e->ransac_iters < 1)) return VH_ERR_INVALID_ARG;
  if (mono && (!rand8 || mono->ransac_iters < 1 || (int64_t)S * vote_steps * mono->ransac_iters > (int64_t)1 << 31)) return VH_ERR_INVALID_ARG;
  if (vote_dense >= 1 && !e && !mono) return VH_ERR_INVALID_ARG;  // the dense stages classify under the batch's motion
  if (vote_dense >= 2 && mono) return VH_ERR_INVALID_ARG;         // (the reference has no mono refit)
  if (vote_tail && vote_dense < 1) return VH_ERR_INVALID_ARG;                         // the tail stages read the dense stages' inlier lists
  if ((vote_tail & VH_POST_TAIL_COV) && !e) return VH_ERR_INVALID_ARG;                // the covariance is the stereo motion's
  if ((vote_tail & ~(uint32_t)VH_POST_TAIL_COV) && !mono) return VH_ERR_INVALID_ARG;  // refit and pose the mono model's
  if ((int64_t)S * vote_steps > 65535) return VH_ERR_UNSUPPORTED;  // (the tally and the monocular kernels put the list on grid.y: fewer steps per batch)
  if (!allocated || last_method < 0) return VH_ERR_STATE;
  if (e && last_method != VH_METHOD_QUAD) return VH_ERR_STATE;        // the stereo estimator needs both cameras of both frames
  if (mono && last_method == VH_METHOD_STEREO) return VH_ERR_STATE;   // the monocular one the left camera of both frames
  int64_t need = 0, grid = 0;
  int32_t rc = bucket_need(max_features, bw, bh, &need, &grid);
  if (rc) return rc;
  cap_ps = std::min(cap_ps, mcap);
  if (cap_ps > VH_VOTE_LIST_MAX) return VH_ERR_UNSUPPORTED;  // (16-bit hull links; the sweep's angular hash has VH_VOTE_HASH_MAX slots in LDS)
  if (vbatch.empty()) {
    // The ring is allocated batch by batch on first use: it must fit the device NOW, or a later begin call -- with steps
    // already moved -- fails in hipMalloc.  Steps per batch are halved until vote_batches batches fit 80 % of the free
    // memory; if a single step per batch does not fit, nothing has moved yet and the caller is told so.
    size_t free_b = 0, total_b = 0;
    VH_HIP(hipMemGetInfo(&free_b, &total_b));
    const auto ring_bytes = [&](int32_t steps) {
      const int32_t P = steps * S;
      const size_t post = (e ? sizeof(double) * 4 * (size_t)P * (size_t)need : 0) + (mono ? (size_t)vh_mono_scratch_bytes(P, (int32_t)need, mono->ransac_iters) : 0) +
                          sizeof(double) * 6 * (size_t)P + sizeof(int32_t) * 2 * (size_t)P +
                          sizeof(int32_t) * (size_t)steps * (e ? (size_t)S * e->ransac_iters * 3 : (mono ? (size_t)S * mono->ransac_iters * 8 : 0)) +
                          (vote_dense ? VoteDense::bytes_for((size_t)P, (size_t)std::max(cap_ps, 4), mono != nullptr) : 0) +
                          (vote_tail ? VoteTail::bytes_for((size_t)P, (size_t)std::max(cap_ps, 4), vote_tail) : 0);
      return (double)vote_batches * (double)(VhVoteBuffers::bytes_for(P, cap_ps, (int32_t)need, (int32_t)grid) + post);
    };
    int32_t steps = vote_steps;
    while (steps > 1 && ring_bytes(steps) > 0.8 * (double)free_b) steps = (steps + 1) / 2;
    if (ring_bytes(steps) > 0.8 * (double)free_b) {
      t_last_error = "the post stage's ring of batches does not fit the device's free memory even at one step per batch";
      return VH_ERR_CAPACITY;
    }
    vote_steps = steps;
    vbatch.resize((size_t)vote_batches);
    vstep.assign((size_t)vote_steps * vote_batches, VoteStep{});
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    static const int prio_env = [] { const char *ev = getenv("VH_VOTE_STREAM_PRIO"); return ev ? atoi(ev) : 1; }();  // 1: lowest, 0: normal, -1: highest
    const int prio = prio_env > 0 ? prio_lo : (prio_env < 0 ? prio_hi : 0);
    for (int k = 0; k < kVoteStreams; k++)
      if (!vote_stream[k]) VH_HIP(vote_stream[k].create(prio));
    for (auto &b : vbatch) { VH_HIP(b.ev_prep.create()); VH_HIP(b.ev_done.create()); }
  }
  VoteBatch *b = &vbatch[(size_t)vote_cur];
  const size_t rand_per_step = e ? (size_t)S * e->ransac_iters * 3 : (mono ? (size_t)S * mono->ransac_iters * 8 : 0);
  const auto same = [&](const VoteBatch &q) {
    return q.method == last_method && q.rule == vote_rule && q.max_features == max_features && q.bw == bw && q.bh == bh && q.has_ego == (e != nullptr) &&
           q.has_mono == (mono != nullptr) && (!e || memcmp(&q.ego, e, sizeof(*e)) == 0) && (!mono || memcmp(&q.mono, mono, sizeof(*mono)) == 0) &&
           q.vb.v.cap >= cap_ps && q.want_lists == (want_lists != 0) && q.dense_mode == vote_dense && q.tail == vote_tail;
  };
  if (b->steps > 0 && (b->launched || b->steps >= vote_steps || !same(*b))) {  // the batch is closed (full, flushed, or configured differently): next one
    if ((rc = vote_launch(*b, vote_cur))) return rc;
    const int32_t next = (vote_cur + 1) % vote_batches;
    // the ring has come round: the next batch's results must have been handed out (checked before anything moves, so
    // that the caller can finish those steps and begin this one again)
    if (vbatch[(size_t)next].launched && vbatch[(size_t)next].busy && vbatch[(size_t)next].handed < vbatch[(size_t)next].steps) return VH_ERR_STATE;
    vote_cur = next;
    b = &vbatch[(size_t)vote_cur];
  }
  if (b->steps == 0 || b->launched) {  // start the batch
    if (b->launched) {  // a batch of the previous round: its kernels must be done
      if (b->busy && b->handed < b->steps) return VH_ERR_STATE;
      VH_HIP(hipEventSynchronize(b->ev_done));
    }
    b->steps = 0; b->launched = false; b->busy = false; b->handed = 0;
    const int32_t P = vote_steps * S;
    // (the classification's launch grid: lists x tiles of the slots the batch will have)
    if (vote_dense && !inlier_grid_ok(P, (std::max(b->vb.v.cap, cap_ps) + VH_INLIER_TILE - 1) / VH_INLIER_TILE)) return VH_ERR_UNSUPPORTED;
    if ((vote_tail & VH_POST_TAIL_MONO_POSE) && !mono_pose_grid_ok(P, std::max(b->vb.v.cap, cap_ps))) return VH_ERR_UNSUPPORTED;  // (the pose's per-record launches.  Not reachable today: the tail needs a dense mode, and the line above refuses at 2^24 tiles of 1 024 records, long before lists * ceil(cap / 64) reaches 2^30; it stands for the day that limit moves)
    if (b->vb.v.cap < cap_ps || b->vb.out_cap < need || b->vb.v.P < P || b->vb.v.nb_max < grid) {
      if (b->vb.block) {  // a batch grows (longer lists than the ring was sized for): only if the difference fits
        size_t free_b = 0, total_b = 0;
        VH_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t want = VhVoteBuffers::bytes_for(P, cap_ps, (int32_t)need, (int32_t)grid);
        if (want > b->vb.bytes && want - b->vb.bytes > free_b) { t_last_error = "the post stage's batch cannot grow: device memory exhausted"; return VH_ERR_CAPACITY; }
      }
      b->vb.release();
      VH_HIP(b->vb.alloc(P, cap_ps, (int32_t)need, (int32_t)grid));
      VH_HIP(b->vb.upload_lfsr());
    }
    const int32_t ocap = b->vb.out_cap;
    const auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t b_rand = up(sizeof(int32_t) * rand_per_step * vote_steps), b_xyz = up(e ? sizeof(double) * 4 * (size_t)P * ocap : 0), b_tr = up(sizeof(double) * 6 * (size_t)P),
                 b_ok = up(sizeof(int32_t) * 2 * (size_t)P), b_mono = mono ? (size_t)vh_mono_scratch_bytes(P, ocap, mono->ransac_iters) : 0;
    if (b->block_bytes < b_rand + b_xyz + b_tr + b_ok + b_mono || b->rand_per_step != rand_per_step) {
      b->block_bytes = 0;
      VH_HIP(b->block.alloc(b_rand + b_xyz + b_tr + b_ok + b_mono + 256));
      b->block_bytes = b_rand + b_xyz + b_tr + b_ok + b_mono;
    }
    uint8_t *blk = b->block.as<uint8_t>();
    b->d_rand = (int32_t *)blk; b->d_xyz = (double *)(blk + b_rand); b->d_tr = (double *)(blk + b_rand + b_xyz);
    b->d_ok = (int32_t *)(blk + b_rand + b_xyz + b_tr); b->d_mono = blk + b_rand + b_xyz + b_tr + b_ok;
    b->rand_per_step = rand_per_step;
    if (b->h_rand_ints < rand_per_step * (size_t)vote_steps) {
      b->h_rand_ints = 0;
      VH_HIP(b->h_rand.alloc(rand_per_step * (size_t)vote_steps, hipHostMallocDefault));
      b->h_rand_ints = rand_per_step * (size_t)vote_steps;
    }
    if (b->h_lists < P) {
      b->h_lists = 0;
      VH_HIP(b->h_tr.alloc(6 * (size_t)P, hipHostMallocDefault));
      VH_HIP(b->h_ok.alloc(2 * (size_t)P, hipHostMallocDefault));
      VH_HIP(b->h_cnt.alloc((size_t)P, hipHostMallocDefault));
      VH_HIP(b->h_meta.alloc((size_t)P, hipHostMallocDefault));
      b->h_lists = P;
    }
    if (want_lists && (!b->h_out || b->h_out_cap < ocap)) {
      VH_HIP(b->h_out.alloc((size_t)P * ocap, hipHostMallocDefault));
      b->h_out_cap = ocap;
    }
    b->method = last_method; b->rule = vote_rule; b->max_features = max_features; b->bw = bw; b->bh = bh; b->has_ego = e != nullptr; b->has_mono = mono != nullptr;
    if (e) b->ego = *e;
    if (mono) b->mono = *mono;
    b->want_lists = want_lists != 0;
    b->dense_mode = 0;  // (until its block exists: a refused allocation leaves a batch that launches nothing of it)
    if (vote_dense && (rc = vote_dense_alloc(*b, P, mono != nullptr))) return rc;
    b->dense_mode = vote_dense;
    b->tail = 0;
    if (vote_tail && (rc = vote_tail_alloc(*b, P, vote_tail))) return rc;
    b->tail = vote_tail;
  }
  // the step's lists leave the matcher's buffer behind the emission that wrote them; the next emission waits for that (ev_down)
  VH_HIP(hipStreamWaitEvent(down_stream, ev_post[last_buf], 0));
  vh_launch_vote_prep(b->vb.v, b->steps * S, S, (const vh_p_match *)mt.d_matches, mcap, mt.d_match_count, mcap, mt.d_overflow, votes_on(last_method) ? 1 : 0, down_stream);
  VH_HIP(hipGetLastError());
  if (rand_per_step) {
    // through the batch's page-locked slot of this step: an asynchronous copy from the caller's pageable array would
    // make the host wait until the stream reaches it (behind the step's emission), and the array is only borrowed
    int32_t *hr = b->h_rand + rand_per_step * (size_t)b->steps;
    memcpy(hr, e ? rand3 : rand8, sizeof(int32_t) * rand_per_step);
    VH_HIP(hipMemcpyAsync(b->d_rand + rand_per_step * (size_t)b->steps, hr, sizeof(int32_t) * rand_per_step, hipMemcpyHostToDevice, down_stream));
  }
  VH_HIP(hipEventRecord(b->ev_prep, down_stream));
  VH_HIP(hipEventRecord(ev_down, down_stream)); mt.ev_down_valid = true;
  VoteStep &st = vstep[(size_t)(post_dev_seq % (int64_t)vstep.size())];
  st.batch = vote_cur; st.pos = b->steps; st.open = true;
  b->steps++; b->busy = true;
  post_dev_seq++;
  if (b->steps >= vote_steps) return vote_launch(*b, vote_cur);
  return VH_OK;
}

// The members of *t that the caller's t->size covers (include/viso_hip.h: vh_post_tail), the others null
static int32_t tail_outputs(const vh_post_tail *t, vh_post_tail &o) {
  memset(&o, 0, sizeof(o));
  if (!t) return VH_OK;
  if (t->size < 8 || (t->size - 8) % 8) return VH_ERR_INVALID_ARG;
  memcpy(&o, t, std::min<size_t>(t->size, sizeof(o)));
  return VH_OK;
}

// (d, t, nullable: the dense and the tail stages' outputs, include/viso_hip.h: vh_post_dense, vh_post_tail)
int32_t Group::post_finish_device(int32_t age, double *tr, int32_t *ok, int32_t *ninl, vh_p_match *out, int32_t out_cap, int32_t *out_counts,
                                  const vh_post_dense *d, const vh_post_tail *t_in) {
  vh_post_tail t;
  { const int32_t rt = tail_outputs(t_in, t); if (rt) return rt; }
  const bool d_records = d && (d->voted_pm || d->flags || d->inlier_pm || d->src_pos);
  if (age < 0 || ((out || d_records) && out_cap < 1)) return VH_ERR_INVALID_ARG;
  if (vstep.empty() || post_dev_seq - 1 - age < 0 || age >= (int64_t)vstep.size()) return VH_ERR_STATE;
  VoteStep &st = vstep[(size_t)((post_dev_seq - 1 - age) % (int64_t)vstep.size())];
  if (!st.open) return VH_ERR_STATE;
  VoteBatch &b = vbatch[(size_t)st.batch];
  if (d) {  // an output the step's mode did not produce: refused before anything happens to the step
    const bool any = d->voted_counts || d->inlier_counts || d->tr_refit || d->ok_refit || d->n_updates || d->model || d_records;
    if (any && b.dense_mode < 1) return VH_ERR_STATE;
    if ((d->tr_refit || d->ok_refit || d->n_updates) && b.dense_mode < 2) return VH_ERR_STATE;
    if (d->model && !b.has_mono) return VH_ERR_STATE;
  }
  // (the same for the tail's outputs and the step's mask)
  if (((t.cov || t.ssr || t.ok_cov) && !(b.tail & VH_POST_TAIL_COV)) || ((t.model_refit || t.ok_model || t.w) && !(b.tail & VH_POST_TAIL_MONO_REFIT)) ||
      ((t.tr_pose || t.ok_pose || t.pose) && !(b.tail & VH_POST_TAIL_MONO_POSE)) || (t.refine && !(b.tail & VH_POST_TAIL_MONO_REFINE)))
    return VH_ERR_STATE;
  int32_t rc = vote_launch(b, st.batch);  // (a batch that is not full yet is closed and launched now)
  if (rc) return rc;
  VH_HIP(hipEventSynchronize(b.ev_done));
  st.open = false;
  b.handed++;
  if (b.handed >= b.steps) b.busy = false;
  const size_t p0 = (size_t)st.pos * S, P = (size_t)b.steps * S;
  if ((b.has_ego || b.has_mono) && (!tr || !ok || !ninl)) return VH_ERR_INVALID_ARG;
  if (out && !b.want_lists) return VH_ERR_STATE;
  if (b.has_ego || b.has_mono) {
    memcpy(tr, b.h_tr + 6 * p0, sizeof(double) * 6 * (size_t)S);
    memcpy(ok, b.h_ok + p0, sizeof(int32_t) * (size_t)S);
    memcpy(ninl, b.h_ok + P + p0, sizeof(int32_t) * (size_t)S);
  }
  if (out_counts) memcpy(out_counts, b.h_cnt + p0, sizeof(int32_t) * (size_t)S);
  // One refused list does not void the step: the healthy streams are delivered, a refused stream reports
  // ok = 0, n_inliers = 0, tr = 0, counts = -1, and the call returns the error (capacity before unsupported).
  int32_t ret = VH_OK;
  for (int32_t s = 0; s < S; s++) {
    const VhVoteMeta &m = b.h_meta[p0 + s];
    const bool bad = m.status != VH_VOTE_OK && m.status != VH_VOTE_SKIP;
    if (m.status == VH_VOTE_TRUNCATED) ret = VH_ERR_CAPACITY;
    else if (bad && ret == VH_OK) ret = VH_ERR_UNSUPPORTED;
    if (bad) {
      if (b.has_ego || b.has_mono) { for (int k = 0; k < 6; k++) tr[6 * (size_t)s + k] = 0.0; ok[s] = 0; ninl[s] = 0; }
      if (out_counts) out_counts[s] = -1;
      continue;
    }
    if (out) {
      const int32_t k = b.h_cnt[p0 + s];
      if (k > out_cap) { ret = VH_ERR_CAPACITY; if (out_counts) out_counts[s] = -1; continue; }
      memcpy(out + (size_t)s * out_cap, b.h_out + (p0 + s) * (size_t)b.vb.out_cap, sizeof(vh_p_match) * (size_t)k);
    }
  }
  // The tail stages' outputs: everything came down with the batch.  A refused stream's are the zero records.
  for (int32_t s = 0; s < S && b.tail; s++) {
    const size_t p = p0 + (size_t)s;
    const VhVoteMeta &m = b.h_meta[p];
    const bool bad = m.status != VH_VOTE_OK && m.status != VH_VOTE_SKIP;
    const TailLists &h = b.tl.h;
    const auto give = [&](auto *dst, const auto *src, size_t n) {
      if (!dst) return;
      if (bad) memset(dst + n * (size_t)s, 0, sizeof(*dst) * n); else memcpy(dst + n * (size_t)s, src + n * p, sizeof(*dst) * n);
    };
    give(t.cov, h.cov, 36); give(t.ssr, h.ssr, 1); give(t.ok_cov, h.ok_cov, 1);
    give(t.model_refit, h.model, 1); give(t.ok_model, h.ok_model, 1); give(t.w, h.w, 2);
    give(t.tr_pose, h.tr, 6); give(t.ok_pose, h.ok_pose, 1); give(t.pose, h.pose, 1); give(t.refine, h.refine, 1);
  }
  if (!d || b.dense_mode < 1) return ret;
  // The dense stages' outputs.  The small ones came down with the batch; the records of this step's lists are copied out
  // of the batch's buffers now (they stay as they are until the ring comes round to the batch).
  const VoteDense &q = b.dn;
  const size_t L = (size_t)q.h_lists, cap = (size_t)b.vb.v.cap;
  for (int32_t s = 0; s < S; s++) {
    const size_t p = p0 + (size_t)s;
    const int32_t voted = q.h_int[p];  // (-1: the gate's mark of a refused list)
    const bool bad = voted < 0;
    int32_t n_in = bad ? -1 : q.h_int[L + p], n_voted = voted;
    if (!bad && (((d->voted_pm || d->flags) && voted > out_cap) || ((d->inlier_pm || d->src_pos) && n_in > out_cap))) {
      ret = VH_ERR_CAPACITY;
      n_in = n_voted = -1;
    }
    if (d->voted_counts) d->voted_counts[s] = n_voted;
    if (d->inlier_counts) d->inlier_counts[s] = n_in;
    const bool refit = b.dense_mode >= 2 && !bad;
    if (d->ok_refit) d->ok_refit[s] = refit ? q.h_int[2 * L + p] : 0;
    if (d->n_updates) d->n_updates[s] = refit ? q.h_int[3 * L + p] : 0;
    if (d->tr_refit) for (int k = 0; k < 6; k++) d->tr_refit[6 * (size_t)s + k] = refit ? q.h_tr[6 * p + k] : 0.0;
    if (d->model) { if (bad) memset(d->model + s, 0, sizeof(vh_mono_model)); else d->model[s] = q.h_model[p]; }
    if (n_voted > 0) {
      if (d->voted_pm) VH_HIP(hipMemcpy(d->voted_pm + (size_t)s * out_cap, b.vb.v.pm + p * cap, sizeof(vh_p_match) * (size_t)n_voted, hipMemcpyDeviceToHost));
      if (d->flags) VH_HIP(hipMemcpy(d->flags + (size_t)s * out_cap, q.d_flags + p * cap, (size_t)n_voted, hipMemcpyDeviceToHost));
    }
    if (n_in > 0) {
      if (d->inlier_pm) VH_HIP(hipMemcpy(d->inlier_pm + (size_t)s * out_cap, q.d_out + p * cap, sizeof(vh_p_match) * (size_t)n_in, hipMemcpyDeviceToHost));
      if (d->src_pos) VH_HIP(hipMemcpy(d->src_pos + (size_t)s * out_cap, q.d_src + p * cap, sizeof(int32_t) * (size_t)n_in, hipMemcpyDeviceToHost));
    }
  }
  return ret;
}

uint32_t lfsr_next(uint32_t x) { return vh_lfsr_next(x); }  // (vh_vote.h: shared with the device form of the shuffle)

// Matcher::bucketFeatures (matcher.cpp:140-187) without the fixed
// buckets[126][256] capacity.
void bucket_host(std::vector<vh_p_match> &pm, int32_t max_features, float bw, float bh) {
  float u_max = 0, v_max = 0;
  for (auto &m : pm) { if (m.u1c > u_max) u_max = m.u1c; if (m.v1c > v_max) v_max = m.v1c; }
  const int32_t cols = (int32_t)floorf(u_max / bw) + 1, rows = (int32_t)floorf(v_max / bh) + 1;
  std::vector<std::vector<vh_p_match>> buckets((size_t)cols * rows);
  for (auto &m : pm) {
    const int32_t u = (int32_t)floorf(m.u1c / bw), v = (int32_t)floorf(m.v1c / bh);
    buckets[(size_t)v * cols + u].push_back(m);
  }
  pm.clear();
  uint32_t rnd = 5;
  for (auto &b : buckets) {
    const int32_t len = (int32_t)b.size();
    for (int32_t i = 1; i < len; i++) {  // random_shuffle, matcher.cpp:126-138
      const int32_t j = (int32_t)(rnd % (uint32_t)(i + 1));
      rnd = lfsr_next(rnd);
      std::swap(b[i], b[j]);
    }
    for (int32_t j = 0, k = 0; j < len; j++) { pm.push_back(b[j]); if (++k >= max_features) break; }
  }
}

int32_t bucket_records(const vh_p_match *pm, int32_t n, int32_t max_features, float bw, float bh, vh_p_match *out, int32_t out_cap,
                       std::vector<int32_t> &work) {
  float u_max = 0, v_max = 0;
  for (int32_t i = 0; i < n; i++) { if (pm[i].u1c > u_max) u_max = pm[i].u1c; if (pm[i].v1c > v_max) v_max = pm[i].v1c; }
  const int32_t cols = (int32_t)floorf(u_max / bw) + 1, rows = (int32_t)floorf(v_max / bh) + 1, nb = cols * rows;
  // counting sort of the record indices by bucket (row-major), stable: the reference appends in list order
  work.assign((size_t)nb + 1 + (size_t)n, 0);
  int32_t *start = work.data(), *idx = work.data() + nb + 1;
  const auto bucket_of = [&](const vh_p_match &m) { return (int32_t)floorf(m.v1c / bh) * cols + (int32_t)floorf(m.u1c / bw); };
  for (int32_t i = 0; i < n; i++) start[bucket_of(pm[i]) + 1]++;
  for (int32_t b = 0; b < nb; b++) start[b + 1] += start[b];
  {
    std::vector<int32_t> cur(start, start + nb);
    for (int32_t i = 0; i < n; i++) idx[cur[bucket_of(pm[i])]++] = i;
  }
  uint32_t rnd = 5;
  int32_t kept = 0;
  for (int32_t b = 0; b < nb; b++) {
    int32_t *v = idx + start[b];
    const int32_t len = start[b + 1] - start[b];
    for (int32_t i = 1; i < len; i++) {  // random_shuffle, matcher.cpp:126-138
      const int32_t j = (int32_t)(rnd % (uint32_t)(i + 1));
      rnd = lfsr_next(rnd);
      std::swap(v[i], v[j]);
    }
    for (int32_t j = 0, k = 0; j < len; j++) { if (kept < out_cap) out[kept] = pm[v[j]]; kept++; if (++k >= max_features) break; }
  }
  return kept;
}

int32_t prior_statistics(const vh_params &p, const int32_t dims[3], int32_t method, const vh_p_match *pm, int32_t n, float *ranges) {
  const float bs = (float)p.match_binsize, R = (float)p.match_radius;
  const int32_t ubn = (int32_t)ceilf((float)dims[0] / bs), vbn = (int32_t)ceilf((float)dims[1] / bs);  // matcher.cpp:282-283
  const int32_t nst = method == VH_METHOD_QUAD ? 4 : 2;
  const size_t nb = (size_t)ubn * vbn;
  std::vector<uint8_t> seen(nb, 0);
  for (size_t k = 0; k < nb * 16; k++) ranges[k] = (k & 1) ? R : -R;
  for (int32_t i = 0; i < n; i++) {
    const vh_p_match &m = pm[i];
    float d[8] = {0, 0, 0, 0, 0, 0, 0, 0}, u, v;
    if (method == VH_METHOD_FLOW) {
      d[0] = m.u1p - m.u1c; d[1] = m.v1p - m.v1c; d[2] = m.u1c - m.u1p; d[3] = m.v1c - m.v1p;
      u = m.u1c; v = m.v1c;
    } else if (method == VH_METHOD_STEREO) {
      d[0] = m.u2c - m.u1c; d[2] = m.u1c - m.u2c;
      u = m.u1c; v = m.v1c;
    } else {
      d[0] = m.u2p - m.u1p; d[2] = m.u2c - m.u2p; d[3] = m.v2c - m.v2p; d[4] = m.u1c - m.u2c; d[6] = m.u1p - m.u1c; d[7] = m.v1p - m.v1c;
      u = m.u1p; v = m.v1p;
    }
    bool finite = std::isfinite(u) && std::isfinite(v);
    for (int32_t k = 0; k < 2 * nst; k++) finite = finite && std::isfinite(d[k]);
    if (!finite) return VH_ERR_INVALID_ARG;
    // the bin of the reference point, kept in float until it is inside [-1, bin count] (any finite coordinate)
    const int32_t ub = (int32_t)std::min(std::max(floorf(u / bs), -1.0f), (float)ubn);
    const int32_t vb = (int32_t)std::min(std::max(floorf(v / bs), -1.0f), (float)vbn);
    const auto clampi = [](int32_t x, int32_t nbin) { return std::min(std::max(x, 0), nbin - 1); };
    for (int32_t y = clampi(vb - 1, vbn); y <= clampi(vb + 1, vbn); y++)
      for (int32_t x = clampi(ub - 1, ubn); x <= clampi(ub + 1, ubn); x++) {
        const size_t b = (size_t)y * ubn + x;
        float *r = ranges + b * 16;
        for (int32_t st = 0; st < nst; st++)
          for (int32_t ax = 0; ax < 2; ax++) {
            float &lo = r[4 * st + 2 * ax], &hi = r[4 * st + 2 * ax + 1];
            const float x_ = d[2 * st + ax];
            if (!seen[b]) { lo = x_; hi = x_; }
            else { lo = std::min(lo, x_); hi = std::max(hi, x_); }
          }
        seen[b] = 1;
      }
  }
  for (size_t b = 0; b < nb; b++) {
    if (!seen[b]) continue;  // no observation: +-radius, not widened
    for (int32_t st = 0; st < nst; st++)
      for (int32_t ax = 0; ax < 2; ax++) {
        float &lo = ranges[b * 16 + 4 * st + 2 * ax], &hi = ranges[b * 16 + 4 * st + 2 * ax + 1];
        const float dd = hi - lo;
        if (dd < 20.0f) { const float h = ceilf((20.0f - dd) / 2.0f); lo -= h; hi += h; }
      }
  }
  return VH_OK;
}

}  // namespace vh_engine
