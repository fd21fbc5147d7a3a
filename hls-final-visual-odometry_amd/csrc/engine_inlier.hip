// engine_inlier.hip -- motion inliers: VisualOdometryStereo::getInlier on whole lists under a caller-given motion and
// VisualOdometryMono::getInlier under a caller-given epipolar model (kernels_inlier.hip), on the device-resident lists
// of a handle and on caller-owned lists; the stereo motion refined on such lists (kernels_refit.hip: the handle's
// compacted inlier lists, or caller-owned lists); and their part of the ABI.
#include "engine.h"
#include <optional>

namespace vh_engine {

// The flag pass of either test, then the scan and the scatter both share.  g: the handle whose profile takes the
// scopes (none for the stateless entries).
void launch_inliers(const InlierTest &t, VhInlierArgs &a, hipStream_t st, Group *g) {
  std::optional<Scope> sc;
  if (g) sc.emplace(g, t.is_mono ? "inlier_flag_mono" : "inlier_flag", st);
  if (t.is_mono) {
    a.mono_threshold = t.mono->inlier_threshold;
    vh_launch_inlier_flag_mono(a, st);
  } else {
    a.e = *t.ego;
    vh_launch_inlier_flag(a, st);
  }
  sc.reset();
  if (g) sc.emplace(g, "inlier_compact", st);
  vh_launch_inlier_compact(a, st);
}

int32_t Group::motion_inliers(const InlierTest &t, const int32_t *ok, int32_t *counts) {
  if (!(t.on_device ? t.params_ok() : t.args_ok() && ok) || !counts) return VH_ERR_INVALID_ARG;
  // the stereo test reads the right camera's columns; the mono test the left camera's flow, which flow and quad lists carry
  if (!allocated || !(last_method == VH_METHOD_QUAD || (t.is_mono && last_method == VH_METHOD_FLOW))) return VH_ERR_STATE;
  const int32_t tiles = (mcap + VH_INLIER_TILE - 1) / VH_INLIER_TILE;
  if (!inlier_grid_ok(S, tiles)) return VH_ERR_UNSUPPORTED;
  inl.valid = false;
  size_t bytes = 0;
  const bool first = !inl.d_flags;
  if (first) {  // one block: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(static_cast<InlierArrays &>(inl), &bytes, false, (size_t)S, (size_t)S * mcap, (size_t)tiles);
    if (rc) return rc;
    inl.tiles = tiles;
  }
  if (t.is_mono && !inl.d_model) {  // the models of the mono test: a block of their own, so that the stereo path allocates what it always did
    const int32_t rc = dmalloc(&inl.d_model, (size_t)S, false);
    if (rc) {
      if (first) {  // (nothing has used the main block yet, and no other block of `inl` exists) -- the refused call leaves the handle as it found it
        dfree(inl.d_flags); device_bytes -= (int64_t)bytes;
        inl = InlierState();
      }
      return rc;
    }
  }
  // on the post stream, behind the emission of the lists: the lists the getters serve
  const vh_p_match *d_lists = nullptr;
  const int32_t *d_counts = nullptr;
  bool replaced = false;
  { const int32_t rc = stage_host_lists(inl.host, post_stream, replaced, d_lists, d_counts); if (rc) return rc; }
  inl.n_list.assign((size_t)S, 0); inl.n_inl.assign((size_t)S, 0);
  if (!t.on_device) {  // (on_device: a refit put them there)
    if (t.is_mono) VH_HIP(hipMemcpyAsync(inl.d_model, t.model, sizeof(vh_mono_model) * (size_t)S, hipMemcpyHostToDevice, post_stream));
    else VH_HIP(hipMemcpyAsync(inl.d_tr, t.tr, sizeof(double) * 6 * (size_t)S, hipMemcpyHostToDevice, post_stream));
    VH_HIP(hipMemcpyAsync(inl.d_ok, ok, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, post_stream));
  }
  VhInlierArgs a{};
  a.lists = VhLists::slots(d_lists, mcap, d_counts, mcap, S);
  a.tiles_per_list = inl.tiles;
  a.tr = t.is_mono ? nullptr : inl.d_tr; a.model = t.is_mono ? inl.d_model : nullptr; a.ok = inl.d_ok; a.out_stride = mcap;
  a.flags = inl.d_flags; a.tile_cnt = inl.d_tiles; a.n_inl = inl.d_ninl; a.out = inl.d_out; a.src_pos = inl.d_src;
  launch_inliers(t, a, post_stream, this);
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(inl.n_inl.data(), inl.d_ninl, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(inl.n_list.data(), d_counts, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(mt.h_overflow, mt.d_overflow, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  inl.truncated = false;
  for (int32_t s = 0; s < S; s++) {
    if (inl.n_list[s] > mcap || mt.h_overflow[s]) inl.truncated = true;
    inl.n_list[s] = std::min(inl.n_list[s], mcap);
    counts[s] = inl.n_inl[s];
  }
  inl.valid = true; inl.seq = match_seq; inl.gen++; inl.mono = t.is_mono; inl.from_host = replaced;
  return inl.truncated ? VH_ERR_CAPACITY : VH_OK;
}

// The Gauss-Newton loop of src/viso_stereo.cpp:126-139 on the compacted inlier lists of the current stereo classification,
// from the tr / ok it was made under; reclassify: the classification again under the result, queued behind the refit.
int32_t Group::refit_motion(const vh_ego_params *e, int32_t reclassify, double *tr_out, int32_t *ok_out, int32_t *n_updates, int32_t *counts) {
  if (!e || !tr_out || !ok_out || !n_updates || !counts) return VH_ERR_INVALID_ARG;
  // (a push ends the pair the lists belong to: last_method)
  if (!inliers_current() || inl.mono || last_method != VH_METHOD_QUAD) return VH_ERR_STATE;
  if (!rft.d_tr) {  // one block: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(rft, nullptr, false, (size_t)S);
    if (rc) return rc;
  }
  VhRefitArgs a{};
  a.e = *e;
  a.lists = inlier_lists();
  a.tr_in = inl.d_tr; a.ok_in = inl.d_ok;
  a.tr_out = rft.d_tr; a.ok_out = rft.d_ok; a.n_updates = rft.d_nupd;
  { Scope sc(this, "motion_refit", post_stream); vh_launch_refit(a, post_stream); }
  VH_HIP(hipGetLastError());
  return refit_finish(e, reclassify, rft, tr_out, ok_out, n_updates, counts);
}

int32_t Group::refit_finish(const vh_ego_params *e, int32_t reclassify, const RefitState &r, double *tr_out, int32_t *ok_out, int32_t *n_updates,
                            int32_t *counts) {
  // the results come down behind the refit whatever happens to the classification after it
  VH_HIP(hipMemcpyAsync(tr_out, r.d_tr, sizeof(double) * 6 * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ok_out, r.d_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(n_updates, r.d_nupd, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  if (!reclassify) {
    for (int32_t s = 0; s < S; s++) counts[s] = inl.n_inl[s];
    VH_HIP(hipStreamSynchronize(post_stream));
    return check_violation();
  }
  // the refined motion becomes the one the flag kernel reads: the host does not wait in between, and the one wait of the
  // classification covers the downloads above
  VH_HIP(hipMemcpyAsync(inl.d_tr, r.d_tr, sizeof(double) * 6 * (size_t)S, hipMemcpyDeviceToDevice, post_stream));
  VH_HIP(hipMemcpyAsync(inl.d_ok, r.d_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToDevice, post_stream));
  InlierTest t = InlierTest::stereo(e, nullptr);
  t.on_device = true;
  const int32_t rc = motion_inliers(t, nullptr, counts);
  // (an error there may have returned before its wait: the caller's arrays must be complete when this call returns)
  if (rc != VH_OK && rc != VH_ERR_CAPACITY) (void)hipStreamSynchronize(post_stream);
  return rc;
}

int32_t Group::get_inlier_flags(int32_t s, uint8_t *out, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || capo < 0 || (capo > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!inliers_current()) return VH_ERR_STATE;
  *n = inl.n_list[s];
  bool over = inl.truncated;
  const int32_t rc = get_slot(out, inl.d_flags, s, *n, capo, false, over);
  return rc ? rc : over ? VH_ERR_CAPACITY : VH_OK;
}

int32_t Group::get_inlier_matches(int32_t s, vh_p_match *out, int32_t *src_pos, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || capo < 0 || (capo > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!inliers_current()) return VH_ERR_STATE;
  *n = inl.n_inl[s];
  bool over = inl.truncated;
  int32_t rc = get_slot(out, inl.d_out, s, *n, capo, false, over);
  if (!rc && src_pos) rc = get_slot(src_pos, inl.d_src, s, *n, capo, false, over);
  return rc ? rc : over ? VH_ERR_CAPACITY : VH_OK;
}

int32_t Group::get_inlier_matches_all(vh_p_match *out, int32_t *src_pos, int32_t cap_per_stream, int32_t *counts) {
  if (!out || !counts || cap_per_stream < 0) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < S; s++) counts[s] = 0;
  if (!inliers_current()) return VH_ERR_STATE;
  bool over = inl.truncated;
  for (int32_t s = 0; s < S; s++) {
    counts[s] = inl.n_inl[s];
    int32_t rc = get_slot(out + (size_t)s * cap_per_stream, inl.d_out, s, counts[s], cap_per_stream, true, over);
    if (!rc && src_pos) rc = get_slot(src_pos + (size_t)s * cap_per_stream, inl.d_src, s, counts[s], cap_per_stream, true, over);
    if (rc) return rc;
  }
  VH_HIP(hipStreamSynchronize(post_stream));
  return over ? VH_ERR_CAPACITY : VH_OK;
}

}  // namespace vh_engine

using namespace vh_engine;

// The stateless classification under either test: validation, one device block, the uploads, the flag launch of the
// test, the scan and the scatter, the downloads.
static int32_t inliers_stateless(const InlierTest &t, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                                 const int32_t *ok, uint8_t *flags, int32_t *n_inliers, vh_p_match *inlier_pm, int32_t *src_pos) {
  if (!t.params_ok() || n_sets < 0) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan sp;
  if (!t.args_ok() || !ok || !n_inliers || packed_args(offsets, n_sets, pm, sp)) return VH_ERR_INVALID_ARG;
  if (sp.total > 0 && !flags) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) n_inliers[s] = 0;
  if (sp.total == 0) return VH_OK;
  if (packed_limit(sp, n_sets)) return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets, tiles = (size_t)((sp.longest + VH_INLIER_TILE - 1) / VH_INLIER_TILE);
  // one block: the arrays of a classification | the records up to offsets[n_sets] | offsets | (mono) the models
  InlierArrays ia;
  PackedArrays in;
  vh_mono_model *d_model = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    ia.carve(c, lists, (size_t)sp.end, tiles);
    in.carve(c, sp, lists);
    d_model = c.ptr<vh_mono_model>(t.is_mono ? lists : 0);
  }));
  VH_HIP(blk.up_lists(in, pm, offsets, sp, lists));
  if (t.is_mono) VH_HIP(blk.up(d_model, t.model, lists));
  else VH_HIP(blk.up(ia.d_tr, t.tr, 6 * lists));
  VH_HIP(blk.up(ia.d_ok, ok, lists));
  VhInlierArgs a{};
  a.lists = VhLists::packed(in.d_pm, in.d_off, n_sets);
  a.tiles_per_list = (int32_t)tiles;
  a.tr = t.is_mono ? nullptr : ia.d_tr;  // (each flag kernel reads its own of the two)
  a.model = t.is_mono ? d_model : nullptr;
  a.ok = ia.d_ok;
  a.flags = ia.d_flags; a.out = ia.d_out; a.src_pos = ia.d_src; a.tile_cnt = ia.d_tiles; a.n_inl = ia.d_ninl;
  launch_inliers(t, a, nullptr, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(n_inliers, ia.d_ninl, lists));
  VH_HIP(blk.down(flags + sp.first, ia.d_flags + sp.first, (size_t)sp.total));
  // (the compacted lists: list s's n_inliers[s] records at offsets[s]; what lies behind them in its slice is not written)
  for (int32_t s = 0; s < n_sets && (inlier_pm || src_pos); s++) {
    const size_t o = (size_t)offsets[s], k = (size_t)n_inliers[s];
    if (!k) continue;
    if (inlier_pm) VH_HIP(blk.down(inlier_pm + o, ia.d_out + o, k));
    if (src_pos) VH_HIP(blk.down(src_pos + o, ia.d_src + o, k));
  }
  return VH_OK;
}

// The stateless refit: validation as inliers_stateless, one device block (records | offsets | tr, ok in | tr, ok, updates
// out), one launch.
extern "C" int32_t vh_refit_motion(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                               const double *tr_in, const int32_t *ok_in, double *tr_out, int32_t *ok_out, int32_t *n_updates) {
  if (!e || n_sets < 0) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan sp;
  if (!tr_in || !ok_in || !tr_out || !ok_out || !n_updates || packed_args(offsets, n_sets, pm, sp)) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) {
    ok_out[s] = 0; n_updates[s] = 0;
    for (int32_t m = 0; m < 6; m++) tr_out[6 * (size_t)s + m] = 0;
  }
  if (sp.total == 0) return VH_OK;
  if (packed_limit(sp, n_sets)) return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets;
  PackedArrays in;
  double *d_tr = nullptr; int32_t *d_ok = nullptr;
  RefitState out;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) { in.carve(c, sp, lists); d_tr = c.ptr<double>(6 * lists); d_ok = c.ptr<int32_t>(lists); out.carve(c, lists); }));
  VH_HIP(blk.up_lists(in, pm, offsets, sp, lists));
  VH_HIP(blk.up(d_tr, tr_in, 6 * lists));
  VH_HIP(blk.up(d_ok, ok_in, lists));
  VhRefitArgs a{};
  a.e = *e;
  a.lists = VhLists::packed(in.d_pm, in.d_off, n_sets);
  a.tr_in = d_tr; a.ok_in = d_ok;
  a.tr_out = out.d_tr; a.ok_out = out.d_ok; a.n_updates = out.d_nupd;
  vh_launch_refit(a, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(tr_out, out.d_tr, 6 * lists));
  VH_HIP(blk.down(ok_out, out.d_ok, lists));
  VH_HIP(blk.down(n_updates, out.d_nupd, lists));
  return VH_OK;
}

extern "C" {

int32_t vh_group_refit_motion(vh_group *g, const vh_ego_params *e, int32_t reclassify, double *tr_out, int32_t *ok_out,
                              int32_t *n_updates, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->refit_motion(e, reclassify, tr_out, ok_out, n_updates, counts);
}
int32_t vh_match_refit_motion(vh_matcher *m, const vh_ego_params *e, int32_t reclassify, double *tr_out, int32_t *ok_out,
                              int32_t *n_updates, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->refit_motion(e, reclassify, tr_out, ok_out, n_updates, count);
}
int32_t vh_motion_inliers(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                          const double *tr, const int32_t *ok, uint8_t *flags, int32_t *n_inliers, vh_p_match *inlier_pm,
                          int32_t *src_pos) {
  return inliers_stateless(InlierTest::stereo(e, tr), device, n_sets, pm, offsets, ok, flags, n_inliers, inlier_pm, src_pos);
}
int32_t vh_motion_inliers_mono(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                               const vh_mono_model *model, const int32_t *ok, uint8_t *flags, int32_t *n_inliers,
                               vh_p_match *inlier_pm, int32_t *src_pos) {
  return inliers_stateless(InlierTest::monocular(e, model), device, n_sets, pm, offsets, ok, flags, n_inliers, inlier_pm, src_pos);
}
int32_t vh_group_motion_inliers(vh_group *g, const vh_ego_params *e, const double *tr, const int32_t *ok, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->motion_inliers(InlierTest::stereo(e, tr), ok, counts);
}
int32_t vh_match_inliers(vh_matcher *m, const vh_ego_params *e, const double *tr, int32_t ok, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->motion_inliers(InlierTest::stereo(e, tr), &ok, count);
}
int32_t vh_group_motion_inliers_mono(vh_group *g, const vh_mono_params *e, const vh_mono_model *model, const int32_t *ok, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->motion_inliers(InlierTest::monocular(e, model), ok, counts);
}
int32_t vh_match_inliers_mono(vh_matcher *m, const vh_mono_params *e, const vh_mono_model *model, int32_t ok, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->motion_inliers(InlierTest::monocular(e, model), &ok, count);
}
int32_t vh_group_get_inlier_flags(vh_group *g, int32_t stream, uint8_t *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_inlier_flags(stream, out, cap, n);
}
int32_t vh_group_get_inlier_matches(vh_group *g, int32_t stream, vh_p_match *pm_out, int32_t *src_pos_out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_inlier_matches(stream, pm_out, src_pos_out, cap, n);
}
int32_t vh_group_get_inlier_matches_all(vh_group *g, vh_p_match *pm_out, int32_t *src_pos_out, int32_t cap_per_stream, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_inlier_matches_all(pm_out, src_pos_out, cap_per_stream, counts);
}
int32_t vh_get_inlier_matches(vh_matcher *m, vh_p_match *pm_out, int32_t *src_pos_out, int32_t cap, int32_t *n) {
  return vh_group_get_inlier_matches((vh_group *)m, 0, pm_out, src_pos_out, cap, n);
}
int32_t vh_group_inliers_device(vh_group *g, const uint8_t **d_flags, const vh_p_match **d_matches, const int32_t **d_src_pos, int64_t *stride) {
  Group *gq = (Group *)g;
  if (!gq || !d_flags || !d_matches || !d_src_pos || !stride) return VH_ERR_INVALID_ARG;
  if (!gq->inliers_current()) return VH_ERR_STATE;
  *d_flags = gq->inl.d_flags; *d_matches = gq->inl.d_out; *d_src_pos = gq->inl.d_src; *stride = gq->mcap;
  return VH_OK;
}

}  // extern "C"
