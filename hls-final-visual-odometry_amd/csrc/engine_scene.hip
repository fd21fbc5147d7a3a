// engine_scene.hip -- the 3-d points of whole lists, stereo and mono (kernels_scene.hip): on the compacted inlier lists of
// a handle's current classification, under the motion / pose the device holds for it, and on caller-owned lists; and
// their part of the ABI.
#include "engine.h"

namespace vh_engine {

static bool scene_params_ok(const vh_scene_params *sp) { return sp && (sp->frame == 0 || sp->frame == 1); }

// Stereo (e): under the tr / ok the classification was made under (inl.d_tr / inl.d_ok).  Mono (m): under the pose the
// last pose_mono left in mps.d_pose / mps.d_ok for this very classification.  Nothing goes up but Tw.
int32_t Group::scene_points(const vh_ego_params *e, const vh_mono_params *m, const vh_scene_params *sp, const double *Tw, int32_t *counts,
                            bool world) {
  const bool mono = m != nullptr;
  if ((!e && !m) || !scene_params_ok(sp) || !counts) return VH_ERR_INVALID_ARG;
  if (world && !traj_current(mono)) return VH_ERR_STATE;
  if (!inliers_current() || inl.mono != mono) return VH_ERR_STATE;
  // (a push ends the pair the lists belong to: last_method)
  if (mono ? !(last_method == VH_METHOD_QUAD || last_method == VH_METHOD_FLOW) : last_method != VH_METHOD_QUAD) return VH_ERR_STATE;
  if (mono && !(mps.d_pose && mps.pose_seq == match_seq && mps.pose_gen == inl.gen)) return VH_ERR_STATE;
  const int32_t tiles = (mcap + VH_SCENE_TILE - 1) / VH_SCENE_TILE;
  if (!scn.d_out) {  // one block, before any launch: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(static_cast<SceneArrays &>(scn), nullptr, false, (size_t)S, (size_t)S * mcap, (size_t)tiles);
    if (rc) return rc;
    scn.tiles = tiles;
  }
  scn.valid = false;
  scn.n.assign((size_t)S, 0);
  if (world) {
    // the kernel reads the top rows of a 16-double record per list: the chosen matrix of every pose record, device to device
    const double *src = sp->frame == 0 ? trj.d_out->Tw_prev : trj.d_out->Tw_cur;
    VH_HIP(hipMemcpy2DAsync(scn.d_Tw, sizeof(double) * 16, src, sizeof(vh_traj_pose), sizeof(double) * 16, (size_t)S, hipMemcpyDeviceToDevice,
                            post_stream));
  } else if (Tw) VH_HIP(hipMemcpyAsync(scn.d_Tw, Tw, sizeof(double) * 16 * (size_t)S, hipMemcpyHostToDevice, post_stream));
  VhSceneArgs a{};
  if (mono) a.m = *m; else a.e = *e;
  a.sp = *sp;
  a.lists = inlier_lists();
  a.tiles_per_list = scn.tiles;
  a.tr = mono ? nullptr : inl.d_tr; a.pose = mono ? mps.d_pose : nullptr; a.ok = mono ? mps.d_ok : inl.d_ok;
  a.Tw = Tw || world ? scn.d_Tw : nullptr; a.src = inl.d_src; a.out_stride = mcap;
  a.tile_cnt = scn.d_tiles; a.n_out = scn.d_n; a.out = scn.d_out;
  { Scope sc(this, "scene_points", post_stream); vh_launch_scene_points(a, mono, post_stream); }
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(scn.n.data(), scn.d_n, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  for (int32_t s = 0; s < S; s++) counts[s] = scn.n[s];
  scn.valid = true; scn.seq = match_seq;
  return VH_OK;
}

int32_t Group::get_scene_points(int32_t s, vh_scene_point *out, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || capo < 0 || (capo > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!scene_current()) return VH_ERR_STATE;
  *n = scn.n[s];
  bool over = false;
  const int32_t rc = get_slot(out, scn.d_out, s, *n, capo, false, over);
  return rc ? rc : over ? VH_ERR_CAPACITY : VH_OK;
}

int32_t Group::get_scene_points_all(vh_scene_point *out, int32_t cap_per_stream, int32_t *counts) {
  if (!out || !counts || cap_per_stream < 0) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < S; s++) counts[s] = 0;
  if (!scene_current()) return VH_ERR_STATE;
  bool over = false;
  for (int32_t s = 0; s < S; s++) {
    counts[s] = scn.n[s];
    const int32_t rc = get_slot(out + (size_t)s * cap_per_stream, scn.d_out, s, counts[s], cap_per_stream, true, over);
    if (rc) return rc;
  }
  VH_HIP(hipStreamSynchronize(post_stream));
  return over ? VH_ERR_CAPACITY : VH_OK;
}

}  // namespace vh_engine

using namespace vh_engine;

// The stateless form of either kind: validation as the classification's, one device block (records | offsets | tr or pose,
// ok | Tw | tile counts | counts | points), three launches.
static int32_t scene_stateless(const vh_ego_params *e, const vh_mono_params *m, const vh_scene_params *sp, int32_t device, int32_t n_sets,
                               const vh_p_match *pm, const int32_t *offsets, const double *tr, const vh_mono_pose *pose, const int32_t *ok,
                               const double *Tw, vh_scene_point *out, int32_t *counts) {
  const bool mono = m != nullptr;
  if ((!e && !m) || !scene_params_ok(sp) || n_sets < 0) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan span;
  if (!(mono ? (const void *)pose : (const void *)tr) || !ok || !counts || packed_args(offsets, n_sets, pm, span)) return VH_ERR_INVALID_ARG;
  if (span.total > 0 && !out) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) counts[s] = 0;
  if (span.total == 0) return VH_OK;
  if (packed_limit(span, n_sets)) return VH_ERR_UNSUPPORTED;
  const size_t lists = (size_t)n_sets, tiles = (size_t)((span.longest + VH_SCENE_TILE - 1) / VH_SCENE_TILE);  // (lists * tiles < 2^26 under the limits above)
  const int32_t rc = select_device(device);
  if (rc) return rc;
  PackedArrays in;
  double *d_tr = nullptr, *d_Tw = nullptr; vh_mono_pose *d_pose = nullptr;
  int32_t *d_ok = nullptr, *d_tiles = nullptr, *d_n = nullptr;
  vh_scene_point *d_out = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    in.carve(c, span, lists);
    if (mono) d_pose = c.ptr<vh_mono_pose>(lists); else d_tr = c.ptr<double>(6 * lists);
    d_ok = c.ptr<int32_t>(lists);
    d_Tw = c.ptr<double>(Tw ? 16 * lists : 0); d_tiles = c.ptr<int32_t>(lists * tiles); d_n = c.ptr<int32_t>(lists);
    d_out = c.ptr<vh_scene_point>((size_t)span.end);
  }));
  VH_HIP(blk.up_lists(in, pm, offsets, span, lists));
  if (mono) VH_HIP(blk.up(d_pose, pose, lists));
  else VH_HIP(blk.up(d_tr, tr, 6 * lists));
  VH_HIP(blk.up(d_ok, ok, lists));
  if (Tw) VH_HIP(blk.up(d_Tw, Tw, 16 * lists));
  VhSceneArgs a{};
  if (mono) a.m = *m; else a.e = *e;
  a.sp = *sp;
  a.lists = VhLists::packed(in.d_pm, in.d_off, n_sets);
  a.tiles_per_list = (int32_t)tiles;
  a.tr = d_tr; a.pose = d_pose; a.ok = d_ok; a.Tw = Tw ? d_Tw : nullptr;
  a.tile_cnt = d_tiles; a.n_out = d_n; a.out = d_out;
  vh_launch_scene_points(a, mono, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(counts, d_n, lists));
  // (list s's counts[s] points at offsets[s]; what lies behind them in its slice is not written)
  for (int32_t s = 0; s < n_sets; s++) {
    const size_t o = (size_t)offsets[s], k = (size_t)counts[s];
    if (k) VH_HIP(blk.down(out + o, d_out + o, k));
  }
  return VH_OK;
}

extern "C" {

void vh_default_scene_params(vh_scene_params *sp) {
  if (!sp) return;
  sp->frame = 1; sp->min_disp = 0.0f; sp->max_depth = 0.0; sp->max_err = 0.0;
}
int32_t vh_scene_points_stereo(const vh_ego_params *e, const vh_scene_params *sp, int32_t device, int32_t n_sets, const vh_p_match *pm,
                               const int32_t *offsets, const double *tr, const int32_t *ok, const double *Tw, vh_scene_point *out,
                               int32_t *counts) {
  if (!e) return VH_ERR_INVALID_ARG;
  return scene_stateless(e, nullptr, sp, device, n_sets, pm, offsets, tr, nullptr, ok, Tw, out, counts);
}
int32_t vh_scene_points_mono(const vh_mono_params *e, const vh_scene_params *sp, int32_t device, int32_t n_sets, const vh_p_match *pm,
                             const int32_t *offsets, const vh_mono_pose *pose, const int32_t *ok, const double *Tw, vh_scene_point *out,
                             int32_t *counts) {
  if (!e) return VH_ERR_INVALID_ARG;
  return scene_stateless(nullptr, e, sp, device, n_sets, pm, offsets, nullptr, pose, ok, Tw, out, counts);
}
int32_t vh_group_scene_points_stereo(vh_group *g, const vh_ego_params *e, const vh_scene_params *sp, const double *Tw, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!e) return VH_ERR_INVALID_ARG;
  return gq->scene_points(e, nullptr, sp, Tw, counts);
}
int32_t vh_match_scene_points_stereo(vh_matcher *m, const vh_ego_params *e, const vh_scene_params *sp, const double *Tw, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1 || !e) return VH_ERR_INVALID_ARG;
  return gq->scene_points(e, nullptr, sp, Tw, count);
}
int32_t vh_group_scene_points_mono(vh_group *g, const vh_mono_params *e, const vh_scene_params *sp, const double *Tw, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!e) return VH_ERR_INVALID_ARG;
  return gq->scene_points(nullptr, e, sp, Tw, counts);
}
int32_t vh_match_scene_points_mono(vh_matcher *m, const vh_mono_params *e, const vh_scene_params *sp, const double *Tw, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1 || !e) return VH_ERR_INVALID_ARG;
  return gq->scene_points(nullptr, e, sp, Tw, count);
}
int32_t vh_group_get_scene_points(vh_group *g, int32_t stream, vh_scene_point *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_scene_points(stream, out, cap, n);
}
int32_t vh_group_get_scene_points_all(vh_group *g, vh_scene_point *out, int32_t cap_per_stream, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_scene_points_all(out, cap_per_stream, counts);
}
int32_t vh_get_scene_points(vh_matcher *m, vh_scene_point *out, int32_t cap, int32_t *n) {
  return vh_group_get_scene_points((vh_group *)m, 0, out, cap, n);
}
int32_t vh_group_scene_points_device(vh_group *g, const vh_scene_point **d_points, int64_t *stride) {
  Group *gq = (Group *)g;
  if (!gq || !d_points || !stride) return VH_ERR_INVALID_ARG;
  if (!gq->scene_current()) return VH_ERR_STATE;
  *d_points = gq->scn.d_out; *stride = gq->mcap;
  return VH_OK;
}

}  // extern "C"
