// engine_lmk_refit.hip -- the stereo motion refined with the landmarks as the 3-d prior (kernels_lmk_refit.hip): on a
// handle's compacted inlier lists, its current tracked lists, the predecessor list's landmark states and the trajectory's
// pose of the previous camera, all on the device; on caller-owned lists; and their part of the ABI.
#include "engine.h"

namespace vh_engine {

static bool lmk_refit_params_ok(const vh_lmk_refit_params *rp) { return rp && rp->min_obs >= 1 && rp->reserved == 0; }

// The inlier lists and the tr / ok of the current stereo classification (refit_motion's), the prev of the tracked list
// through the inliers' positions, the states of buffer trk_cur ^ 1 under Group::landmarks' validity rule.  Only the
// params and a caller-given Tw_prev go up.
int32_t Group::refit_motion_landmarks(const vh_ego_params *e, const vh_lmk_refit_params *rp, const double *Tw_prev, int32_t reclassify,
                                      double *tr_out, int32_t *ok_out, int32_t *n_updates, int32_t *n_used, int32_t *counts) {
  if (seq) return VH_ERR_UNSUPPORTED;  // checked first (its rows' poses and states belong to the same call)
  if (!e || !lmk_refit_params_ok(rp) || !tr_out || !ok_out || !n_updates || !n_used || !counts) return VH_ERR_INVALID_ARG;
  if (!inliers_current() || inl.mono || last_method != VH_METHOD_QUAD) return VH_ERR_STATE;  // where refit_motion returns it
  if (!trk_on || !trk_cur_valid || inl.from_host) return VH_ERR_STATE;  // (src_pos numbers the list the classification read: it must be the tracked one)
  if (!Tw_prev && !traj_on) return VH_ERR_STATE;
  if (!lrf.d_prior) {  // one block, before any launch: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(static_cast<LmkRefitArrays &>(lrf), nullptr, false, (size_t)S, (size_t)S * mcap);
    if (rc) return rc;
  }
  lrf.valid = false;
  const int32_t cur = trk_cur, pred = trk_cur ^ 1;
  const bool has_prev = lmk.d_out && trk_pred_valid && lmk.state_seq[pred] >= 0 && lmk.state_seq[pred] == trk_fill_seq[pred];
  if (Tw_prev) VH_HIP(hipMemcpyAsync(lrf.d_Tw, Tw_prev, sizeof(double) * 16 * (size_t)S, hipMemcpyHostToDevice, post_stream));
  else if (trj.d_out) {  // the pose before this pair's step: the base once a call has latched it, else the current one
    const vh_traj_carry *src = trj.latched ? trj.d_base : trj.d_cur;
    VH_HIP(hipMemcpy2DAsync(lrf.d_Tw, sizeof(double) * 16, src->Tw, sizeof(vh_traj_carry), sizeof(double) * 16, (size_t)S,
                            hipMemcpyDeviceToDevice, post_stream));
  } else {  // no step was made yet: every chain stands at its start
    lrf.h_Tw.assign(16 * (size_t)S, 0.0);
    for (size_t q = 0; q < 16 * (size_t)S; q++) lrf.h_Tw[q] = traj_T0.empty() ? (q % 16 % 5 == 0 ? 1.0 : 0.0) : traj_T0[q];
    VH_HIP(hipMemcpyAsync(lrf.d_Tw, lrf.h_Tw.data(), sizeof(double) * 16 * (size_t)S, hipMemcpyHostToDevice, post_stream));
  }
  VhLmkRefitArgs a{};
  a.e = *e; a.rp = *rp;
  a.lists = inlier_lists();
  a.tiles_per_list = (mcap + VH_SCENE_TILE - 1) / VH_SCENE_TILE;
  a.src_pos = inl.d_src; a.trk = tk.d_trk + (size_t)cur * S * mcap; a.trk_counts = tk.d_tcount + (size_t)cur * S; a.slot_stride = mcap;
  if (has_prev) { a.prev = lmk.d_state[pred]; a.prev_counts = tk.d_tcount + (size_t)pred * S; a.prev_stride = mcap; }
  a.Tw = lrf.d_Tw; a.prior = lrf.d_prior; a.n_used = lrf.d_nused;
  a.tr_in = inl.d_tr; a.ok_in = inl.d_ok;
  a.tr_out = lrf.out.d_tr; a.ok_out = lrf.out.d_ok; a.n_updates = lrf.out.d_nupd;
  // (the lists were compacted, the tracks linked, the states and the poses written on the post stream: it orders this behind all)
  { Scope sc(this, "refit_prior", post_stream); VH_HIP(vh_launch_refit_prior(a, post_stream)); }
  { Scope sc(this, "refit_prior_fit", post_stream); vh_launch_refit_prior_fit(a, post_stream); }
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(n_used, lrf.d_nused, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  lrf.n = inl.n_inl;  // (a reclassification below replaces the lists; the priors stay those of the lists the fit read)
  const int64_t at = match_seq;
  const int32_t rc = refit_finish(e, reclassify, lrf.out, tr_out, ok_out, n_updates, counts);
  if (rc == VH_OK || rc == VH_ERR_CAPACITY) { lrf.valid = true; lrf.seq = at; }
  return rc;
}

int32_t Group::get_refit_priors(int32_t s, vh_refit_prior *out, int32_t capo, int32_t *n) {
  if (!n || s < 0 || s >= S || capo < 0 || (capo > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!(allocated && lrf.valid && lrf.seq == match_seq)) return VH_ERR_STATE;
  *n = lrf.n[s];
  bool over = false;
  const int32_t rc = get_slot(out, lrf.d_prior, s, *n, capo, false, over);
  return rc ? rc : over ? VH_ERR_CAPACITY : VH_OK;
}

}  // namespace vh_engine

using namespace vh_engine;

extern "C" {

void vh_default_lmk_refit_params(vh_lmk_refit_params *rp) {
  if (!rp) return;
  rp->min_obs = 2; rp->reserved = 0; rp->max_depth_ratio = 0.0;
}

// One device block (records | offsets | prev_pos | states | their offsets | Tw | tr, ok in | priors | n_used | tr, ok,
// updates out), one memset and two launches.  Every refusal for an argument comes before anything is written.
int32_t vh_refit_motion_landmarks(const vh_ego_params *e, const vh_lmk_refit_params *rp, int32_t device, int32_t n_sets, const vh_p_match *pm,
                                  const int32_t *offsets, const int32_t *prev_pos, const vh_landmark_state *prev, const int32_t *prev_offsets,
                                  const double *Tw_prev, const double *tr_in, const int32_t *ok_in, double *tr_out, int32_t *ok_out,
                                  int32_t *n_updates, int32_t *n_used, vh_refit_prior *prior) {
  if (!e || !lmk_refit_params_ok(rp) || n_sets < 0 || (prev != nullptr) != (prev_offsets != nullptr)) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan sp, pv;
  if (!Tw_prev || !tr_in || !ok_in || !tr_out || !ok_out || !n_updates || !n_used || packed_args(offsets, n_sets, pm, sp)) return VH_ERR_INVALID_ARG;
  if (sp.total > 0 && !prev_pos) return VH_ERR_INVALID_ARG;
  if (prev_offsets && check_offsets(prev_offsets, n_sets, pv)) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) {
    ok_out[s] = 0; n_updates[s] = 0; n_used[s] = 0;
    for (int32_t m = 0; m < 6; m++) tr_out[6 * (size_t)s + m] = 0;
  }
  if (sp.total == 0) return VH_OK;
  if (packed_limit(sp, n_sets) || pv.longest > kListMax) return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets, tiles = (size_t)((sp.longest + VH_SCENE_TILE - 1) / VH_SCENE_TILE);  // (lists * tiles < 2^26 under the limits above)
  PackedArrays in;
  int32_t *d_ppos = nullptr, *d_voff = nullptr, *d_ok = nullptr;
  vh_landmark_state *d_prev = nullptr;
  double *d_Tw = nullptr, *d_tr = nullptr;
  LmkRefitArrays w;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    in.carve(c, sp, lists); d_ppos = c.ptr<int32_t>((size_t)sp.end);
    d_prev = c.ptr<vh_landmark_state>(prev ? (size_t)pv.end : 0); d_voff = c.ptr<int32_t>(prev ? lists + 1 : 0);
    d_tr = c.ptr<double>(6 * lists); d_ok = c.ptr<int32_t>(lists);
    w.carve(c, lists, (size_t)sp.end);
  }));
  d_Tw = w.d_Tw;
  VH_HIP(blk.up_lists(in, pm, offsets, sp, lists));
  VH_HIP(blk.up(d_ppos + sp.first, prev_pos + sp.first, (size_t)sp.total));
  if (prev) {
    if (pv.total > 0) VH_HIP(blk.up(d_prev + pv.first, prev + pv.first, (size_t)pv.total));
    VH_HIP(blk.up(d_voff, prev_offsets, lists + 1));
  }
  VH_HIP(blk.up(d_Tw, Tw_prev, 16 * lists));
  VH_HIP(blk.up(d_tr, tr_in, 6 * lists));
  VH_HIP(blk.up(d_ok, ok_in, lists));
  VhLmkRefitArgs a{};
  a.e = *e; a.rp = *rp;
  a.lists = VhLists::packed(in.d_pm, in.d_off, n_sets);
  a.tiles_per_list = (int32_t)tiles;
  a.prev_pos = d_ppos;
  if (prev) { a.prev = d_prev; a.prev_offsets = d_voff; }
  a.Tw = d_Tw; a.prior = w.d_prior; a.n_used = w.d_nused;
  a.tr_in = d_tr; a.ok_in = d_ok;
  a.tr_out = w.out.d_tr; a.ok_out = w.out.d_ok; a.n_updates = w.out.d_nupd;
  VH_HIP(vh_launch_refit_prior(a, nullptr));
  vh_launch_refit_prior_fit(a, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(tr_out, w.out.d_tr, 6 * lists));
  VH_HIP(blk.down(ok_out, w.out.d_ok, lists));
  VH_HIP(blk.down(n_updates, w.out.d_nupd, lists));
  VH_HIP(blk.down(n_used, w.d_nused, lists));
  if (prior) VH_HIP(blk.down(prior + sp.first, w.d_prior + sp.first, (size_t)sp.total));
  return VH_OK;
}

int32_t vh_group_refit_motion_landmarks(vh_group *g, const vh_ego_params *e, const vh_lmk_refit_params *rp, const double *Tw_prev,
                                        int32_t reclassify, double *tr_out, int32_t *ok_out, int32_t *n_updates, int32_t *n_used,
                                        int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->refit_motion_landmarks(e, rp, Tw_prev, reclassify, tr_out, ok_out, n_updates, n_used, counts);
}
int32_t vh_match_refit_motion_landmarks(vh_matcher *m, const vh_ego_params *e, const vh_lmk_refit_params *rp, const double *Tw_prev,
                                        int32_t reclassify, double *tr_out, int32_t *ok_out, int32_t *n_updates, int32_t *n_used,
                                        int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->refit_motion_landmarks(e, rp, Tw_prev, reclassify, tr_out, ok_out, n_updates, n_used, count);
}
int32_t vh_group_get_refit_priors(vh_group *g, int32_t stream, vh_refit_prior *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_refit_priors(stream, out, cap, n);
}

}  // extern "C"
