// engine_trajectory.hip -- the camera's pose in the world accumulated from the motions (kernels_trajectory.hip): on
// caller-owned chains of rows; on a handle, from the motion the device holds for the current classification, one chain per
// stream of a group, one chain over the rows of a sequence handle's chunks; and its part of the ABI.
#include "engine.h"

namespace vh_engine {

static bool traj_params_ok(const vh_traj_params *tp) { return tp && (tp->on_fail == VH_TRAJ_HOLD || tp->on_fail == VH_TRAJ_REPEAT); }

static vh_traj_carry traj_start(const double *T0) {
  vh_traj_carry c{};
  for (int32_t q = 0; q < 16; q++) c.Tw[q] = T0 ? T0[q] : (q % 5 == 0 ? 1.0 : 0.0);
  return c;
}

int32_t Group::set_trajectory(const vh_traj_params *tp, const double *T0) {
  if (allocated) return VH_ERR_STATE;  // before the first push only
  if (!tp) { traj_on = false; traj_T0.clear(); tcov_on = false; tcov_S0.clear(); return VH_OK; }  // (the covariance needs the poses)
  if (!traj_params_ok(tp)) return VH_ERR_INVALID_ARG;
  traj_on = true; traj_params = *tp; traj_params.reserved = 0;
  traj_T0.clear();
  if (T0) traj_T0.assign(T0, T0 + 16 * (size_t)traj_chains());
  return VH_OK;
}

// A push has succeeded.  shifted: a new pair -- where the pair before it was stepped, the next call latches the base again;
// where it was not (or its step was undone), the base still is the pose in front of the new pair.  A replace push undoes
// the step: d_cur is stale until the next call recomputes it from the base.
void Group::traj_pushed(bool shifted) {
  if (!traj_on) return;
  if (shifted && trj.stepped) trj.latched = false;
  trj.stepped = false; trj.valid = false;
}

int32_t Group::traj_source(int32_t source, const double *&d_tr, const int32_t *&d_ok) const {
  const bool mono = source == VH_TRAJ_MONO;
  // (Group::scene_points' tests, in its order)
  if (!inliers_current() || inl.mono != mono) return VH_ERR_STATE;
  if (mono ? !(last_method == VH_METHOD_QUAD || last_method == VH_METHOD_FLOW) : last_method != VH_METHOD_QUAD) return VH_ERR_STATE;
  if (mono && !(mps.d_pose && mps.pose_seq == match_seq && mps.pose_gen == inl.gen)) return VH_ERR_STATE;
  d_tr = mono ? mps.d_tr : inl.d_tr; d_ok = mono ? mps.d_ok : inl.d_ok;
  return VH_OK;
}

int32_t Group::trajectory(int32_t source, vh_traj_pose *out) {
  if (source != VH_TRAJ_STEREO && source != VH_TRAJ_MONO) return VH_ERR_INVALID_ARG;
  if (!traj_on) return VH_ERR_STATE;
  if (tcov_on && source == VH_TRAJ_MONO) return VH_ERR_UNSUPPORTED;  // (a 5x5 covariance and a scale without one)
  const double *d_tr = nullptr; const int32_t *d_ok = nullptr;
  { const int32_t rc = traj_source(source, d_tr, d_ok); if (rc) return rc; }
  if (tcov_on) {  // before any launch or latch; its block before the poses': refused, the poses' state is as it was
    if (!tcov_input_current()) return VH_ERR_STATE;
    const int32_t rc = tcov_alloc();
    if (rc) return rc;
  }
  const size_t chains = (size_t)traj_chains();
  if (!trj.d_out) {  // one block, before any launch: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(static_cast<TrajArrays &>(trj), nullptr, false, (size_t)S, chains);
    if (rc) return rc;
    // every chain's start: the one time a pose goes up
    std::vector<vh_traj_carry> start(chains);
    for (size_t c = 0; c < chains; c++) start[c] = traj_start(traj_T0.empty() ? nullptr : traj_T0.data() + 16 * c);
    VH_HIP(hipMemcpy(trj.d_cur, start.data(), sizeof(vh_traj_carry) * chains, hipMemcpyHostToDevice));
    trj.latched = trj.stepped = trj.valid = false;
  }
  trj.valid = false;
  if (!trj.latched) {
    VH_HIP(hipMemcpyAsync(trj.d_base, trj.d_cur, sizeof(vh_traj_carry) * chains, hipMemcpyDeviceToDevice, post_stream));
    if (tcov_on) VH_HIP(hipMemcpyAsync(tcv.d_base, tcv.d_cur, sizeof(vh_traj_cov_carry) * chains, hipMemcpyDeviceToDevice, post_stream));
    trj.latched = true;
  }
  VhTrajArgs a{};
  a.p = traj_params;
  a.n_chains = (int32_t)chains; a.rows_per_chain = seq ? S : 1;
  // a sequence handle: row 0 of the first chunk and the rows behind a short chunk hold no pair
  a.pair_lo = seq && seq_first == 0 ? 1 : 0; a.pair_hi = seq ? std::min(std::max(seq_n, 0), S) : 1;
  a.tr = d_tr; a.ok = d_ok;
  a.carry_in = trj.d_base; a.out = trj.d_out; a.carry_out = trj.d_cur;
  // (the motion was written on the post stream: the same stream orders this behind it)
  { Scope sc(this, "trajectory", post_stream); vh_launch_trajectory(a, post_stream); }
  VH_HIP(hipGetLastError());
  if (tcov_on) {
    tcov_launch(d_tr, d_ok, a.pair_lo, a.pair_hi);
    VH_HIP(hipGetLastError());
  }
  trj.stepped = true;
  if (out) VH_HIP(hipMemcpyAsync(out, trj.d_out, sizeof(vh_traj_pose) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipStreamSynchronize(post_stream));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  trj.valid = true; trj.seq = match_seq; trj.gen = inl.gen; trj.source = source;
  return VH_OK;
}

int32_t Group::get_poses(vh_traj_pose *out) {
  if (!out) return VH_ERR_INVALID_ARG;
  if (!traj_on || !trj.d_out || !trj.valid) return VH_ERR_STATE;
  VH_HIP(hipMemcpy(out, trj.d_out, sizeof(vh_traj_pose) * (size_t)S, hipMemcpyDeviceToHost));
  return VH_OK;
}

// both carries: whether or not the current pair was stepped already, the chain goes on from T
int32_t Group::set_pose(int32_t s, const double *T) {
  if (!T || s < 0 || s >= traj_chains()) return VH_ERR_INVALID_ARG;
  if (!traj_on) return VH_ERR_STATE;
  for (int32_t q = 0; q < 16; q++) if (!std::isfinite(T[q])) return VH_ERR_INVALID_ARG;
  if (!trj.d_out) {  // nothing on the device yet: the chain's start
    if (traj_T0.empty()) for (int32_t c = 0; c < traj_chains(); c++) for (int32_t q = 0; q < 16; q++) traj_T0.push_back(q % 5 == 0 ? 1.0 : 0.0);
    std::copy(T, T + 16, traj_T0.begin() + 16 * (size_t)s);
    return tcov_on ? tcov_set(s, nullptr, true) : VH_OK;
  }
  const vh_traj_carry c = traj_start(T);
  VH_HIP(hipStreamSynchronize(post_stream));
  VH_HIP(hipMemcpy(trj.d_base + s, &c, sizeof c, hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(trj.d_cur + s, &c, sizeof c, hipMemcpyHostToDevice));
  trj.valid = false;
  return tcov_on ? tcov_set(s, nullptr, true) : VH_OK;
}

}  // namespace vh_engine

using namespace vh_engine;

extern "C" {

void vh_default_traj_params(vh_traj_params *tp) {
  if (!tp) return;
  tp->on_fail = VH_TRAJ_HOLD; tp->reserved = 0;
}

// One device block (offsets | tr | ok | T0 | carry in | poses | carry out), one launch.
int32_t vh_trajectory(const vh_traj_params *tp, int32_t device, int32_t n_chains, const int32_t *offsets, const double *tr, const int32_t *ok,
                      const double *T0, const vh_traj_carry *carry_in, vh_traj_pose *out, vh_traj_carry *carry_out) {
  if (!traj_params_ok(tp) || n_chains < 0) return VH_ERR_INVALID_ARG;
  if (n_chains == 0) return VH_OK;
  ListSpan sp;
  if (check_offsets(offsets, n_chains, sp) || (sp.total > 0 && (!tr || !ok || !out))) return VH_ERR_INVALID_ARG;
  if (n_chains > (1 << 24)) return VH_ERR_UNSUPPORTED;
  const size_t chains = (size_t)n_chains;
  if (sp.total == 0) {  // every chain ends where it starts
    if (carry_out) for (size_t c = 0; c < chains; c++) carry_out[c] = carry_in ? carry_in[c] : traj_start(T0 ? T0 + 16 * c : nullptr);
    return VH_OK;
  }
  const int32_t rc = select_device(device);
  if (rc) return rc;
  int32_t *d_off = nullptr, *d_ok = nullptr; double *d_tr = nullptr, *d_T0 = nullptr;
  vh_traj_carry *d_cin = nullptr, *d_cout = nullptr; vh_traj_pose *d_out = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    d_off = c.ptr<int32_t>(chains + 1); d_tr = c.ptr<double>(6 * (size_t)sp.end); d_ok = c.ptr<int32_t>((size_t)sp.end);
    d_T0 = c.ptr<double>(T0 && !carry_in ? 16 * chains : 0); d_cin = c.ptr<vh_traj_carry>(carry_in ? chains : 0);
    d_out = c.ptr<vh_traj_pose>((size_t)sp.end); d_cout = c.ptr<vh_traj_carry>(chains);
  }));
  VH_HIP(blk.up(d_off, offsets, chains + 1));
  VH_HIP(blk.up(d_tr + 6 * (size_t)sp.first, tr + 6 * (size_t)sp.first, 6 * (size_t)sp.total));
  VH_HIP(blk.up(d_ok + sp.first, ok + sp.first, (size_t)sp.total));
  if (carry_in) VH_HIP(blk.up(d_cin, carry_in, chains));
  else if (T0) VH_HIP(blk.up(d_T0, T0, 16 * chains));
  VhTrajArgs a{};
  a.p = *tp;
  a.n_chains = n_chains; a.offsets = d_off;
  a.pair_lo = 0; a.pair_hi = INT32_MAX;
  a.tr = d_tr; a.ok = d_ok; a.T0 = carry_in ? nullptr : (T0 ? d_T0 : nullptr); a.carry_in = carry_in ? d_cin : nullptr;
  a.out = d_out; a.carry_out = d_cout;
  vh_launch_trajectory(a, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(out + sp.first, d_out + sp.first, (size_t)sp.total));
  if (carry_out) VH_HIP(blk.down(carry_out, d_cout, chains));
  return VH_OK;
}

int32_t vh_group_set_trajectory(vh_group *g, const vh_traj_params *tp, const double *T0) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->seq) return VH_ERR_UNSUPPORTED;  // one chain over the rows: vh_sequence_set_trajectory
  return gq->set_trajectory(tp, T0);
}
int32_t vh_sequence_set_trajectory(vh_group *g, const vh_traj_params *tp, const double *T0) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (!gq->seq) return VH_ERR_UNSUPPORTED;
  return gq->set_trajectory(tp, T0);
}
int32_t vh_set_trajectory(vh_matcher *m, const vh_traj_params *tp, const double *T0) {
  Group *gq = (Group *)m;
  if (!gq || gq->S != 1 || gq->seq) return VH_ERR_INVALID_ARG;
  return gq->set_trajectory(tp, T0);
}
int32_t vh_group_trajectory(vh_group *g, int32_t source, vh_traj_pose *out) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->trajectory(source, out);
}
int32_t vh_match_trajectory(vh_matcher *m, int32_t source, vh_traj_pose *out) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->trajectory(source, out);
}
int32_t vh_group_get_poses(vh_group *g, vh_traj_pose *out) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_poses(out);
}
int32_t vh_get_pose(vh_matcher *m, vh_traj_pose *out) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->get_poses(out);
}
int32_t vh_group_poses_device(vh_group *g, const vh_traj_pose **d_poses, int64_t *stride) {
  Group *gq = (Group *)g;
  if (!gq || !d_poses || !stride) return VH_ERR_INVALID_ARG;
  if (!gq->traj_on || !gq->trj.d_out || !gq->trj.valid) return VH_ERR_STATE;
  *d_poses = gq->trj.d_out; *stride = 1;
  return VH_OK;
}
int32_t vh_group_set_pose(vh_group *g, int32_t stream, const double *T) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->set_pose(stream, T);
}
int32_t vh_group_scene_points_stereo_world(vh_group *g, const vh_ego_params *e, const vh_scene_params *sp, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!e) return VH_ERR_INVALID_ARG;
  return gq->scene_points(e, nullptr, sp, nullptr, counts, true);
}
int32_t vh_group_scene_points_mono_world(vh_group *g, const vh_mono_params *e, const vh_scene_params *sp, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!e) return VH_ERR_INVALID_ARG;
  return gq->scene_points(nullptr, e, sp, nullptr, counts, true);
}
int32_t vh_match_scene_points_stereo_world(vh_matcher *m, const vh_ego_params *e, const vh_scene_params *sp, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1 || !e) return VH_ERR_INVALID_ARG;
  return gq->scene_points(e, nullptr, sp, nullptr, count, true);
}
int32_t vh_match_scene_points_mono_world(vh_matcher *m, const vh_mono_params *e, const vh_scene_params *sp, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1 || !e) return VH_ERR_INVALID_ARG;
  return gq->scene_points(nullptr, e, sp, nullptr, count, true);
}

}  // extern "C"
