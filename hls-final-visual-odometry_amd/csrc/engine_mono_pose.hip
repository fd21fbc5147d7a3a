// engine_mono_pose.hip -- the pose tail of the mono estimator on whole lists (kernels_mono_pose.hip), plain or with the
// winner refined before the tail (kernels_mono_pose_refine.hip): on the compacted
// inlier lists of a handle's current mono classification, under the model it was made under, and on caller-owned lists;
// and its part of the ABI.
#include "engine.h"

namespace vh_engine {

// E, the candidates, chirality, the ground-plane vote and tr over the compacted inlier lists of the current mono
// classification, under the model / ok it was made under (inl.d_model / inl.d_ok).
int32_t Group::pose_mono(const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose, int32_t *counts, bool refined, vh_mono_refine *refine) {
  if (!e || !tr || !ok) return VH_ERR_INVALID_ARG;
  // (a push ends the pair the lists belong to: last_method)
  if (!inliers_current() || !inl.mono || !(last_method == VH_METHOD_QUAD || last_method == VH_METHOD_FLOW)) return VH_ERR_STATE;
  if (!mono_pose_grid_ok(S, mcap)) return VH_ERR_UNSUPPORTED;
  const bool first = !mps.d_hdr;
  size_t block = 0;
  if (first) {  // one block, before any launch: a refused allocation leaves nothing behind
    Carver c;
    const size_t slots = (size_t)S * (size_t)mcap;
    const size_t o_dist = c.take<double>(slots), o_d = c.take<double>(slots), o_hdr = c.take<double>((size_t)S * VH_MONO_POSE_HDR);
    const size_t o_tr = c.take<double>(6 * (size_t)S), o_pose = c.take<vh_mono_pose>((size_t)S), o_ok = c.take<int32_t>((size_t)S);
    uint8_t *d = nullptr;
    const int32_t rc = dmalloc(&d, c.bytes(), false);
    if (rc) return rc;
    block = c.bytes();
    mps.d_dist = (double *)(d + o_dist); mps.d_d = (double *)(d + o_d); mps.d_hdr = (double *)(d + o_hdr);
    mps.d_tr = (double *)(d + o_tr); mps.d_pose = (vh_mono_pose *)(d + o_pose); mps.d_ok = (int32_t *)(d + o_ok);
  }
  if (refined && !mps.d_refine) {  // the refinement's records: a block of their own, so that the plain pose allocates what it always did
    Carver c;
    c.take<vh_mono_refine>((size_t)S);
    uint8_t *d = nullptr;
    const int32_t rc = dmalloc(&d, c.bytes(), false);
    if (rc) {
      if (first) {  // (nothing has used the main block yet) -- the refused call leaves the handle as it found it
        dfree(mps.d_dist); device_bytes -= (int64_t)block;
        mps = MonoPoseState();
      }
      return rc;
    }
    mps.d_refine = (vh_mono_refine *)d;
  }
  VhMonoPoseArgs a{};
  a.e = *e;
  a.pm = inl.d_out; a.pm_stride = mcap; a.counts = inl.d_ninl; a.count_cap = mcap; a.n_lists = S;
  a.cap = mcap; a.slot_stride = mcap;
  a.model = inl.d_model; a.ok_in = inl.d_ok;
  a.hdr = mps.d_hdr; a.dist = mps.d_dist; a.d = mps.d_d; a.tr = mps.d_tr; a.ok = mps.d_ok; a.pose = mps.d_pose;
  for (int32_t k = 0; k < VH_MONO_POSE_STAGES; k++) {
    {
      Scope sc(this, vh_mono_pose_scope(k), post_stream);
      vh_launch_mono_pose_stage(a, k, post_stream);
    }
    if (refined && k == 1) {  // between the chirality count and the tail, which reads what it leaves in the headers; a scope of its own, after the stage's has closed
      Scope sr(this, "mono_pose_refine", post_stream);
      vh_launch_mono_pose_refine(a, mps.d_refine, post_stream);
    }
  }
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(tr, mps.d_tr, sizeof(double) * 6 * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ok, mps.d_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  if (pose) VH_HIP(hipMemcpyAsync(pose, mps.d_pose, sizeof(vh_mono_pose) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  if (refined && refine) VH_HIP(hipMemcpyAsync(refine, mps.d_refine, sizeof(vh_mono_refine) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  if (counts) for (int32_t s = 0; s < S; s++) counts[s] = inl.n_inl[s];
  mps.pose_seq = -1;  // (should the wait fail, d_pose is nobody's)
  VH_HIP(hipStreamSynchronize(post_stream));
  mps.pose_seq = match_seq; mps.pose_gen = inl.gen;
  return check_violation();
}

}  // namespace vh_engine

using namespace vh_engine;

// The stateless form: validation as the mono refit's, one device block (records | offsets | model, ok in | dist, d |
// headers | tr, ok, pose out | refine out), six launches, seven with the refinement.
static int32_t mono_pose_stateless(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                                   const vh_mono_model *model, const int32_t *ok_in, double *tr, int32_t *ok, vh_mono_pose *pose,
                                   bool refined, vh_mono_refine *refine) {
  if (!e || n_sets < 0) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan sp;
  if (!model || !ok_in || !tr || !ok || check_offsets(offsets, n_sets, sp)) return VH_ERR_INVALID_ARG;
  const int64_t nmax = sp.longest, end = sp.end, total = sp.total;
  if (total > 0 && !pm) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) {
    ok[s] = 0;
    for (int32_t q = 0; q < 6; q++) tr[6 * (size_t)s + q] = 0;
    if (pose) { pose[s] = vh_mono_pose{}; pose[s].candidate = -1; pose[s].reason = ok_in[s] ? 2 : 1; }
    if (refine) { refine[s] = vh_mono_refine{}; refine[s].status = 1; }
  }
  if (total == 0) return VH_OK;
  if (nmax > (1 << VH_TRACK_POS_BITS) - 1 || !inlier_grid_ok(n_sets, (nmax + VH_INLIER_TILE - 1) / VH_INLIER_TILE) || !mono_pose_grid_ok(n_sets, nmax))
    return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets;
  Carver c;
  const size_t o_pm = c.take<vh_p_match>((size_t)end), o_off = c.take<int32_t>(lists + 1);
  const size_t o_model = c.take<vh_mono_model>(lists), o_okin = c.take<int32_t>(lists);
  const size_t o_dist = c.take<double>((size_t)end), o_d = c.take<double>((size_t)end), o_hdr = c.take<double>(lists * VH_MONO_POSE_HDR);
  const size_t o_tr = c.take<double>(6 * lists), o_pose = c.take<vh_mono_pose>(lists), o_ok = c.take<int32_t>(lists);
  const size_t o_ref = refined ? c.take<vh_mono_refine>(lists) : 0;
  DeviceBlock blk;
  VH_HIP(blk.alloc(c.bytes()));
  uint8_t *d = blk.as<uint8_t>();
  const size_t first = (size_t)sp.first;
  VH_HIP(hipMemcpy(d + o_pm + sizeof(vh_p_match) * first, pm + first, sizeof(vh_p_match) * (size_t)total, hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(d + o_off, offsets, sizeof(int32_t) * (lists + 1), hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(d + o_model, model, sizeof(vh_mono_model) * lists, hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(d + o_okin, ok_in, sizeof(int32_t) * lists, hipMemcpyHostToDevice));
  VhMonoPoseArgs a{};
  a.e = *e;
  a.pm = (const vh_p_match *)(d + o_pm); a.offsets = (const int32_t *)(d + o_off); a.n_lists = n_sets;
  a.cap = nmax;
  a.model = (const vh_mono_model *)(d + o_model); a.ok_in = (const int32_t *)(d + o_okin);
  a.hdr = (double *)(d + o_hdr); a.dist = (double *)(d + o_dist); a.d = (double *)(d + o_d);
  a.tr = (double *)(d + o_tr); a.ok = (int32_t *)(d + o_ok); a.pose = (vh_mono_pose *)(d + o_pose);
  for (int32_t k = 0; k < VH_MONO_POSE_STAGES; k++) {
    vh_launch_mono_pose_stage(a, k, nullptr);
    if (refined && k == 1) vh_launch_mono_pose_refine(a, (vh_mono_refine *)(d + o_ref), nullptr);
  }
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(hipMemcpy(tr, a.tr, sizeof(double) * 6 * lists, hipMemcpyDeviceToHost));
  VH_HIP(hipMemcpy(ok, a.ok, sizeof(int32_t) * lists, hipMemcpyDeviceToHost));
  if (pose) VH_HIP(hipMemcpy(pose, a.pose, sizeof(vh_mono_pose) * lists, hipMemcpyDeviceToHost));
  if (refined && refine) VH_HIP(hipMemcpy(refine, d + o_ref, sizeof(vh_mono_refine) * lists, hipMemcpyDeviceToHost));
  return VH_OK;
}

extern "C" {

int32_t vh_pose_mono(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                     const vh_mono_model *model, const int32_t *ok_in, double *tr, int32_t *ok, vh_mono_pose *pose) {
  return mono_pose_stateless(e, device, n_sets, pm, offsets, model, ok_in, tr, ok, pose, false, nullptr);
}
int32_t vh_pose_mono_refined(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                             const vh_mono_model *model, const int32_t *ok_in, double *tr, int32_t *ok, vh_mono_pose *pose,
                             vh_mono_refine *refine) {
  return mono_pose_stateless(e, device, n_sets, pm, offsets, model, ok_in, tr, ok, pose, true, refine);
}
int32_t vh_group_pose_mono(vh_group *g, const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->pose_mono(e, tr, ok, pose, counts);
}
int32_t vh_match_pose_mono(vh_matcher *m, const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->pose_mono(e, tr, ok, pose, nullptr);
}
int32_t vh_group_pose_mono_refined(vh_group *g, const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose,
                                   vh_mono_refine *refine, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->pose_mono(e, tr, ok, pose, counts, true, refine);
}
int32_t vh_match_pose_mono_refined(vh_matcher *m, const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose,
                                   vh_mono_refine *refine) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->pose_mono(e, tr, ok, pose, nullptr, true, refine);
}

}  // extern "C"
