// engine_mono_pose.hip -- the pose tail of the mono estimator on whole lists (kernels_mono_pose.hip), plain or with the
// winner refined before the tail (kernels_mono_pose_refine.hip): on the compacted
// inlier lists of a handle's current mono classification, under the model it was made under, and on caller-owned lists;
// and its part of the ABI.
#include "engine.h"
#include <optional>

namespace vh_engine {

void launch_mono_pose(const VhMonoPoseArgs &a, bool refined, vh_mono_refine *refine, hipStream_t st, Group *g) {
  std::optional<Scope> sc;
  for (int32_t k = 0; k < VH_MONO_POSE_STAGES; k++) {
    if (g) sc.emplace(g, vh_mono_pose_scope(k), st);
    vh_launch_mono_pose_stage(a, k, st);
    sc.reset();
    if (!(refined && k == 1)) continue;
    // between the chirality count and the tail, which reads what it leaves in the headers; a scope of its own, after the stage's has closed
    if (g) sc.emplace(g, "mono_pose_refine", st);
    vh_launch_mono_pose_refine(a, refine, st);
    sc.reset();
  }
}

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
    const int32_t rc = dmalloc_carved(static_cast<MonoPoseArrays &>(mps), &block, false, (size_t)S, (size_t)S * mcap, (size_t)VH_MONO_POSE_HDR);
    if (rc) return rc;
  }
  if (refined && !mps.d_refine) {  // the refinement's records: a block of their own, so that the plain pose allocates what it always did
    uint8_t *d = nullptr;
    const int32_t rc = dmalloc(&d, up256(sizeof(vh_mono_refine) * (size_t)S), false);
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
  a.lists = inlier_lists();
  a.cap = mcap; a.slot_stride = mcap;
  a.model = inl.d_model; a.ok_in = inl.d_ok;
  a.hdr = mps.d_hdr; a.dist = mps.d_dist; a.d = mps.d_d; a.tr = mps.d_tr; a.ok = mps.d_ok; a.pose = mps.d_pose;
  launch_mono_pose(a, refined, mps.d_refine, post_stream, this);
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
  if (!model || !ok_in || !tr || !ok || packed_args(offsets, n_sets, pm, sp)) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) {
    ok[s] = 0;
    for (int32_t q = 0; q < 6; q++) tr[6 * (size_t)s + q] = 0;
    if (pose) { pose[s] = vh_mono_pose{}; pose[s].candidate = -1; pose[s].reason = ok_in[s] ? 2 : 1; }
    if (refine) { refine[s] = vh_mono_refine{}; refine[s].status = 1; }
  }
  if (sp.total == 0) return VH_OK;
  if (packed_limit(sp, n_sets) || !mono_pose_grid_ok(n_sets, sp.longest)) return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets;
  PackedArrays in;
  vh_mono_model *d_model = nullptr; int32_t *d_okin = nullptr;
  MonoPoseArrays out;  // (offsets[n_sets] slots: dist and d of list s begin at offsets[s])
  vh_mono_refine *d_refine = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    in.carve(c, sp, lists);
    d_model = c.ptr<vh_mono_model>(lists); d_okin = c.ptr<int32_t>(lists);
    out.carve(c, lists, (size_t)sp.end, VH_MONO_POSE_HDR);
    if (refined) d_refine = c.ptr<vh_mono_refine>(lists);
  }));
  VH_HIP(blk.up_lists(in, pm, offsets, sp, lists));
  VH_HIP(blk.up(d_model, model, lists));
  VH_HIP(blk.up(d_okin, ok_in, lists));
  VhMonoPoseArgs a{};
  a.e = *e;
  a.lists = VhLists::packed(in.d_pm, in.d_off, n_sets);
  a.cap = sp.longest;
  a.model = d_model; a.ok_in = d_okin;
  a.hdr = out.d_hdr; a.dist = out.d_dist; a.d = out.d_d; a.tr = out.d_tr; a.ok = out.d_ok; a.pose = out.d_pose;
  launch_mono_pose(a, refined, d_refine, nullptr, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(tr, out.d_tr, 6 * lists));
  VH_HIP(blk.down(ok, out.d_ok, lists));
  if (pose) VH_HIP(blk.down(pose, out.d_pose, lists));
  if (refined && refine) VH_HIP(blk.down(refine, d_refine, lists));
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
