// engine_mono_refit.hip -- the epipolar model refitted on whole lists (kernels_mono_refit.hip): on the compacted inlier
// lists of a handle's current mono classification, from the model it was made under, and on caller-owned lists; and its
// part of the ABI.
#include "engine.h"

namespace vh_engine {

// fundamentalMatrix over the compacted inlier lists of the current mono classification, from the model / ok it was made
// under (inl.d_model / inl.d_ok); reclassify: the classification again under the result, queued behind the refit.
int32_t Group::refit_model_mono(const vh_mono_params *e, int32_t reclassify, vh_mono_model *model_out, int32_t *ok_out, double *w_out,
                                int32_t *counts) {
  if (!e || !model_out || !ok_out || !w_out || !counts) return VH_ERR_INVALID_ARG;
  // (a push ends the pair the lists belong to: last_method)
  if (!inliers_current() || !inl.mono || !(last_method == VH_METHOD_QUAD || last_method == VH_METHOD_FLOW)) return VH_ERR_STATE;
  if (!mrf.d_model) {  // one block, before any launch: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(mrf, nullptr, false, (size_t)S);
    if (rc) return rc;
  }
  VhMonoRefitArgs a{};
  a.lists = inlier_lists();
  a.model_in = inl.d_model; a.ok_in = inl.d_ok;
  a.model_out = mrf.d_model; a.ok_out = mrf.d_ok; a.w_out = mrf.d_w;
  { Scope sc(this, "mono_refit", post_stream); vh_launch_mono_refit(a, post_stream); }
  VH_HIP(hipGetLastError());
  // the results come down behind the refit whatever happens to the classification after it
  VH_HIP(hipMemcpyAsync(model_out, mrf.d_model, sizeof(vh_mono_model) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ok_out, mrf.d_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(w_out, mrf.d_w, sizeof(double) * 2 * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  if (!reclassify) {
    for (int32_t s = 0; s < S; s++) counts[s] = inl.n_inl[s];
    VH_HIP(hipStreamSynchronize(post_stream));
    return check_violation();
  }
  // the refined model becomes the one the flag kernel reads: the host does not wait in between, and the one wait of the
  // classification covers the downloads above
  VH_HIP(hipMemcpyAsync(inl.d_model, mrf.d_model, sizeof(vh_mono_model) * (size_t)S, hipMemcpyDeviceToDevice, post_stream));
  VH_HIP(hipMemcpyAsync(inl.d_ok, mrf.d_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToDevice, post_stream));
  InlierTest t = InlierTest::monocular(e, nullptr);
  t.on_device = true;
  const int32_t rc = motion_inliers(t, nullptr, counts);
  // (an error there may have returned before its wait: the caller's arrays must be complete when this call returns)
  if (rc != VH_OK && rc != VH_ERR_CAPACITY) (void)hipStreamSynchronize(post_stream);
  return rc;
}

}  // namespace vh_engine

using namespace vh_engine;

// The stateless form: validation as the stereo refit's, one device block (records | offsets | model, ok in | model, ok, w
// out), one launch.
extern "C" int32_t vh_refit_model_mono(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                                    const vh_mono_model *model_in, const int32_t *ok_in, vh_mono_model *model_out, int32_t *ok_out,
                                    double *w_out) {
  if (!e || n_sets < 0) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan sp;
  if (!model_in || !ok_in || !model_out || !ok_out || !w_out || packed_args(offsets, n_sets, pm, sp)) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) {
    ok_out[s] = 0; w_out[2 * (size_t)s] = 0; w_out[2 * (size_t)s + 1] = 0;
    model_out[s] = vh_mono_model{};
  }
  if (sp.total == 0) return VH_OK;
  if (packed_limit(sp, n_sets)) return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets;
  PackedArrays in;
  vh_mono_model *d_model = nullptr, *d_model_out = nullptr; int32_t *d_ok = nullptr, *d_ok_out = nullptr; double *d_w = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    in.carve(c, sp, lists);
    d_model = c.ptr<vh_mono_model>(lists); d_ok = c.ptr<int32_t>(lists);
    d_model_out = c.ptr<vh_mono_model>(lists); d_ok_out = c.ptr<int32_t>(lists); d_w = c.ptr<double>(2 * lists);
  }));
  VH_HIP(blk.up_lists(in, pm, offsets, sp, lists));
  VH_HIP(blk.up(d_model, model_in, lists));
  VH_HIP(blk.up(d_ok, ok_in, lists));
  VhMonoRefitArgs a{};
  a.lists = VhLists::packed(in.d_pm, in.d_off, n_sets);
  a.model_in = d_model; a.ok_in = d_ok;
  a.model_out = d_model_out; a.ok_out = d_ok_out; a.w_out = d_w;
  vh_launch_mono_refit(a, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(model_out, d_model_out, lists));
  VH_HIP(blk.down(ok_out, d_ok_out, lists));
  VH_HIP(blk.down(w_out, d_w, 2 * lists));
  return VH_OK;
}

extern "C" {

int32_t vh_group_refit_model_mono(vh_group *g, const vh_mono_params *e, int32_t reclassify, vh_mono_model *model_out, int32_t *ok_out,
                                  double *w_out, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->refit_model_mono(e, reclassify, model_out, ok_out, w_out, counts);
}
int32_t vh_match_refit_model_mono(vh_matcher *m, const vh_mono_params *e, int32_t reclassify, vh_mono_model *model_out, int32_t *ok_out,
                                  double *w_out, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->refit_model_mono(e, reclassify, model_out, ok_out, w_out, count);
}

}  // extern "C"
