// engine_cov.hip -- the covariance of a stereo motion over whole lists (kernels_cov.hip): on the compacted inlier lists
// of a handle's current stereo classification, under the motion it was made under or a caller-given one, and on
// caller-owned lists; and its part of the ABI.
#include "engine.h"

namespace vh_engine {

// tr == nullptr: the tr / ok the classification was made under (inl.d_tr / inl.d_ok: after a reclassifying refit, the
// refined motion); nothing goes up.  Otherwise the caller's motion on the same lists.
int32_t Group::motion_covariance(const vh_ego_params *e, const double *tr, const int32_t *ok, double *cov, double *ssr, int32_t *ok_out,
                                 int32_t *counts) {
  if (!e || !cov || !ssr || !ok_out || !counts || (tr != nullptr) != (ok != nullptr)) return VH_ERR_INVALID_ARG;
  if (!inliers_current() || inl.mono || last_method != VH_METHOD_QUAD) return VH_ERR_STATE;  // where refit_motion returns it
  if (!cv.d_cov) {  // one block, before any launch: a refused allocation leaves nothing behind
    const int32_t rc = dmalloc_carved(cv, nullptr, false, (size_t)S);
    if (rc) return rc;
  }
  if (tr) {
    VH_HIP(hipMemcpyAsync(cv.d_tr, tr, sizeof(double) * 6 * (size_t)S, hipMemcpyHostToDevice, post_stream));
    VH_HIP(hipMemcpyAsync(cv.d_okin, ok, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, post_stream));
  }
  cv.seq = -1;  // (until this call has ended well)
  VhCovArgs a{};
  a.e = *e;
  a.lists = inlier_lists();
  a.tr = tr ? cv.d_tr : inl.d_tr; a.ok = tr ? cv.d_okin : inl.d_ok;
  a.cov = cv.d_cov; a.ssr = cv.d_ssr; a.ok_out = cv.d_ok;
  { Scope sc(this, "motion_cov", post_stream); vh_launch_motion_cov(a, post_stream); }
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(cov, cv.d_cov, sizeof(double) * 36 * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ssr, cv.d_ssr, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ok_out, cv.d_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  for (int32_t s = 0; s < S; s++) counts[s] = inl.n_inl[s];
  VH_HIP(hipStreamSynchronize(post_stream));
  { const int32_t rv_ = check_violation(); if (rv_) return rv_; }
  cv.seq = match_seq; cv.gen = inl.gen; cv.own_tr = tr == nullptr;
  return VH_OK;
}

}  // namespace vh_engine

using namespace vh_engine;

// The stateless form: validation as the refit's, one device block (records | offsets | tr, ok in | cov, ssr, ok out), one launch.
extern "C" int32_t vh_motion_covariance(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                                    const double *tr, const int32_t *ok, double *cov, double *ssr, int32_t *ok_out) {
  if (!e || n_sets < 0) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan sp;
  if (!tr || !ok || !cov || !ssr || !ok_out || packed_args(offsets, n_sets, pm, sp)) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) {
    ok_out[s] = 0; ssr[s] = 0;
    for (int32_t m = 0; m < 36; m++) cov[36 * (size_t)s + m] = 0;
  }
  if (sp.total == 0) return VH_OK;
  if (packed_limit(sp, n_sets)) return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets;
  PackedArrays in;
  double *d_tr = nullptr, *d_cov = nullptr, *d_ssr = nullptr; int32_t *d_ok = nullptr, *d_ok_out = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    in.carve(c, sp, lists);
    d_tr = c.ptr<double>(6 * lists); d_ok = c.ptr<int32_t>(lists);
    d_cov = c.ptr<double>(36 * lists); d_ssr = c.ptr<double>(lists); d_ok_out = c.ptr<int32_t>(lists);
  }));
  VH_HIP(blk.up_lists(in, pm, offsets, sp, lists));
  VH_HIP(blk.up(d_tr, tr, 6 * lists));
  VH_HIP(blk.up(d_ok, ok, lists));
  VhCovArgs a{};
  a.e = *e;
  a.lists = VhLists::packed(in.d_pm, in.d_off, n_sets);
  a.tr = d_tr; a.ok = d_ok;
  a.cov = d_cov; a.ssr = d_ssr; a.ok_out = d_ok_out;
  vh_launch_motion_cov(a, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(cov, d_cov, 36 * lists));
  VH_HIP(blk.down(ssr, d_ssr, lists));
  VH_HIP(blk.down(ok_out, d_ok_out, lists));
  return VH_OK;
}

extern "C" {

int32_t vh_group_motion_covariance(vh_group *g, const vh_ego_params *e, const double *tr, const int32_t *ok, double *cov, double *ssr,
                                   int32_t *ok_out, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->motion_covariance(e, tr, ok, cov, ssr, ok_out, counts);
}
int32_t vh_match_motion_covariance(vh_matcher *m, const vh_ego_params *e, const double *tr, const int32_t *ok, double *cov, double *ssr,
                                   int32_t *ok_out, int32_t *count) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->motion_covariance(e, tr, ok, cov, ssr, ok_out, count);
}

}  // extern "C"
