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
    Carver c;
    const size_t o_cov = c.take<double>(36 * (size_t)S), o_ssr = c.take<double>((size_t)S), o_ok = c.take<int32_t>((size_t)S);
    const size_t o_tr = c.take<double>(6 * (size_t)S), o_okin = c.take<int32_t>((size_t)S);
    uint8_t *d = nullptr;
    const int32_t rc = dmalloc(&d, c.bytes(), false);
    if (rc) return rc;
    cv.d_cov = (double *)(d + o_cov); cv.d_ssr = (double *)(d + o_ssr); cv.d_ok = (int32_t *)(d + o_ok);
    cv.d_tr = (double *)(d + o_tr); cv.d_okin = (int32_t *)(d + o_okin);
  }
  if (tr) {
    VH_HIP(hipMemcpyAsync(cv.d_tr, tr, sizeof(double) * 6 * (size_t)S, hipMemcpyHostToDevice, post_stream));
    VH_HIP(hipMemcpyAsync(cv.d_okin, ok, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, post_stream));
  }
  VhCovArgs a{};
  a.e = *e;
  a.pm = inl.d_out; a.pm_stride = mcap; a.counts = inl.d_ninl; a.count_cap = mcap; a.n_lists = S;
  a.tr = tr ? cv.d_tr : inl.d_tr; a.ok = tr ? cv.d_okin : inl.d_ok;
  a.cov = cv.d_cov; a.ssr = cv.d_ssr; a.ok_out = cv.d_ok;
  {
    Scope sc(this, "motion_cov", post_stream);
    vh_launch_motion_cov(a, post_stream);
  }
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(cov, cv.d_cov, sizeof(double) * 36 * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ssr, cv.d_ssr, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  VH_HIP(hipMemcpyAsync(ok_out, cv.d_ok, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, post_stream));
  for (int32_t s = 0; s < S; s++) counts[s] = inl.n_inl[s];
  VH_HIP(hipStreamSynchronize(post_stream));
  return check_violation();
}

}  // namespace vh_engine

using namespace vh_engine;

// The stateless form: validation as the refit's, one device block (records | offsets | tr, ok in | cov, ssr, ok out), one launch.
static int32_t covariance_stateless(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                                    const double *tr, const int32_t *ok, double *cov, double *ssr, int32_t *ok_out) {
  if (!e || n_sets < 0) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan sp;
  if (!tr || !ok || !cov || !ssr || !ok_out || check_offsets(offsets, n_sets, sp)) return VH_ERR_INVALID_ARG;
  const int64_t nmax = sp.longest, end = sp.end, total = sp.total;
  if (total > 0 && !pm) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) {
    ok_out[s] = 0; ssr[s] = 0;
    for (int32_t m = 0; m < 36; m++) cov[36 * (size_t)s + m] = 0;
  }
  if (total == 0) return VH_OK;
  if (nmax > (1 << VH_TRACK_POS_BITS) - 1 || !inlier_grid_ok(n_sets, (nmax + VH_INLIER_TILE - 1) / VH_INLIER_TILE)) return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets;
  Carver c;
  const size_t o_pm = c.take<vh_p_match>((size_t)end), o_off = c.take<int32_t>(lists + 1);
  const size_t o_tr = c.take<double>(6 * lists), o_ok = c.take<int32_t>(lists);
  const size_t o_cov = c.take<double>(36 * lists), o_ssr = c.take<double>(lists), o_ok2 = c.take<int32_t>(lists);
  DeviceBlock blk;
  VH_HIP(blk.alloc(c.bytes()));
  uint8_t *d = blk.as<uint8_t>();
  const size_t first = (size_t)sp.first;
  VH_HIP(hipMemcpy(d + o_pm + sizeof(vh_p_match) * first, pm + first, sizeof(vh_p_match) * (size_t)total, hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(d + o_off, offsets, sizeof(int32_t) * (lists + 1), hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(d + o_tr, tr, sizeof(double) * 6 * lists, hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(d + o_ok, ok, sizeof(int32_t) * lists, hipMemcpyHostToDevice));
  VhCovArgs a{};
  a.e = *e;
  a.pm = (const vh_p_match *)(d + o_pm); a.offsets = (const int32_t *)(d + o_off); a.n_lists = n_sets;
  a.tr = (const double *)(d + o_tr); a.ok = (const int32_t *)(d + o_ok);
  a.cov = (double *)(d + o_cov); a.ssr = (double *)(d + o_ssr); a.ok_out = (int32_t *)(d + o_ok2);
  vh_launch_motion_cov(a, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(hipMemcpy(cov, a.cov, sizeof(double) * 36 * lists, hipMemcpyDeviceToHost));
  VH_HIP(hipMemcpy(ssr, a.ssr, sizeof(double) * lists, hipMemcpyDeviceToHost));
  VH_HIP(hipMemcpy(ok_out, a.ok_out, sizeof(int32_t) * lists, hipMemcpyDeviceToHost));
  return VH_OK;
}

extern "C" {

int32_t vh_motion_covariance(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                             const double *tr, const int32_t *ok, double *cov, double *ssr, int32_t *ok_out) {
  return covariance_stateless(e, device, n_sets, pm, offsets, tr, ok, cov, ssr, ok_out);
}
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
