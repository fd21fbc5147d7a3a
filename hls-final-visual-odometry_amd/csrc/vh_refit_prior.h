// vh_refit_prior.h -- the one copy of the rule of the motion refit on the landmarks (include/viso_hip_lmk_refit.h, steps 1-4;
// DESIGN.md section 4.25): which 3-d point a record of a quad list enters the fit with -- the landmark of its track,
// brought into the previous camera's frame, or its own triangulation from the previous pair.  Included by
// kernels_lmk_refit.hip (one lane per record) and, for the host, by tests/cpp/lmk_refit_check.cpp; both are built with
// -ffp-contract=off: double, every product and sum rounds on its own, sums are added left to right.
#ifndef VH_REFIT_PRIOR_H
#define VH_REFIT_PRIOR_H
#include "vh_ego.h"
#include "../../include/viso_hip_lmk_refit.h"

// The sums of the predecessor record's state as the caller loaded them (in_range: 0 <= prev_pos < n_prev and a
// predecessor exists; where it is false nothing was loaded and the other values are not looked at).
struct VhPriorState {
  bool in_range;
  double sw, swx, swy, swz;
  int32_t n_obs;
};

VH_EGO_HD bool vh_prior_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // (false for NaN and both infinities)

// own: the record's point of the previous pair (ego_observe); Tw: row-major 4x4, the previous camera to the world
VH_EGO_HD vh_refit_prior vh_refit_prior_point(const EgoObs &own, const VhPriorState &st, const double *Tw, const vh_lmk_refit_params &rp) {
  vh_refit_prior r;
  r.X = own.X; r.Y = own.Y; r.Z = own.Z; r.source = 0;
  if (!st.in_range) { r.reason = 1; return r; }
  if (st.n_obs < rp.min_obs) { r.reason = 2; return r; }
  const double mx = st.swx / st.sw, my = st.swy / st.sw, mz = st.swz / st.sw;
  const double dx = mx - Tw[3], dy = my - Tw[7], dz = mz - Tw[11];
  const double Lx = Tw[0] * dx + Tw[4] * dy + Tw[8] * dz;
  const double Ly = Tw[1] * dx + Tw[5] * dy + Tw[9] * dz;
  const double Lz = Tw[2] * dx + Tw[6] * dy + Tw[10] * dz;
  if (st.sw <= 0 || !(vh_prior_finite(mx) && vh_prior_finite(my) && vh_prior_finite(mz) && vh_prior_finite(Lx) && vh_prior_finite(Ly) &&
                      vh_prior_finite(Lz))) { r.reason = 3; return r; }
  if (Lz <= 0) { r.reason = 4; return r; }
  if (rp.max_depth_ratio > 1) {
    const double q = Lz / own.Z, lo = 1.0 / rp.max_depth_ratio;
    if (!vh_prior_finite(q) || q < lo || q > rp.max_depth_ratio) { r.reason = 5; return r; }
  }
  r.X = Lx; r.Y = Ly; r.Z = Lz; r.source = 1; r.reason = 0;
  return r;
}

#endif
