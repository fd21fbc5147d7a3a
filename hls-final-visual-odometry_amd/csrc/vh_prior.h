// vh_prior.h -- the motion prior of quad matching, once (device only): the position stock libviso2 predicts for the
// previous-right -> current-right hop of a circle and the cost term findMatch adds for it (src/matcher.cpp:257-262).
// Used by the table form of that hop (kernels_prior.hip) and by the ranged form of multi-stage matching
// (kernels_chain.hip).  Every product and sum rounds on its own as on the reference's x86 build: the functions switch
// contraction off themselves, whatever the unit that includes them is compiled with.
#ifndef VH_PRIOR_H
#define VH_PRIOR_H

#include "vh_dev.h"
#include <math.h>

struct VhPrediction { double u, v; };

// The prediction [upstream-recollection]: the 3-d point of the (1p, 2p) pair of the DRIVING feature, moved by t and
// projected into the current right image.  z2c = 0 gives an infinite or NaN position: vh_prior_cost's literal tests
// decide what that means.
__device__ __forceinline__ VhPrediction vh_prior_predict(const double *__restrict__ t, double f, double cu, double cv, double base, int32_t u1p,
                                                         int32_t v1p, int32_t u2p) {
#pragma clang fp contract(off)
  double d = (double)u1p - (double)u2p;
  if (d < 1.0) d = 1.0;
  const double x1p = ((double)u1p - cu) * base / d, y1p = ((double)v1p - cv) * base / d, z1p = f * base / d;
  const double x2c = t[0] * x1p + t[1] * y1p + t[2] * z1p + t[3] - base;
  const double y2c = t[4] * x1p + t[5] * y1p + t[6] * z1p + t[7];
  const double z2c = t[8] * x1p + t[9] * y1p + t[10] * z1p + t[11];
  VhPrediction r;
  r.u = f * x2c / z2c + cu; r.v = f * y2c / z2c + cv;
  return r;
}

// cost of candidate uv2 (u | v << 16) with descriptor distance sad: SAD + 4 * ||(u2, v2) - (u_, v_)|| in double when
// both coordinates of the prediction are >= 0 (:257), SAD alone otherwise.  sqrt is the correctly rounded one, the sum
// under it rounds twice.
__device__ __forceinline__ double vh_prior_cost(uint32_t sad, uint32_t uv2, double u_, double v_) {
#pragma clang fp contract(off)
  double cost = (double)sad;
  if (u_ >= 0 && v_ >= 0) {
    const double du = (double)(int32_t)(uv2 & 0xFFFFu) - u_, dv = (double)(int32_t)(uv2 >> 16) - v_;
    cost += 4 * sqrt(du * du + dv * dv);
  }
  return cost;
}

#endif
