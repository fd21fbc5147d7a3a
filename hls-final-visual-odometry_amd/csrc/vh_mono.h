// vh_mono.h -- the per-record functions of VisualOdometryMono, once (host and device): the two rounding steps of
// normalizeFeaturePoints on one coordinate, the Sampson distance test of getInlier and the row of fundamentalMatrix's
// system.  kernels_mono.hip (the estimator), kernels_inlier.hip (the classification of whole lists under a given model)
// and kernels_mono_refit.hip (the model refitted on whole lists) include it; all are built with -ffp-contract=off, so
// every product and sum rounds on its own as on the reference's x86 build.
#ifndef VH_MONO_H
#define VH_MONO_H

#include <stdint.h>
#include <math.h>
#include "../../include/viso_hip.h"
// Host and device, as vh_ego.h: tests/cpp/mono_inlier_check.cpp and mono_refit_check.cpp compile this header for the host.
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define VH_MONO_HD __device__ __forceinline__
#else
#define VH_MONO_HD inline
struct float4 { float x, y, z, w; };
#endif

// normalizeFeaturePoints on one coordinate (src/viso_mono.cpp:190-200, :216-225): the centroid is subtracted in
// double and the difference stored into the match's float field, then that float is scaled in double and stored into
// the float field again -- one rounding to float per step.
VH_MONO_HD float mono_center(float u, double c) { return (float)((double)u - c); }
VH_MONO_HD float mono_scale(float q, double s) { return (float)((double)q * s); }

// Sampson distance test of getInlier (src/viso_mono.cpp:283-309); q = normalised (u1p, v1p, u1c, v1c)
VH_MONO_HD bool sampson_inlier(const double *F, const float4 q, double thr) {
  const double u1 = q.x, v1 = q.y, u2 = q.z, v2 = q.w;
  const double Fx1u = F[0] * u1 + F[1] * v1 + F[2], Fx1v = F[3] * u1 + F[4] * v1 + F[5], Fx1w = F[6] * u1 + F[7] * v1 + F[8];
  const double Ftx2u = F[0] * u2 + F[3] * v2 + F[6], Ftx2v = F[1] * u2 + F[4] * v2 + F[7];
  const double x2tFx1 = u2 * Fx1u + v2 * Fx1v + Fx1w;
  const double d = x2tFx1 * x2tFx1 / (Fx1u * Fx1u + Fx1v * Fx1v + Ftx2u * Ftx2u + Ftx2v * Ftx2v);
  return fabs(d) < thr;
}

// One record of a whole list in the frame of a model the estimator exported (vh_mono_model: the centroids c, the
// scales s): normalised as mono_norm does -> (u1p, v1p, u1c, v1c).
VH_MONO_HD float4 mono_normalise(const vh_mono_model &m, float u1p, float v1p, float u1c, float v1c) {
  float4 q;
  q.x = mono_scale(mono_center(u1p, m.c[0]), m.s[0]); q.y = mono_scale(mono_center(v1p, m.c[1]), m.s[0]);
  q.z = mono_scale(mono_center(u1c, m.c[2]), m.s[1]); q.w = mono_scale(mono_center(v1c, m.c[3]), m.s[1]);
  return q;
}

// The same record tested under the model's F (the refit F of the normalised frame) as mono_final_a lists the inliers.
VH_MONO_HD bool mono_is_inlier(const vh_mono_model &m, float u1p, float v1p, float u1c, float v1c, double thr) {
  return sampson_inlier(m.F, mono_normalise(m, u1p, v1p, u1c, v1c), thr);
}

// One row of fundamentalMatrix's system (src/viso_mono.cpp:244-252) from a normalised record q = (u1p, v1p, u1c, v1c):
// the products are float products of the match's float fields, as the reference's, then widened to double.
VH_MONO_HD void mono_row9(const float4 q, double *r) {
  r[0] = (double)(q.z * q.x); r[1] = (double)(q.z * q.y); r[2] = (double)q.z;
  r[3] = (double)(q.w * q.x); r[4] = (double)(q.w * q.y); r[5] = (double)q.w;
  r[6] = (double)q.x; r[7] = (double)q.y; r[8] = 1.0;
}

#endif
