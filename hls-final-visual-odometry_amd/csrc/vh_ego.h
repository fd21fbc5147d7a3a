// vh_ego.h -- the stereo reprojection model of VisualOdometryStereo, once: the rotation and its derivatives, the
// prediction of one match, the inlier test of getInlier, and one match's rows of the normal equations with their 6x6
// solve (updateParameters).  kernels_ego.hip (the estimator), kernels_inlier.hip (the classification of whole lists
// under a given motion), kernels_refit.hip (Gauss-Newton on whole lists) and kernels_cov.hip (the covariance of a motion
// over whole lists) include it; all are built with
// -ffp-contract=off, so every product and sum rounds on its own as on the reference's x86 build.
#ifndef VH_EGO_H
#define VH_EGO_H

#include <stdint.h>
#include <math.h>
#include "../../include/viso_hip.h"
// Host and device, as vh_gauss_jordan.h: tests/cpp/inlier_check.cpp and refit_check.cpp compile this header for the host.
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define VH_EGO_HD __device__ __forceinline__
#ifndef SVD_HD
#define SVD_HD __device__ __forceinline__
#endif
#else
#define VH_EGO_HD inline
#endif
#include "vh_gauss_jordan.h"

struct EgoRot {
  double r[9], drx[9], dry[9], drz[9];
};

VH_EGO_HD void ego_rot(const double tr[6], EgoRot &R) {
  const double sx = sin(tr[0]), cx = cos(tr[0]), sy = sin(tr[1]), cy = cos(tr[1]), sz = sin(tr[2]), cz = cos(tr[2]);
  R.r[0] = +cy * cz; R.r[1] = -cy * sz; R.r[2] = +sy;
  R.r[3] = +sx * sy * cz + cx * sz; R.r[4] = -sx * sy * sz + cx * cz; R.r[5] = -sx * cy;
  R.r[6] = -cx * sy * cz + sx * sz; R.r[7] = +cx * sy * sz + sx * cz; R.r[8] = +cx * cy;
  R.drx[0] = 0; R.drx[1] = 0; R.drx[2] = 0;
  R.drx[3] = +cx * sy * cz - sx * sz; R.drx[4] = -cx * sy * sz - sx * cz; R.drx[5] = -cx * cy;
  R.drx[6] = +sx * sy * cz + cx * sz; R.drx[7] = -sx * sy * sz + cx * cz; R.drx[8] = -sx * cy;
  R.dry[0] = -sy * cz; R.dry[1] = +sy * sz; R.dry[2] = +cy;
  R.dry[3] = +sx * cy * cz; R.dry[4] = -sx * cy * sz; R.dry[5] = +sx * sy;
  R.dry[6] = -cx * cy * cz; R.dry[7] = +cx * cy * sz; R.dry[8] = -cx * sy;
  R.drz[0] = -cy * sz; R.drz[1] = -cy * cz; R.drz[2] = 0;
  R.drz[3] = -sx * sy * sz + cx * cz; R.drz[4] = -sx * sy * cz - cx * sz; R.drz[5] = 0;
  R.drz[6] = +cx * sy * sz + sx * cz; R.drz[7] = +cx * sy * cz - sx * sz; R.drz[8] = 0;
}

struct EgoObs { double u1c, v1c, u2c, v2c, X, Y, Z; };

// prediction of one match under (R, t): p_predict of computeResidualsAndJacobian (src/viso_stereo.cpp:317-321)
VH_EGO_HD void ego_predict(const vh_ego_params &e, const EgoRot &R, const double tr[6], const EgoObs &o, double p[4],
                                            double &X1c, double &Y1c, double &Z1c) {
  X1c = R.r[0] * o.X + R.r[1] * o.Y + R.r[2] * o.Z + tr[3];
  Y1c = R.r[3] * o.X + R.r[4] * o.Y + R.r[5] * o.Z + tr[4];
  Z1c = R.r[6] * o.X + R.r[7] * o.Y + R.r[8] * o.Z + tr[5];
  const double X2c = X1c - e.base;
  p[0] = e.f * X1c / Z1c + e.cu;
  p[1] = e.f * Y1c / Z1c + e.cv;
  p[2] = e.f * X2c / Z1c + e.cu;
  p[3] = e.f * Y1c / Z1c + e.cv;
}

// One match as getInlier sees it under a motion of its own (kernels_inlier.hip): the 3-d point of the previous pair
// (src/viso_stereo.cpp:80-86) beside the current observation.  std::max(u1p - u2p, 0.0001f): a NaN difference stays NaN.
VH_EGO_HD EgoObs ego_observe(const vh_ego_params &e, float u1p, float v1p, float u2p, float u1c, float v1c, float u2c, float v2c) {
  const float df0 = u1p - u2p, df = df0 < 0.0001f ? 0.0001f : df0;
  const double d = (double)df;
  EgoObs o;
  o.X = (u1p - e.cu) * e.base / d;
  o.Y = (v1p - e.cv) * e.base / d;
  o.Z = e.f * e.base / d;
  o.u1c = u1c; o.v1c = v1c; o.u2c = u2c; o.v2c = v2c;
  return o;
}

// squared reprojection error test of getInlier (src/viso_stereo.cpp:171-174)
VH_EGO_HD bool ego_is_inlier(const vh_ego_params &e, const EgoRot &R, const double tr[6], const EgoObs &o) {
  double p[4], a, b, c;
  ego_predict(e, R, tr, o, p, a, b, c);
  const double d0 = o.u1c - p[0], d1 = o.v1c - p[1], d2 = o.u2c - p[2], d3 = o.v2c - p[3];
  return d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3 < e.inlier_threshold * e.inlier_threshold;
}

// Adds the four rows of one match to the normal equations: acc[0..20] = upper triangle of
// J^T J (row-major, m <= n), acc[21..26] = J^T r; rows in the reference's order (u1, v1, u2, v2).
// WITH_SSR (kernels_cov.hip): acc has 28 entries, acc[27] += the four squared weighted residuals, in that order.
template <bool WITH_SSR = false>
VH_EGO_HD void ego_accumulate(const vh_ego_params &e, const EgoRot &R, const double tr[6], const EgoObs &o, double *acc) {
  double p[4], X1c, Y1c, Z1c;
  ego_predict(e, R, tr, o, p, X1c, Y1c, Z1c);
  double weight = 1.0;
  if (e.reweighting) weight = 1.0 / (fabs(o.u1c - e.cu) / fabs(e.cu) + 0.05);
  const double X2c = X1c - e.base;
  double Jr[4][6];
#pragma unroll
  for (int32_t j = 0; j < 6; j++) {
    double X1cd, Y1cd, Z1cd;
    if (j == 0) { X1cd = 0; Y1cd = R.drx[3] * o.X + R.drx[4] * o.Y + R.drx[5] * o.Z; Z1cd = R.drx[6] * o.X + R.drx[7] * o.Y + R.drx[8] * o.Z; }
    else if (j == 1) { X1cd = R.dry[0] * o.X + R.dry[1] * o.Y + R.dry[2] * o.Z; Y1cd = R.dry[3] * o.X + R.dry[4] * o.Y + R.dry[5] * o.Z; Z1cd = R.dry[6] * o.X + R.dry[7] * o.Y + R.dry[8] * o.Z; }
    else if (j == 2) { X1cd = R.drz[0] * o.X + R.drz[1] * o.Y; Y1cd = R.drz[3] * o.X + R.drz[4] * o.Y; Z1cd = R.drz[6] * o.X + R.drz[7] * o.Y; }
    else { X1cd = j == 3 ? 1 : 0; Y1cd = j == 4 ? 1 : 0; Z1cd = j == 5 ? 1 : 0; }
    Jr[0][j] = weight * e.f * (X1cd * Z1c - X1c * Z1cd) / (Z1c * Z1c);
    Jr[1][j] = weight * e.f * (Y1cd * Z1c - Y1c * Z1cd) / (Z1c * Z1c);
    Jr[2][j] = weight * e.f * (X1cd * Z1c - X2c * Z1cd) / (Z1c * Z1c);
    Jr[3][j] = weight * e.f * (Y1cd * Z1c - Y1c * Z1cd) / (Z1c * Z1c);
  }
  const double obs[4] = {o.u1c, o.v1c, o.u2c, o.v2c};
#pragma unroll
  for (int32_t row = 0; row < 4; row++) {
    const double res = weight * (obs[row] - p[row]);
    int32_t k = 0;
#pragma unroll
    for (int32_t m = 0; m < 6; m++)
#pragma unroll
      for (int32_t n = m; n < 6; n++) acc[k++] += Jr[row][m] * Jr[row][n];
#pragma unroll
    for (int32_t m = 0; m < 6; m++) acc[21 + m] += Jr[row][m] * res;
    if (WITH_SSR) acc[27] += res * res;
  }
}

// Matrix::solve for the 6x6 normal equations: acc as produced by ego_accumulate is unpacked into the full symmetric
// matrix, vh_gauss_jordan.h does the rest; on success b = the solution.
VH_EGO_HD bool ego_solve(const double acc[27], double (&b)[6]) {
  double A[6][6];
  int32_t k = 0;
#pragma unroll
  for (int32_t m = 0; m < 6; m++)
#pragma unroll
    for (int32_t n = m; n < 6; n++) { A[m][n] = acc[k]; A[n][m] = acc[k]; k++; }
#pragma unroll
  for (int32_t m = 0; m < 6; m++) b[m] = acc[21 + m];
  return vh_gauss_jordan<6>(A, b);
}

#endif
