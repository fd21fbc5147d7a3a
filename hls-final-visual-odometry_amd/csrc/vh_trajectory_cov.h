// vh_trajectory_cov.h -- the rule of the pose covariance, once (include/viso_hip.h): one row's
// Ad and Q = G C G^T, whether the row has a covariance of its own, and one element of the two products of
// Sigma' = Ad (Sigma + Q) Ad^T.  kernels_trajectory_cov.hip includes it, built with -ffp-contract=off, so every product and
// sum rounds on its own; tests/cpp/trajectory_cov_check.cpp compiles it for the host.  Which rows step is vh_trajectory.h's
// traj_inverse / traj_action.
#ifndef VH_TRAJECTORY_COV_H
#define VH_TRAJECTORY_COV_H

#include "vh_trajectory.h"

// rows of a chain one round of trajectory_cov_kernel takes: 39 doubles of a row lie in LDS, 128 rows are 39 KiB
#define VH_TRAJ_COV_ROUND 128
// the distinct entries of Ad: R row-major, then [t]x R row-major; entry 18 stands for Ad's zeros
#define VH_TRAJ_COV_AD 18
// the upper triangle of Q, row-major (i <= j)
#define VH_TRAJ_COV_Q 21

// where element (i, j) of a symmetric 6x6 lies in its packed upper triangle
VH_EGO_HD int32_t traj_cov_sym(int32_t i, int32_t j) {
  const int32_t a = i < j ? i : j, b = i < j ? j : i;
  return 6 * a - a * (a - 1) / 2 + (b - a);
}

// where element (r, c) of Ad = [[R, 0], [[t]x R, R]] lies among the VH_TRAJ_COV_AD packed entries (18: a zero)
VH_EGO_HD int32_t traj_cov_ad_index(int32_t r, int32_t c) {
  if (r < 3) return c < 3 ? 3 * r + c : VH_TRAJ_COV_AD;
  return c < 3 ? 9 + 3 * (r - 3) + c : 3 * (r - 3) + (c - 3);
}

// Steps 1 - 3 for one row that is accepted: Ad (packed), Q (packed) -> 1 where the row has a covariance of its own
// (ok_cov != 0, C and Q finite).  G: column k of the upper-left block is vee(R^T dR_k), the lower-right block is R^T.
VH_EGO_HD int32_t traj_cov_row(const double tr[6], const double C[36], int32_t ok_cov, double (&Ad)[VH_TRAJ_COV_AD], double (&Q)[VH_TRAJ_COV_Q]) {
  EgoRot R;
  ego_rot(tr, R);
  double G[6][6];
#pragma unroll
  for (int32_t i = 0; i < 6; i++)
#pragma unroll
    for (int32_t j = 0; j < 6; j++) G[i][j] = 0.0;
#pragma unroll
  for (int32_t k = 0; k < 3; k++) {
    const double *dR = k == 0 ? R.drx : k == 1 ? R.dry : R.drz;
    // W = R^T dR: W[a][b] = sum_m R[m][a] * dR[m][b]; vee(W) = (W[2][1], W[0][2], W[1][0])
    double w21 = 0.0, w02 = 0.0, w10 = 0.0;
#pragma unroll
    for (int32_t m = 0; m < 3; m++) {
      w21 += R.r[3 * m + 2] * dR[3 * m + 1];
      w02 += R.r[3 * m + 0] * dR[3 * m + 2];
      w10 += R.r[3 * m + 1] * dR[3 * m + 0];
    }
    G[0][k] = w21; G[1][k] = w02; G[2][k] = w10;
  }
#pragma unroll
  for (int32_t a = 0; a < 3; a++)
#pragma unroll
    for (int32_t b = 0; b < 3; b++) G[3 + a][3 + b] = R.r[3 * b + a];
  bool fin = true;
#pragma unroll
  for (int32_t q = 0; q < 36; q++) fin = fin && traj_finite(C[q]);
  // Q = G C G^T: a row of W = G C in full, then the row's entries of the upper triangle
#pragma unroll
  for (int32_t i = 0; i < 6; i++) {
    double W[6];
#pragma unroll
    for (int32_t j = 0; j < 6; j++) {
      double c = 0.0;
#pragma unroll
      for (int32_t k = 0; k < 6; k++) c += G[i][k] * C[6 * k + j];
      W[j] = c;
    }
#pragma unroll
    for (int32_t j = i; j < 6; j++) {
      double c = 0.0;
#pragma unroll
      for (int32_t k = 0; k < 6; k++) c += W[k] * G[j][k];
      Q[traj_cov_sym(i, j)] = c;
      fin = fin && traj_finite(c);
    }
  }
  // Ad: R, and [t]x R with c = 0; c += [t]x[i][m] * R[m][j]
  const double tx[3][3] = {{0.0, -tr[5], tr[4]}, {tr[5], 0.0, -tr[3]}, {-tr[4], tr[3], 0.0}};
#pragma unroll
  for (int32_t q = 0; q < 9; q++) Ad[q] = R.r[q];
#pragma unroll
  for (int32_t i = 0; i < 3; i++)
#pragma unroll
    for (int32_t j = 0; j < 3; j++) {
      double c = 0.0;
#pragma unroll
      for (int32_t m = 0; m < 3; m++) c += tx[i][m] * R.r[3 * m + j];
      Ad[9 + 3 * i + j] = c;
    }
  return ok_cov != 0 && fin ? 1 : 0;
}

// One element of either product of step 4: c = 0; c += a[k] * b[k], k = 0..5, all six terms
VH_EGO_HD double traj_cov_dot(const double a[6], const double b[6]) {
  double c = 0.0;
#pragma unroll
  for (int32_t k = 0; k < 6; k++) c += a[k] * b[k];
  return c;
}

#endif
