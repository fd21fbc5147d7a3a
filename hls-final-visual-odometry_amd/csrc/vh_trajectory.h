// vh_trajectory.h -- the rule of the trajectory, once (include/viso_hip.h): one row's
// T = transformationVectorToMatrix(tr), Tinv = Matrix::inv(T), its status, what a not accepted row does under either
// policy, and one element of P * Tinv.  kernels_trajectory.hip includes it, built with -ffp-contract=off, so every product
// and sum rounds on its own as on the reference's x86 build; tests/cpp/trajectory_check.cpp compiles it for the host.
#ifndef VH_TRAJECTORY_H
#define VH_TRAJECTORY_H

#include "vh_ego.h"

// rows of a chain one round of trajectory_kernel takes: phase A's lanes, the rows whose Tinv lie in LDS at a time
#define VH_TRAJ_ROUND 256

#define VH_TRAJ_ACCEPTED  0
#define VH_TRAJ_NOT_OK    1
#define VH_TRAJ_NONFINITE 2
#define VH_TRAJ_REFUSED   3
#define VH_TRAJ_NO_PAIR   4

VH_EGO_HD bool traj_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)

// Steps 1 - 3 for one row: Tinv (row-major; defined where the status is 0) and the status.  Matrix::inv is B = eye(4);
// B.solve(T): the register form of the elimination with the four unit right-hand sides at once (vh_gauss_jordan.h), the
// pivot search done once; nothing leaves the registers.
VH_EGO_HD int32_t traj_inverse(const double tr[6], int32_t ok, double (&Tinv)[16]) {
#pragma unroll
  for (int32_t q = 0; q < 16; q++) Tinv[q] = 0.0;
  if (ok < 0) return VH_TRAJ_NO_PAIR;
  if (ok == 0) return VH_TRAJ_NOT_OK;
  bool fin = true;
#pragma unroll
  for (int32_t q = 0; q < 6; q++) fin = fin && traj_finite(tr[q]);
  if (!fin) return VH_TRAJ_NONFINITE;
  EgoRot R;
  ego_rot(tr, R);
  double A[4][4], B[4][4];
#pragma unroll
  for (int32_t i = 0; i < 3; i++) {
    A[i][0] = R.r[3 * i + 0]; A[i][1] = R.r[3 * i + 1]; A[i][2] = R.r[3 * i + 2]; A[i][3] = tr[3 + i];
  }
  A[3][0] = 0.0; A[3][1] = 0.0; A[3][2] = 0.0; A[3][3] = 1.0;
#pragma unroll
  for (int32_t i = 0; i < 4; i++)
#pragma unroll
    for (int32_t j = 0; j < 4; j++) B[i][j] = i == j ? 1.0 : 0.0;
  const bool solved = vh_gauss_jordan_nb<4, 4>(A, B);
#pragma unroll
  for (int32_t i = 0; i < 4; i++)
#pragma unroll
    for (int32_t j = 0; j < 4; j++) Tinv[4 * i + j] = B[i][j];
  if (!solved) return VH_TRAJ_REFUSED;
#pragma unroll
  for (int32_t q = 0; q < 16; q++) fin = fin && traj_finite(Tinv[q]);
  return fin ? VH_TRAJ_ACCEPTED : VH_TRAJ_NONFINITE;
}

// Step 4's choice for a row of `status`: 1 multiply by the row's own Tinv (which becomes the last accepted one, step + 1),
// 2 multiply by the last accepted Tinv again, 0 hold.
VH_EGO_HD int32_t traj_action(int32_t status, int32_t on_fail, int32_t has_tinv) {
  if (status == VH_TRAJ_ACCEPTED) return 1;
  if (status != VH_TRAJ_NO_PAIR && on_fail == VH_TRAJ_REPEAT && has_tinv) return 2;
  return 0;
}

// Element (i, j) of P * M as Matrix::operator* forms it: prow = P[i][0..3], mcol = M[0..3][j]
VH_EGO_HD double traj_dot(const double prow[4], const double mcol[4]) {
  double c = 0.0;
#pragma unroll
  for (int32_t k = 0; k < 4; k++) c += prow[k] * mcol[k];
  return c;
}

#endif
