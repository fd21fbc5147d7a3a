// vh_mono_refine.h -- the arithmetic of the mono pose refinement, once: Gauss-Newton on the signed
// Sampson distance of every record over (R, unit t), five parameters -- a left rotation omega and two coordinates tau in
// the tangent plane of the unit sphere at t.  The reference has no counterpart; the contract is the project's own
// (include/viso_hip.h) and the test suite restates it in numpy, operation for operation:
//   mr_basis      B = (b0, b1) at t: m the first index of the smallest |t_m|, b0 = normalise(e_m - t_m t), b1 = t x b0
//   mr_uniforms   what is the same for every record of an update: E = [t]x R, E_k = [t]x [e_k]x R (omega_k),
//                 E_k = [b_k]x R (tau_k), B
//   mr_record     a record's two normalised positions
//   mr_residual   r = f n / sqrt(s) and the complete analytic J[5] (the derivative of 1 / sqrt(s) included)
//   mr_accumulate J^T J (15, upper triangle by rows), J^T r (5), r^2 (1)
//   mr_step       R <- Exp([omega]x) R by Rodrigues (I + [omega]x below |omega| = 1e-12), t <- normalise(t + tau0 b0 + tau1 b1)
//   mr_angle      the angle between two rotations / two unit vectors from the length of their difference
// Every sum is written with its brackets: built with -ffp-contract=off, every product and sum rounds on its own.  Only
// mr_step (sin) and mr_angle (asin) use the mathematical library.  No array is indexed by data (no private memory).
// Host and device, as vh_mono_pose.h: tests/cpp/mono_refine_check.cpp compiles this header for the host.
#ifndef VH_MONO_REFINE_H
#define VH_MONO_REFINE_H

#include <stdint.h>
#include <math.h>
#include "vh_rank2.h"  // VH_RANK2_D / _DI, matmul

namespace {

#define VH_MR_PARAMS 5
#define VH_MR_ACC 21       /* 15 of J^T J, 5 of J^T r, r^2 */
#define VH_MR_UNIFORMS 54  /* E[9], E_k[5][9] */

VH_RANK2_DI void mr_skew(double v0, double v1, double v2, double *S) {
  S[0] = 0.0; S[1] = -v2; S[2] = v1;
  S[3] = v2; S[4] = 0.0; S[5] = -v0;
  S[6] = -v1; S[7] = v0; S[8] = 0.0;
}

VH_RANK2_DI void mr_basis(const double *t, double *B) {
  int32_t m = 0;
  if (fabs(t[1]) < fabs(t[0])) m = 1;
  if (fabs(t[2]) < fabs(m == 0 ? t[0] : t[1])) m = 2;
  const double tm = m == 0 ? t[0] : (m == 1 ? t[1] : t[2]);
  double v[3];
  for (int32_t q = 0; q < 3; q++) v[q] = (q == m ? 1.0 : 0.0) - tm * t[q];
  const double nv = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  for (int32_t q = 0; q < 3; q++) B[q] = v[q] / nv;
  B[3] = t[1] * B[2] - t[2] * B[1];
  B[4] = t[2] * B[0] - t[0] * B[2];
  B[5] = t[0] * B[1] - t[1] * B[0];
}

// U[0..8] = E, U[9 + 9 k ..] = E_k in the order of the parameters; B[6]
VH_RANK2_DI void mr_uniforms(const double *R, const double *t, double *U, double *B) {
  double T[9], G[9], GR[9];
  mr_skew(t[0], t[1], t[2], T);
  matmul(T, 3, 3, R, 3, U);
  for (int32_t k = 0; k < 3; k++) {
    mr_skew(k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, G);
    matmul(G, 3, 3, R, 3, GR);  // (exact: a signed selection of R's rows)
    matmul(T, 3, 3, GR, 3, U + 9 + 9 * k);
  }
  mr_basis(t, B);
  for (int32_t k = 0; k < 2; k++) {
    mr_skew(B[3 * k], B[3 * k + 1], B[3 * k + 2], G);
    matmul(G, 3, 3, R, 3, U + 36 + 9 * k);
  }
}

struct MrRecord { double xp0, xp1, xc0, xc1; };
VH_RANK2_DI MrRecord mr_record(double f, double cu, double cv, float u1p, float v1p, float u1c, float v1c) {
  MrRecord x;
  x.xp0 = ((double)u1p - cu) / f; x.xp1 = ((double)v1p - cv) / f;
  x.xc0 = ((double)u1c - cu) / f; x.xc1 = ((double)v1c - cv) / f;
  return x;
}

// n = xc^T M xp, a = M xp (rows 0, 1), b = M^T xc (rows 0, 1); the third coordinates are 1
VH_RANK2_DI void mr_forms(const double *M, const MrRecord &x, double &n, double &a0, double &a1, double &b0, double &b1) {
  a0 = (M[0] * x.xp0 + M[1] * x.xp1) + M[2];
  a1 = (M[3] * x.xp0 + M[4] * x.xp1) + M[5];
  const double a2 = (M[6] * x.xp0 + M[7] * x.xp1) + M[8];
  b0 = (M[0] * x.xc0 + M[3] * x.xc1) + M[6];
  b1 = (M[1] * x.xc0 + M[4] * x.xc1) + M[7];
  n = (x.xc0 * a0 + x.xc1 * a1) + a2;
}

VH_RANK2_DI void mr_residual(double f, const double *U, const MrRecord &x, double &r, double *J) {
  double n, a0, a1, b0, b1;
  mr_forms(U, x, n, a0, a1, b0, b1);
  const double s = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
  const double q = sqrt(s);
  r = (f * n) / q;
  const double den = (2.0 * s) * q;
#pragma unroll
  for (int32_t k = 0; k < VH_MR_PARAMS; k++) {
    double dn, da0, da1, db0, db1;
    mr_forms(U + 9 + 9 * k, x, dn, da0, da1, db0, db1);
    const double ds = 2.0 * (((a0 * da0 + a1 * da1) + b0 * db0) + b1 * db1);
    J[k] = f * (dn / q - (n * ds) / den);
  }
}

VH_RANK2_DI void mr_accumulate(double r, const double *J, double *acc) {
  int32_t k = 0;
#pragma unroll
  for (int32_t i = 0; i < VH_MR_PARAMS; i++)
#pragma unroll
    for (int32_t j = i; j < VH_MR_PARAMS; j++) acc[k++] += J[i] * J[j];
#pragma unroll
  for (int32_t i = 0; i < VH_MR_PARAMS; i++) acc[15 + i] += J[i] * r;
  acc[20] += r * r;
}

// delta = (omega[3], tau[2]); R [9] and t [3] are stepped in place
VH_RANK2_DI void mr_step(const double *delta, double *R, double *t) {
  const double w0 = delta[0], w1 = delta[1], w2 = delta[2];
  const double th2 = (w0 * w0 + w1 * w1) + w2 * w2, th = sqrt(th2);
  double W[9], X[9], Rn[9];
  mr_skew(w0, w1, w2, W);
  if (th < 1e-12) {
    for (int32_t q = 0; q < 9; q++) X[q] = (q % 4 == 0 ? 1.0 : 0.0) + W[q];
  } else {
    double W2[9];
    matmul(W, 3, 3, W, 3, W2);
    const double h = sin(0.5 * th);
    const double ca = sin(th) / th, cb = (2.0 * (h * h)) / th2;  // (1 - cos th) / th^2 without the cancellation
    for (int32_t q = 0; q < 9; q++) X[q] = ((q % 4 == 0 ? 1.0 : 0.0) + ca * W[q]) + cb * W2[q];
  }
  matmul(X, 3, 3, R, 3, Rn);
  for (int32_t q = 0; q < 9; q++) R[q] = Rn[q];
  double B[6], u[3];
  mr_basis(t, B);
  for (int32_t q = 0; q < 3; q++) u[q] = (t[q] + delta[3] * B[q]) + delta[4] * B[3 + q];
  const double nu = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  for (int32_t q = 0; q < 3; q++) t[q] = u[q] / nu;
}

// 2 asin(|a - b| / chord), chord = 2 sqrt 2 for two rotations (n = 9), 2 for two unit vectors (n = 3)
VH_RANK2_DI double mr_angle(const double *a, const double *b, int32_t n) {
  double d2 = 0.0;
  for (int32_t q = 0; q < n; q++) { const double d = a[q] - b[q]; d2 += d * d; }
  const double chord = n == 9 ? 2.0 * sqrt(2.0) : 2.0;
  return 2.0 * asin(fmin(1.0, sqrt(d2) / chord));
}

}  // namespace

#endif
