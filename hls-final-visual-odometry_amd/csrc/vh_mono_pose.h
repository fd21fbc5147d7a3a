// vh_mono_pose.h -- the pieces of VisualOdometryMono's pose tail (reference src/viso_mono.cpp:83-158, :317-399), once:
// F out of the normalised frame and the essential matrix, EtoRt's four (R, t) candidates with their projection
// matrices, triangulateChieral's linear triangulation of one record, the point in front and its two coordinates, and
// the six motion parameters.  kernels_mono_pose.hip (the tail laid out for whole lists) is built from all of it;
// kernels_mono.hip (the estimator's tail on a bucketed list) takes transpose3 and det3 from here.  The other functions
// RESTATE what mono_final_a, mono_tri and mono_final_c hold inline, statement for statement: calling them from those
// kernels changed the instructions the compiler emits for them (LDS addressing and scheduling of mono_final_a and
// mono_final_c, 27 lines of mono_tri: DESIGN.md section 4.17), so those kernels keep their text -- a change to either
// copy is a change to both, and tests/test_mono_pose.py holds the two to each other on the device.  Both files are built
// with -ffp-contract=off, so every product and sum rounds on its own as on the reference's x86 build.
// Host and device, as vh_mono.h: tests/cpp/mono_pose_check.cpp compiles this header for the host.
#ifndef VH_MONO_POSE_H
#define VH_MONO_POSE_H

#include <stdint.h>
#include <math.h>
#include "vh_rank2.h"  // matmul, rank2_3x3, svd_static.h

namespace {

VH_RANK2_D void transpose3(const double *A, double *T) {
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T[j * 3 + i] = A[i * 3 + j];
}
// Matrix::det of a 3x3 (src/matrix.cpp:400-415) over Matrix::lu (:514-572)
VH_RANK2_D double det3(const double *M) {
  double a[3][3], vv[3], big, dum, sum, temp, d = 1.0;
  int imax = 0;
  bool ok = true;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) a[i][j] = M[i * 3 + j];
  for (int i = 0; i < 3 && ok; i++) {
    big = 0.0;
    for (int j = 0; j < 3; j++) if ((temp = fabs(a[i][j])) > big) big = temp;
    if (big == 0.0) { ok = false; break; }
    vv[i] = 1.0 / big;
  }
  if (ok)
    for (int j = 0; j < 3; j++) {
      for (int i = 0; i < j; i++) {
        sum = a[i][j];
        for (int k = 0; k < i; k++) sum -= a[i][k] * a[k][j];
        a[i][j] = sum;
      }
      big = 0.0;
      for (int i = j; i < 3; i++) {
        sum = a[i][j];
        for (int k = 0; k < j; k++) sum -= a[i][k] * a[k][j];
        a[i][j] = sum;
        if ((dum = vv[i] * fabs(sum)) >= big) { big = dum; imax = i; }
      }
      if (j != imax) {
        for (int k = 0; k < 3; k++) { dum = a[imax][k]; a[imax][k] = a[j][k]; a[j][k] = dum; }
        d = -d;
        vv[imax] = vv[j];
      }
      if (j != 2) {
        dum = 1.0 / a[j][j];
        for (int i = j + 1; i < 3; i++) a[i][j] *= dum;
      }
    }
  for (int i = 0; i < 3; i++) d *= a[i][i];
  return d;
}

// F (normalised frame, in place) -> ~Tc*F*Tp, E = ~K*F*K, rank 2 again (src/viso_mono.cpp:83-94).  Tp, Tc: the
// matrices of normalizeFeaturePoints (:226-227), K = {f, 0, cu, 0, f, cv, 0, 0, 1}.
VH_RANK2_DI void mono_pose_essential(const double *Tp, const double *Tc, const double *K, double *F, double *E) {
  double T1[9], T2[9], Kt[9];
  transpose3(Tc, T1); matmul(T1, 3, 3, F, 3, T2); matmul(T2, 3, 3, Tp, 3, F);
  transpose3(K, Kt); matmul(Kt, 3, 3, F, 3, T2); matmul(T2, 3, 3, K, 3, E);
  rank2_3x3(E, T1);
  for (int32_t q = 0; q < 9; q++) E[q] = T1[q];
}

// EtoRt (src/viso_mono.cpp:317-346) and the projection matrices of triangulateChieral (:370-375): Ra[9], Rb[9], t0[3];
// P1[12] = [K | 0]; P2[4][12] of the candidates (Ra, t0), (Ra, -t0), (Rb, t0), (Rb, -t0).
VH_RANK2_DI void mono_pose_candidates(const double *E, const double *K, double *Ra, double *Rb, double *t0, double *P1, double *P2) {
  const double Wm[9] = {0, -1, 0, +1, 0, 0, 0, 0, 1}, Zm[9] = {0, +1, 0, -1, 0, 0, 0, 0, 0};
  double U[9], V[9], Ut[9], Vt[9], Wt[9], T[9], T1[9];
  {
    double Ur[3][3], Sr[3], Vr[3][3];
#pragma unroll
    for (int32_t i = 0; i < 3; i++)
#pragma unroll
      for (int32_t q = 0; q < 3; q++) Ur[i][q] = E[i * 3 + q];
    svd_static<3, 3>(Ur, Sr, Vr);
#pragma unroll
    for (int32_t i = 0; i < 3; i++)
#pragma unroll
      for (int32_t q = 0; q < 3; q++) { U[i * 3 + q] = Ur[i][q]; V[i * 3 + q] = Vr[i][q]; }
  }
  transpose3(U, Ut); transpose3(V, Vt); transpose3(Wm, Wt);
  matmul(U, 3, 3, Zm, 3, T1); matmul(T1, 3, 3, Ut, 3, T);
  matmul(U, 3, 3, Wm, 3, T1); matmul(T1, 3, 3, Vt, 3, Ra);
  matmul(U, 3, 3, Wt, 3, T1); matmul(T1, 3, 3, Vt, 3, Rb);
  t0[0] = T[2 * 3 + 1]; t0[1] = T[0 * 3 + 2]; t0[2] = T[1 * 3 + 0];
  if (det3(Ra) < 0) for (int32_t q = 0; q < 9; q++) Ra[q] = -Ra[q];
  if (det3(Rb) < 0) for (int32_t q = 0; q < 9; q++) Rb[q] = -Rb[q];
  for (int32_t i = 0; i < 3; i++) for (int32_t j = 0; j < 4; j++) P1[i * 4 + j] = j < 3 ? K[i * 3 + j] : 0.0;
  for (int32_t c = 0; c < 4; c++) {
    const double *R = c < 2 ? Ra : Rb;
    double Rt[12];
    for (int32_t i = 0; i < 3; i++) { for (int32_t j = 0; j < 3; j++) Rt[i * 4 + j] = R[i * 3 + j]; Rt[i * 4 + 3] = (c & 1) ? -t0[i] : t0[i]; }
    matmul(K, 3, 3, Rt, 4, P2 + 12 * c);
  }
}

// triangulateChieral's linear triangulation of one record (src/viso_mono.cpp:378-387): the direction of the smallest
// singular value of the 4x4 system, up to sign (no U: svd_static.h) -- every use of it is a quotient or a product of two
// components, the same for x and -x.  The record's float fields are widened to double by the products.
VH_RANK2_DI void mono_pose_triangulate(const double *P1, const double *P2, float u1p, float v1p, float u1c, float v1c, double (&x)[4]) {
  double J[4][4], w4[4], V4[4][4];
#pragma unroll
  for (int32_t j = 0; j < 4; j++) {
    J[0][j] = P1[2 * 4 + j] * u1p - P1[0 * 4 + j];
    J[1][j] = P1[2 * 4 + j] * v1p - P1[1 * 4 + j];
    J[2][j] = P2[2 * 4 + j] * u1c - P2[0 * 4 + j];
    J[3][j] = P2[2 * 4 + j] * v1c - P2[1 * 4 + j];
  }
  svd_static_last_v_unsigned<4, 4>(J, w4, V4, x);
}
// ... and its test: in front of both cameras (:389-396)
VH_RANK2_DI bool mono_pose_in_front_of_both(const double *P1, const double *P2, const double (&x)[4]) {
  double a = 0.0, b = 0.0;
  for (int32_t j = 0; j < 4; j++) a += P1[2 * 4 + j] * x[j];
  for (int32_t j = 0; j < 4; j++) b += P2[2 * 4 + j] * x[j];
  return a * x[3] > 0 && b * x[3] > 0;
}

// the winner of the four chirality counts: the first with the strictly largest (src/viso_mono.cpp:353), -1 where none is positive
VH_RANK2_DI int32_t mono_pose_winner(const int32_t *cnt) {
  int32_t cbest = -1, max_in = 0;
  for (int32_t c = 0; c < 4; c++) if (cnt[c] > max_in) { max_in = cnt[c]; cbest = c; }
  return cbest;
}

// X / X(3,:) of one point (src/viso_mono.cpp:100); a zero w gives the zero point
VH_RANK2_DI void mono_pose_point(double X0, double X1, double X2, double wq, double &x, double &y, double &z) {
  x = 0; y = 0; z = 0;
  if (wq != 0) { x = X0 / wq; y = X1 / wq; z = X2 / wq; }
}
// the L1 distance of a point in front (:108) and its ground-plane coordinate ~n * x_plane, n = (cos(-pitch), sin(-pitch)) (:125-128)
VH_RANK2_DI double mono_pose_dist(double x, double y, double z) { return fabs(x) + fabs(y) + fabs(z); }
VH_RANK2_DI double mono_pose_plane(double n0, double n1, double y, double z) {
  double dd = 0.0;
  dd += n0 * y; dd += n1 * z;
  return dd;
}

// The six motion parameters (src/viso_mono.cpp:143-158) from the winning rotation R, the unsigned translation t0 with
// the candidate's sign, the camera height and the plane's coordinate dref.
VH_RANK2_DI void mono_pose_tr(const double *R, const double *t0, int32_t cbest, double height, double dref, double *tr) {
  double t[3];
  for (int32_t q = 0; q < 3; q++) { const double tq = (cbest & 1) ? -t0[q] : t0[q]; t[q] = (tq * height) / dref; }
  const double ry = asin(R[0 * 3 + 2]);
  tr[0] = asin(-R[1 * 3 + 2] / cos(ry));
  tr[1] = ry;
  tr[2] = asin(-R[0 * 3 + 1] / cos(ry));
  tr[3] = t[0]; tr[4] = t[1]; tr[5] = t[2];
}

}  // namespace

#endif
