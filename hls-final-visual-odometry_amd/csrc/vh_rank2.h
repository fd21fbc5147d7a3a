// vh_rank2.h -- the rank-2 step of fundamentalMatrix on a 3x3, once: kernels_mono.hip (every hypothesis, the estimator's
// refit, the essential matrix), kernels_mono_refit.hip (the refit on whole lists) and kernels_mono_pose.hip (the pose tail
// on whole lists) include it; all are built with -ffp-contract=off.  Host and device, as vh_mono.h:
// tests/cpp/mono_pose_check.cpp compiles it for the host.
#ifndef VH_RANK2_H
#define VH_RANK2_H

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#ifndef SVD_HD
#define SVD_HD __device__ __forceinline__
#endif
#define VH_RANK2_D __device__
#define VH_RANK2_DI __device__ __forceinline__
#else
#define VH_RANK2_D inline
#define VH_RANK2_DI inline
#endif
#include "svd_static.h"

namespace {

// C = A (ma x na) * B (na x nb): Matrix::operator* (src/matrix.cpp:263-277), sums from 0, k ascending
VH_RANK2_D void matmul(const double *A, int ma, int na, const double *B, int nb, double *C) {
  for (int i = 0; i < ma; i++)
    for (int j = 0; j < nb; j++) {
      double c = 0.0;
      for (int k = 0; k < na; k++) c += A[i * na + k] * B[k * nb + j];
      C[i * nb + j] = c;
    }
}
// Matrix::svd of a 3x3 followed by U * diag(W with W[2] = 0) * ~V (src/viso_mono.cpp:262-265, :91-94).
// The factors live in registers (svd_static.h: every index static after unrolling).
// (returns svd_static's zero-pivot flag, see fundamental8)
VH_RANK2_DI bool rank2_3x3(const double *M, double *out) {
  double U[3][3], w[3], V[3][3], a[9], D[9], UD[9], Vt[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) U[i][j] = M[i * 3 + j];
  const bool zero_pivot = svd_static<3, 3>(U, w, V);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { a[i * 3 + j] = U[i][j]; Vt[j * 3 + i] = V[i][j]; D[i * 3 + j] = 0.0; }
  D[0] = w[0]; D[4] = w[1]; D[8] = 0.0;
  matmul(a, 3, 3, D, 3, UD);
  matmul(UD, 3, 3, Vt, 3, out);
  return zero_pivot;
}

}  // namespace

#endif
