// vh_gauss_jordan.h -- Matrix::solve (reference src/matrix.cpp:417-504) for an N x N system with one right-hand side:
// Gauss-Jordan elimination with full pivoting, singular below 1e-20.  On success b holds the solution (A is destroyed).
//
// Every array index is a compile-time constant after unrolling -- the pivot's row and column (data-dependent in the
// original) select among the N rows / columns by predicates -- so the system lives in registers: with dynamic indices
// the 6x6 system of the stereo estimator sat in private memory, and the 22 dependent solves of a hypothesis were 85 %
// of ego_kernel (1.2 of 1.4 ms per batch of bucketed lists, tools/ego_phases.py).  The arithmetic applied to the
// elements, and its order, are the original's.  A is the full matrix (the reference fills all N * N entries).
//
// irow / icol are declared outside the loop over the pivots, where the original declares them (src/matrix.cpp:435):
// a pivot search selects an entry whenever it looks at one that is not NaN (`>= big` with big = 0), so they keep a
// value from the pivot before only when every candidate entry of a step is NaN -- and then the original reuses it.
// (Its first step would read them uninitialised; here they start at 0.)
//
// Host and device: SVD_HD as in svd_static.h (tests/cpp/gauss_jordan_check.cpp compiles this header for the host).
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef SVD_HD
#define SVD_HD inline
#endif

template <int N> SVD_HD bool vh_gauss_jordan(double (&A)[N][N], double (&b)[N]) {
  int32_t ipiv[N];
#pragma unroll
  for (int32_t q = 0; q < N; q++) ipiv[q] = 0;
  int32_t irow = 0, icol = 0;
#pragma unroll
  for (int32_t i = 0; i < N; i++) {
    double big = 0.0;
#pragma unroll
    for (int32_t j = 0; j < N; j++)
#pragma unroll
      for (int32_t k = 0; k < N; k++) {
        const double v = fabs(A[j][k]);
        if (ipiv[j] != 1 && ipiv[k] == 0 && v >= big) { big = v; irow = j; icol = k; }
      }
#pragma unroll
    for (int32_t q = 0; q < N; q++) ipiv[q] += q == icol ? 1 : 0;
    // rows irow and icol change places (nothing moves when they are the same row)
    double ri[N], rc[N], bi = 0.0, bc = 0.0;
#pragma unroll
    for (int32_t l = 0; l < N; l++) { ri[l] = 0.0; rc[l] = 0.0; }
#pragma unroll
    for (int32_t r = 0; r < N; r++) {
#pragma unroll
      for (int32_t l = 0; l < N; l++) { ri[l] = r == irow ? A[r][l] : ri[l]; rc[l] = r == icol ? A[r][l] : rc[l]; }
      bi = r == irow ? b[r] : bi; bc = r == icol ? b[r] : bc;
    }
#pragma unroll
    for (int32_t r = 0; r < N; r++) {
#pragma unroll
      for (int32_t l = 0; l < N; l++) A[r][l] = r == icol ? ri[l] : (r == irow ? rc[l] : A[r][l]);
      b[r] = r == icol ? bi : (r == irow ? bc : b[r]);
    }
    // the pivot row (now row icol) is ri, its right-hand side bi
    double piv = 0.0;
#pragma unroll
    for (int32_t l = 0; l < N; l++) piv = l == icol ? ri[l] : piv;
    if (fabs(piv) < 1e-20) return false;
    const double pivinv = 1.0 / piv;
#pragma unroll
    for (int32_t l = 0; l < N; l++) ri[l] = (l == icol ? 1.0 : ri[l]) * pivinv;
    bi *= pivinv;
#pragma unroll
    for (int32_t ll = 0; ll < N; ll++) {
      double dum = 0.0;
#pragma unroll
      for (int32_t l = 0; l < N; l++) dum = l == icol ? A[ll][l] : dum;
      const bool prow = ll == icol;
#pragma unroll
      for (int32_t l = 0; l < N; l++) {
        const double cur = l == icol ? 0.0 : A[ll][l];
        A[ll][l] = prow ? ri[l] : cur - ri[l] * dum;
      }
      b[ll] = prow ? bi : b[ll] - bi * dum;
    }
  }
  return true;
}

// The register form with NB right-hand sides: B [N][NB], column q being a right-hand side of its own; on success B holds
// the solutions (the inverse, for the unit matrix).  The pivot search, the exchange and the elimination of A run once;
// what is applied to a column of B is what the form above applies to b, so a column equals that right-hand side solved
// alone, bit for bit.  A function of its own: the form above is untouched by it.  (vh_trajectory.h: the 4x4 inverse.)
template <int N, int NB> SVD_HD bool vh_gauss_jordan_nb(double (&A)[N][N], double (&B)[N][NB]) {
  int32_t ipiv[N];
#pragma unroll
  for (int32_t q = 0; q < N; q++) ipiv[q] = 0;
  int32_t irow = 0, icol = 0;
#pragma unroll
  for (int32_t i = 0; i < N; i++) {
    double big = 0.0;
#pragma unroll
    for (int32_t j = 0; j < N; j++)
#pragma unroll
      for (int32_t k = 0; k < N; k++) {
        const double v = fabs(A[j][k]);
        if (ipiv[j] != 1 && ipiv[k] == 0 && v >= big) { big = v; irow = j; icol = k; }
      }
#pragma unroll
    for (int32_t q = 0; q < N; q++) ipiv[q] += q == icol ? 1 : 0;
    double ri[N], rc[N], bi[NB], bc[NB];
#pragma unroll
    for (int32_t l = 0; l < N; l++) { ri[l] = 0.0; rc[l] = 0.0; }
#pragma unroll
    for (int32_t q = 0; q < NB; q++) { bi[q] = 0.0; bc[q] = 0.0; }
#pragma unroll
    for (int32_t r = 0; r < N; r++) {
#pragma unroll
      for (int32_t l = 0; l < N; l++) { ri[l] = r == irow ? A[r][l] : ri[l]; rc[l] = r == icol ? A[r][l] : rc[l]; }
#pragma unroll
      for (int32_t q = 0; q < NB; q++) { bi[q] = r == irow ? B[r][q] : bi[q]; bc[q] = r == icol ? B[r][q] : bc[q]; }
    }
#pragma unroll
    for (int32_t r = 0; r < N; r++) {
#pragma unroll
      for (int32_t l = 0; l < N; l++) A[r][l] = r == icol ? ri[l] : (r == irow ? rc[l] : A[r][l]);
#pragma unroll
      for (int32_t q = 0; q < NB; q++) B[r][q] = r == icol ? bi[q] : (r == irow ? bc[q] : B[r][q]);
    }
    double piv = 0.0;
#pragma unroll
    for (int32_t l = 0; l < N; l++) piv = l == icol ? ri[l] : piv;
    if (fabs(piv) < 1e-20) return false;
    const double pivinv = 1.0 / piv;
#pragma unroll
    for (int32_t l = 0; l < N; l++) ri[l] = (l == icol ? 1.0 : ri[l]) * pivinv;
#pragma unroll
    for (int32_t q = 0; q < NB; q++) bi[q] *= pivinv;
#pragma unroll
    for (int32_t ll = 0; ll < N; ll++) {
      double dum = 0.0;
#pragma unroll
      for (int32_t l = 0; l < N; l++) dum = l == icol ? A[ll][l] : dum;
      const bool prow = ll == icol;
#pragma unroll
      for (int32_t l = 0; l < N; l++) {
        const double cur = l == icol ? 0.0 : A[ll][l];
        A[ll][l] = prow ? ri[l] : cur - ri[l] * dum;
      }
#pragma unroll
      for (int32_t q = 0; q < NB; q++) B[ll][q] = prow ? bi[q] : B[ll][q] - bi[q] * dum;
    }
  }
  return true;
}

// The same elimination with NB right-hand sides, on arrays in addressable memory: A [N][N] and B [N][NB], row-major,
// both changed in place; on success B holds the solutions (the inverse, for the unit matrix).  The pivot's row and
// column index the arrays as they do in the original, so this is for memory where a data-dependent index is free -- the
// LDS of kernels_cov.hip, the host -- and not for private arrays (see above).  A function of its own: the register
// form above is untouched by it.  The pivot rule, irow / icol and the arithmetic on every element are those above, so a
// column of B equals the single right-hand side solved alone, bit for bit.
template <int N, int NB> SVD_HD bool vh_gauss_jordan_mem(double *__restrict__ A, double *__restrict__ B) {
  static_assert(N <= 8, "ipiv packs a 4-bit count per column");
  uint32_t ipiv = 0;  // nibble q: how often column q was chosen (ipiv[q] above; more than once only when every candidate of a step is NaN)
  int32_t irow = 0, icol = 0;
  for (int32_t i = 0; i < N; i++) {
    double big = 0.0;
    for (int32_t j = 0; j < N; j++)
      for (int32_t k = 0; k < N; k++) {
        const double v = fabs(A[N * j + k]);
        if (((ipiv >> (4 * j)) & 15u) != 1u && ((ipiv >> (4 * k)) & 15u) == 0u && v >= big) { big = v; irow = j; icol = k; }
      }
    ipiv += 1u << (4 * icol);
    if (irow != icol) {
      for (int32_t l = 0; l < N; l++) { const double t = A[N * irow + l]; A[N * irow + l] = A[N * icol + l]; A[N * icol + l] = t; }
      for (int32_t l = 0; l < NB; l++) { const double t = B[NB * irow + l]; B[NB * irow + l] = B[NB * icol + l]; B[NB * icol + l] = t; }
    }
    const double piv = A[N * icol + icol];
    if (fabs(piv) < 1e-20) return false;
    const double pivinv = 1.0 / piv;
    A[N * icol + icol] = 1.0;
    for (int32_t l = 0; l < N; l++) A[N * icol + l] *= pivinv;
    for (int32_t l = 0; l < NB; l++) B[NB * icol + l] *= pivinv;
    for (int32_t ll = 0; ll < N; ll++) {
      if (ll == icol) continue;
      const double dum = A[N * ll + icol];
      A[N * ll + icol] = 0.0;
      for (int32_t l = 0; l < N; l++) A[N * ll + l] -= A[N * icol + l] * dum;
      for (int32_t l = 0; l < NB; l++) B[NB * ll + l] -= B[NB * icol + l] * dum;
    }
  }
  return true;
}
