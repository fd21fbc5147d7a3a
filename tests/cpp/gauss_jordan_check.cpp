// CPU check of hls-final-visual-odometry_amd/csrc/vh_gauss_jordan.h, the one Matrix::solve of the device code (the 3x3
// normal equations of recon_kernel, the 6x6 ones of ego_kernel).  The header is plain C++, so it is compiled for the host
// here and compared BIT FOR BIT with
//   - the two solvers it replaced, kept below as they were (old_recon_solve3, old_ego_solve), on random symmetric
//     systems and on the edge systems: zero matrix, singular below 1e-20, largest entry off the diagonal in every step,
//     equal-magnitude ties (which `>=` resolves towards the last entry);
//   - Matrix::solve written with the original's dynamic indices (solve_dynamic: irow / icol declared outside the pivot
//     loop, src/matrix.cpp:435), on all of these AND on systems in which every candidate of a pivot search is NaN -- the
//     one case in which the former 6x6 solver, which reset irow / icol for every pivot, chose differently.
// Built and run by tests/test_egomotion.py::test_gauss_jordan_header_equals_the_solvers_it_replaced.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include "../../hls-final-visual-odometry_amd/csrc/vh_gauss_jordan.h"

// ---- the former solvers, verbatim (kernels_recon.hip, kernels_ego.hip) -----------------------------------------------
// Matrix::solve (src/matrix.cpp:417-504) for the 3x3 system: Gauss-Jordan with full pivoting, singular below 1e-20.
// The pivot's row and column select among the three rows / columns by predicates; the arithmetic and its order are the
// original's.  A is the full matrix (the reference fills all nine entries; A[m][n] and A[n][m] are the same sums).
static bool old_recon_solve3(double (&A)[3][3], double (&b)[3]) {
  int32_t ipiv[3] = {0, 0, 0};
  int32_t irow = 0, icol = 0;  // (kept from pivot to pivot, as the original's are: a search that finds nothing -- NaN -- reuses them)
#pragma unroll
  for (int32_t i = 0; i < 3; i++) {
    double big = 0.0;
#pragma unroll
    for (int32_t j = 0; j < 3; j++)
#pragma unroll
      for (int32_t k = 0; k < 3; k++) {
        const double v = fabs(A[j][k]);
        if (ipiv[j] != 1 && ipiv[k] == 0 && v >= big) { big = v; irow = j; icol = k; }
      }
#pragma unroll
    for (int32_t q = 0; q < 3; q++) ipiv[q] += q == icol ? 1 : 0;
    // rows irow and icol change places (nothing moves when they are the same row)
    double ri[3], rc[3], bi = 0.0, bc = 0.0;
#pragma unroll
    for (int32_t l = 0; l < 3; l++) { ri[l] = 0.0; rc[l] = 0.0; }
#pragma unroll
    for (int32_t r = 0; r < 3; r++) {
#pragma unroll
      for (int32_t l = 0; l < 3; l++) { ri[l] = r == irow ? A[r][l] : ri[l]; rc[l] = r == icol ? A[r][l] : rc[l]; }
      bi = r == irow ? b[r] : bi; bc = r == icol ? b[r] : bc;
    }
#pragma unroll
    for (int32_t r = 0; r < 3; r++) {
#pragma unroll
      for (int32_t l = 0; l < 3; l++) A[r][l] = r == icol ? ri[l] : (r == irow ? rc[l] : A[r][l]);
      b[r] = r == icol ? bi : (r == irow ? bc : b[r]);
    }
    // the pivot row (now row icol) is ri, its right-hand side bi
    double piv = 0.0;
#pragma unroll
    for (int32_t l = 0; l < 3; l++) piv = l == icol ? ri[l] : piv;
    if (fabs(piv) < 1e-20) return false;
    const double pivinv = 1.0 / piv;
#pragma unroll
    for (int32_t l = 0; l < 3; l++) ri[l] = (l == icol ? 1.0 : ri[l]) * pivinv;
    bi *= pivinv;
#pragma unroll
    for (int32_t ll = 0; ll < 3; ll++) {
      double dum = 0.0;
#pragma unroll
      for (int32_t l = 0; l < 3; l++) dum = l == icol ? A[ll][l] : dum;
      const bool prow = ll == icol;
#pragma unroll
      for (int32_t l = 0; l < 3; l++) {
        const double cur = l == icol ? 0.0 : A[ll][l];
        A[ll][l] = prow ? ri[l] : cur - ri[l] * dum;
      }
      b[ll] = prow ? bi : b[ll] - bi * dum;
    }
  }
  return true;
}

// Matrix::solve for the 6x6 system (src/matrix.cpp:417-504): Gauss-Jordan with full pivoting,
// singular below 1e-20.  acc as produced by ego_accumulate; on success b = the solution.
// Every array index is a compile-time constant after unrolling -- the pivot's row and column (data-dependent in
// the original) select among the six rows / columns by predicates -- so the system lives in registers: with
// dynamic indices it sat in private memory, and the 22 dependent solves of a hypothesis were 85 % of the
// kernel (1.2 of 1.4 ms per batch of bucketed lists, tools/ego_phases.py).  The arithmetic applied to the
// elements, and its order, are the original's.
static bool old_ego_solve(const double acc[27], double b[6]) {
  double A[6][6];
  {
    int32_t k = 0;
#pragma unroll
    for (int32_t m = 0; m < 6; m++)
#pragma unroll
      for (int32_t n = m; n < 6; n++) { A[m][n] = acc[k]; A[n][m] = acc[k]; k++; }
#pragma unroll
    for (int32_t m = 0; m < 6; m++) b[m] = acc[21 + m];
  }
  int32_t ipiv[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int32_t i = 0; i < 6; i++) {
    double big = 0.0;
    int32_t irow = 0, icol = 0;
#pragma unroll
    for (int32_t j = 0; j < 6; j++)
#pragma unroll
      for (int32_t k = 0; k < 6; k++) {
        const double v = fabs(A[j][k]);
        if (ipiv[j] != 1 && ipiv[k] == 0 && v >= big) { big = v; irow = j; icol = k; }
      }
#pragma unroll
    for (int32_t q = 0; q < 6; q++) ipiv[q] += q == icol ? 1 : 0;
    // rows irow and icol change places (nothing moves when they are the same row)
    double ri[6], rc[6], bi = 0.0, bc = 0.0;
#pragma unroll
    for (int32_t l = 0; l < 6; l++) { ri[l] = 0.0; rc[l] = 0.0; }
#pragma unroll
    for (int32_t r = 0; r < 6; r++) {
#pragma unroll
      for (int32_t l = 0; l < 6; l++) { ri[l] = r == irow ? A[r][l] : ri[l]; rc[l] = r == icol ? A[r][l] : rc[l]; }
      bi = r == irow ? b[r] : bi; bc = r == icol ? b[r] : bc;
    }
#pragma unroll
    for (int32_t r = 0; r < 6; r++) {
#pragma unroll
      for (int32_t l = 0; l < 6; l++) A[r][l] = r == icol ? ri[l] : (r == irow ? rc[l] : A[r][l]);
      b[r] = r == icol ? bi : (r == irow ? bc : b[r]);
    }
    // the pivot row (now row icol) is ri, its right-hand side bi
    double piv = 0.0;
#pragma unroll
    for (int32_t l = 0; l < 6; l++) piv = l == icol ? ri[l] : piv;
    if (fabs(piv) < 1e-20) return false;
    const double pivinv = 1.0 / piv;
#pragma unroll
    for (int32_t l = 0; l < 6; l++) ri[l] = (l == icol ? 1.0 : ri[l]) * pivinv;
    bi *= pivinv;
#pragma unroll
    for (int32_t ll = 0; ll < 6; ll++) {
      double dum = 0.0;
#pragma unroll
      for (int32_t l = 0; l < 6; l++) dum = l == icol ? A[ll][l] : dum;
      const bool prow = ll == icol;
#pragma unroll
      for (int32_t l = 0; l < 6; l++) {
        const double cur = l == icol ? 0.0 : A[ll][l];
        A[ll][l] = prow ? ri[l] : cur - ri[l] * dum;
      }
      b[ll] = prow ? bi : b[ll] - bi * dum;
    }
  }
  return true;
}

// ---- Matrix::solve with dynamic indices, one right-hand side ---------------------------------------------------------
template <int N> static bool solve_dynamic(double (&A)[N][N], double (&b)[N]) {
  int ipiv[N], icol = 0, irow = 0;
  for (int j = 0; j < N; j++) ipiv[j] = 0;
  for (int i = 0; i < N; i++) {
    double big = 0.0;
    for (int j = 0; j < N; j++)
      if (ipiv[j] != 1)
        for (int k = 0; k < N; k++)
          if (ipiv[k] == 0)
            if (fabs(A[j][k]) >= big) { big = fabs(A[j][k]); irow = j; icol = k; }
    ++ipiv[icol];
    if (irow != icol) {
      for (int l = 0; l < N; l++) { const double t = A[irow][l]; A[irow][l] = A[icol][l]; A[icol][l] = t; }
      const double t = b[irow]; b[irow] = b[icol]; b[icol] = t;
    }
    if (fabs(A[icol][icol]) < 1e-20) return false;
    const double pivinv = 1.0 / A[icol][icol];
    A[icol][icol] = 1.0;
    for (int l = 0; l < N; l++) A[icol][l] *= pivinv;
    b[icol] *= pivinv;
    for (int ll = 0; ll < N; ll++)
      if (ll != icol) {
        const double dum = A[ll][icol];
        A[ll][icol] = 0.0;
        for (int l = 0; l < N; l++) A[ll][l] -= A[icol][l] * dum;
        b[ll] -= b[icol] * dum;
      }
  }
  return true;
}

template <int N> struct Sys { double A[N][N], b[N]; };

static bool old_solve(Sys<3> &s) { return old_recon_solve3(s.A, s.b); }
static bool old_solve(Sys<6> &s) {  // ego_solve read the packed upper triangle and the right-hand side from one array
  double acc[27], out[6];
  int k = 0;
  for (int m = 0; m < 6; m++) for (int n = m; n < 6; n++) acc[k++] = s.A[m][n];
  for (int m = 0; m < 6; m++) acc[21 + m] = s.b[m];
  const bool ok = old_ego_solve(acc, out);
  memcpy(s.b, out, sizeof(out));
  return ok;
}

// bit for bit; two NaNs count as equal whatever their payloads
template <int N> static bool same(bool ra, const double (&a)[N], bool rb, const double (&b)[N]) {
  if (ra != rb) return false;
  for (int i = 0; i < N; i++) if (memcmp(&a[i], &b[i], 8) && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
  return true;
}

// -> bit 0: differs from the former solver, bit 1: differs from solve_dynamic
template <int N> static int check(const Sys<N> &in, bool *ok_out = nullptr) {
  Sys<N> a = in, b = in, c = in;
  const bool ra = vh_gauss_jordan<N>(a.A, a.b), rb = old_solve(b), rc = solve_dynamic<N>(c.A, c.b);
  if (ok_out) *ok_out = ra;
  return (same<N>(ra, a.b, rb, b.b) ? 0 : 1) | (same<N>(ra, a.b, rc, c.b) ? 0 : 2);
}

template <int N> static Sys<N> symmetric(std::mt19937 &rng, int kind) {
  std::normal_distribution<double> nd;
  Sys<N> s;
  for (int m = 0; m < N; m++) for (int n = m; n < N; n++) s.A[m][n] = s.A[n][m] = nd(rng);
  for (int m = 0; m < N; m++) s.b[m] = nd(rng);
  if (kind == 1) {  // J^T J of N + 1 rows, as the kernels build it
    double J[N + 1][N];
    for (auto &r : J) for (auto &x : r) x = nd(rng) * 100;
    for (int m = 0; m < N; m++) for (int n = 0; n < N; n++) { double t = 0; for (auto &r : J) t += r[m] * r[n]; s.A[m][n] = t; }
  }
  if (kind == 2) for (int m = 0; m < N; m++) for (int n = 0; n < N; n++) s.A[m][n] = std::round(s.A[m][n] * 2);  // small integers: zeros and ties
  if (kind == 3) for (int n = 0; n < N; n++) s.A[N - 1][n] = s.A[n][N - 1] = n == N - 1 ? s.A[0][0] : s.A[0][n];  // a repeated row and column: rank deficient
  return s;
}

template <int N> static int run(int trials, unsigned seed) {
  std::mt19937 rng(seed);
  int bad_old = 0, bad_dyn = 0, solved = 0;
  auto one = [&](const Sys<N> &s) { bool ok; const int r = check<N>(s, &ok); bad_old += r & 1; bad_dyn += (r >> 1) & 1; solved += ok ? 1 : 0; return ok; };
  for (int t = 0; t < trials; t++) one(symmetric<N>(rng, t % 4));
  printf("vh_gauss_jordan<%d>: %d random systems (%d solved), %d differ from the former solver, %d from Matrix::solve\n", N, trials, solved, bad_old, bad_dyn);
  int bad = bad_old + bad_dyn, edge_bad = 0;
  bad_old = bad_dyn = 0;
  Sys<N> s;
  // zero matrix: singular at the first pivot
  memset(&s, 0, sizeof(s)); s.b[0] = 1;
  if (one(s)) edge_bad++;
  // singular below 1e-20: a diagonal whose last entry is under the limit, and one just above it
  memset(&s, 0, sizeof(s));
  for (int m = 0; m < N; m++) { s.A[m][m] = m + 1; s.b[m] = 1; }
  s.A[N - 1][N - 1] = 0.99e-20;
  if (one(s)) edge_bad++;
  s.A[N - 1][N - 1] = 1.01e-20;
  if (!one(s)) edge_bad++;
  // the largest entry off the diagonal in every step: an anti-diagonal matrix of growing entries (every pivot swaps rows)
  memset(&s, 0, sizeof(s));
  for (int m = 0; m < N; m++) { s.A[m][N - 1 - m] = 2 + (m < N - 1 - m ? m : N - 1 - m); s.b[m] = m + 1; }
  if (!one(s)) edge_bad++;
  // ... and a full symmetric one: small diagonal, large off-diagonal entries
  for (int m = 0; m < N; m++) for (int n = 0; n < N; n++) s.A[m][n] = m == n ? 0.01 * (m + 1) : 3 + m + n + 0.5 * (m > n ? m - n : n - m);
  one(s);
  // equal-magnitude ties: all ones with alternating signs (rank one: singular at the second pivot), the identity, and
  // a matrix whose entries all have magnitude 2 with independent rows
  for (int m = 0; m < N; m++) for (int n = 0; n < N; n++) s.A[m][n] = (m + n) % 2 ? -1.0 : 1.0;
  if (one(s)) edge_bad++;
  for (int m = 0; m < N; m++) for (int n = 0; n < N; n++) s.A[m][n] = m == n ? 1.0 : 0.0;
  if (!one(s)) edge_bad++;
  for (int m = 0; m < N; m++) for (int n = 0; n < N; n++) s.A[m][n] = (m & n & 1) ^ ((m & n) >> 1 & 1) ^ ((m & n) >> 2 & 1) ? -2.0 : 2.0;  // a Hadamard pattern where N allows it
  one(s);
  printf("vh_gauss_jordan<%d>: edge systems, %d differ from the former solver, %d from Matrix::solve, %d unexpected outcomes\n", N, bad_old, bad_dyn, edge_bad);
  return bad + bad_old + bad_dyn + edge_bad;
}

// Every candidate of a pivot search NaN, after a first pivot away from (0, 0): all entries NaN but A[2][3] = A[3][2] = 1,
// so that the first search ends at (3, 2) and every later one finds nothing.  Matrix::solve goes on with (3, 2); the
// former 6x6 solver went back to (0, 0).  Neither stops: |NaN| < 1e-20 is false.
static int run_nan() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int bad = 0, differ_old = 0;
  for (int variant = 0; variant < 3; variant++) {
    Sys<6> s;
    for (auto &r : s.A) for (auto &x : r) x = nan;
    for (int m = 0; m < 6; m++) s.b[m] = m + 1;
    s.A[2][3] = s.A[3][2] = 1.0;
    if (variant == 1) s.A[0][0] = 0.5;                            // a finite entry away from the pivot: the elimination turns it into NaN
    if (variant == 2) { s.A[2][2] = 0.25; s.A[3][3] = 0.25; }     // finite entries in the pivot's own row and column
    bool ok;
    const int r = check<6>(s, &ok);
    differ_old += r & 1;
    bad += (r >> 1) & 1;
    printf("vh_gauss_jordan<6>: NaN system %d returns %s, %s Matrix::solve, %s the former solver\n", variant, ok ? "true" : "false",
           (r & 2) ? "DIFFERS from" : "equals", (r & 1) ? "differs from" : "equals");
  }
  Sys<6> all;
  for (auto &r : all.A) for (auto &x : r) x = nan;
  for (auto &x : all.b) x = 1;
  const int r = check<6>(all);  // nothing is ever selected: both forms stay at (0, 0)
  printf("vh_gauss_jordan<6>: all-NaN system, %d differing from either\n", r ? 1 : 0);
  printf("vh_gauss_jordan<6>: NaN systems, %d differ from Matrix::solve, %d of 3 from the former solver\n", bad + (r ? 1 : 0), differ_old);
  return bad + (r ? 1 : 0);
}

int main() {
  int bad = run<3>(4000, 1) + run<6>(4000, 2);
  bad += run_nan();
  printf("%d failures\n", bad);
  return bad ? 1 : 0;
}
