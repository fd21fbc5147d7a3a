// kernels_recon.hip -- 3-d points from lost feature tracks, batched, on gfx950.
//
// Replaces, for every lost track of one or more Reconstruction::update calls in one launch, what update runs on a
// lost track (reference src/reconstruction.cpp:131-142):
//   Reconstruction::initPoint                       (src/reconstruction.cpp:153-182) over Matrix::svd (src/matrix.cpp:579-802)
//   Reconstruction::pointType                       (src/reconstruction.cpp:235-261)
//   Reconstruction::refinePoint / updatePoint / computeObservations / computePredictionsAndJacobian
//                                                   (src/reconstruction.cpp:184-207, 263-349)
//   Matrix::solve on the 3x3 normal equations       (src/matrix.cpp:417-504; vh_gauss_jordan.h)
//   Reconstruction::pointDistance, rayAngle         (src/reconstruction.cpp:209-233)
// The tables the reference keeps per frame (P_total, Tr_inv_total, Tr_total) come from the host (vh_recon.h).
//
// One LANE per track, double precision, built with -ffp-contract=off so that a*b+c rounds twice as on the reference's
// x86 build.  Every sum of the reference is a sequential left-to-right sum over the track's frames whose order is part
// of the result, and a track is a few frames long: there is nothing inside a track to share between lanes without
// changing the order, so the parallelism is the number of tracks (thousands per update, millions per replay).  The host
// hands the tracks out sorted by length (order[]), so that the lanes of a wave run the same number of frames.
// The Jacobian is not stored: frame by frame, its two rows are added to the nine sums, which is the order in which
// the reference's loops over i = 0 .. 2 len - 1 add them.  All per-lane arrays are indexed by compile-time constants after
// unrolling (svd_static.h, vh_gauss_jordan.h), so they live in registers.
// The only device-library functions are sqrt (correctly rounded) and acos (the ray angle: to rounding, not bit for bit).
#include "vh_recon.h"
#include "../../include/viso_hip.h"
#include <math.h>
#define SVD_HD __device__ __forceinline__
#include "svd_static.h"
#include "vh_gauss_jordan.h"

namespace {

#define RECON_T 64

// row `row` of (4x4 M) * (x, y, z, 1) in Matrix::operator*'s order (src/matrix.cpp:271-276): C = 0, C += A[i][k] * B[k], k ascending
__device__ __forceinline__ double recon_row4(const double *M, int32_t row, double x, double y, double z, double w) {
  double c = 0.0;
  c += M[4 * row + 0] * x; c += M[4 * row + 1] * y; c += M[4 * row + 2] * z; c += M[4 * row + 3] * w;
  return c;
}

__global__ void __launch_bounds__(RECON_T)
recon_kernel(vh_recon_params r, double road0, double road1, double road2, double road3, const double *__restrict__ frames,
             int32_t n_tracks, const int32_t *__restrict__ order, const int32_t *__restrict__ first_frame,
             const int32_t *__restrict__ offsets, const float *__restrict__ pixels, float *__restrict__ points,
             int32_t *__restrict__ status, double *__restrict__ metrics) {
  const int32_t lane = blockIdx.x * RECON_T + threadIdx.x;
  if (lane >= n_tracks) return;
  const int32_t t = order[lane];
  const int32_t first = first_frame[t], off = offsets[t], len = offsets[t + 1] - off, last = first + len - 1;
  const float2 *px = (const float2 *)pixels + off;
  const double *F1 = frames + (int64_t)first * VH_RECON_FRAME_DOUBLES, *F2 = frames + (int64_t)last * VH_RECON_FRAME_DOUBLES;
  float p[3] = {0.f, 0.f, 0.f};
  double dist = 0.0, angle = 0.0;
  int32_t st = VH_RECON_ACCEPTED;
  do {
    // update's own test (src/reconstruction.cpp:131): `pixels.size() >= min_track_length` compares UNSIGNED there, so a negative
    // min_track_length is a huge one and every track is short
    if (r.min_track_length < 0 || len < r.min_track_length) { st = VH_RECON_SHORT; break; }
    {  // initPoint (src/reconstruction.cpp:153-182)
      const float2 p1 = px[0], p2 = px[len - 1];
      const double *P1 = F1 + VH_RECON_P, *P2 = F2 + VH_RECON_P;
      double J[4][4], w4[4], V4[4][4], x[4];
#pragma unroll
      for (int32_t j = 0; j < 4; j++) {
        J[0][j] = P1[2 * 4 + j] * p1.x - P1[0 * 4 + j];
        J[1][j] = P1[2 * 4 + j] * p1.y - P1[1 * 4 + j];
        J[2][j] = P2[2 * 4 + j] * p2.x - P2[0 * 4 + j];
        J[3][j] = P2[2 * 4 + j] * p2.y - P2[1 * 4 + j];
      }
      // The last column of V up to sign, without U (svd_static.h).  Its sign does not reach the result: w is that
      // column's fourth component rounded to float, rounding and fabs commute with negation, and every coordinate is
      // the quotient V[i][3] / w, in which IEEE division gives (-a) / (-b) == a / b bit for bit.
      svd_static_last_v_unsigned<4, 4>(J, w4, V4, x);
      const float w = (float)x[3];
      if (fabs((double)w) < 1e-10) { st = VH_RECON_INFINITY; break; }
#pragma unroll
      for (int32_t i = 0; i < 3; i++) p[i] = (float)(x[i] / (double)w);
    }
    {  // pointType (src/reconstruction.cpp:235-261)
      const double x1c2 = recon_row4(F1 + VH_RECON_TINV, 2, p[0], p[1], p[2], 1.0);
      const double *T2 = F2 + VH_RECON_TINV;
      const double x2c0 = recon_row4(T2, 0, p[0], p[1], p[2], 1.0), x2c1 = recon_row4(T2, 1, p[0], p[1], p[2], 1.0),
                   x2c2 = recon_row4(T2, 2, p[0], p[1], p[2], 1.0), x2c3 = recon_row4(T2, 3, p[0], p[1], p[2], 1.0);
      double x2r1 = 0.0;
      x2r1 += road0 * x2c0; x2r1 += road1 * x2c1; x2r1 += road2 * x2c2; x2r1 += road3 * x2c3;
      int32_t type = 2;                                // obstacle
      if (x1c2 <= 1 || x2c2 <= 1) type = -1;           // not visible
      else if (x2r1 > 0.5) type = 0;                   // below road
      else if (x2r1 > -1) type = 1;                    // road
      if (!(type >= r.point_type)) { st = VH_RECON_TYPE; break; }
    }
    {  // refinePoint (src/reconstruction.cpp:184-207): updatePoint(t, p, 1, 1e-5) until `iter++ > 20 || CONVERGED`
      int32_t iter = 0;
      bool converged = false, updated = true;
      while (updated) {
        // updatePoint (src/reconstruction.cpp:263-307) over computePredictionsAndJacobian (:316-349)
        double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, B0 = 0.0, B1 = 0.0, B2 = 0.0;
        bool singular = false;
        const double X = p[0], Y = p[1], Z = p[2];
        for (int32_t k = 0; k < len; k++) {
          const double *P = F1 + (int64_t)k * VH_RECON_FRAME_DOUBLES + VH_RECON_P;
          const double P00 = P[0], P01 = P[1], P02 = P[2], P03 = P[3], P10 = P[4], P11 = P[5], P12 = P[6], P13 = P[7],
                       P20 = P[8], P21 = P[9], P22 = P[10], P23 = P[11];
          const float2 ob = px[k];
          const double a = P00 * X + P01 * Y + P02 * Z + P03;
          const double b = P10 * X + P11 * Y + P12 * Z + P13;
          const double c = P20 * X + P21 * Y + P22 * Z + P23;
          const double cc = c * c;
          if (cc < 1e-10) { singular = true; break; }
          const double j0 = (P00 * c - P20 * a) / cc, j1 = (P01 * c - P21 * a) / cc, j2 = (P02 * c - P22 * a) / cc;
          const double j3 = (P10 * c - P20 * b) / cc, j4 = (P11 * c - P21 * b) / cc, j5 = (P12 * c - P22 * b) / cc;
          const double ru = (double)ob.x - a / c, rv = (double)ob.y - b / c;
          // rows 2k and 2k+1 of the sums of :283-294
          A00 += j0 * j0; A01 += j0 * j1; A02 += j0 * j2; A11 += j1 * j1; A12 += j1 * j2; A22 += j2 * j2;
          B0 += j0 * ru; B1 += j1 * ru; B2 += j2 * ru;
          A00 += j3 * j3; A01 += j3 * j4; A02 += j3 * j5; A11 += j4 * j4; A12 += j4 * j5; A22 += j5 * j5;
          B0 += j3 * rv; B1 += j4 * rv; B2 += j5 * rv;
        }
        updated = false;
        if (!singular) {
          double A[3][3] = {{A00, A01, A02}, {A01, A11, A12}, {A02, A12, A22}}, B[3] = {B0, B1, B2};
          if (vh_gauss_jordan<3>(A, B)) {
#pragma unroll
            for (int32_t i = 0; i < 3; i++) p[i] = (float)((double)p[i] + 1.0 * B[i]);
            converged = fabs(B[0]) < 1e-5 && fabs(B[1]) < 1e-5 && fabs(B[2]) < 1e-5;
            updated = !converged;
          }
        }
        if (iter++ > 20 || converged) break;
      }
      if (!converged) { st = VH_RECON_NOT_REFINED; break; }
    }
    {  // pointDistance (src/reconstruction.cpp:209-215)
      const double *C = frames + (int64_t)((first + last) / 2) * VH_RECON_FRAME_DOUBLES + VH_RECON_C;
      const double dx = C[0] - p[0], dy = C[1] - p[1], dz = C[2] - p[2];
      dist = sqrt(dx * dx + dy * dy + dz * dz);
    }
    {  // rayAngle (src/reconstruction.cpp:217-233)
      const double *C1 = F1 + VH_RECON_C, *C2 = F2 + VH_RECON_C;
      double v1[3], v2[3], n1 = 0.0, n2 = 0.0;
#pragma unroll
      for (int32_t i = 0; i < 3; i++) { v1[i] = C1[i] - p[i]; v2[i] = C2[i] - p[i]; }
#pragma unroll
      for (int32_t i = 0; i < 3; i++) { n1 += v1[i] * v1[i]; n2 += v2[i] * v2[i]; }
      n1 = sqrt(n1); n2 = sqrt(n2);
      if (n1 < 1e-10 || n2 < 1e-10) angle = 1000;
      else {
        double dot = 0.0;
#pragma unroll
        for (int32_t i = 0; i < 3; i++) dot += (v1[i] / n1) * (v2[i] / n2);
        angle = acos(fabs(dot)) * 180.0 / M_PI;
      }
    }
    if (!(dist < r.max_dist && angle > r.min_angle)) st = VH_RECON_FAR_OR_NARROW;
  } while (false);
  points[3 * (int64_t)t + 0] = p[0]; points[3 * (int64_t)t + 1] = p[1]; points[3 * (int64_t)t + 2] = p[2];
  status[t] = st;
  if (metrics) { metrics[2 * (int64_t)t + 0] = dist; metrics[2 * (int64_t)t + 1] = angle; }
}

}  // namespace

void vh_launch_recon(const vh_recon_params &r, const double road[4], const double *frames, int32_t n_tracks, const int32_t *order,
                     const int32_t *first_frame, const int32_t *offsets, const float *pixels, float *points, int32_t *status,
                     double *metrics, hipStream_t st) {
  if (n_tracks < 1) return;
  recon_kernel<<<(n_tracks + RECON_T - 1) / RECON_T, RECON_T, 0, st>>>(r, road[0], road[1], road[2], road[3], frames, n_tracks, order,
                                                                     first_frame, offsets, pixels, points, status, metrics);
}
