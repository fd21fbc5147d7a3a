// kernels_cov.hip -- the covariance of a stereo motion over whole match lists, on gfx950.
//
// For every list of a call in one launch, at a FIXED motion tr[6] (no update is made):
//   J (4N x 6) and r (4N): the rows ego_observe + ego_accumulate form per record at tr -- computeResidualsAndJacobian
//   (reference src/viso_stereo.cpp:274-330), weighted as there under `reweighting`;
//   A = J^T J, ssr = sum r^2 (ego_accumulate<true>: one accumulator beside the 21 + 6 of the refit);
//   cov = ssr / (4N - 6) * A^-1, A^-1 by Matrix::solve on the six unit right-hand sides (vh_gauss_jordan_mem), the
//   upper triangle mirrored.
// Double precision, built with -ffp-contract=off; only sin / cos come from the device library.  `reweighting` is read;
// inlier_threshold and ransac_iters are not.
//
// One COV_T-lane workgroup per list, as the refit's: wave 0 builds the rotation and hands it over through LDS, every lane
// keeps it in scalar registers; lane t adds the records t, t + COV_T, .. (ascending) to its acc[28] (a record is three
// 16-byte loads, its 3-d point computed again); vh_wave_sum joins the lanes, thread 0 adds the waves' totals in ascending
// order, eliminates and writes.  The elimination's pivot row and column are data: its 6 x 6 system and the six
// right-hand sides live in LDS, where a data-dependent index costs nothing (in private memory it would be scratch).
// The order of additions is a function of the list's length alone: no atomics, the same bytes from run to run, whatever
// else the launch holds.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_ego.h"

namespace {

#define COV_T VH_REFIT_THREADS
#define COV_W (COV_T / 64)

// a value that is the same on every lane of the wave, moved to scalar registers
__device__ __forceinline__ double cov_uniform(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__global__ void __launch_bounds__(COV_T)
motion_cov_kernel(VhCovArgs a) {
  __shared__ double sAcc[COV_W][28];
  __shared__ double sRot[36];
  __shared__ double sA[36], sB[36];
  const int32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const VhList L = vh_list(a.lists, s);
  const int32_t n = L.n;
  double *cov = a.cov + 36 * (int64_t)s;
  if (!a.ok[s] || n < 6) {  // (no motion) / the rule of the refit -- tr is not read
    if (tid < 36) cov[tid] = 0;
    if (tid == 0) { a.ssr[s] = 0; a.ok_out[s] = 0; }
    return;
  }
  double tr[6];
#pragma unroll
  for (int32_t m = 0; m < 6; m++) tr[m] = cov_uniform(a.tr[6 * (int64_t)s + m]);
  if (w == 0) {  // the rotation and its derivatives, once
    EgoRot R0;
    ego_rot(tr, R0);
    if (lane == 0)
      for (int32_t m = 0; m < 9; m++) { sRot[m] = R0.r[m]; sRot[9 + m] = R0.drx[m]; sRot[18 + m] = R0.dry[m]; sRot[27 + m] = R0.drz[m]; }
  }
  __syncthreads();
  EgoRot R;
#pragma unroll
  for (int32_t m = 0; m < 9; m++) {
    R.r[m] = cov_uniform(sRot[m]); R.drx[m] = cov_uniform(sRot[9 + m]);
    R.dry[m] = cov_uniform(sRot[18 + m]); R.drz[m] = cov_uniform(sRot[27 + m]);
  }
  double acc[28];
#pragma unroll
  for (int32_t q = 0; q < 28; q++) acc[q] = 0;
  for (int32_t i = tid; i < n; i += COV_T) {
    // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c} {i1c, u2c, v2c, i2c}
    const float4 *p = (const float4 *)(L.pm + i);
    const float4 q0 = p[0], q1 = p[1], q2 = p[2];
    ego_accumulate<true>(a.e, R, tr, ego_observe(a.e, q0.x, q0.y, q0.w, q1.z, q1.w, q2.y, q2.z), acc);
  }
#pragma unroll
  for (int32_t q = 0; q < 28; q++) {
    const double v = vh_wave_sum(acc[q]);
    if (lane == 0) sAcc[w][q] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  // A in full (the reference fills all 36 entries) beside the unit matrix
  int32_t k = 0;
#pragma unroll
  for (int32_t m = 0; m < 6; m++)
#pragma unroll
    for (int32_t c = m; c < 6; c++) {
      double v = sAcc[0][k];
#pragma unroll
      for (int32_t j = 1; j < COV_W; j++) v += sAcc[j][k];
      sA[6 * m + c] = v; sA[6 * c + m] = v;
      k++;
    }
#pragma unroll
  for (int32_t q = 0; q < 36; q++) sB[q] = q % 7 == 0 ? 1.0 : 0.0;
  double ssr = sAcc[0][27];
#pragma unroll
  for (int32_t j = 1; j < COV_W; j++) ssr += sAcc[j][27];
  bool good = vh_gauss_jordan_mem<6, 6>(sA, sB);
  const double sigma2 = ssr / (double)(4 * n - 6);
  double c[21];
  k = 0;
  good = good && isfinite(ssr);
#pragma unroll
  for (int32_t m = 0; m < 6; m++)
#pragma unroll
    for (int32_t q = m; q < 6; q++) { c[k] = sigma2 * sB[6 * m + q]; good = good && isfinite(c[k]); k++; }
  k = 0;
#pragma unroll
  for (int32_t m = 0; m < 6; m++)
#pragma unroll
    for (int32_t q = m; q < 6; q++) { const double v = good ? c[k] : 0.0; cov[6 * m + q] = v; cov[6 * q + m] = v; k++; }
  a.ssr[s] = good ? ssr : 0.0;
  a.ok_out[s] = good ? 1 : 0;
}

}  // namespace

// grid: a.lists.n_lists workgroups (the caller keeps it below 2^24)
void vh_launch_motion_cov(const VhCovArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(motion_cov_kernel, dim3(a.lists.n_lists), dim3(COV_T), 0, st, a);
}
