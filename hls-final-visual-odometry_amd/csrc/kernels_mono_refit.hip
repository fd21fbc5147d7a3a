// kernels_mono_refit.hip -- the epipolar model refitted on whole match lists, on gfx950.
//
// For every list of a call in one launch, fundamentalMatrix (reference src/viso_mono.cpp:235-266) over EVERY record of the
// list, in the normalised frame of the model the list comes with (vh_mono_model: its c, s are copied, not recomputed):
//   a (N x 9): a record normalised as the estimator does (mono_normalise) and the row the estimator's own refit forms of
//     it (mono_row9: float products, widened to double) -- vh_mono.h;
//   M = sum a a^T: the 45 sums of the upper triangle, mirrored;
//   f = the right singular vector of M for its smallest singular value: the project's Matrix::svd restatement
//     (svd_static.h) on the 9 x 9 M, the column of V that its descending sort puts last.  M is symmetric positive
//     semi-definite: these are the right singular vectors of the N x 9 system the reference decomposes.  Matrix::svd's
//     own sign normalisation is not applied: f is negated when its dot product with the incoming F is negative;
//   F = the rank-2 step of :262-265 on f (rank2_3x3, vh_rank2.h).
// Double precision, built with -ffp-contract=off; no function of the device library is called.
//
// One MRF_T-lane workgroup per list: lane t adds the records t, t + MRF_T, .. (ascending) to its acc[45] (a record is
// two 16-byte loads: its last third is not fetched); vh_wave_sum joins the lanes of a wave, thread 0 adds the waves'
// totals in ascending order and finishes alone -- the 9 x 9 decomposition without U, the sign, the 3 x 3 step, all in
// registers (256 VGPRs and 167 AGPRs, no scratch).  That tail of one lane is the candidate for most of the kernel's time
// (issuing the loads of four trips together changed 0.128 ms to 0.124 ms at S = 256 and was not kept).  The order of
// additions is a function of the list's length alone: no atomics, the same bytes from run to run, whatever else the launch holds.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_mono.h"
#include "vh_rank2.h"

namespace {

#define MRF_T VH_REFIT_THREADS
#define MRF_W (MRF_T / 64)

__global__ void __launch_bounds__(MRF_T)
mono_refit_kernel(VhMonoRefitArgs a) {
  __shared__ double sAcc[MRF_W][45];
  const int32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const VhList L = vh_list(a.lists, s);
  const int32_t n = L.n;
  double *mo = (double *)(a.model_out + s);  // 16 doubles: c[4], s[2], F[9], valid
  if (!a.ok_in[s] || n < 10) {  // (no model to refine) / inliers.size() >= 10, src/viso_mono.cpp:76 -- model_in is not read
    if (tid < 16) mo[tid] = 0;
    if (tid == 0) { a.ok_out[s] = 0; a.w_out[2 * (int64_t)s] = 0; a.w_out[2 * (int64_t)s + 1] = 0; }
    return;
  }
  const vh_mono_model m = a.model_in[s];  // the same for the whole workgroup: uniform loads
  double acc[45];
#pragma unroll
  for (int32_t q = 0; q < 45; q++) acc[q] = 0;
  for (int32_t i = tid; i < n; i += MRF_T) {
    // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c}
    const float4 *p = (const float4 *)(L.pm + i);
    const float4 q0 = p[0], q1 = p[1];
    double r[9];
    mono_row9(mono_normalise(m, q0.x, q0.y, q1.z, q1.w), r);
    int32_t k = 0;
#pragma unroll
    for (int32_t j = 0; j < 9; j++)
#pragma unroll
      for (int32_t c = j; c < 9; c++) acc[k++] += r[j] * r[c];
  }
#pragma unroll
  for (int32_t q = 0; q < 45; q++) {
    const double v = vh_wave_sum(acc[q]);
    if (lane == 0) sAcc[w][q] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  double U[9][9], w9[9], V[9][9], f[9], F[9];
  {
    int32_t k = 0;
#pragma unroll
    for (int32_t j = 0; j < 9; j++)
#pragma unroll
      for (int32_t c = j; c < 9; c++) {
        double v = sAcc[0][k];
#pragma unroll
        for (int32_t q = 1; q < MRF_W; q++) v += sAcc[q][k];
        U[j][c] = v; U[c][j] = v;
        k++;
      }
  }
  svd_static_last_v_unsigned<9, 9>(U, w9, V, f);  // (w9 comes back sorted, descending)
  double dot = 0.0;
#pragma unroll
  for (int32_t q = 0; q < 9; q++) dot += f[q] * m.F[q];
  if (dot < 0.0) {  // (a zero or NaN product leaves f as it is)
#pragma unroll
    for (int32_t q = 0; q < 9; q++) f[q] = -f[q];
  }
  rank2_3x3(f, F);
  bool good = isfinite(w9[8]) && isfinite(w9[7]);
#pragma unroll
  for (int32_t q = 0; q < 9; q++) good = good && isfinite(F[q]);
#pragma unroll
  for (int32_t q = 0; q < 4; q++) mo[q] = good ? m.c[q] : 0.0;
  mo[4] = good ? m.s[0] : 0.0; mo[5] = good ? m.s[1] : 0.0;
#pragma unroll
  for (int32_t q = 0; q < 9; q++) mo[6 + q] = good ? F[q] : 0.0;
  mo[15] = good ? 1.0 : 0.0;
  a.w_out[2 * (int64_t)s] = good ? w9[8] : 0.0;
  a.w_out[2 * (int64_t)s + 1] = good ? w9[7] : 0.0;
  a.ok_out[s] = good ? 1 : 0;
}

}  // namespace

// grid: a.lists.n_lists workgroups (the caller keeps it below 2^24)
void vh_launch_mono_refit(const VhMonoRefitArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(mono_refit_kernel, dim3(a.lists.n_lists), dim3(MRF_T), 0, st, a);
}
