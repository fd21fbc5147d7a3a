// kernels_refit.hip -- the stereo motion refined on whole match lists, on gfx950.
//
// Replaces, for every list of a call in one launch:
//   the "final optimization" of VisualOdometryStereo::estimateMotion   (reference src/viso_stereo.cpp:126-139)
//   ...::updateParameters(.., 1, 1e-8) with computeObservations and computeResidualsAndJacobian   (:179-330)
//   Matrix::solve on the 6x6 normal equations                          (src/matrix.cpp:417-504; vh_gauss_jordan.h)
// for any quad list, every record of it active, from a caller-given start tr[6] -- vh_ego.h, the estimator's own device
// functions.  Double precision, built with -ffp-contract=off; only sin / cos come from the device library.
// `reweighting` is read; inlier_threshold and ransac_iters are not.
//
// One REFIT_T-lane workgroup per list, the whole Gauss-Newton loop inside the launch (the number of updates depends on
// the data: no host round trip per update).  Per update:
//   wave 0 builds the rotation and its derivatives and hands them over through LDS; every lane keeps them in scalar
//   registers (they are the same for the whole workgroup);
//   lane t adds the rows of the records t, t + REFIT_T, .. (ascending) to its acc[27]; a record is three 16-byte loads
//   and its 3-d point is computed again (ego_observe) rather than kept in a work buffer;
//   vh_wave_sum joins the 64 lanes of a wave, thread 0 adds the waves' totals in ascending order, solves, steps the
//   state in LDS and posts UPDATED / CONVERGED / FAILED.
// The order of additions is a function of the list's length alone: no atomics, the same bytes from run to run, whatever
// else the launch holds.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_ego.h"

namespace {

#define REFIT_T VH_REFIT_THREADS
#define REFIT_W (REFIT_T / 64)

// a value that is the same on every lane of the wave, moved to scalar registers
__device__ __forceinline__ double refit_uniform(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__global__ void __launch_bounds__(REFIT_T)
refit_kernel(VhRefitArgs a) {
  __shared__ double sAcc[REFIT_W][27];
  __shared__ double sRot[36], sTr[6];
  __shared__ int32_t sFlag;
  const int32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const VhList L = vh_list(a.lists, s);
  const int32_t n = L.n;
  if (!a.ok_in[s] || n < 6) {  // (no start to refine) / inliers.size() >= 6, src/viso_stereo.cpp:127 -- tr_in is not read
    if (tid == 0) { a.ok_out[s] = 0; a.n_updates[s] = 0; for (int32_t m = 0; m < 6; m++) a.tr_out[6 * (int64_t)s + m] = 0; }
    return;
  }
  if (tid < 6) sTr[tid] = a.tr_in[6 * (int64_t)s + tid];
  __syncthreads();
  int32_t iter = 0, calls = 0;
  bool success = false;
  for (;;) {  // src/viso_stereo.cpp:128-135
    if (w == 0) {  // the rotation and its derivatives, once per update
      double t6[6];
      for (int32_t m = 0; m < 6; m++) t6[m] = sTr[m];
      EgoRot R0;
      ego_rot(t6, R0);
      if (lane == 0)
        for (int32_t m = 0; m < 9; m++) { sRot[m] = R0.r[m]; sRot[9 + m] = R0.drx[m]; sRot[18 + m] = R0.dry[m]; sRot[27 + m] = R0.drz[m]; }
    }
    __syncthreads();
    EgoRot R;
    double tr[6];
#pragma unroll
    for (int32_t m = 0; m < 9; m++) {
      R.r[m] = refit_uniform(sRot[m]); R.drx[m] = refit_uniform(sRot[9 + m]);
      R.dry[m] = refit_uniform(sRot[18 + m]); R.drz[m] = refit_uniform(sRot[27 + m]);
    }
#pragma unroll
    for (int32_t m = 0; m < 6; m++) tr[m] = refit_uniform(sTr[m]);
    double acc[27];
#pragma unroll
    for (int32_t q = 0; q < 27; q++) acc[q] = 0;
    for (int32_t i = tid; i < n; i += REFIT_T) {
      // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c} {i1c, u2c, v2c, i2c}
      const float4 *p = (const float4 *)(L.pm + i);
      const float4 q0 = p[0], q1 = p[1], q2 = p[2];
      ego_accumulate(a.e, R, tr, ego_observe(a.e, q0.x, q0.y, q0.w, q1.z, q1.w, q2.y, q2.z), acc);
    }
#pragma unroll
    for (int32_t q = 0; q < 27; q++) {
      const double v = vh_wave_sum(acc[q]);
      if (lane == 0) sAcc[w][q] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double tot[27], bsol[6];
#pragma unroll
      for (int32_t q = 0; q < 27; q++) {
        double v = sAcc[0][q];
#pragma unroll
        for (int32_t k = 1; k < REFIT_W; k++) v += sAcc[k][q];
        tot[q] = v;
      }
      int32_t flag = 2;  // FAILED
      if (ego_solve(tot, bsol)) {
        flag = 1;        // CONVERGED
        for (int32_t m = 0; m < 6; m++) { sTr[m] += bsol[m]; if (fabs(bsol[m]) > 1e-8) flag = 0; }
      }
      sFlag = flag;
    }
    __syncthreads();
    const int32_t flag = sFlag;
    calls++;
    if (flag == 2) { success = false; break; }
    if (flag == 1) { success = true; break; }
    if (iter++ > 100) { success = false; break; }  // still UPDATED after 102 updates
  }
  if (tid == 0) {
    a.ok_out[s] = success ? 1 : 0;
    a.n_updates[s] = calls;
    for (int32_t m = 0; m < 6; m++) a.tr_out[6 * (int64_t)s + m] = success ? sTr[m] : 0.0;  // the reference returns an empty vector on failure
  }
}

}  // namespace

// grid: a.lists.n_lists workgroups (the caller keeps it below 2^24)
void vh_launch_refit(const VhRefitArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(refit_kernel, dim3(a.lists.n_lists), dim3(REFIT_T), 0, st, a);
}
