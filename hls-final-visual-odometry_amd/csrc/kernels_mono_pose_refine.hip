// kernels_mono_pose_refine.hip -- the mono pose refined on whole match lists, on gfx950.
//
// Between mono_pose_tri and mono_pose_front, for every list of a call in one launch: from the winner of the chirality
// counts, Gauss-Newton on the signed Sampson distance of EVERY record over (R, unit t) -- five parameters, a left
// rotation and two coordinates in the tangent plane of the unit sphere at t -- then one more accumulation at the
// converged pose and cov = ssr / (N - 5) * (J^T J)^-1.  The arithmetic is vh_mono_refine.h's, the contract
// include/viso_hip.h's; neither the reference nor stock libviso2 has a counterpart.  Where the refinement converges the
// refined R, t and projection matrix replace the winner's in the list's header (R in its Ra / Rb slot, t with the winner's
// sign taken out again in t0, K [R | t] in the winner's P2): mono_pose_front, _rank, _vote and _finish read them there,
// unchanged.  Where it does not, the header is not written and those four give vh_pose_mono's bytes.
//
// One MR_T-lane workgroup per list, the whole loop inside the launch (the number of updates depends on the data), as
// refit_kernel has it.  Per pass:
//   wave 0 builds E, the five E_k and the basis B (mr_uniforms) and hands them over through LDS; every lane moves them
//   to scalar registers (they are the same for the whole workgroup) -- as far as they fit: 54 doubles are 108 SGPRs, more
//   than the budget, and the compiler keeps 106 SGPRs and parks 87 further scalar values in lanes of VGPRs (v_writelane /
//   v_readlane around the record loop; no scratch).  refit_kernel's 42 values fit; these do not.  DESIGN.md section 4.18
//   has the measured cost;
//   lane t adds the records t, t + MR_T, .. (ascending) to its acc[21]; a record is two 16-byte loads;
//   vh_wave_sum joins the 64 lanes of a wave; thread 0 adds the waves' totals in ascending order, solves (Matrix::solve on
//   a system in LDS, where the pivot's data-dependent row and column cost nothing), steps the state in LDS and posts
//   what comes next: another update, the covariance pass, or the end.
// The order of additions is a function of the list's length alone: no atomics, the same bytes from run to run, whatever
// else the launch holds.  Double precision, built with -ffp-contract=off; sin and asin come from the device library.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_mono_pose.h"    // mono_pose_winner, matmul
#include "vh_mono_refine.h"
#include "vh_gauss_jordan.h"

namespace {

#define MR_T VH_REFIT_THREADS
#define MR_W (MR_T / 64)
enum { MR_UPDATE = 0, MR_COV = 1, MR_END = 2 };  // what the next pass is

// a value that is the same on every lane of the wave, moved to scalar registers
__device__ __forceinline__ double mr_uniform(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// sum q of the waves' totals, in ascending order of the waves
__device__ __forceinline__ double mr_total(const double (*sAcc)[VH_MR_ACC], int32_t q) {
  double v = sAcc[0][q];
#pragma unroll
  for (int32_t k = 1; k < MR_W; k++) v += sAcc[k][q];
  return v;
}

__global__ void __launch_bounds__(MR_T)
mono_pose_refine_kernel(VhMonoPoseArgs a, vh_mono_refine *out) {
  __shared__ double sAcc[MR_W][VH_MR_ACC];
  __shared__ double sU[VH_MR_UNIFORMS], sBas[6];
  __shared__ double sR[9], sT[3], sR0[9], sT0[3];
  __shared__ double sA[25], sB[25];
  __shared__ int32_t sNext;
  const int32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const VhList L = vh_list(a.lists, s);
  const int32_t n = L.n;
  double *hdr = a.hdr + (int64_t)s * VH_MONO_POSE_HDR;
  const int32_t *ih = (const int32_t *)(hdr + MP_H_INT);
  int32_t cnt[4];
  for (int32_t c = 0; c < 4; c++) cnt[c] = ih[c];
  const int32_t cbest = ih[MP_I_REASON] != 0 ? -1 : mono_pose_winner(cnt);  // (reasons 1, 2; no winner is reason 3)
  vh_mono_refine *res = out + s;
  if (cbest < 0) {  // nothing to refine (the same for the whole workgroup)
    if (tid < 6) res->B[tid] = 0.0;
    if (tid < 25) res->cov[tid] = 0.0;
    if (tid == 0) { res->ssr_start = 0.0; res->ssr = 0.0; res->moved_R = 0.0; res->moved_t = 0.0; res->status = 1; res->n_updates = 0; }
    return;
  }
  if (tid < 9) { const double v = hdr[MP_H_RT + (cbest < 2 ? 0 : 9) + tid]; sR[tid] = v; sR0[tid] = v; }
  if (tid < 3) { const double t0 = hdr[MP_H_RT + 18 + tid], v = (cbest & 1) ? -t0 : t0; sT[tid] = v; sT0[tid] = v; }
  __syncthreads();
  // thread 0 alone keeps these
  int32_t status = 0, updates = 0;
  double ssr_start = 0.0, ssr = 0.0;
  for (int32_t pass = MR_UPDATE; pass != MR_END;) {
    if (w == 0) {  // E, the E_k and B, once per pass
      double R[9], t[3], U[VH_MR_UNIFORMS], B[6];
#pragma unroll
      for (int32_t q = 0; q < 9; q++) R[q] = sR[q];
#pragma unroll
      for (int32_t q = 0; q < 3; q++) t[q] = sT[q];
      mr_uniforms(R, t, U, B);
      if (lane == 0) {
#pragma unroll
        for (int32_t q = 0; q < VH_MR_UNIFORMS; q++) sU[q] = U[q];
#pragma unroll
        for (int32_t q = 0; q < 6; q++) sBas[q] = B[q];
      }
    }
    __syncthreads();
    double U[VH_MR_UNIFORMS];
#pragma unroll
    for (int32_t q = 0; q < VH_MR_UNIFORMS; q++) U[q] = mr_uniform(sU[q]);
    double acc[VH_MR_ACC];
#pragma unroll
    for (int32_t q = 0; q < VH_MR_ACC; q++) acc[q] = 0;
    for (int32_t i = tid; i < n; i += MR_T) {
      // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c}
      const float4 *p = (const float4 *)(L.pm + i);
      const float4 q0 = p[0], q1 = p[1];
      double r, J[VH_MR_PARAMS];
      mr_residual(a.e.f, U, mr_record(a.e.f, a.e.cu, a.e.cv, q0.x, q0.y, q1.z, q1.w), r, J);
      mr_accumulate(r, J, acc);
    }
#pragma unroll
    for (int32_t q = 0; q < VH_MR_ACC; q++) {
      const double v = vh_wave_sum(acc[q]);
      if (lane == 0) sAcc[w][q] = v;
    }
    __syncthreads();
    if (tid == 0) {
      // the waves' totals in ascending order; A in full (Matrix::solve reads all 25 entries), g, ssr
      bool sums_ok = true;
      int32_t k = 0;
      for (int32_t m = 0; m < 5; m++)
        for (int32_t c = m; c < 5; c++) { const double v = mr_total(sAcc, k++); sums_ok = sums_ok && isfinite(v); sA[5 * m + c] = v; sA[5 * c + m] = v; }
      for (int32_t m = 0; m < 5; m++) { const double v = mr_total(sAcc, 15 + m); sums_ok = sums_ok && isfinite(v); sB[m] = v; }
      const double ss = mr_total(sAcc, 20);
      sums_ok = sums_ok && isfinite(ss);
      if (pass == MR_UPDATE && updates == 0 && isfinite(ss)) ssr_start = ss;
      int32_t next = MR_END;
      if (!sums_ok) status = 4;
      else if (pass == MR_UPDATE) {
        if (!vh_gauss_jordan_mem<5, 1>(sA, sB)) status = 2;
        else {
          double delta[5], R[9], t[3];
          bool small = true;
#pragma unroll
          for (int32_t m = 0; m < 5; m++) { delta[m] = -sB[m]; small = small && fabs(delta[m]) < 1e-8; }
#pragma unroll
          for (int32_t q = 0; q < 9; q++) R[q] = sR[q];
#pragma unroll
          for (int32_t q = 0; q < 3; q++) t[q] = sT[q];
          mr_step(delta, R, t);
          bool fin = true;
#pragma unroll
          for (int32_t q = 0; q < 9; q++) { sR[q] = R[q]; fin = fin && isfinite(R[q]); }
#pragma unroll
          for (int32_t q = 0; q < 3; q++) { sT[q] = t[q]; fin = fin && isfinite(t[q]); }
          updates++;
          if (!fin) status = 4;
          else if (small) next = MR_COV;
          else if (updates >= 102) status = 3;
          else next = MR_UPDATE;
        }
      } else {  // the covariance at the converged pose: A^-1 on the five unit right-hand sides, then into sA
        for (int32_t q = 0; q < 25; q++) sB[q] = q % 6 == 0 ? 1.0 : 0.0;
        if (!vh_gauss_jordan_mem<5, 5>(sA, sB)) status = 2;
        else {
          const double sigma2 = ss / (double)(n - 5);
          bool fin = true;
          for (int32_t m = 0; m < 5; m++)
            for (int32_t c = m; c < 5; c++) { const double v = sigma2 * sB[5 * m + c]; fin = fin && isfinite(v); sA[5 * m + c] = v; sA[5 * c + m] = v; }
          if (!fin) status = 4;
          ssr = ss;
        }
      }
      sNext = next;
    }
    __syncthreads();
    pass = sNext;
  }
  if (tid != 0) return;
  const bool good = status == 0;  // (a refused refinement: zeros, and the header stays the winner's)
  for (int32_t q = 0; q < 25; q++) res->cov[q] = good ? sA[q] : 0.0;
  for (int32_t q = 0; q < 6; q++) res->B[q] = good ? sBas[q] : 0.0;  // (the covariance pass built it at the converged t)
  res->ssr_start = ssr_start; res->ssr = good ? ssr : 0.0;
  res->status = status; res->n_updates = updates;
  if (!good) { res->moved_R = 0.0; res->moved_t = 0.0; return; }
  double R[9], t[3], R0[9], T0[3];
#pragma unroll
  for (int32_t q = 0; q < 9; q++) { R[q] = sR[q]; R0[q] = sR0[q]; }
#pragma unroll
  for (int32_t q = 0; q < 3; q++) { t[q] = sT[q]; T0[q] = sT0[q]; }
  res->moved_R = mr_angle(R, R0, 9); res->moved_t = mr_angle(t, T0, 3);
  // the winner's slot of the header, as mono_pose_candidates fills it
  const double K[9] = {a.e.f, 0, a.e.cu, 0, a.e.f, a.e.cv, 0, 0, 1};
  double Rt[12], P2[12];
#pragma unroll
  for (int32_t i = 0; i < 3; i++) {
#pragma unroll
    for (int32_t j = 0; j < 3; j++) Rt[i * 4 + j] = R[i * 3 + j];
    Rt[i * 4 + 3] = t[i];
  }
  matmul(K, 3, 3, Rt, 4, P2);
#pragma unroll
  for (int32_t q = 0; q < 9; q++) hdr[MP_H_RT + (cbest < 2 ? 0 : 9) + q] = R[q];
#pragma unroll
  for (int32_t q = 0; q < 3; q++) hdr[MP_H_RT + 18 + q] = (cbest & 1) ? -t[q] : t[q];
#pragma unroll
  for (int32_t q = 0; q < 12; q++) hdr[MP_H_P2 + 12 * cbest + q] = P2[q];
}

}  // namespace

// grid: a.lists.n_lists workgroups (the caller keeps it below 2^24)
void vh_launch_mono_pose_refine(const VhMonoPoseArgs &a, vh_mono_refine *refine, hipStream_t st) {
  hipLaunchKernelGGL(mono_pose_refine_kernel, dim3(a.lists.n_lists), dim3(MR_T), 0, st, a, refine);
}
