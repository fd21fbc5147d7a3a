// kernels_trajectory_cov.hip -- the covariance of the camera's pose propagated along a chain, on gfx950 (DESIGN.md
// section 4.24): Sigma' = Ad (Sigma + Q) Ad^T row by row, the rule of vh_trajectory_cov.h, beside trajectory_kernel and in
// its shape.
//
// One workgroup of VH_TRAJ_COV_ROUND lanes per chain, the chain's rows in rounds of VH_TRAJ_COV_ROUND:
//   phase A  one lane per row of the round: the status (traj_inverse, as the pose kernel forms it), Ad and Q = G C G^T in
//            registers, whether the row has a covariance of its own; the 18 distinct entries of Ad and the 21 of Q go to
//            LDS element-major (sAd[element][row]), entry 18 of sAd being the zero every zero of Ad is read from.
//   phase B  the first wave, lane 6 i + j owning Sigma[i][j] in a register, walks the round's rows in order.  S = Sigma + Q
//            is lane-local.  U[i][j] = sum_k Ad[i][k] S[k][j] needs column j of S, Sigma'[a][b] = sum_k U[a][k] Ad[b][k]
//            (a = min(i, j), b = max(i, j): both lanes of a mirrored pair form the same sum, so Sigma' is symmetric without
//            a third exchange) needs row a of U: six ds_bpermute pairs each, the values never pass through memory.  Row
//            i and row b of the row's Ad, its element of Q, status and flag are read from LDS one row ahead.  Lanes 36..63
//            walk along as copies of lanes 0..27 (a shuffle reads active lanes only) and store nothing.
// Sigma, Ad_last (each lane its two rows), Q_last (each lane its element) and the counters stay in registers from round to
// round and leave through carry_out.  No scan over matrices, no atomics, no scratch, no workgroup waits for another.
#include "vh_trajectory_cov.h"
#include "vh_dev.h"

namespace {

__global__ void __launch_bounds__(VH_TRAJ_COV_ROUND)
trajectory_cov_kernel(VhTrajCovArgs a) {
  __shared__ double sAd[VH_TRAJ_COV_AD + 1][VH_TRAJ_COV_ROUND];
  __shared__ double sQ[VH_TRAJ_COV_Q][VH_TRAJ_COV_ROUND];
  __shared__ int32_t sStatus[VH_TRAJ_COV_ROUND];   // status | own << 8
  const int32_t c = blockIdx.x, tid = threadIdx.x;
  const int64_t row0 = a.offsets ? (int64_t)a.offsets[c] : (int64_t)c * a.rows_per_chain;
  const int64_t n = a.offsets ? (int64_t)a.offsets[c + 1] - row0 : (int64_t)a.rows_per_chain;
  // what the lanes of phase B carry (the other lanes hold the start values and never use them)
  const int32_t e = (tid & 63) < 36 ? (tid & 63) : (tid & 63) - 36, i = e / 6, j = e % 6;
  const int32_t lo = i < j ? i : j, hi = i < j ? j : i, qe = traj_cov_sym(i, j);
  const bool owner = tid < 36;
  int32_t ixi[6], ixb[6];   // where row i and row hi of Ad lie in sAd
#pragma unroll
  for (int32_t k = 0; k < 6; k++) { ixi[k] = traj_cov_ad_index(i, k); ixb[k] = traj_cov_ad_index(hi, k); }
  double Sg = 0.0, qlast = 0.0, lasti[6], lastb[6];
#pragma unroll
  for (int32_t k = 0; k < 6; k++) { lasti[k] = 0.0; lastb[k] = 0.0; }
  int32_t step = 0, has_ad = 0, has_q = 0, n_filled = 0;
  if (a.carry_in) {
    const vh_traj_cov_carry &ci = a.carry_in[c];
    Sg = ci.cov[e]; qlast = ci.Q_last[e]; n_filled = ci.n_filled; step = ci.step; has_ad = ci.has_ad ? 1 : 0; has_q = ci.has_q ? 1 : 0;
#pragma unroll
    for (int32_t k = 0; k < 6; k++) { lasti[k] = ci.Ad_last[6 * i + k]; lastb[k] = ci.Ad_last[6 * hi + k]; }
  } else if (a.Sigma0) {
    Sg = a.Sigma0[36 * (int64_t)c + e];
  }
  sAd[VH_TRAJ_COV_AD][tid] = 0.0;
  for (int64_t base = 0; base < n; base += VH_TRAJ_COV_ROUND) {
    const int32_t rows = (int32_t)(n - base < VH_TRAJ_COV_ROUND ? n - base : VH_TRAJ_COV_ROUND);
    __syncthreads();  // phase B of the round before has read its rows
    if (tid < rows) {
      const int64_t k = base + tid, r = row0 + k;
      double tr[6], Tinv[16];
#pragma unroll
      for (int32_t q = 0; q < 6; q++) tr[q] = a.tr[6 * r + q];
      const int32_t ok = (k >= a.pair_lo && k < a.pair_hi) ? a.ok[r] : -1;
      const int32_t status = traj_inverse(tr, ok, Tinv);
      double Ad[VH_TRAJ_COV_AD], Q[VH_TRAJ_COV_Q];
      int32_t own = 0;
      if (status == VH_TRAJ_ACCEPTED) {
        double C[36];
#pragma unroll
        for (int32_t q = 0; q < 36; q++) C[q] = a.cov[36 * r + q];
        own = traj_cov_row(tr, C, a.ok_cov[r], Ad, Q);
      } else {
#pragma unroll
        for (int32_t q = 0; q < VH_TRAJ_COV_AD; q++) Ad[q] = 0.0;
#pragma unroll
        for (int32_t q = 0; q < VH_TRAJ_COV_Q; q++) Q[q] = 0.0;
      }
      sStatus[tid] = status | (own << 8);
#pragma unroll
      for (int32_t q = 0; q < VH_TRAJ_COV_AD; q++) sAd[q][tid] = Ad[q];
#pragma unroll
      for (int32_t q = 0; q < VH_TRAJ_COV_Q; q++) sQ[q][tid] = Q[q];
    }
    __syncthreads();
    if (tid < 64) {
      double mi[6], mb[6], mq = sQ[qe][0];
      int32_t word = sStatus[0];
#pragma unroll
      for (int32_t k = 0; k < 6; k++) { mi[k] = sAd[ixi[k]][0]; mb[k] = sAd[ixb[k]][0]; }
      for (int32_t t = 0; t < rows; t++) {
        // the next row's operands, under this row's products (the last row of the round reads row 0 again)
        const int32_t tn = t + 1 < rows ? t + 1 : 0;
        double ni[6], nb[6];
        const double nq = sQ[qe][tn];
        const int32_t word_n = sStatus[tn];
#pragma unroll
        for (int32_t k = 0; k < 6; k++) { ni[k] = sAd[ixi[k]][tn]; nb[k] = sAd[ixb[k]][tn]; }
        const int32_t status = word & 255, own = word >> 8;
        const int32_t act = traj_action(status, a.p.on_fail, has_ad);
        if (act == 1) {
#pragma unroll
          for (int32_t k = 0; k < 6; k++) { lasti[k] = mi[k]; lastb[k] = mb[k]; }
          has_ad = 1; step++;
        }
        const bool mine = act == 1 && own;
        if (mine) { qlast = mq; has_q = 1; }
        if (act && !mine) n_filled++;
        const double S = Sg + (mine ? mq : a.fill_scale * qlast);
        double scol[6], urow[6];
#pragma unroll
        for (int32_t k = 0; k < 6; k++) scol[k] = __shfl(S, 6 * k + j);
        const double U = traj_cov_dot(lasti, scol);  // (act 1 and 2 both step with what `last` now holds)
#pragma unroll
        for (int32_t k = 0; k < 6; k++) urow[k] = __shfl(U, 6 * lo + k);
        const double next = traj_cov_dot(urow, lastb);
        Sg = act ? next : Sg;
        if (owner) {
          vh_traj_cov &o = a.out[row0 + base + t];
          o.cov[e] = Sg;
          if (e == 0) { o.status = status; o.step = step; o.n_filled = n_filled; o.reserved = 0; }
        }
        word = word_n; mq = nq;
#pragma unroll
        for (int32_t k = 0; k < 6; k++) { mi[k] = ni[k]; mb[k] = nb[k]; }
      }
    }
  }
  if (a.carry_out && owner) {
    vh_traj_cov_carry &co = a.carry_out[c];
    co.cov[e] = Sg; co.Q_last[e] = qlast;
    if (j == 0) {
#pragma unroll
      for (int32_t k = 0; k < 6; k++) co.Ad_last[6 * i + k] = lasti[k];
    }
    if (e == 0) { co.n_filled = n_filled; co.has_ad = has_ad; co.has_q = has_q; co.step = step; }
  }
}

}  // namespace

void vh_launch_trajectory_cov(const VhTrajCovArgs &a, hipStream_t st) {
  if (a.n_chains <= 0) return;
  trajectory_cov_kernel<<<a.n_chains, VH_TRAJ_COV_ROUND, 0, st>>>(a);
}
