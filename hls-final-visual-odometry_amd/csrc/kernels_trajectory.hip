// kernels_trajectory.hip -- the camera's pose in the world accumulated from the motions, on gfx950 (DESIGN.md section
// 4.23): pose = pose * Matrix::inv(motion) row by row along a chain, the rule of vh_trajectory.h.
//
// One workgroup of VH_TRAJ_ROUND lanes per chain, the chain's rows in rounds of VH_TRAJ_ROUND:
//   phase A  one lane per row of the round: T from tr (six sin / cos), the 4x4 Gauss-Jordan elimination in registers, the
//            status; Tinv goes to LDS element-major (sTinv[element][row]: consecutive lanes, consecutive addresses).
//            This is the part of the work that is parallel.
//   phase B  the first 16 lanes, lane e = 4 i + j owning element (i, j) of the running pose P in a register, walk the
//            round's rows in order.  A lane's row of P sits in the four lanes of its quad: a quad-permute DPP move
//            broadcasts each, so the exchange never leaves the VALU; the four products are independent and the four sums
//            the dependent chain of a row.  Column j of the row's Tinv and its status are read from LDS one row ahead.
//            Every lane writes its element of Tw_prev and Tw_cur as it goes, lane 0 the status and the step.
// P, the last accepted Tinv (each lane its column) and step stay in those 16 lanes' registers from round to round and
// leave through carry_out.  Products do not reassociate: no scan over matrices, the order is the demo loop's.
// No atomics, no scratch, no workgroup waits for another.
#include "vh_trajectory.h"
#include "vh_dev.h"

namespace {

// the value of lane 4 * (lane / 4) + K of the caller's quad
template <int K> __device__ __forceinline__ double quad_bcast(double v) {
  constexpr int ctrl = K | (K << 2) | (K << 4) | (K << 6);  // quad_perm:[K, K, K, K]
  const int32_t lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xf, 0xf, false);
  const int32_t hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(VH_TRAJ_ROUND)
trajectory_kernel(VhTrajArgs a) {
  __shared__ double sTinv[16][VH_TRAJ_ROUND];
  __shared__ int32_t sStatus[VH_TRAJ_ROUND];
  const int32_t c = blockIdx.x, tid = threadIdx.x;
  const int64_t row0 = a.offsets ? (int64_t)a.offsets[c] : (int64_t)c * a.rows_per_chain;
  const int64_t n = a.offsets ? (int64_t)a.offsets[c + 1] - row0 : (int64_t)a.rows_per_chain;
  // what the 16 lanes of phase B carry (the other lanes hold the start values and never use them)
  const int32_t e = tid & 15, i = e >> 2, j = e & 3;
  double P = i == j ? 1.0 : 0.0, last[4] = {0.0, 0.0, 0.0, 0.0};
  int32_t step = 0, has_tinv = 0;
  if (a.carry_in) {
    const vh_traj_carry &ci = a.carry_in[c];
    P = ci.Tw[e]; step = ci.step; has_tinv = ci.has_tinv ? 1 : 0;
#pragma unroll
    for (int32_t k = 0; k < 4; k++) last[k] = ci.Tinv[4 * k + j];
  } else if (a.T0) {
    P = a.T0[16 * (int64_t)c + e];
  }
  for (int64_t base = 0; base < n; base += VH_TRAJ_ROUND) {
    const int32_t rows = (int32_t)(n - base < VH_TRAJ_ROUND ? n - base : VH_TRAJ_ROUND);
    __syncthreads();  // phase B of the round before has read its rows
    if (tid < rows) {
      const int64_t k = base + tid, r = row0 + k;
      double tr[6], Tinv[16];
#pragma unroll
      for (int32_t q = 0; q < 6; q++) tr[q] = a.tr[6 * r + q];
      const int32_t ok = (k >= a.pair_lo && k < a.pair_hi) ? a.ok[r] : -1;
      sStatus[tid] = traj_inverse(tr, ok, Tinv);
#pragma unroll
      for (int32_t q = 0; q < 16; q++) sTinv[q][tid] = Tinv[q];
    }
    __syncthreads();
    if (tid < 16) {
      double m[4];
      int32_t status = sStatus[0];
#pragma unroll
      for (int32_t k = 0; k < 4; k++) m[k] = sTinv[4 * k + j][0];
      for (int32_t t = 0; t < rows; t++) {
        // the next row's column and status, under this row's products (the last row of the round reads row 0 again)
        const int32_t tn = t + 1 < rows ? t + 1 : 0;
        double mn[4];
        const int32_t status_n = sStatus[tn];
#pragma unroll
        for (int32_t k = 0; k < 4; k++) mn[k] = sTinv[4 * k + j][tn];
        const int32_t act = traj_action(status, a.p.on_fail, has_tinv);
        if (act == 1) {
#pragma unroll
          for (int32_t k = 0; k < 4; k++) last[k] = m[k];
          has_tinv = 1; step++;
        }
        const double prev = P;
        const double prow[4] = {quad_bcast<0>(P), quad_bcast<1>(P), quad_bcast<2>(P), quad_bcast<3>(P)};
        const double prod = traj_dot(prow, last);  // (act 1 and 2 both multiply by what `last` now holds)
        P = act ? prod : P;
        vh_traj_pose &o = a.out[row0 + base + t];
        o.Tw_prev[e] = prev; o.Tw_cur[e] = P;
        if (e == 0) { o.status = status; o.step = step; o.reserved[0] = 0; o.reserved[1] = 0; }
        status = status_n;
#pragma unroll
        for (int32_t k = 0; k < 4; k++) m[k] = mn[k];
      }
    }
  }
  if (a.carry_out && tid < 16) {
    vh_traj_carry &co = a.carry_out[c];
    co.Tw[e] = P;
#pragma unroll
    for (int32_t k = 0; k < 4; k++) if (i == k) co.Tinv[4 * k + j] = last[k];
    if (e == 0) { co.step = step; co.has_tinv = has_tinv; co.reserved[0] = 0; co.reserved[1] = 0; }
  }
}

}  // namespace

void vh_launch_trajectory(const VhTrajArgs &a, hipStream_t st) {
  if (a.n_chains <= 0) return;
  trajectory_kernel<<<a.n_chains, VH_TRAJ_ROUND, 0, st>>>(a);
}
