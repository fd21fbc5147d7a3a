// kernels_lmk_refit.hip -- the stereo motion refined on whole match lists with the landmarks as the 3-d prior, on gfx950
// (DESIGN.md section 4.25).
//
//   refit_prior      one lane per record, tiles of LRF_T records, grid = lists x tiles as kernels_landmark.hip's: the
//                    record's own point of the previous pair (ego_observe), its position in the predecessor list
//                    (prev_pos, or the track record's prev through src_pos), at most one 48-byte state gathered from
//                    that list, the rule of vh_refit_prior.h, the 32-byte prior written as two 16-byte stores; a wave
//                    counts its source == 1 records (ballot) and lane 0 adds the count to n_used[list]: an integer
//                    sum, the same whatever the order.
//   refit_prior_fit  kernels_refit.hip's loop from the same vh_ego.h calls -- one LRF_T-lane workgroup per list, the
//                    whole Gauss-Newton loop inside the launch, the rotation in scalar registers, lane t adding the
//                    records t, t + LRF_T, .. in ascending order, vh_wave_sum, thread 0 adding the waves' totals and
//                    solving, three barriers per update -- with X, Y, Z loaded from the prior (32 bytes) beside the two
//                    record words that hold u1c, v1c, u2c, v2c, in the place of three words and ego_observe.
// Double precision, built with -ffp-contract=off.  The order of additions is a function of the list's length alone, and
// the same function as refit_kernel's: a list whose records all fall back gives refit_kernel's bytes.  Plain vector
// stores, no floating-point atomic, nothing waits for another workgroup.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_refit_prior.h"

namespace {

#define LRF_T VH_SCENE_TILE
#define LRF_W (LRF_T / 64)
static_assert(LRF_T == VH_REFIT_THREADS, "refit_prior_fit adds in refit_kernel's order");
static_assert(sizeof(vh_refit_prior) == 32 && sizeof(vh_landmark_state) == 48 && sizeof(vh_p_match) == 48 && sizeof(vh_track) == 24,
              "the vector loads and stores below");

// first element of list s in prior / prev_pos / src_pos
__device__ __forceinline__ int64_t lrf_first(const VhLists &l, int32_t s) { return l.offsets ? (int64_t)l.offsets[s] : (int64_t)s * l.pm_stride; }

__device__ __forceinline__ int32_t lrf_count(const int32_t *counts, int32_t s, int64_t stride) {
  return (int32_t)min((int64_t)max(counts[s], 0), stride);
}

__global__ void __launch_bounds__(LRF_T)
refit_prior_kernel(VhLmkRefitArgs a) {
  const int32_t s = blockIdx.x / a.tiles_per_list, tile = blockIdx.x % a.tiles_per_list;
  const int32_t tid = threadIdx.x, lane = tid & 63;
  const VhList L = vh_list(a.lists, s);
  if ((int64_t)tile * LRF_T >= L.n) return;  // (uniform)
  const int64_t i = (int64_t)tile * LRF_T + tid;
  bool used = false;
  if (i < L.n) {
    const int64_t r = lrf_first(a.lists, s) + i;
    // {u1p, v1p, i1p, u2p}: the previous pair's columns are all the own point reads
    const float4 q0 = *(const float4 *)(L.pm + i);
    const EgoObs own = ego_observe(a.e, q0.x, q0.y, q0.w, 0.f, 0.f, 0.f, 0.f);
    int32_t p = -1;
    if (a.prev_pos) p = a.prev_pos[r];
    else {
      const int32_t j = a.src_pos[r];
      if (j >= 0 && j < lrf_count(a.trk_counts, s, a.slot_stride)) p = a.trk[(int64_t)s * a.slot_stride + j].prev;
    }
    int64_t prev0 = 0;
    int32_t n_prev = 0;
    if (a.prev) {
      if (a.prev_offsets) { prev0 = a.prev_offsets[s]; n_prev = a.prev_offsets[s + 1] - a.prev_offsets[s]; }
      else { prev0 = (int64_t)s * a.prev_stride; n_prev = lrf_count(a.prev_counts, s, a.prev_stride); }
    }
    VhPriorState st;
    st.in_range = p >= 0 && p < n_prev;
    st.sw = st.swx = st.swy = st.swz = 0.0; st.n_obs = 0;
    if (st.in_range) {
      const vh_landmark_state *q = a.prev + prev0 + p;
      const double2 u = ((const double2 *)q)[0], v = ((const double2 *)q)[1];
      st.sw = u.x; st.swx = u.y; st.swy = v.x; st.swz = v.y; st.n_obs = ((const int2 *)q)[4].x;
    }
    const vh_refit_prior pr = vh_refit_prior_point(own, st, a.Tw + 16 * (int64_t)s, a.rp);
    double2 *o = (double2 *)(a.prior + r);
    o[0] = make_double2(pr.X, pr.Y);
    o[1] = make_double2(pr.Z, __longlong_as_double((long long)(((uint64_t)(uint32_t)pr.reason << 32) | (uint32_t)pr.source)));
    used = pr.source == 1;
  }
  const int32_t cnt = __popcll(__ballot(used));
  if (lane == 0 && cnt) atomicAdd(a.n_used + s, cnt);
}

// a value that is the same on every lane of the wave, moved to scalar registers
__device__ __forceinline__ double lrf_uniform(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__global__ void __launch_bounds__(LRF_T)
refit_prior_fit_kernel(VhLmkRefitArgs a) {
  __shared__ double sAcc[LRF_W][27];
  __shared__ double sRot[36], sTr[6];
  __shared__ int32_t sFlag;
  const int32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const VhList L = vh_list(a.lists, s);
  const int32_t n = L.n;
  if (!a.ok_in[s] || n < 6) {  // vh_refit_motion's refusals; tr_in is not read
    if (tid == 0) { a.ok_out[s] = 0; a.n_updates[s] = 0; for (int32_t m = 0; m < 6; m++) a.tr_out[6 * (int64_t)s + m] = 0; }
    return;
  }
  const vh_refit_prior *prior = a.prior + lrf_first(a.lists, s);
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
      R.r[m] = lrf_uniform(sRot[m]); R.drx[m] = lrf_uniform(sRot[9 + m]);
      R.dry[m] = lrf_uniform(sRot[18 + m]); R.drz[m] = lrf_uniform(sRot[27 + m]);
    }
#pragma unroll
    for (int32_t m = 0; m < 6; m++) tr[m] = lrf_uniform(sTr[m]);
    double acc[27];
#pragma unroll
    for (int32_t q = 0; q < 27; q++) acc[q] = 0;
    for (int32_t i = tid; i < n; i += LRF_T) {
      // {v2p, i2p, u1c, v1c} {i1c, u2c, v2c, i2c} of the record, {X, Y} {Z, ..} of its prior
      const float4 *p = (const float4 *)(L.pm + i);
      const float4 q1 = p[1], q2 = p[2];
      const double2 xy = *(const double2 *)(prior + i);
      EgoObs o;
      o.X = xy.x; o.Y = xy.y; o.Z = prior[i].Z;
      o.u1c = q1.z; o.v1c = q1.w; o.u2c = q2.y; o.v2c = q2.z;
      ego_accumulate(a.e, R, tr, o, acc);
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
        for (int32_t k = 1; k < LRF_W; k++) v += sAcc[k][q];
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

hipError_t vh_launch_refit_prior(const VhLmkRefitArgs &a, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(a.n_used, 0, sizeof(int32_t) * (size_t)a.lists.n_lists, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(refit_prior_kernel, dim3((uint32_t)a.lists.n_lists * (uint32_t)a.tiles_per_list), dim3(LRF_T), 0, st, a);
  return hipSuccess;
}

void vh_launch_refit_prior_fit(const VhLmkRefitArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(refit_prior_fit_kernel, dim3(a.lists.n_lists), dim3(LRF_T), 0, st, a);
}
