// kernels_mono_pose.hip -- the pose tail of the mono estimator on whole match lists, on gfx950.
//
// For every list of a call, from the epipolar model the list comes with (vh_mono_model: the F of the normalised frame),
// the rest of VisualOdometryMono::estimateMotion (reference src/viso_mono.cpp:83-158): F out of the model's frame, E,
// EtoRt's four (R, t) candidates, triangulateChieral's count over EVERY record, the points in front under the winner,
// smallerThanMedian's median of their L1 distances, the ground-plane vote, the six motion parameters.  The arithmetic
// is the estimator's own (vh_mono_pose.h, shared with kernels_mono.hip); those kernels put one workgroup on a list and
// run the O(N^2) median and vote inside it, which at the thousands of records of a dense inlier list leaves the chip
// idle.  Here every O(N) and O(N^2) step is spread over the list:
//   mono_pose_head    one lane per list: E, the candidates and their projection matrices into the list's header, the
//                     four counts zeroed, the refusals that need no record (no model, fewer than 10 records);
//   mono_pose_tri     one lane per (record, candidate), 64 records per workgroup: a 4x4 decomposition in registers, one
//                     ballot and one integer atomicAdd per wave and candidate; no point is stored;
//   mono_pose_front   one workgroup per list: the winner (the first candidate with the strictly largest count), the
//                     triangulation again under it (the same instructions: the same bits), the points in front compacted
//                     in list order, dist[] and d[];
//   mono_pose_rank    one lane per point i, 256 per workgroup: its rank among all dist[j], ties broken by position; the
//                     lane of rank np / 2 writes the median;
//   mono_pose_vote    one lane per point i: sum_j exp(-(d[j] - d[i])^2 * weight) over all j in ascending order from 0,
//                     four independent exponentials per trip added in the original's order;
//   mono_pose_finish  one wave per list: the first i with the largest sum (a maximum is exact: the lanes take i, i + 64,
//                     .. and the wave keeps the larger sum, the smaller index on ties -- what the ascending scan finds),
//                     scale, tr, the finiteness test, vh_mono_pose.
// rank and vote stage the list through LDS in tiles of VH_MONO_POSE_TILE elements that every workgroup of the list reads
// in the same order; workgroups beyond a list's np return at once.  Every sum and count is in an order fixed by the
// list's length alone (the integer counts are order-free): the same bytes from run to run, whatever else the launch
// holds.  Double precision, built with -ffp-contract=off; exp, asin, cos, sin come from the device library.
#include "vh_dev.h"
#include "vh_wave.h"
#include "vh_mono_pose.h"

namespace {

#define MP_T 256
#define MP_TILE VH_MONO_POSE_TILE
// (the header of a list, MP_H_* / MP_I_*: vh_dev.h)

struct MpList {
  VhList l;
  double *hdr, *dist, *d;
  int32_t *ih;
};
__device__ __forceinline__ MpList mp_list(const VhMonoPoseArgs &a, int32_t s) {
  MpList L;
  L.l = vh_list(a.lists, s);
  L.hdr = a.hdr + (int64_t)s * VH_MONO_POSE_HDR;
  L.ih = (int32_t *)(L.hdr + MP_H_INT);
  const int64_t base = a.lists.offsets ? (int64_t)a.lists.offsets[s] : (int64_t)s * a.slot_stride;
  L.dist = a.dist + base; L.d = a.d + base;
  return L;
}

// ------------------------------------------------------------------ mono_pose_head
__global__ void __launch_bounds__(64)
mono_pose_head_kernel(VhMonoPoseArgs a) {
  const int32_t s = blockIdx.x;
  if (threadIdx.x != 0) return;
  const MpList L = mp_list(a, s);
  for (int32_t c = 0; c < 4; c++) L.ih[c] = 0;
  L.ih[MP_I_BEST] = -1; L.ih[MP_I_NP] = 0;
  L.hdr[MP_H_MED] = 0.0;
  const int32_t reason = !a.ok_in[s] ? 1 : (L.l.n < 10 ? 2 : 0);  // (no model: it is not read) / src/viso_mono.cpp:45
  L.ih[MP_I_REASON] = reason;
  if (reason) return;
  const vh_mono_model m = a.model[s];
  const double sp = m.s[0], sc = m.s[1];
  // normalizeFeaturePoints' matrices (src/viso_mono.cpp:226-227), from the model's centroids and scales
  const double Tp[9] = {sp, 0, -sp * m.c[0], 0, sp, -sp * m.c[1], 0, 0, 1}, Tc[9] = {sc, 0, -sc * m.c[2], 0, sc, -sc * m.c[3], 0, 0, 1};
  const double K[9] = {a.e.f, 0, a.e.cu, 0, a.e.f, a.e.cv, 0, 0, 1};
  double F[9], E[9];
  for (int32_t q = 0; q < 9; q++) F[q] = m.F[q];
  mono_pose_essential(Tp, Tc, K, F, E);
  double *Ra = L.hdr + MP_H_RT;
  mono_pose_candidates(E, K, Ra, Ra + 9, Ra + 18, L.hdr + MP_H_P1, L.hdr + MP_H_P2);
}

// ------------------------------------------------------------------- mono_pose_tri
// grid: tiles * n_lists workgroups, tiles = ceil(cap / 64); lane = (record, candidate) as mono_tri_kernel has it
__global__ void __launch_bounds__(256)
mono_pose_tri_kernel(VhMonoPoseArgs a, int32_t tiles) {
  const int32_t s = blockIdx.x / tiles, tile = blockIdx.x % tiles, tid = threadIdx.x, lane = tid & 63, c = tid & 3;
  const MpList L = mp_list(a, s);
  if (L.ih[MP_I_REASON] != 0 || (int64_t)tile * 64 >= L.l.n) return;
  const int32_t i = tile * 64 + (tid >> 2);
  const double *P1 = L.hdr + MP_H_P1, *P2 = L.hdr + MP_H_P2 + 12 * c;
  bool good = false;
  if (i < L.l.n) {
    const vh_p_match &m = L.l.pm[i];
    double x[4];
    mono_pose_triangulate(P1, P2, m.u1p, m.v1p, m.u1c, m.v1c, x);
    good = mono_pose_in_front_of_both(P1, P2, x);
  }
  const uint64_t bal = __ballot(good);
  if (lane < 4) {  // lane c of each wave adds up the wave's lanes of candidate c
    const int32_t n = __popcll(bal & (0x1111111111111111ull << lane));
    if (n) atomicAdd(L.ih + lane, n);
  }
}

// ----------------------------------------------------------------- mono_pose_front
__global__ void __launch_bounds__(MP_T)
mono_pose_front_kernel(VhMonoPoseArgs a) {
  __shared__ int32_t sWave[MP_T / 64], sBase;
  const int32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const MpList L = mp_list(a, s);
  const int32_t before = L.ih[MP_I_REASON];
  int32_t cnt[4];
  for (int32_t c = 0; c < 4; c++) cnt[c] = L.ih[c];
  if (tid == 0) sBase = 0;
  __syncthreads();  // (every lane has read the header before lane 0 writes to it)
  if (before != 0) return;
  const int32_t cbest = mono_pose_winner(cnt);
  if (cbest < 0) {  // (the reference dereferences an empty matrix here)
    if (tid == 0) L.ih[MP_I_REASON] = 3;
    return;
  }
  // X / X(3,:), the points in front in list order, their L1 distance and ground-plane coordinate (src/viso_mono.cpp:100-128)
  const double *P1 = L.hdr + MP_H_P1, *P2 = L.hdr + MP_H_P2 + 12 * cbest;
  const double n0 = cos(-a.e.pitch), n1 = sin(-a.e.pitch);
  const int32_t N = L.l.n;
  for (int32_t i0 = 0; i0 < N; i0 += MP_T) {
    const int32_t i = i0 + tid;
    double x = 0, y = 0, z = 0;
    if (i < N) {
      const vh_p_match &m = L.l.pm[i];
      double X[4];
      mono_pose_triangulate(P1, P2, m.u1p, m.v1p, m.u1c, m.v1c, X);
      mono_pose_point(X[0], X[1], X[2], X[3], x, y, z);
    }
    const bool front = i < N && z > 0;
    const VhCompact c = vh_compact4(front, sWave, wv, lane);
    if (front) {
      const int32_t p = sBase + c.pos;
      L.dist[p] = mono_pose_dist(x, y, z);
      L.d[p] = mono_pose_plane(n0, n1, y, z);
    }
    __syncthreads();
    if (tid == 0) sBase += c.total;
    __syncthreads();
  }
  if (tid == 0) {
    const int32_t np = sBase;
    L.ih[MP_I_BEST] = cbest; L.ih[MP_I_NP] = np;
    L.hdr[MP_H_MED] = __longlong_as_double(0x7FF8000000000000ll);  // (the median of a list in which no element has rank np / 2: only with NaN distances)
    if (np < 10) L.ih[MP_I_REASON] = 4;  // src/viso_mono.cpp:105
  }
}

// ------------------------------------------------------------------ mono_pose_rank
// smallerThanMedian's median (src/viso_mono.cpp:162-185) as the element of rank np / 2, its rank found by counting:
// elements smaller, or equal and earlier.  grid: tiles * n_lists workgroups, tiles = ceil(cap / MP_T).
__global__ void __launch_bounds__(MP_T)
mono_pose_rank_kernel(VhMonoPoseArgs a, int32_t tiles) {
  __shared__ double sT[MP_TILE];
  const int32_t s = blockIdx.x / tiles, tile = blockIdx.x % tiles, tid = threadIdx.x;
  const MpList L = mp_list(a, s);
  const int32_t np = L.ih[MP_I_NP];
  if (L.ih[MP_I_REASON] != 0 || (int64_t)tile * MP_T >= np) return;  // (the same for the whole workgroup)
  const int32_t i = tile * MP_T + tid;
  const bool mine = i < np;
  const double v = mine ? L.dist[i] : 0.0;
  int32_t rank = 0;
  for (int32_t j0 = 0; j0 < np; j0 += MP_TILE) {
    const int32_t nb = min(MP_TILE, np - j0);
    for (int32_t k = tid; k < nb; k += MP_T) sT[k] = L.dist[j0 + k];
    __syncthreads();
    if (mine) {
      int32_t j = 0;
      for (; j + 8 <= nb; j += 8) {  // (eight loads in flight per trip; the count does not care about the order)
        double o[8];
#pragma unroll
        for (int32_t q = 0; q < 8; q++) o[q] = sT[j + q];
#pragma unroll
        for (int32_t q = 0; q < 8; q++) rank += (o[q] < v || (o[q] == v && j0 + j + q < i)) ? 1 : 0;
      }
      for (; j < nb; j++) { const double o = sT[j]; rank += (o < v || (o == v && j0 + j < i)) ? 1 : 0; }
    }
    __syncthreads();
  }
  if (mine && rank == np / 2) L.hdr[MP_H_MED] = v;
}

// ------------------------------------------------------------------ mono_pose_vote
// The ground-plane vote (src/viso_mono.cpp:124-142): the sum of point i replaces its distance, which is dead.
__global__ void __launch_bounds__(MP_T)
mono_pose_vote_kernel(VhMonoPoseArgs a, int32_t tiles) {
  __shared__ double sT[MP_TILE];
  const int32_t s = blockIdx.x / tiles, tile = blockIdx.x % tiles, tid = threadIdx.x;
  const MpList L = mp_list(a, s);
  const int32_t np = L.ih[MP_I_NP];
  if (L.ih[MP_I_REASON] != 0 || (int64_t)tile * MP_T >= np) return;
  const double median = L.hdr[MP_H_MED];
  if (median > a.e.motion_threshold) return;  // src/viso_mono.cpp:113 (mono_pose_finish reports it)
  const double sigma = median / 50.0, weight = 1.0 / (2.0 * sigma * sigma);
  const int32_t i = tile * MP_T + tid;
  const double di = i < np ? L.d[i] : 0.0;
  const bool active = i < np && di > median / a.e.motion_threshold;
  double sum = 0;
  for (int32_t j0 = 0; j0 < np; j0 += MP_TILE) {
    const int32_t nb = min(MP_TILE, np - j0);
    for (int32_t k = tid; k < nb; k += MP_T) sT[k] = L.d[j0 + k];
    __syncthreads();
    if (active) {
      int32_t j = 0;
      for (; j + 4 <= nb; j += 4) {  // four independent exponentials per trip, added in the original's order
        double t[4];
#pragma unroll
        for (int32_t q = 0; q < 4; q++) { const double dq = sT[j + q] - di; t[q] = exp(-dq * dq * weight); }
#pragma unroll
        for (int32_t q = 0; q < 4; q++) sum += t[q];
      }
      for (; j < nb; j++) { const double q = sT[j] - di; sum += exp(-q * q * weight); }
    }
    __syncthreads();
  }
  if (i < np) L.dist[i] = sum;
}

// ---------------------------------------------------------------- mono_pose_finish
__global__ void __launch_bounds__(64)
mono_pose_finish_kernel(VhMonoPoseArgs a) {
  const int32_t s = blockIdx.x, lane = threadIdx.x;
  const MpList L = mp_list(a, s);
  int32_t reason = L.ih[MP_I_REASON];
  const int32_t cbest = L.ih[MP_I_BEST], np = L.ih[MP_I_NP];
  const double median = reason == 0 ? L.hdr[MP_H_MED] : 0.0;
  if (reason == 0 && median > a.e.motion_threshold) reason = 5;
  double best_sum = 0;
  int32_t best_idx = 0x7FFFFFFF;
  if (reason == 0) {
    for (int32_t i = lane; i < np; i += 64) { const double v = L.dist[i]; if (v > best_sum) { best_sum = v; best_idx = i; } }
#pragma unroll
    for (int32_t d = 32; d >= 1; d >>= 1) {
      const double os = __shfl_xor(best_sum, d);
      const int32_t oi = __shfl_xor(best_idx, d);
      if (os > best_sum || (os == best_sum && oi < best_idx)) { best_sum = os; best_idx = oi; }
    }
    if (best_idx == 0x7FFFFFFF) best_idx = 0;  // (no sum above zero: the reference's best_idx stays 0)
  }
  if (lane != 0) return;
  vh_mono_pose P;
  for (int32_t q = 0; q < 9; q++) P.R[q] = 0.0;
  for (int32_t q = 0; q < 3; q++) P.t[q] = 0.0;
  P.scale = 0.0; P.median = 0.0; P.plane = 0.0;
  for (int32_t c = 0; c < 4; c++) P.chirality[c] = reason >= 3 || reason == 0 ? L.ih[c] : 0;
  P.candidate = -1; P.n_front = 0; P.reserved_ = 0;
  double tr[6] = {0, 0, 0, 0, 0, 0};
  if (reason == 0 || reason >= 4) {
    const double *R = L.hdr + MP_H_RT + (cbest < 2 ? 0 : 9), *t0 = L.hdr + MP_H_RT + 18;
    for (int32_t q = 0; q < 9; q++) P.R[q] = R[q];
    for (int32_t q = 0; q < 3; q++) P.t[q] = (cbest & 1) ? -t0[q] : t0[q];
    P.candidate = cbest; P.n_front = np;
    if (reason != 4) P.median = median;
    if (reason == 0) {
      const double dref = L.d[best_idx];
      P.plane = dref;
      if (fabs(dref) < 1e-20) reason = 6;  // (Matrix::operator/ exits the reference here)
      else {
        P.scale = a.e.height / dref;
        mono_pose_tr(R, t0, cbest, a.e.height, dref, tr);
      }
    }
    bool finite = isfinite(P.median) && isfinite(P.plane);
    for (int32_t q = 0; q < 9; q++) finite = finite && isfinite(P.R[q]);
    for (int32_t q = 0; q < 3; q++) finite = finite && isfinite(P.t[q]);
    for (int32_t q = 0; q < 6; q++) finite = finite && isfinite(tr[q]);
    if (reason == 0 && !finite) reason = 7;
  }
  P.reason = reason;
  for (int32_t q = 0; q < 6; q++) a.tr[6 * (int64_t)s + q] = reason == 0 ? tr[q] : 0.0;
  a.ok[s] = reason == 0 ? 1 : 0;
  a.pose[s] = P;
}

}  // namespace

const char *vh_mono_pose_scope(int32_t k) {
  static const char *const names[VH_MONO_POSE_STAGES] = {"mono_pose_head", "mono_pose_tri", "mono_pose_front", "mono_pose_rank", "mono_pose_vote",
                                                         "mono_pose_finish"};
  return names[k];
}

// The caller keeps n_lists * ceil(cap / 64) below 2^31.  The per-record grids are sized for lists as long as cap; the
// workgroups beyond a list's length (rank, vote: beyond its points in front) return at once.
void vh_launch_mono_pose_stage(const VhMonoPoseArgs &a, int32_t k, hipStream_t st) {
  const int32_t t64 = (int32_t)((a.cap + 63) / 64), t256 = (int32_t)((a.cap + MP_T - 1) / MP_T);
  const uint32_t lists = (uint32_t)a.lists.n_lists;
  switch (k) {
    case 0: hipLaunchKernelGGL(mono_pose_head_kernel, dim3(lists), dim3(64), 0, st, a); break;
    case 1: hipLaunchKernelGGL(mono_pose_tri_kernel, dim3(lists * (uint32_t)t64), dim3(256), 0, st, a, t64); break;
    case 2: hipLaunchKernelGGL(mono_pose_front_kernel, dim3(lists), dim3(MP_T), 0, st, a); break;
    case 3: hipLaunchKernelGGL(mono_pose_rank_kernel, dim3(lists * (uint32_t)t256), dim3(MP_T), 0, st, a, t256); break;
    case 4: hipLaunchKernelGGL(mono_pose_vote_kernel, dim3(lists * (uint32_t)t256), dim3(MP_T), 0, st, a, t256); break;
    default: hipLaunchKernelGGL(mono_pose_finish_kernel, dim3(lists), dim3(64), 0, st, a); break;
  }
}
