// vh_landmark.h -- the one copy of the landmark rule (include/viso_hip.h, steps 1-5; DESIGN.md sections 4.21 and 4.22):
// the register form of vh_landmark_state, and what one record of a track does to it.  Included by kernels_landmark.hip
// (one lane per record, the predecessor's state gathered) and kernels_landmark_chain.hip (one lane per track head, the
// state carried from row to row), both built with -ffp-contract=off: double, every product and sum rounds on its own,
// sums are added left to right.
#ifndef VH_LANDMARK_H
#define VH_LANDMARK_H
#include "vh_dev.h"

static_assert(sizeof(vh_landmark_state) == 48 && sizeof(vh_scene_point) == 32, "the vector loads and stores below");

// list s of a call's three families (VhLandmarkArgs)
struct LmkList {
  int64_t rec0, pt0, prev0;    // first element of the list in trk / state_out / out / obs, in pts, in prev
  int32_t n, n_pt, n_prev;
};
__device__ __forceinline__ int32_t lmk_count(const int32_t *counts, int32_t s, int64_t stride) {
  return (int32_t)min((int64_t)max(counts[s], 0), stride);
}
__device__ __forceinline__ LmkList lmk_list(const VhLandmarkArgs &a, int32_t s) {
  LmkList L;
  if (a.rec_offsets) { L.rec0 = a.rec_offsets[s]; L.n = a.rec_offsets[s + 1] - a.rec_offsets[s]; }
  else { L.rec0 = (int64_t)s * a.rec_stride; L.n = lmk_count(a.rec_counts, s, a.rec_stride); }
  if (a.pt_offsets) { L.pt0 = a.pt_offsets[s]; L.n_pt = a.pt_offsets[s + 1] - a.pt_offsets[s]; }
  else { L.pt0 = (int64_t)s * a.pt_stride; L.n_pt = lmk_count(a.pt_counts, s, a.pt_stride); }
  L.prev0 = 0; L.n_prev = 0;
  if (a.prev) {
    if (a.prev_offsets) { L.prev0 = a.prev_offsets[s]; L.n_prev = a.prev_offsets[s + 1] - a.prev_offsets[s]; }
    else { L.prev0 = (int64_t)s * a.prev_stride; L.n_prev = lmk_count(a.prev_counts, s, a.prev_stride); }
  }
  return L;
}

struct LmkState {
  double sw, swx, swy, swz;
  int32_t n_obs, n_missed;
};
__device__ __forceinline__ LmkState lmk_zero() { LmkState st; st.sw = st.swx = st.swy = st.swz = 0.0; st.n_obs = st.n_missed = 0; return st; }
__device__ __forceinline__ LmkState lmk_load(const vh_landmark_state *p) {
  const double2 a = ((const double2 *)p)[0], b = ((const double2 *)p)[1];
  const int2 c = ((const int2 *)p)[4];
  LmkState st;
  st.sw = a.x; st.swx = a.y; st.swy = b.x; st.swz = b.y; st.n_obs = c.x; st.n_missed = c.y;
  return st;
}
// the 48 bytes as three 16-byte stores
__device__ __forceinline__ void lmk_store(vh_landmark_state *p, const LmkState &st) {
  double2 *o = (double2 *)p;
  o[0] = make_double2(st.sw, st.swx);
  o[1] = make_double2(st.swy, st.swz);
  ((int4 *)o)[2] = make_int4(st.n_obs, st.n_missed, 0, 0);
}

// One record.  st: the state it carries in (step 1 is the caller's: the predecessor's state, or zeros), the state to
// store out (step 4 is the caller's too).  pt: the record's scene point, null where it has none; its first 16 bytes
// {x, y, z, sigma_z} are loaded here, and only where there is one.  -> the record emits a landmark (step 5).
__device__ __forceinline__ bool lmk_step(LmkState &st, const vh_landmark_params &lp, const vh_scene_point *pt) {
  bool keep = false;
  if (!pt) {                                                         // 2. no observation
    if (st.n_obs > 0) {
      st.n_missed += 1;
      if (lp.max_missed >= 0 && st.n_missed > lp.max_missed) st = lmk_zero();
    }
  } else {                                                           // 3. the observation
    const float4 p = *(const float4 *)pt;
    const double x = p.x, y = p.y, z = p.z, sg = p.w;
    const double wt = sg > 0.0 ? 1.0 / (sg * sg) : 1.0;
    if (st.n_obs > 0) {
      const double T = lp.max_dist + lp.gate_sigma * sg;
      if (T > 0.0) {
        const double dx = x - st.swx / st.sw, dy = y - st.swy / st.sw, dz = z - st.swz / st.sw;
        if (dx * dx + dy * dy + dz * dz > T * T) st = lmk_zero();
      }
    }
    st.sw += wt; st.swx += wt * x; st.swy += wt * y; st.swz += wt * z;
    st.n_obs += 1; st.n_missed = 0;
    if (!(isfinite(st.sw) && isfinite(st.swx) && isfinite(st.swy) && isfinite(st.swz))) st = lmk_zero();
    else keep = st.n_obs >= lp.min_obs;                              // 5.
  }
  return keep;
}

#endif
