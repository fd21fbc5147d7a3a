// engine_lists.h -- the host plumbing every entry point shares, free of HIP: the checks of caller-owned lists (packed
// behind offsets, or strided with counts) and of dims, the carving of one device block into arrays, and the arrays of
// every whole-list stage's block.  Only standard headers and the ABI's codes and records: a plain
// host compiler builds tests/cpp/engine_lists_check.cpp from it.
#ifndef VH_ENGINE_LISTS_H
#define VH_ENGINE_LISTS_H
#include "../../include/viso_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace vh_engine {

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// n lists packed behind offsets[n + 1]: list s is [offsets[s], offsets[s + 1])
struct ListSpan { int64_t first = 0, end = 0, total = 0, longest = 0; };  // offsets[0], offsets[n], their difference, the longest list
// refuses a null pointer, a negative offsets[0] and a decreasing pair; n = 0 judges offsets[0] alone
inline int32_t check_offsets(const int32_t *offsets, int32_t n, ListSpan &out) {
  out = ListSpan();
  if (!offsets || offsets[0] < 0) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n; s++) {
    if (offsets[s + 1] < offsets[s]) return VH_ERR_INVALID_ARG;
    out.longest = std::max<int64_t>(out.longest, (int64_t)offsets[s + 1] - offsets[s]);
  }
  out.first = offsets[0]; out.end = offsets[std::max(n, 0)]; out.total = out.end - out.first;
  return VH_OK;
}

// What the whole-list kernels are launched under (engine.h asserts that they are vh_dev.h's VH_TRACK_POS_MASK and VH_INLIER_TILE)
constexpr int64_t kListMax = (1 << 24) - 1;  // the longest list a handle holds
constexpr int64_t kInlierTile = 1024;
// the launch grid is lists x tiles workgroups of 256 threads
inline bool inlier_grid_ok(int64_t lists, int64_t tiles) { return tiles <= 65535 && lists * tiles < ((int64_t)1 << 24); }
// vh_launch_mono_pose_stage needs lists * ceil(cap / 64) workgroups in one grid dimension
inline bool mono_pose_grid_ok(int64_t lists, int64_t cap) { return lists * ((cap + 63) / 64) < ((int64_t)1 << 30); }

// The checks every packed-list stateless entry shares, in the two steps its refusals come in.  An entry judges its own
// pointers beside packed_args, zeroes its outputs and returns VH_OK at total = 0 between the two, and adds its own limit
// behind packed_limit.
// 1. VH_ERR_INVALID_ARG: what check_offsets refuses, and lists that hold records without a records pointer
inline int32_t packed_args(const int32_t *offsets, int32_t n, const void *pm, ListSpan &out) {
  if (check_offsets(offsets, n, out) || (out.total > 0 && !pm)) return VH_ERR_INVALID_ARG;
  return VH_OK;
}
// 2. VH_ERR_UNSUPPORTED: a list longer than any handle holds, or more classification tiles than one launch grid takes
inline int32_t packed_limit(const ListSpan &sp, int32_t n) {
  if (sp.longest > kListMax || !inlier_grid_ok(n, (sp.longest + kInlierTile - 1) / kInlierTile)) return VH_ERR_UNSUPPORTED;
  return VH_OK;
}

// n strided lists, list l = counts[l] records at l * stride: refuses a null pointer and a count outside [0, stride]
inline int32_t check_counts(const int32_t *counts, int64_t n, int64_t stride, int32_t &longest) {
  longest = 0;
  if (!counts) return VH_ERR_INVALID_ARG;
  for (int64_t l = 0; l < n; l++) {
    if (counts[l] < 0 || counts[l] > stride) return VH_ERR_INVALID_ARG;
    longest = std::max(longest, counts[l]);
  }
  return VH_OK;
}

// {width, height, bytes per line}: positive sides of at most 16384; need_pitch: a line holds its width
inline int32_t check_dims(const int32_t *dims, bool need_pitch) {
  if (!dims || dims[0] <= 0 || dims[1] <= 0 || (need_pitch && dims[2] < dims[0])) return VH_ERR_INVALID_ARG;
  if (dims[0] > 16384 || dims[1] > 16384) return VH_ERR_UNSUPPORTED;
  return VH_OK;
}

// Cuts one block into arrays that each begin on a multiple of 256 bytes, in the order they are taken.  Without a base
// it only measures (ptr gives null), so the size is known before the allocation and the same calls give the pointers after it.
struct Carver {
  uint8_t *base = nullptr;
  size_t next = 0, end = 0;  // where the next array begins / where the last one ends
  explicit Carver(void *b = nullptr) : base((uint8_t *)b) {}
  template <class T> size_t take(size_t count) {  // -> the array's offset
    const size_t o = next;
    end = o + sizeof(T) * count; next = up256(end);
    return o;
  }
  template <class T> T *ptr(size_t count) {
    const size_t o = take<T>(count);
    return base ? (T *)(base + o) : nullptr;
  }
  size_t bytes() const { return next; }  // every array rounded up to 256
  size_t tight() const { return end; }   // the last array as long as it is
};

// The arrays of one classification inside one device block: flags | records | positions | tile counts | counts | ok | tr
struct InlierArrays {
  uint8_t *d_flags = nullptr;   // [slots]
  vh_p_match *d_out = nullptr;  // [slots] the inlier records of each list, in list order
  int32_t *d_src = nullptr;     // [slots] their positions in the list
  int32_t *d_tiles = nullptr;   // [lists][tiles]
  int32_t *d_ninl = nullptr, *d_ok = nullptr;  // [lists]
  double *d_tr = nullptr;       // [lists][6]
  void carve(Carver &c, size_t lists, size_t slots, size_t tiles) {
    d_flags = c.ptr<uint8_t>(slots); d_out = c.ptr<vh_p_match>(slots); d_src = c.ptr<int32_t>(slots);
    d_tiles = c.ptr<int32_t>(lists * tiles); d_ninl = c.ptr<int32_t>(lists); d_ok = c.ptr<int32_t>(lists);
    d_tr = c.ptr<double>(6 * lists);
  }
  // ... at the front of a block at `base` -> the carver behind them: bytes() is the block's size, further takes lie behind the arrays
  Carver carve(void *base, size_t lists, size_t slots, size_t tiles) {
    Carver c(base);
    carve(c, lists, slots, tiles);
    return c;
  }
};

// The records and offsets of a packed-list entry's block: records [offsets[n]] (the slots in front of offsets[0] stay
// unwritten) | offsets [n + 1]
struct PackedArrays {
  vh_p_match *d_pm = nullptr;
  int32_t *d_off = nullptr;
  void carve(Carver &c, const ListSpan &sp, size_t lists) { d_pm = c.ptr<vh_p_match>((size_t)sp.end); d_off = c.ptr<int32_t>(lists + 1); }
};

// ---- the arrays of a handle's first-use blocks, one struct per stage: carve(c, ...) takes them from c in the block's order ----
// The motion refined on the compacted inlier lists (vh_group_refit_motion): the
// kernel joins its partial sums in LDS, so the outputs are all of it.
struct RefitState {
  double *d_tr = nullptr;                      // [S][6]
  int32_t *d_ok = nullptr, *d_nupd = nullptr;  // [S]
  void carve(Carver &c, size_t lists) { d_tr = c.ptr<double>(6 * lists); d_ok = c.ptr<int32_t>(lists); d_nupd = c.ptr<int32_t>(lists); }
};
// The covariance of a motion over the compacted inlier lists (vh_group_motion_covariance): the outputs, and the arrays a caller-given tr / ok go up into.
struct CovState {
  double *d_cov = nullptr;    // [S][36]
  double *d_ssr = nullptr;    // [S]
  int32_t *d_ok = nullptr;    // [S] ok_out
  double *d_tr = nullptr;     // [S][6] the caller's motion (the classification's own stays in inl.d_tr)
  int32_t *d_okin = nullptr;  // [S]
  // what d_cov was last computed under: the match call, the classification (inl.gen), and whether under the
  // classification's own motion (tr = NULL) -- the pose covariance steps under no other
  int64_t seq = -1, gen = -1;
  bool own_tr = false;
  void carve(Carver &c, size_t lists) {
    d_cov = c.ptr<double>(36 * lists); d_ssr = c.ptr<double>(lists); d_ok = c.ptr<int32_t>(lists);
    d_tr = c.ptr<double>(6 * lists); d_okin = c.ptr<int32_t>(lists);
  }
};
// The epipolar model refitted on the compacted inlier lists of a mono classification (vh_group_refit_model_mono, DESIGN.md
// section 4.16): the outputs are all of it.
struct MonoRefitState {
  vh_mono_model *d_model = nullptr;  // [S]
  double *d_w = nullptr;             // [S][2]
  int32_t *d_ok = nullptr;           // [S]
  void carve(Carver &c, size_t lists) { d_model = c.ptr<vh_mono_model>(lists); d_w = c.ptr<double>(2 * lists); d_ok = c.ptr<int32_t>(lists); }
};
// The main block of the mono pose (MonoPoseState, engine.h); hdr: doubles per list header (VH_MONO_POSE_HDR)
struct MonoPoseArrays {
  double *d_dist = nullptr, *d_d = nullptr;  // [slots] ([S][mcap]) the points in front: L1 distance (later the vote's sum), ground-plane coordinate
  double *d_hdr = nullptr;                   // [S][hdr]
  double *d_tr = nullptr;                    // [S][6]
  vh_mono_pose *d_pose = nullptr;            // [S]
  int32_t *d_ok = nullptr;                   // [S]
  void carve(Carver &c, size_t lists, size_t slots, size_t hdr) {
    d_dist = c.ptr<double>(slots); d_d = c.ptr<double>(slots); d_hdr = c.ptr<double>(lists * hdr);
    d_tr = c.ptr<double>(6 * lists); d_pose = c.ptr<vh_mono_pose>(lists); d_ok = c.ptr<int32_t>(lists);
  }
};
// The block of the scene points (SceneState, engine.h)
struct SceneArrays {
  vh_scene_point *d_out = nullptr;  // [slots] ([S][mcap])
  int32_t *d_tiles = nullptr;       // [S][tiles]
  double *d_Tw = nullptr;           // [S][16]
  int32_t *d_n = nullptr;           // [S]
  void carve(Carver &c, size_t lists, size_t slots, size_t tiles) {
    d_out = c.ptr<vh_scene_point>(slots); d_tiles = c.ptr<int32_t>(lists * tiles); d_Tw = c.ptr<double>(16 * lists); d_n = c.ptr<int32_t>(lists);
  }
};
// The block of the landmarks (LandmarkState, engine.h): two state buffers, as the track records have two
struct LandmarkArrays {
  vh_landmark_state *d_state[2] = {nullptr, nullptr};  // [slots] ([S][mcap]) each, indexed by the track buffer
  vh_landmark *d_out = nullptr;     // [slots]
  int32_t *d_obs = nullptr;         // [slots]
  int32_t *d_tiles = nullptr;       // [S][tiles]
  int32_t *d_n = nullptr;           // [S]
  void carve(Carver &c, size_t lists, size_t slots, size_t tiles) {
    d_state[0] = c.ptr<vh_landmark_state>(2 * slots); d_state[1] = d_state[0] ? d_state[0] + slots : nullptr;  // (one array of the five)
    d_out = c.ptr<vh_landmark>(slots); d_obs = c.ptr<int32_t>(slots); d_tiles = c.ptr<int32_t>(lists * tiles); d_n = c.ptr<int32_t>(lists);
  }
  // A sequence handle's block: the rows' states in d_state[0], the carry's (carry_slots records)
  // in d_state[1]; the observation index and the forward links are the halves of one array of 8 bytes per slot.
  int32_t *d_next = nullptr;        // [slots]
  void carve(Carver &c, size_t lists, size_t slots, size_t tiles, size_t carry_slots) {
    d_state[0] = c.ptr<vh_landmark_state>(slots); d_state[1] = c.ptr<vh_landmark_state>(carry_slots);
    d_out = c.ptr<vh_landmark>(slots);
    d_obs = c.ptr<int32_t>(2 * slots); d_next = d_obs ? d_obs + slots : nullptr;
    d_tiles = c.ptr<int32_t>(lists * tiles); d_n = c.ptr<int32_t>(lists);
  }
};
// The block of the trajectory (TrajState, engine.h): the rows' records, and per chain the pose before the current pair and
// the current one
struct TrajArrays {
  vh_traj_pose *d_out = nullptr;                       // [S]
  vh_traj_carry *d_base = nullptr, *d_cur = nullptr;   // [chains]
  void carve(Carver &c, size_t rows, size_t chains) {
    d_out = c.ptr<vh_traj_pose>(rows); d_base = c.ptr<vh_traj_carry>(chains); d_cur = c.ptr<vh_traj_carry>(chains);
  }
};
// The block of the pose covariance (TrajCovState, engine.h): the rows' records, and per chain the carry before the current
// pair and the current one -- TrajArrays' layout
struct TrajCovArrays {
  vh_traj_cov *d_out = nullptr;                            // [S]
  vh_traj_cov_carry *d_base = nullptr, *d_cur = nullptr;   // [chains]
  void carve(Carver &c, size_t rows, size_t chains) {
    d_out = c.ptr<vh_traj_cov>(rows); d_base = c.ptr<vh_traj_cov_carry>(chains); d_cur = c.ptr<vh_traj_cov_carry>(chains);
  }
};
// The caller's index lists of the gain (GainState, engine.h): idx [entries] | ratio [entries] | offsets [S + 1]; the block
// is as long as tight() says
struct GainIndexArrays {
  int32_t *d_idx = nullptr;
  float *d_idx_ratio = nullptr;
  int32_t *d_idx_off = nullptr;
  void carve(Carver &c, size_t entries, size_t lists) { d_idx = c.ptr<int32_t>(entries); d_idx_ratio = c.ptr<float>(entries); d_idx_off = c.ptr<int32_t>(lists + 1); }
};

}  // namespace vh_engine
#endif
