// engine.h -- the Group behind a vh_group / vh_matcher handle, shared by the engine*.hip units:
//   engine.hip        allocation, geometry, the ring and both push paths, profiling, creation
//   engine_match.hip  loop policy, matching (tables and ranged), prior, multi-stage ranges, tracks, load_features
//   engine_post.hip   downloads and getters, outlier removal, estimators, the post pipelines, bucketing, statistics
//   engine_api.hip    the extern "C" ABI of include/viso_hip.h and the stateless primitives
//   vh_poison.h       VH_POISON=1 (test aid): what every allocation below, and vh_vote.h's, fills its fresh buffer with
//   engine_lists.h    free of HIP: the checks of caller-owned lists and of dims, the carving of one block into arrays, the stages' arrays
//   engine_cov.hip    the covariance of a motion over whole lists (kernels_cov.hip) and its part of the ABI
//   engine_mono_refit.hip  the epipolar model refitted on whole lists (kernels_mono_refit.hip) and its part of the ABI
//   engine_mono_pose.hip   the mono pose tail on whole lists (kernels_mono_pose.hip) and its part of the ABI
//   engine_scene.hip  the 3-d points of whole lists (kernels_scene.hip) and their part of the ABI
//   engine_landmark.hip  the scene points fused along the tracks (kernels_landmark.hip, kernels_landmark_chain.hip) and their part of the ABI
//   engine_trajectory.hip  the camera's pose accumulated from the motions (kernels_trajectory.hip) and its part of the ABI
//   engine_trajectory_cov.hip  the pose's covariance along the same chains (kernels_trajectory_cov.hip) and its part of the ABI
//   engine_lmk_refit.hip  the motion refined with the landmarks as the 3-d prior (kernels_lmk_refit.hip) and its part of the ABI
//   engine_inlier.hip motion inliers of the lists (kernels_inlier.hip), the motion refined on them (kernels_refit.hip) and
//                     their part of the ABI
//   engine_gain.hip   the camera gain over the lists (kernels_gain.hip) and its part of the ABI
#ifndef VH_ENGINE_H
#define VH_ENGINE_H
#include "vh_dev.h"
#include "../../include/viso_hip.h"
#include "vh_poison.h"
#include "vh_vote.h"
#include "vh_recon.h"
#include "engine_lists.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace vh_engine {

// Ring slots per stream.  Three are the minimum for detecting frame t+1 while frame t is matched
// against t-1 -- but then the detection of t+2 overwrites the slot of t-1 and has to wait for the
// emission of match t, and the search of t+2 for that detection: both chains idle ~6 % of a step
// (rocprofv3 timeline, KITTI, S = 256).  With four, detection runs a whole frame ahead and neither
// stream waits for the other.  VH_RING=3 rebuilds the old ring.
#ifndef VH_RING
#define VH_RING 4
#endif
static_assert(VH_RING >= 3 && VH_RING <= 8, "ring slots");

extern thread_local std::string t_last_error;  // (defined in engine.hip)

#define VH_HIP(call)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      t_last_error = std::string(#call) + ": " + hipGetErrorString(e_);                       \
      return VH_ERR_HIP;                                                                      \
    }                                                                                         \
  } while (0)

// every extern "C" entry on a handle begins with it
#define ENTER(gq)                                   \
  if (!(gq)) return VH_ERR_INVALID_ARG;             \
  { hipError_t e_ = hipSetDevice((gq)->device);     \
    if (e_ != hipSuccess) { t_last_error = hipGetErrorString(e_); return VH_ERR_HIP; } }

inline int32_t round_up(int32_t x, int32_t m) { return (x + m - 1) / m * m; }

// ---- owners: move-only, each releases what it holds in its destructor and on reset() / assignment of {} ------------
// page-locked host memory; `dev` is its device address when it was allocated hipHostMallocMapped
template <class T> struct HostBlock {
  T *p = nullptr;
  void *dev = nullptr;
  HostBlock() = default;
  HostBlock(HostBlock &&o) noexcept : p(o.p), dev(o.dev) { o.p = nullptr; o.dev = nullptr; }
  HostBlock &operator=(HostBlock &&o) noexcept { std::swap(p, o.p); std::swap(dev, o.dev); return *this; }
  ~HostBlock() { reset(); }
  void reset() { if (p) (void)hipHostFree(p); p = nullptr; dev = nullptr; }
  hipError_t alloc(size_t count, unsigned flags) {
    reset();
    hipError_t e = hipHostMalloc((void **)&p, sizeof(T) * count, flags);
    if (e != hipSuccess) p = nullptr;
    else {
      vh_poison_host(p, sizeof(T) * count);
      if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer(&dev, p, 0);
    }
    return e;
  }
  operator T *() const { return p; }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
  Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }  // (lazy sites call it every time)
  operator hipEvent_t() const { return e; }
};
// `owned` is false for a handle that aliases another stream (match / post stream of a small group)
struct Stream {
  hipStream_t s = nullptr;
  bool owned = false;
  Stream() = default;
  Stream(Stream &&o) noexcept : s(o.s), owned(o.owned) { o.s = nullptr; }
  Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); std::swap(owned, o.owned); return *this; }
  ~Stream() { if (s && owned) (void)hipStreamDestroy(s); }
  hipError_t create() { owned = true; return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  hipError_t create(int priority) { owned = true; return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
  void alias(hipStream_t o) { s = o; owned = false; }
  operator hipStream_t() const { return s; }
};
// one hipMalloc'ed block: an entry of a group's arena (Group::allocs), or a block outside it
struct DeviceBlock {
  void *p = nullptr;
  DeviceBlock() = default;
  explicit DeviceBlock(void *q) : p(q) {}
  DeviceBlock(DeviceBlock &&o) noexcept : p(o.p) { o.p = nullptr; }
  DeviceBlock &operator=(DeviceBlock &&o) noexcept { std::swap(p, o.p); return *this; }
  ~DeviceBlock() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) {
    *this = DeviceBlock();
    const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 1));
    if (e != hipSuccess) { p = nullptr; return e; }
    return vh_poison_device(p, bytes);  // (a block its owner zeroes is poisoned first and zeroed second)
  }
  template <class T> T *as() const { return (T *)p; }
};
// The one device block of a stateless entry.  The entry describes its arrays once, in a function over a Carver (DESIGN.md
// section 4.0): alloc calls it without a base to measure, allocates, and calls it again to bind the pointers.  The copies
// are blocking; every member answers with HIP's code, for VH_HIP.
struct StagedBlock {
  DeviceBlock blk;
  template <class F> hipError_t alloc(F &&arrays) {
    Carver measure;
    arrays(measure);
    const hipError_t e = blk.alloc(measure.bytes());
    if (e != hipSuccess) return e;
    Carver bind(blk.p);
    arrays(bind);
    return hipSuccess;
  }
  template <class T> static hipError_t up(T *dev, const T *host, size_t count) { return hipMemcpy(dev, host, sizeof(T) * count, hipMemcpyHostToDevice); }
  template <class T> static hipError_t down(T *host, const T *dev, size_t count) { return hipMemcpy(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost); }
  // the records [offsets[0], offsets[n]) to the slots of the same numbers, and the n + 1 offsets
  static hipError_t up_lists(const PackedArrays &d, const vh_p_match *pm, const int32_t *offsets, const ListSpan &sp, size_t lists) {
    const hipError_t e = sp.total > 0 ? up(d.d_pm + sp.first, pm + sp.first, (size_t)sp.total) : hipSuccess;
    return e != hipSuccess ? e : up(d.d_off, offsets, lists + 1);
  }
};
// VhVoteBuffers (vh_vote.h) is released by hand; this one releases itself
struct VoteBuffers : VhVoteBuffers {
  VoteBuffers() = default;
  VoteBuffers(VoteBuffers &&o) noexcept : VhVoteBuffers(o) { static_cast<VhVoteBuffers &>(o) = VhVoteBuffers{}; }
  VoteBuffers &operator=(VoteBuffers &&o) noexcept { std::swap<VhVoteBuffers>(*this, o); return *this; }
  ~VoteBuffers() { release(); }
};

struct ProfEntry {
  std::vector<std::pair<Event, Event>> pending;
  double ms = 0;
  int64_t launches = 0;
};

// ---- the arena-owned pointers of a group, with the sizes and flags that go with them, one struct per feature: ------
// Group::release() resets each by assignment
struct DetectScratch {
  uint64_t *d_rec = nullptr;
  int32_t *d_chunk_count = nullptr;
  uint8_t *d_half = nullptr;  // half-resolution images [S*2]
};
struct MatchTables {
  int32_t *d_best = nullptr, *d_best2[2] = {nullptr, nullptr};
  int4 *d_chain = nullptr, *d_chain2[2] = {nullptr, nullptr};
  int32_t *d_mchunk2[2] = {nullptr, nullptr};  // [S][cap/256] survivors per emission chunk, one buffer per match-table buffer (each launch's emission zeroes the other one)
  int32_t *d_redo = nullptr;     // [2][S] queries the speculative searches had to search again, per table buffer (reset by emit_matches)
  float4 *d_ref2[2] = {nullptr, nullptr};  // refinement > 0: the refined coordinates of each match-table buffer ([S][cap][2] float4)
  uint32_t *d_mask = nullptr;
  uint32_t epoch = 0;
  // A buffer that was allocated but not cleared yet: set at the allocation, reset only once the clearing memsets are queued,
  // so a match call that fails between the two leaves the duty to the next one
  bool mask_fresh = false;       // the flow method's pixel mask (mask_epoch())
  void *d_matches = nullptr;
  int32_t *d_match_count = nullptr;
  int32_t *d_overflow = nullptr; // [S] 1: a feature set of the stream's last match held more records than cap
  HostBlock<int32_t> h_overflow; // page-locked mirror for the asynchronous download
  // per stream {match count, overflow flag, queries searched again, queries searched} of the last launch on each
  // buffer, written by emit_matches into host-mapped page-locked memory: valid after ev_post[buf]
  HostBlock<int4> h_out[2];
  // small groups (serial): the match records are written to host-mapped memory as well, so getMatches is an
  // event wait and a host copy instead of a device->host transfer of its own
  HostBlock<vh_p_match> h_matches;
  bool ev_down_valid = false;    // a download of the lists is (or was) in flight: the next emission waits for ev_down
  bool stats_pending[2] = {false, false}, stats_was_spec[2] = {false, false};
  int32_t stats_npass[2] = {0, 0};
  int32_t tiles_hint = 0;  // query tiles per (pass, stream) row seen by an earlier launch (0: none yet)
};
// host-image staging, S images per camera, two slots: the upload of frame t+1
// does not wait for the detection of frame t, only for that of frame t-1
struct Staging {
  uint8_t *d_stage_buf[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  uint8_t *d_stage[2] = {nullptr, nullptr};  // the slot of the last push_host
  bool ev_stage_valid[2] = {false, false};
  size_t stage_bytes = 0;
};
// tr16 of match(): [S][16] row-major motion estimates for the quad method's prior (kernels_prior.hip)
struct Prior {
  double *d_prior_tr = nullptr;
  HostBlock<double> h_prior_tr;  // page-locked staging, two slots (one per table buffer): the caller's array is only borrowed
};
struct TrackTables {
  uint32_t *d_ttab = nullptr, *d_ttabp = nullptr;  // [slots][cap] bids by i1c; [S][cap] bids by i1p
  vh_track *d_trk = nullptr;                       // [slots][mcap]
  int32_t *d_tcount = nullptr;                     // [slots]
  bool trk_fresh = false;  // allocated, not cleared yet (as MatchTables::mask_fresh; trk_queue() clears them on the post stream)
};
// The group estimators' scratch (random values, 3-d points, results) belongs to the group and only grows: a
// hipFree per call would drain the detect/match/post pipeline (it synchronises the device).
struct EgoScratch {
  int32_t *d_ego_rand = nullptr, *d_ego_ok = nullptr;
  double *d_ego_xyz = nullptr, *d_ego_tr = nullptr;
  size_t ego_rand_n = 0;
  uint8_t *d_mono_scratch = nullptr;
  int32_t *d_mono_rand = nullptr;
  vh_mono_model *d_mono_model = nullptr;  // [S] vh_group_estimate_motion_mono_model's output, allocated by its first call
  size_t mono_rand_n = 0;
  int32_t mono_scratch_iters = 0;
};
struct PostSlot {
  HostBlock<vh_p_match> h_pm;   // page-locked [S][cap_ps]
  HostBlock<int32_t> h_cnt;     // page-locked [S] (+ [S] overflow flags)
  int32_t cap_ps = 0, width = 0, method = -1;  // allocated / downloaded records per stream
  Event ev;
  bool pending = false;
};
struct HostPost {
  PostSlot slot[2];
  HostBlock<vh_p_match> h_bucket;  // [S][bcap]
  vh_p_match *d_bucket = nullptr;
  HostBlock<int32_t> h_bcnt;
  int32_t *d_bcnt = nullptr, bcap = 0;
  int32_t *d_post_rand = nullptr; size_t post_rand_n = 0;
  uint8_t *d_post_mono = nullptr; int32_t post_mono_iters = 0;
  double *d_post_xyz = nullptr, *d_post_tr = nullptr; int32_t *d_post_ok = nullptr;
};
struct Ranges {
  int32_t *d_ranges = nullptr;   // [S][ubn * vbn][4 stages][4] integer windows
  HostBlock<int32_t> h_ranges;   // page-locked staging
};

// The per-frame tables of Reconstruction (vh_recon.h), built one frame at a time (engine_recon.hip: recon_table_push)
struct ReconTable {
  double total[16], inv[16];   // Tr_total.back() and its inverse
  int64_t first = 0;           // frame of frames[0]
  std::vector<double> frames;  // VH_RECON_FRAME_DOUBLES per frame
  int64_t count() const { return (int64_t)(frames.size() / VH_RECON_FRAME_DOUBLES); }
};
// Reconstruction on a sequence handle or a group (vh_sequence_set_reconstruction, vh_group_set_reconstruction;
// engine_recon.hip, DESIGN.md sections 4.8 and 4.9): the ring of compact records and the gather buffers, outside the
// arena (the gather buffers grow), counted in `bytes`.  vh_reconstruct_lists runs on a transient one.
// A "frame" is a frame of a sequence handle or a step of a group; it holds `lists` lists: 1, or one per stream.
struct ReconHistory {
  bool on = false;
  vh_recon_params params{};
  int32_t history = 0;
  // the chunk (group: the step, a chunk of one row) of the last match call, recorded when it was queued
  bool m_valid = false, m_done = false;
  bool replaced = false;  // group: a replace push since the last match call -- the next lists have no predecessor
  int64_t m_first = 0;
  int32_t m_lo = 0, m_rows = 0, m_buf = 0;  // (m_buf: group, the track buffer of that step's lists)
  int32_t pushes_since_match = 0;
  // the chain of lists stored so far: unbroken up to frame `last`; has_pending: the list of frame `last` is in the ring
  bool chain = false, has_pending = false;
  int64_t last = 0;
  std::vector<ReconTable> tables;      // one per stream, all over the same frames
  std::vector<vh_recon_track> result;  // of the last call: stream after stream, each sorted
  std::vector<int32_t> res_off, accepted;  // [lists + 1] where each stream's records begin / [lists] its accepted ones
  // device
  DeviceBlock b_ring, b_count, b_totals;
  int32_t ring_slots = 0, ring_lists = 0, ring_cap = 0;  // frames, lists per frame, records per list
  struct Grown { DeviceBlock b; size_t bytes = 0; } g_tails, g_first, g_off, g_order, g_px, g_pts, g_st, g_met, g_frames;
  int64_t bytes = 0;
  void drop_chain() { chain = has_pending = false; }
  void release_device() {  // (the work using it must have completed)
    b_ring = DeviceBlock(); b_count = DeviceBlock(); b_totals = DeviceBlock();
    for (Grown *g : {&g_tails, &g_first, &g_off, &g_order, &g_px, &g_pts, &g_st, &g_met, &g_frames}) { g->b = DeviceBlock(); g->bytes = 0; }
    ring_slots = ring_lists = ring_cap = 0; bytes = 0;
    drop_chain(); m_valid = m_done = false;
  }
};

// Which per-record test a classification launches, with what the caller gave for it: VisualOdometryStereo::getInlier
// under tr[lists][6], or VisualOdometryMono::getInlier under model[lists].
struct InlierTest {
  const vh_ego_params *ego = nullptr;
  const double *tr = nullptr;
  const vh_mono_params *mono = nullptr;
  const vh_mono_model *model = nullptr;
  bool is_mono = false;
  bool on_device = false;  // tr (mono: model) and ok are what the handle's block holds already (Group::refit_motion, refit_model_mono); nothing goes up
  static InlierTest stereo(const vh_ego_params *e, const double *tr) { InlierTest t; t.ego = e; t.tr = tr; return t; }
  static InlierTest monocular(const vh_mono_params *e, const vh_mono_model *m) { InlierTest t; t.mono = e; t.model = m; t.is_mono = true; return t; }
  bool params_ok() const { return is_mono ? mono != nullptr : ego != nullptr; }
  bool args_ok() const { return params_ok() && (is_mono ? model != nullptr : tr != nullptr); }
};

static_assert(kListMax == (int64_t)VH_TRACK_POS_MASK && kInlierTile == VH_INLIER_TILE, "engine_lists.h restates both");

// The lists as the getters return them once a list was replaced on the host (vh_remove_outliers, vh_bucket_features), staged
// on the device by Group::stage_host_lists: one arena block, allocated by the first need.
struct HostLists {
  vh_p_match *d_pm = nullptr;   // [S][mcap]
  int32_t *d_cnt = nullptr;     // [S]
  std::vector<int32_t> h_cnt;   // the replaced lists' counts, alive until the uploads have run
};

// Motion inliers of the handle's lists (vh_group_motion_inliers; engine_inlier.hip): one arena
// block, allocated by the first call, cut into the arrays below.  Nothing here exists on a handle that never calls it.
struct InlierState : InlierArrays {      // [S][mcap], [S][tiles], [S], [S][6]
  vh_mono_model *d_model = nullptr;  // [S] a block of its own, allocated by the first mono classification
  HostLists host;                    // its own copy: it must outlive a vh_group_gain_indices that stages other lists
  int32_t tiles = 0;
  bool mono = false;                      // the classification is a mono one
  bool from_host = false;                 // it read `host` (a list was replaced on the host), not the emission's lists
  bool valid = false, truncated = false;  // a classification exists (of the lists of match call `seq`) / of a truncated list
  int64_t seq = 0;
  int64_t gen = 0;                        // classifications made so far: what was computed on one's lists is stale after the next
  std::vector<int32_t> n_list, n_inl;     // [S] records classified, inliers
};

// The mono pose over the compacted inlier lists of a mono classification (vh_group_pose_mono; engine_mono_pose.hip,
// DESIGN.md section 4.17): one arena block, allocated by the first call.
struct MonoPoseState : MonoPoseArrays {
  vh_mono_refine *d_refine = nullptr;        // [S] a block of its own, allocated by the first vh_group_pose_mono_refined
  // d_pose / d_ok hold the pose of classification `pose_gen` of match call `pose_seq` (Group::scene_points reads them there)
  int64_t pose_seq = -1, pose_gen = -1;
};

// The 3-d points of the compacted inlier lists (vh_group_scene_points_stereo / _mono; engine_scene.hip, DESIGN.md section
// 4.20): one arena block, allocated by the first call.
struct SceneState : SceneArrays {
  int32_t tiles = 0;
  bool valid = false;               // points exist, of the lists of match call `seq`
  int64_t seq = 0;
  std::vector<int32_t> n;           // [S] points per stream
};

// The landmarks of the current tracked lists (vh_group_landmarks; engine_landmark.hip): one arena
// block, allocated by the first call.  State buffer b belongs to track buffer b (Group::trk_cur).
struct LandmarkState : LandmarkArrays {
  int32_t tiles = 0;
  bool valid = false;               // landmarks exist, of the lists of match call `seq`
  int64_t seq = 0;
  int64_t state_seq[2] = {-1, -1};  // the match call whose tracked list each state buffer was computed for (-1: none)
  std::vector<int32_t> n;           // [S] landmarks per stream
  // A sequence handle with vh_sequence_set_landmarks on: d_state[0] holds the states of the
  // chunk's rows, d_state[1] the carry -- the last row's states of the last call on the previous chunk, copied when the
  // first call of the next chunk is queued (the rule of the track carry, whose slot its positions number).
  int32_t carry_src = -1;           // row to copy into the carry before the next launches (-1: none)
  bool carry_valid = false;         // the carry holds the states of the list in the track carry slot
};

// The motion refit on the landmarks (vh_group_refit_motion_landmarks): the arrays of its block
// (here and not in engine_lists.h: the record is the extension header's): the priors, the poses of
// the previous cameras, the counts of landmark points, and the refit's outputs
struct LmkRefitArrays {
  vh_refit_prior *d_prior = nullptr;  // [slots] ([S][mcap]), indexed like the compacted inlier records
  double *d_Tw = nullptr;             // [S][16]
  int32_t *d_nused = nullptr;         // [S]
  RefitState out;
  void carve(Carver &c, size_t lists, size_t slots) {
    d_prior = c.ptr<vh_refit_prior>(slots); d_Tw = c.ptr<double>(16 * lists); d_nused = c.ptr<int32_t>(lists); out.carve(c, lists);
  }
};
// The motion refit on the landmarks (vh_group_refit_motion_landmarks; engine_lmk_refit.hip): one
// arena block, allocated by the first call.
struct LmkRefitState : LmkRefitArrays {
  bool valid = false;               // priors exist, of the inlier lists of match call `seq` as they were when the fit read them
  int64_t seq = 0;
  std::vector<int32_t> n;           // [S] priors per stream
  std::vector<double> h_Tw;         // the chains' start poses, where they go up (the trajectory on, its block not there yet)
};

// The trajectory (vh_group_set_trajectory, vh_group_trajectory; engine_trajectory.hip): one arena
// block, allocated by the first call.  d_base: every chain's carry before the current pair; d_cur: behind it.
struct TrajState : TrajArrays {
  bool latched = false;   // d_base holds the carry the current pair's step starts from
  bool stepped = false;   // d_cur = step(d_base) was computed for the current pair
  bool valid = false;     // d_out holds the records of a call behind the last push (vh_group_get_poses)
  // what the last call stepped under: the match call, the classification (inl.gen) and the source -- the _world entries
  // refuse poses of a motion the current lists were not classified under
  int64_t seq = -1, gen = -1;
  int32_t source = -1;
};

// The pose covariance (vh_group_set_trajectory_covariance; engine_trajectory_cov.hip): one arena
// block, allocated by the first vh_group_trajectory call with the switch on.  latched / stepped / valid are TrajState's.
struct TrajCovState : TrajCovArrays {};

// The camera gain (vh_group_set_gain, vh_group_gain; engine_gain.hip): the ring's left images, one
// arena block allocated with the ring while the switch is on, and the blocks of the gain entries, each allocated by the
// first call that needs it.  Nothing here exists while the switch is off.
struct GainState : GainIndexArrays {  // (the caller's index lists; the block grows)
  uint8_t *d_planes = nullptr;  // [VH_RING][S][H][pitch]: plane (ring slot, row) = left set id >> 1
  int64_t plane = 0;            // bytes per plane: pitch * H
  int32_t pitch = 0;            // W rounded up to 16
  float *d_gain = nullptr;      // [S], and behind it int32 num [S]
  float *d_ratio = nullptr;     // [S][mcap] the ratios over the classification's positions
  int64_t idx_cap = 0;
  size_t idx_bytes = 0;
  HostLists host;               // what the index lists are positions in, once a list was replaced on the host
};

// The dense stages of a batch (vh_group_post_device_dense; engine_post.hip): one block beside the
// batch's own, cut into the arrays of one classification over the batch's P lists of `cap` slots (InlierArrays: its tr /
// ok arrays hold the refit's results) and, behind them, the gate's arrays, the refit's update counts and the mono models;
// and the page-locked mirror of what comes down with the batch's results.  Nothing here exists while the mode is 0.
struct VoteDense {
  DeviceBlock block;
  size_t bytes = 0;
  int32_t lists = 0, cap = 0, tiles = 0;  // what the block was cut for
  bool with_model = false;
  uint8_t *d_flags = nullptr;
  vh_p_match *d_out = nullptr;
  int32_t *d_src = nullptr, *d_tiles = nullptr, *d_ninl = nullptr;
  int32_t *d_ok_refit = nullptr; double *d_tr_refit = nullptr;  // modes 2, 3
  int32_t *d_cnt = nullptr, *d_ok = nullptr, *d_voted = nullptr, *d_nupd = nullptr;  // the gate's counts / ok / markers; updates
  vh_mono_model *d_model = nullptr;
  HostBlock<int32_t> h_int;   // [4][lists]: voted | inliers | ok_refit | n_updates
  HostBlock<double> h_tr;     // [lists][6]
  HostBlock<vh_mono_model> h_model;
  int32_t h_lists = 0; bool h_with_model = false;
  // the pointers into a block at `base` for `lists` lists of `cap` slots (null: none, the size only) -> its bytes
  size_t carve(void *base, size_t lists, size_t cap, bool model) {
    InlierArrays ia;
    Carver c = ia.carve(base, lists, lists * cap, (cap + VH_INLIER_TILE - 1) / VH_INLIER_TILE);
    d_flags = ia.d_flags; d_out = ia.d_out; d_src = ia.d_src; d_tiles = ia.d_tiles; d_ninl = ia.d_ninl;
    d_ok_refit = ia.d_ok; d_tr_refit = ia.d_tr;
    d_cnt = c.ptr<int32_t>(lists); d_ok = c.ptr<int32_t>(lists); d_voted = c.ptr<int32_t>(lists); d_nupd = c.ptr<int32_t>(lists);
    d_model = model ? c.ptr<vh_mono_model>(lists) : nullptr;
    return c.bytes();
  }
  static size_t bytes_for(size_t lists, size_t cap, bool model) { return VoteDense().carve(nullptr, lists, cap, model); }
};

// The per-list outputs of a batch's tail stages (vh_group_post_device_tail): the same arrays on the device and in the
// page-locked mirror they come down into, each present only with its stage's bit.
struct TailLists {
  double *cov = nullptr, *ssr = nullptr; int32_t *ok_cov = nullptr;                    // [lists][36], [lists], [lists]  VH_POST_TAIL_COV
  vh_mono_model *model = nullptr; double *w = nullptr; int32_t *ok_model = nullptr;    // [lists], [lists][2], [lists]   VH_POST_TAIL_MONO_REFIT
  double *tr = nullptr; int32_t *ok_pose = nullptr; vh_mono_pose *pose = nullptr;      // [lists][6], [lists], [lists]   VH_POST_TAIL_MONO_POSE
  vh_mono_refine *refine = nullptr;                                                    // [lists]                        VH_POST_TAIL_MONO_REFINE
  void carve(Carver &c, size_t lists, uint32_t mask) {
    *this = TailLists();
    if (mask & VH_POST_TAIL_COV) { cov = c.ptr<double>(36 * lists); ssr = c.ptr<double>(lists); ok_cov = c.ptr<int32_t>(lists); }
    if (mask & VH_POST_TAIL_MONO_REFIT) { model = c.ptr<vh_mono_model>(lists); w = c.ptr<double>(2 * lists); ok_model = c.ptr<int32_t>(lists); }
    if (mask & VH_POST_TAIL_MONO_POSE) { tr = c.ptr<double>(6 * lists); ok_pose = c.ptr<int32_t>(lists); pose = c.ptr<vh_mono_pose>(lists); }
    if (mask & VH_POST_TAIL_MONO_REFINE) refine = c.ptr<vh_mono_refine>(lists);
  }
};
// The tail stages of a batch (vh_group_post_device_tail; engine_post.hip): one block beside the
// dense stages', cut like it -- the per-list outputs and, with the pose, its headers and the two doubles per record slot --
// and the page-locked mirror of the outputs.  Nothing here exists while the mask is 0.
struct VoteTail {
  DeviceBlock block;
  size_t bytes = 0;
  int32_t lists = 0, cap = 0;  // what the block was cut for
  uint32_t mask = 0;
  TailLists d;
  double *d_hdr = nullptr, *d_dist = nullptr, *d_d = nullptr;  // [lists][VH_MONO_POSE_HDR], [lists][cap], [lists][cap]
  HostBlock<uint8_t> h_block;
  int32_t h_lists = 0; uint32_t h_mask = 0;
  TailLists h;
  size_t carve(void *base, size_t lists, size_t cap, uint32_t m) {
    Carver c(base);
    d.carve(c, lists, m);
    d_hdr = d_dist = d_d = nullptr;
    if (m & VH_POST_TAIL_MONO_POSE) { d_hdr = c.ptr<double>(lists * VH_MONO_POSE_HDR); d_dist = c.ptr<double>(lists * cap); d_d = c.ptr<double>(lists * cap); }
    return c.bytes();
  }
  static size_t bytes_for(size_t lists, size_t cap, uint32_t m) { return VoteTail().carve(nullptr, lists, cap, m); }
};

// a batch of the device post pipeline (engine_post.hip); its blocks live outside the arena
struct VoteBatch {
  VoteBuffers vb;
  int32_t steps = 0;      // steps moved in so far
  bool launched = false;  // the kernel sequence has been queued
  bool busy = false;      // holds steps whose results have not all been handed out
  int32_t handed = 0;
  Event ev_prep, ev_done;
  int32_t method = -1, max_features = 0; float bw = 0, bh = 0;
  int32_t rule = VH_VOTE_REFERENCE;  // the group's vote rule as it was when the batch was started
  bool has_ego = false, has_mono = false;
  vh_ego_params ego{}; vh_mono_params mono{};
  int32_t *d_rand = nullptr; size_t rand_per_step = 0;
  HostBlock<int32_t> h_rand; size_t h_rand_ints = 0;  // page-locked staging of the steps' random draws (the caller's array is only borrowed)
  double *d_xyz = nullptr, *d_tr = nullptr; int32_t *d_ok = nullptr; uint8_t *d_mono = nullptr;
  DeviceBlock block;  // d_rand | d_xyz | d_tr | d_ok | d_mono
  size_t block_bytes = 0;
  // page-locked results
  HostBlock<double> h_tr; HostBlock<int32_t> h_ok, h_cnt; HostBlock<VhVoteMeta> h_meta; HostBlock<vh_p_match> h_out;
  int32_t h_lists = 0, h_out_cap = 0;
  bool want_lists = false;
  int32_t dense_mode = 0;  // vh_group_post_device_dense, as it was when the batch was started
  VoteDense dn;
  uint32_t tail = 0;       // vh_group_post_device_tail, as it was when the batch was started
  VoteTail tl;
  VoteBatch() = default;
  VoteBatch(VoteBatch &&) = default;
  ~VoteBatch() { if (launched && ev_done) (void)hipEventSynchronize(ev_done); }  // (before the members free what the kernels use)
};
struct VoteStep { int32_t batch = -1, pos = 0; bool open = false; };

// A vh_group owns S independent camera streams that are stepped together; a vh_matcher is a group of one.
//
// Nothing is released by hand: the members' destructors do it, in the reverse of the order they are declared in.
// That order is part of the design -- streams, then events, then the device blocks (`allocs`), then the vote batches,
// then the sparse group: so the sparse group (which runs on this group's detect stream) goes first, the vote batches
// are synchronised and freed next, and every device block is freed before the streams are destroyed.
struct Group {
  vh_params p{};
  int32_t device = 0, S = 1;
  int32_t req_features = 0, req_matches = 0;
  // Internal streams: detection+indexing of frame t+1 overlaps the matching
  // of frame t (the ring has VH_RING slots for that).  `stream` is the detect
  // stream (also used by the stateless paths; a sparse group's is its parent's); a caller-owned stream, if set,
  // only orders our work after the caller's (image producers).
  // A third stream (default; VH_POST_STREAM=0: the match stream) takes the short,
  // latency-bound post-processing (chain + emission) of frame t, so that the flow
  // search of frame t+1 follows that of frame t back to back; the match tables are
  // double-buffered for that.
  Stream own_stream, match_stream, post_stream, copy_stream, down_stream;
  static constexpr int32_t kVoteStreams = 4;
  Stream vote_stream[kVoteStreams];
  hipStream_t stream = nullptr, user_stream = nullptr;
  Event ev_tables[2];       // match tables of buffer b complete
  Event ev_post[2];         // post-processing finished reading buffer b
  Event ev_det[VH_RING];    // slot fully detected + indexed
  Event ev_read[VH_RING];   // last match that read the slot
  Event ev_user, ev_stage[2], ev_h2d;
  Event ev_down;            // asynchronous download of the match lists (vh_group_download_matches_async)
  Event ev_stats;           // multi-stage device mode: orders pass 2 behind the statistics
  bool ev_post_valid[2] = {false, false};
  bool ev_read_valid[VH_RING] = {};
  int64_t match_seq = 0;
  // Loop policy of the searches (match()): speculative (no accept test in the loop, the winner
  // verified, failures searched again) or tested.  The speculative loop is ~12 % faster when
  // almost every query's best candidate lies inside its window (0.5 % re-searched on the
  // benchmark frames) and slower once more than ~6 % fail (noisy images full of features
  // without a partner; measured round 3 with grouped second searches: +10 % at 3.3 % re-searched,
  // +3 % at 4.8 %, -1 % at 6.6 %, -6 % at 8.9 %).  Every launch reports (re-searched, searched)
  // with a lag of one or two steps; above 6.5 % the tested loop takes over and the speculative
  // one is probed every 16th launch, below 5.5 % it comes back.  Results never depend on the choice.
  int32_t probe_countdown = 0, force_mode = -1;
  bool spec_mode = true;
  double last_redo_rate = -1;
  bool user_stream_set = false;  // handle 0 is a real stream (the legacy default stream): "unset" is a flag, not a value
  bool failed = false;           // the last push did not complete: no matching until the next successful one
  int32_t pair_prev = 1;
  bool serial = false;
  // Sequence handle (vh_sequence_*): the S rows of a slot are consecutive frames of one camera, a push brings a chunk of
  // seq_n <= S of them and every match links row r to row r - 1 (row 0 to the last row of the previous chunk: vh_row_set).
  bool seq = false;
  int32_t seq_n = 0, seq_n_prev = 0;      // frames of the last chunk / of the one before
  int64_t seq_first = 0, seq_total = 0;   // index in the sequence of the last chunk's first frame / frames pushed so far
  // vh_group_set_multi_stage_device: the vote and the statistics between the passes run on the device, behind pass 1 on the
  // sparse group's post stream (multi_stage_ranges_device); ms_vb holds the S voted sparse lists
  bool ms_device = false;
  // vh_group_set_multi_stage_prior: a match call with a motion estimate hands it to both passes (quad only); off: refused
  bool ms_prior = false;
  static constexpr int32_t kMsVoteLanes = 16;  // lists per wave of the sweep

  bool allocated = false;
  int32_t dims[3] = {0, 0, 0};
  VhGeom g{};
  VhSets sets{};
  // refinement > 0 (kernels_refine.hip): full-resolution du/dv per feature set of the ring, written with the detection of a push
  VhRefine rf{};
  int32_t cap = 0, mcap = 0;
  int32_t pair_cur = 0;
  int64_t frames = 0;
  int32_t stage_slot = 0;
  int32_t last_buf = 0;
  int32_t last_method = -1;
  // A match launch that failed half way leaves the emission's chunk counters and the re-search counters of its table
  // buffer in an unknown state (each emission zeroes the OTHER buffer's counters for the next launch): the next
  // match() puts both buffers back to zero before it queues anything.
  bool match_dirty = false;
  bool fail_next_alloc = false;  // test hook (vh_group_debug_fail_next_alloc)
  int32_t fail_alloc_skip = 0;   // test hook: allocations that still succeed before the requested failure

  // ---- feature tracks (vh_group_set_track_linking; kernels_track.hip) ---------------------
  // Slots of d_ttab / d_trk: a group keeps two lists per stream, buffer b in the slots [b * S, (b + 1) * S): trk_cur is
  // the buffer of the current pair's list, the other one holds the previous step's (the predecessors).  A sequence handle
  // keeps its S rows in the slots [0, S) and the carry -- the last row of the last match call on the previous chunk -- in
  // slot S; the carry is copied when the first match call of the next chunk is queued, so that matching a chunk again
  // still finds the carry of the chunk before it.
  bool trk_on = false;
  uint32_t trk_epoch = 0, trk_cur_epoch = 0, trk_pred_epoch = 0;
  int32_t trk_cur = 0;
  bool trk_cur_valid = false;   // the current pair (sequence: chunk) has a tracked list, bid for at trk_cur_epoch
  bool trk_pred_valid = false;  // group: the other buffer holds the predecessors; sequence: the carry slot is valid
  int32_t trk_carry_src = -1;   // sequence: row to copy into the carry before the next bids (-1: none)
  int64_t trk_serial = 0;       // group: serial of the current frame
  int64_t trk_fill_seq[2] = {-1, -1};  // group: the match call (match_seq) that filled each track buffer; Group::landmarks compares it with LandmarkState::state_seq

  // streams whose current matches were post-processed on the host
  // (vh_remove_outliers / vh_bucket_features): served from here until the next step
  std::vector<std::vector<vh_p_match>> host_matches;
  std::vector<uint8_t> host_filtered;

  bool prof = false;
  std::map<std::string, ProfEntry> prof_entries;

  int64_t post_seq = 0;
  // The device post pipeline.  Measured on MI355X, KITTI, S = 256 (bench.py e2e_matchfeatures, k pairs/s; steps per batch x batches, 64 lists per wave):
  // 4x5 10.4, 8x5 11.7, 16x5 19.9, 32x3 25.3, 32x4 30.4, 48x3 30.2, 64x3 33.9; 1 list per wave, 4x5: 17.9.  A batch takes
  // 0.4-0.5 s from launch to results whatever its size (profiles/r04_vote_trace.txt): the rate is the number of steps in
  // flight over that latency, and a wave of 64 lists costs the chip 1/14 of what 64 single-list waves cost.
  int32_t vote_steps = 64, vote_batches = 3, vote_lanes = 16;
  int32_t vote_dense = 0;     // vh_group_post_device_dense: 0 off, 1 classify, 2 + refit, 3 + classify again
  uint32_t vote_tail = 0;     // vh_group_post_device_tail: the VH_POST_TAIL_* stages behind the dense ones
  int64_t post_dev_seq = 0;   // steps begun
  int32_t vote_cur = 0;       // batch receiving steps
  // vh_group_set_vote_rule: VH_VOTE_REFERENCE (the reference's flow vote under its literal 5; stereo lists are not voted)
  // or VH_VOTE_STOCK (the per-method rule under this handle's two tolerances; every list is voted)
  int32_t vote_rule = VH_VOTE_REFERENCE;
  bool votes_on(int32_t method) const { return method != VH_METHOD_STEREO || vote_rule == VH_VOTE_STOCK; }
  vh_vote_rule rule_for(int32_t method) const { return vh_vote_rule{vote_rule, method, (float)p.outlier_flow_tolerance, (float)p.outlier_disp_tolerance}; }
  std::vector<VoteStep> vstep;  // ring over the steps begun, indexed by sequence number

  std::vector<DeviceBlock> allocs;  // the arena: every dmalloc'ed block, counted in device_bytes
  int64_t device_bytes = 0;
  DetectScratch det;
  MatchTables mt;
  Staging stg;
  Prior pri;
  TrackTables tk;
  EgoScratch ego;
  HostPost post;
  Ranges rg;
  VoteBuffers ms_vb;
  std::vector<VoteBatch> vbatch;
  ReconHistory rh;
  InlierState inl;
  RefitState rft;
  CovState cv;
  MonoRefitState mrf;
  MonoPoseState mps;
  SceneState scn;
  LandmarkState lmk;
  LmkRefitState lrf;
  bool lmk_chain = false;  // vh_sequence_set_landmarks: vh_group_landmarks runs the chain form over the chunk's rows
  // vh_group_set_trajectory: the switch, the policy and the start poses [chains][16] (empty: unit matrices) are settings
  // and survive release(); trj is device state and does not -- after new dims every chain starts from its T0 again
  bool traj_on = false;
  vh_traj_params traj_params{};
  std::vector<double> traj_T0;
  TrajState trj;
  // vh_group_set_trajectory_covariance: settings as the trajectory's (the start covariances [chains][36], empty: zero)
  bool tcov_on = false;
  vh_traj_cov_params tcov_params{};
  std::vector<double> tcov_S0;
  TrajCovState tcv;
  bool gain_on = false;  // vh_group_set_gain: every push keeps the left images (gn.d_planes)
  GainState gn;
  // Multi-stage matching (vh_group_set_multi_stage_matching): `sparse` is a group of its own over the same S streams
  // whose detector runs at the sparse NMS distance (matcher.cpp:621-628) -- its dense set IS the sparse set -- on this
  // group's detect stream, behind every push.  A match runs pass 1 on it, votes and takes the statistics on the host,
  // and searches this group's sets inside rg.d_ranges (kernels_ranged.hip).  On a sequence handle (vh_sequence_set_multi_stage)
  // the sparse group is a sequence group too: it takes the same chunks, rotates its ring with this one's and resolves the
  // rows' sets through the same vh_row_set, so a frame's sparse set is detected once and serves both of its pairs.
  std::unique_ptr<Group> sparse;

  // ---- engine.hip ----
  void drop_host_matches() { std::fill(host_filtered.begin(), host_filtered.end(), 0); }
  int32_t pairs() const { return pair_cur | (pair_prev << 8); }
  // feature sets: ring slots x (left, right) per row, and a sequence handle's empty pair after them (VhMatchArgs::seq_void)
  size_t n_sets() const { return 2 * VH_RING * (size_t)S + (seq ? 2 : 0); }
  VhMatchArgs role_args() const;
  int32_t sync_all();
  int32_t check_violation();
  int32_t stage_host_lists(HostLists &h, hipStream_t st, bool &replaced, const vh_p_match *&pm, const int32_t *&counts);
  void release();
  bool alloc_refused();
  template <class T> int32_t dmalloc(T **out, size_t count, bool zero) {
    void *q = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (alloc_refused()) return VH_ERR_HIP;
    VH_HIP(hipMalloc(&q, bytes));
    allocs.emplace_back(q);
    device_bytes += (int64_t)bytes;
    if (zero) VH_HIP(hipMemsetAsync(q, 0, bytes, stream));
    else VH_HIP(vh_poison_device(q, bytes));  // (vh_poison.h)
    *out = (T *)q;
    return VH_OK;
  }
  // One arena block for the arrays of `a` (a struct of engine_lists.h with a carve(Carver &, args...)): measured on a
  // scratch copy, allocated, bound -- a refused allocation leaves `a` as it was.  tight: the last array as long as it is.
  template <class A, class... Args> int32_t dmalloc_carved(A &a, size_t *bytes, bool tight, Args... args) {
    A scratch;
    Carver measure;
    scratch.carve(measure, args...);
    const size_t n = tight ? measure.tight() : measure.bytes();
    uint8_t *d = nullptr;
    const int32_t rc = dmalloc(&d, n, false);
    if (rc) return rc;
    Carver bind(d);
    a.carve(bind, args...);
    if (bytes) *bytes = n;
    return VH_OK;
  }
  void dfree(void *q);
  static int32_t block_count(int32_t extent, int32_t n);
  int32_t setup_geometry(const int32_t d[3]);
  int32_t ensure(const int32_t d[3]);
  int32_t allocate(const int32_t d[3]);
  int32_t ensure_staging(size_t isz);
  void prof_collect();
  void prof_host(const char *name, std::chrono::steady_clock::time_point t0);
  int32_t zero_bin_counters(int32_t set0, int32_t nsets, int32_t *extra = nullptr, int64_t n_extra = 0);
  int32_t bin_sets(int32_t set0, int32_t nsets, bool staged);
  int32_t push_device(const void *dI1, const void *dI2, int64_t stride, const int32_t d[3], int32_t replace, int32_t rows = -1);
  int32_t push_device_queued(const void *dI1, const void *dI2, int64_t stride, const int32_t d[3], int32_t replace, int32_t rows);
  int32_t push_host(const uint8_t *I1, const uint8_t *I2, int64_t stride, const int32_t d[3], int32_t replace, int32_t rows = -1);

  // ---- engine_match.hip ----
  VhMatchArgs match_args(int32_t method) const;
  bool choose_loop();
  int32_t match_recover();
  size_t n_ranges() const { return (size_t)S * sets.ubn * sets.vbn * 16; }
  int32_t ensure_ranges(bool staging = true);
  int32_t multi_stage_ranges(int32_t method, const double *tr16);
  int32_t ensure_ms_vote();
  int32_t multi_stage_ranges_device(int32_t method, const double *tr16);
  int32_t stage_prior(const double *tr16, int32_t buf, int32_t rows, hipStream_t ms);
  int32_t load_ranges(const float *ranges);
  int32_t match(int32_t method, const double *tr16 = nullptr, bool ranged = false);
  int32_t match_call(int32_t method, const double *tr16, bool ranged);
  int32_t match_queued(int32_t method, const double *tr16, const int32_t *ranges);
  int32_t mask_epoch(hipStream_t st);
  int32_t match_post(int32_t method, const VhMatchArgs &a, int32_t buf, bool ranged, bool spec);
  int32_t trk_slots() const { return seq ? S + 1 : 2 * S; }
  // no list is tracked any more (the tables were cleared, or are about to be)
  void trk_reset_lists() { trk_epoch = trk_cur_epoch = trk_pred_epoch = 0; trk_cur_valid = trk_pred_valid = false; trk_carry_src = -1; }
  void trk_reset() { trk_reset_lists(); trk_cur = 0; trk_serial = 0; trk_fill_seq[0] = trk_fill_seq[1] = -1; }  // ... and the sequence starts again (new dims)
  void trk_pushed(bool shifted, bool first, int32_t prev_chunk_rows);
  int32_t trk_ensure();
  VhTrackArgs trk_args(int32_t rows) const;
  int32_t trk_queue(const VhMatchArgs &a, hipStream_t ps);
  int32_t get_tracks(int32_t s, vh_track *out, int32_t capo, int32_t *n);
  int32_t get_tracks_all(vh_track *out, int32_t cap_per_stream, int32_t *counts);
  int32_t load_features(int32_t role, const int32_t *m, int32_t n);

  // ---- engine_recon.hip ----
  void recon_pushed(bool first, bool shifted);
  void recon_before_link();
  void recon_matched(const VhMatchArgs &a);
  void recon_match_failed() { rh.m_valid = false; rh.drop_chain(); }
  int32_t recon_lists() const { return seq ? 1 : S; }  // lists per frame
  int32_t reconstruct(const double *Tr, int32_t *n_tracks, int32_t *n_accepted);

  // ---- engine_inlier.hip ----
  bool inliers_current() const { return allocated && inl.valid && inl.seq == match_seq; }
  // the compacted inlier lists of the classification: what every stage behind it reads
  VhLists inlier_lists() const { return VhLists::slots(inl.d_out, mcap, inl.d_ninl, mcap, S); }
  // The first min(n, capo) elements of slot s of a device array [S][mcap] into out; queued: on the post stream (the
  // caller waits for it), else blocking.  over: set where the slot holds more than capo.
  template <class T> int32_t get_slot(T *out, const T *d, int32_t s, int32_t n, int32_t capo, bool queued, bool &over) {
    over = over || n > capo;
    const size_t k = (size_t)std::max(std::min(n, capo), 0);
    if (!k) return VH_OK;
    if (queued) VH_HIP(hipMemcpyAsync(out, d + (size_t)s * mcap, sizeof(T) * k, hipMemcpyDeviceToHost, post_stream));
    else VH_HIP(hipMemcpy(out, d + (size_t)s * mcap, sizeof(T) * k, hipMemcpyDeviceToHost));
    return VH_OK;
  }
  int32_t motion_inliers(const InlierTest &t, const int32_t *ok, int32_t *counts);
  int32_t refit_motion(const vh_ego_params *e, int32_t reclassify, double *tr_out, int32_t *ok_out, int32_t *n_updates, int32_t *counts);
  // behind a refit's launches on the post stream: the downloads of r's arrays, then counts -- the classification's, or with
  // reclassify the classification again under r's tr / ok
  int32_t refit_finish(const vh_ego_params *e, int32_t reclassify, const RefitState &r, double *tr_out, int32_t *ok_out, int32_t *n_updates,
                       int32_t *counts);
  int32_t get_inlier_flags(int32_t s, uint8_t *out, int32_t capo, int32_t *n);
  int32_t get_inlier_matches(int32_t s, vh_p_match *out, int32_t *src_pos, int32_t capo, int32_t *n);
  int32_t get_inlier_matches_all(vh_p_match *out, int32_t *src_pos, int32_t cap_per_stream, int32_t *counts);

  // ---- engine_cov.hip ----
  int32_t motion_covariance(const vh_ego_params *e, const double *tr, const int32_t *ok, double *cov, double *ssr, int32_t *ok_out, int32_t *counts);

  // ---- engine_mono_refit.hip ----
  int32_t refit_model_mono(const vh_mono_params *e, int32_t reclassify, vh_mono_model *model_out, int32_t *ok_out, double *w_out, int32_t *counts);

  // ---- engine_mono_pose.hip ----
  // refined: the winner is refined between the chirality count and the tail (vh_group_pose_mono_refined); refine is nullable
  int32_t pose_mono(const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose, int32_t *counts, bool refined = false,
                    vh_mono_refine *refine = nullptr);

  // ---- engine_scene.hip ----
  // e (stereo) or m (mono): the one that is given names the kind
  // world: Tw is the trajectory's poses on the device (Tw_prev for sp->frame 0, Tw_cur for 1), the argument is not read
  int32_t scene_points(const vh_ego_params *e, const vh_mono_params *m, const vh_scene_params *sp, const double *Tw, int32_t *counts,
                       bool world = false);
  bool scene_current() const { return allocated && scn.valid && scn.seq == match_seq; }
  int32_t get_scene_points(int32_t s, vh_scene_point *out, int32_t capo, int32_t *n);
  int32_t get_scene_points_all(vh_scene_point *out, int32_t cap_per_stream, int32_t *counts);

  // ---- engine_landmark.hip ----
  int32_t landmarks(const vh_landmark_params *lp, int32_t *counts);
  int32_t landmarks_chain(const vh_landmark_params *lp, int32_t *counts);  // a sequence handle's
  void lmk_pushed(bool first, int32_t prev_chunk_rows);
  bool landmarks_current() const { return allocated && lmk.valid && lmk.seq == match_seq; }
  int32_t get_landmarks(int32_t s, vh_landmark *out, int32_t capo, int32_t *n);
  int32_t get_landmarks_all(vh_landmark *out, int32_t cap_per_stream, int32_t *counts);

  // ---- engine_lmk_refit.hip ----
  int32_t refit_motion_landmarks(const vh_ego_params *e, const vh_lmk_refit_params *rp, const double *Tw_prev, int32_t reclassify, double *tr_out,
                                 int32_t *ok_out, int32_t *n_updates, int32_t *n_used, int32_t *counts);
  int32_t get_refit_priors(int32_t s, vh_refit_prior *out, int32_t capo, int32_t *n);

  // ---- engine_trajectory.hip ----
  int32_t traj_chains() const { return seq ? 1 : S; }
  int32_t set_trajectory(const vh_traj_params *tp, const double *T0);
  void traj_pushed(bool shifted);
  // the motion of `source` is the one the scene points of the same kind would be computed under -> VH_OK / VH_ERR_STATE
  int32_t traj_source(int32_t source, const double *&d_tr, const int32_t *&d_ok) const;
  int32_t trajectory(int32_t source, vh_traj_pose *out);
  bool traj_current(bool mono) const {
    return allocated && traj_on && trj.d_out && trj.valid && trj.seq == match_seq && trj.gen == inl.gen &&
           trj.source == (mono ? VH_TRAJ_MONO : VH_TRAJ_STEREO);
  }
  int32_t get_poses(vh_traj_pose *out);
  int32_t set_pose(int32_t s, const double *T);

  // ---- engine_trajectory_cov.hip ----
  int32_t set_trajectory_covariance(const vh_traj_cov_params *tcp, const double *Sigma0);
  // the motion covariance on the device is the current classification's own
  bool tcov_input_current() const { return cv.d_cov && cv.seq == match_seq && cv.gen == inl.gen && cv.own_tr; }
  int32_t tcov_alloc();                     // the block and the chains' starts, once
  void tcov_launch(const double *d_tr, const int32_t *d_ok, int32_t pair_lo, int32_t pair_hi);
  int32_t tcov_set(int32_t s, const double *Sigma, bool restart);   // set_pose (restart) / set_pose_covariance
  int32_t get_pose_covariances(vh_traj_cov *out);

  // ---- engine_gain.hip ----
  int32_t gain_copy(const VhImages &im);
  int32_t gain_lists(const int32_t *idx, const int32_t *idx_offsets, float *gain, int32_t *num);

  // ---- engine_post.hip ----
  int32_t get_sparse_device(int32_t s, vh_p_match *out, int32_t capo, int32_t *n);
  int32_t download_async(vh_p_match *out, int32_t cap_per_stream, int32_t *counts);
  int32_t wait_download();
  int32_t get_matches(int32_t s, vh_p_match *out, int32_t capo, int32_t *n);
  int32_t get_features(int32_t s, int32_t which, int32_t *out12, int32_t capo, int32_t *n);
  int32_t get_counts(int32_t *nf, int32_t *nm);
  int32_t get_matches_all(vh_p_match *out, int32_t cap_per_stream, int32_t *counts);
  int32_t fetch_matches(int32_t s);
  int32_t remove_outliers(int32_t s_lo, int32_t s_hi, int32_t threads);
  int32_t estimate_motion(const vh_ego_params *e, const int32_t *rand3, double *tr, int32_t *ok, int32_t *ninl);
  int32_t estimate_motion_mono(const vh_mono_params *e, const int32_t *rand8, double *tr, int32_t *ok, int32_t *ninl, vh_mono_model *model);
  int32_t estimate_results(double *tr, int32_t *ok, int32_t *ninl);
  int32_t post_begin(int32_t cap_ps);
  int32_t post_finish(int32_t age, int32_t max_features, float bw, float bh, int32_t threads, const vh_ego_params *e, const int32_t *rand3,
                      const vh_mono_params *mono, const int32_t *rand8,
                      double *tr, int32_t *ok, int32_t *ninl, vh_p_match *out, int32_t out_cap, int32_t *out_counts, double *host_ms);
  void vote_release() { vbatch.clear(); vstep.clear(); post_dev_seq = 0; vote_cur = 0; }
  int32_t post_device_config(int32_t steps_per_batch, int32_t batches, int32_t lanes);
  int32_t post_device_dense(int32_t mode);
  int32_t post_device_tail(uint32_t stages);
  int32_t post_device_shape(int32_t *steps_per_batch, int32_t *batches) const;
  int32_t vote_dense_alloc(VoteBatch &b, int32_t lists, bool model);
  int32_t vote_tail_alloc(VoteBatch &b, int32_t lists, uint32_t mask);
  int32_t vote_tail_launch(VoteBatch &b, const VhVote &v, const InlierTest &t, VhInlierArgs &a, hipStream_t vs);
  int32_t vote_dense_launch(VoteBatch &b, const VhVote &v, hipStream_t vs);
  int32_t bucket_need(int32_t max_features, float bw, float bh, int64_t *need, int64_t *grid = nullptr) const;
  int32_t vote_launch(VoteBatch &b, int32_t index);
  // vh_launch_vote on lists of `method` under this handle's rule; with profiling on, the tally is timed under a scope of
  // its own (vote_tally: the reference test; vote_tally_flow / _disp / _quad: the stock rule's)
  void vote_run(const VhVote &v, int32_t method, int32_t lanes, int32_t max_features, float bw, float bh, const VhVoteBuffers &vb, hipStream_t st);
  int32_t post_begin_device(int32_t cap_ps, int32_t max_features, float bw, float bh, const vh_ego_params *e, const int32_t *rand3,
                            const vh_mono_params *mono, const int32_t *rand8, int32_t want_lists);
  int32_t post_finish_device(int32_t age, double *tr, int32_t *ok, int32_t *ninl, vh_p_match *out, int32_t out_cap, int32_t *out_counts,
                             const vh_post_dense *d = nullptr, const vh_post_tail *t = nullptr);
};

// times the HIP work queued on `st` during its lifetime under `name` (only while the group profiles)
struct Scope {
  Group *gq; const char *name; hipStream_t st; Event e0, e1;
  Scope(Group *gq_, const char *n, hipStream_t st_) : gq(gq_), name(n), st(st_) {
    if (gq->prof) { (void)e0.create(hipEventDefault); (void)e1.create(hipEventDefault); (void)hipEventRecord(e0, st); }
  }
  ~Scope() {
    if (gq->prof) { (void)hipEventRecord(e1, st); gq->prof_entries[name].pending.emplace_back(std::move(e0), std::move(e1)); }
  }
};

// engine.hip
int32_t check_params(const vh_params *p);
// -DVH_CHECK builds: aborts when the kernels recorded an index violation in d_check (nullable); the work must have completed
int32_t report_violation(const uint32_t *d_check);
// list l of n: counts[l] records from pm + l * stride to dst + l * cap, blocking
int32_t upload_strided_lists(vh_p_match *dst, int64_t cap, const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t n);
int32_t select_device(int32_t device);
int32_t group_new(const vh_params *p, int32_t device, int32_t S, int32_t mf, int32_t mm, Group **out);
// engine_api.hip
// The lists of vh_link_tracks / vh_reconstruct_lists uploaded and linked as the rows of one chain; the blocks are the caller's.
struct LinkedLists {
  std::vector<DeviceBlock> blocks;
  vh_p_match *d_pm = nullptr; vh_track *d_trk = nullptr; int32_t *d_cnt = nullptr; uint32_t *d_check = nullptr;
  int32_t lcap = 0;
  int64_t serial0 = 0;
};
int32_t link_lists_device(int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t n_index, const vh_p_match *carry_pm,
                          const vh_track *carry_trk, int32_t carry_count, int64_t carry_serial, bool has_carry, LinkedLists &out);
// engine_inlier.hip
// The flag pass of either test, then the scan and the scatter, on `st`; g: the handle whose profile takes the scopes (nullable)
void launch_inliers(const InlierTest &t, VhInlierArgs &a, hipStream_t st, Group *g);
// engine_mono_pose.hip
// The six launches of the mono pose on `st`, the refinement between launches 1 and 2 where refined; g: the handle whose
// profile takes a scope per launch (nullable)
void launch_mono_pose(const VhMonoPoseArgs &a, bool refined, vh_mono_refine *refine, hipStream_t st, Group *g);
// engine_post.hip
// Matcher::bucketFeatures (matcher.cpp:140-187) on the records pm[0, n): the selected records are written to
// out (at most out_cap of them) in the reference's order; returns how many the reference would keep.
int32_t bucket_records(const vh_p_match *pm, int32_t n, int32_t max_features, float bw, float bh, vh_p_match *out, int32_t out_cap,
                       std::vector<int32_t> &work);
void bucket_host(std::vector<vh_p_match> &pm, int32_t max_features, float bw, float bh);
// computePriorStatistics of multi-stage matching (include/viso_hip.h: vh_prior_statistics), host side
int32_t prior_statistics(const vh_params &p, const int32_t dims[3], int32_t method, const vh_p_match *pm, int32_t n, float *ranges);

}  // namespace vh_engine
#endif
