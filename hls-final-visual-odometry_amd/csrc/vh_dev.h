// vh_dev.h -- shared host/device declarations of the gfx950 detect+match engine.
//
// Data layout in HBM (all arrays are flat, one allocation per kind, indexed by
// a *set id* or an *image id* so that one kernel launch covers every camera
// stream of a group):
//
//   image id  = stream*2 + cam                      (cam 0 = left, 1 = right)
//   set id    = pair*(2*S) + stream*2 + cam         (pair = ring slot 0..2; the
//               current/previous roles move from slot to slot, never by copy:
//               reference ring buffer src/matcher.cpp:64-79.  Three slots, so
//               that detection of frame t+1 can run while frame t is matched.
//               A sequence handle holds consecutive frames of one camera in the
//               rows of a slot and two more, always empty, sets: vh_row_set)
//
//   feat      [set][cap][12] int32   the reference's packed record
//                                    {u,v,0,c,d1..d8} (src/matcher.cpp:663-671)
//   f_uv      [set][cap]     uint32  u | v<<16, in reference order (compact copy of feat's first two words)
//   s_uv      [set][cap]     uint32  u | v<<16, in *bin order*
//   s_idx     [set][cap]     int32   original feature index of that position
//   s_desc    [set][cap][8]  uint32  32-byte descriptor, in bin order
//   bin_start [set][nbins+1] int32   CSR over bins, bin = (c*ubn+ub)*vbn+vb
//                                    (u-bin major: the iteration order of
//                                    Matcher::findMatch, src/matcher.cpp:243-246)
//   row_start [set][4*H+1]   int32   CSR over (class, v) rows: the stereo search
//                                    (v window of +-disp_tolerance) walks one
//                                    contiguous row range per query
//   r_pos     [set][cap]     int32   row order -> bin-order position
//   rec       [image][nblocks] u64   per NMS block 4 x u16 position codes
//   best      [stream][pass][cap] int32  findMatch result for every query
//   matches   [stream][mcap] p_match (48 B, src/matcher.h:89-104)
#ifndef VH_DEV_H
#define VH_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/viso_hip.h"
#include "../../include/viso_hip_lmk_refit.h"

#define VH_MARGIN 7          // src/matcher.cpp:38
#ifndef VH_CHUNK
#define VH_CHUNK 1024        // NMS blocks per emit workgroup (a multiple of 256)
#endif
#define VH_WAVE 64
// Flow search (kernels_match.hip): a wave is VH_FLOW_P phases of 64/VH_FLOW_P lanes, VH_FLOW_Q
// queries per lane; the phases share one candidate stream.
#ifndef VH_FLOW_Q
#define VH_FLOW_Q 2
#endif
#ifndef VH_FLOW_P
#define VH_FLOW_P 4
#endif
#define VH_TILE_Q (64 * VH_FLOW_Q / VH_FLOW_P)  // queries per flow-search tile
#ifndef VH_SNAKE
#define VH_SNAKE 1  // 0 (experiments): query tiles over the plain bin order (kernels_bin.hip: make_tiles, kernels_match.hip: flow_queries)
#endif
#define VH_NO_CODE 0xFFFFu
// Wave priority of the detection chain's kernels (detect_nms, emit_features, bin_scan, bin_sort): their instructions
// issue ahead of the searches' on a shared SIMD.  The chain is the step's critical path (4 sub-batches x 4 dependent
// kernels, each slowed 2-3x by the searches beside it) while the searches only need their sum of issue slots.
// MI355X, KITTI, S = 256, k pairs/s: priority 0 / 1 / 2 / 3 = 104.8 / 107.2 / 107.3 / 107.2 (round 5, after the
// searches lost 6 % of their instructions; in round 3, with the heavier searches, the same switch was +-0).
#ifndef VH_DET_PRIO
#define VH_DET_PRIO 1
#endif
#define VH_DET_SETPRIO() do { if (VH_DET_PRIO) __builtin_amdgcn_s_setprio(VH_DET_PRIO); } while (0)
// 32-bit match keys SAD << 19 | (bin-order position - first position of the class) serve classes
// of up to 2^19 - 64 features per set (the staged chunks of the searches repeat the last candidate
// of a run under positions up to 63 past it); larger classes take 64-bit keys (kernels_match.hip).
// The detector yields at most one feature per class and NMS block, so only images of more than
// 524 224 blocks can need those.
#define VH_CLASS_POS_BITS 19
#define VH_CLASS_POS_MAX ((1 << VH_CLASS_POS_BITS) - 64)
// first-writer pixel mask of the flow method: epoch << 24 | (2^24 - 1 - i1c); also the
// largest feature capacity per image (2^24 - 1)
#define VH_MASK_IDX_BITS 24

struct VhGeom {
  // full-resolution image
  int32_t W, H, bpl;
  // matching-resolution image (== full unless half_resolution)
  int32_t Wm, Hm, bplm;
  int32_t scale;            // 1, or 2 with half_resolution (src/matcher.cpp:647-649)
  int32_t n, tau;           // nms_n, nms_tau
  int32_t nbx, nby, nblocks, nchunks;
  int32_t tbx, tby;         // NMS blocks per detect tile
  int32_t FW, FH, IW, IH;   // filter-response tile / image tile extents (pixels)
  int32_t IWp, FWp;         // padded LDS row pitches
};

struct VhSets {
  int32_t *feat;
  uint32_t *f_uv;      // [set][cap] u | v << 16 in reference (feature index) order: what the chains and the emission gather
  uint32_t *s_uv;
  int32_t *s_idx;
  uint32_t *s_desc;
  int32_t *bin_start;
  int32_t *hist;
  int32_t *cursor;
  int32_t *tmp_idx;
  int2 *stage;         // [set][nbins][stage_cap] {feature index, rank in its (class, v) row} appended by emit_features (arbitrary order)
  int32_t *count;
  // row index (stereo search): the same records ordered by (class, v)
  int32_t *row_start;  // [set][4*H+1]
  int32_t *row_hist;   // [set][4*H]
  int32_t *row_cursor; // [set][4*H]
  int32_t *r_pos;      // [set][cap] bin-order position of the feature at each row-order position
  int4 *tiles;       // [set][max_tiles] {first snake index, end, class, column of the first} (kernels_bin.hip: make_tiles; the column is
                     // not read by the searches any more: it stays so that a record is one 16-byte store and one scalar load, and for debugging)
  int32_t *tile_cnt; // [set]
  int32_t *snake_pos; // [set][cap] bin-order position of the query with snake index k (bin_sort writes it; read by flow_queries only)
  int32_t cap, nbins, ubn, vbn, binsize, max_tiles;
  uint32_t inv_binsize;  // ceil(2^32 / binsize): x / binsize == __umulhi(x, inv_binsize) for 0 <= x < 2^18
  int32_t W, H;      // dims_c of the matcher (full resolution)
  int32_t stage_cap;   // max features of one class in one bin for features of this detector (geometry bound)
  uint32_t *check;   // [4] -DVH_CHECK builds: {violations, code of the first, its value, its bound}; unused otherwise
};

// Index invariants of the device-side indices (row index -> bin position -> record).  The shipped
// build trusts them (no clamps: DESIGN.md section 2a says why each holds); a -DVH_CHECK build
// verifies every one on the device, records the first violation in VhSets::check and continues with
// the index forced into range, and the host side aborts the process at the next synchronisation
// (engine.hip: check_violation) -- loud, but without a wild access on a shared GPU.
//   codes: 1 rows_tile query position, 2 rows_tile candidate position, 3 row re-search candidate
//          position, 4 bin_sort row slot, 5 emit_features stage slot, 6 bin_sort staged bin length,
//          7 winner position of a search, 8 track_link predecessor position, 9 track_rank successor position,
//          10 recon_store predecessor position of a continued mark, 11 recon_gather position followed through the ring,
//          12 gain_ratio byte offset of a dword inside its image plane, 13 gain_ratio list position of an index entry,
//          14 flow_queries query position gathered through snake_pos,
//          15 landmark_chain successor position followed to the next row
#ifdef VH_CHECK
#define VH_CHECK_RANGE(s_, code_, x_, lo_, hi_)                                          \
  do {                                                                                   \
    if ((x_) < (lo_) || (x_) >= (hi_)) {                                                 \
      if (atomicAdd(&(s_).check[0], 1u) == 0u) {                                         \
        (s_).check[1] = (uint32_t)(code_); (s_).check[2] = (uint32_t)(x_); (s_).check[3] = (uint32_t)(hi_); \
      }                                                                                  \
      (x_) = (lo_) < (hi_) ? (((x_) < (lo_)) ? (lo_) : (hi_) - 1) : (lo_);                \
    }                                                                                    \
  } while (0)
#else
#define VH_CHECK_RANGE(s_, code_, x_, lo_, hi_) do { } while (0)
#endif

struct VhPass {
  int32_t qset;  // role (VH_SET_*) providing the queries
  int32_t cset;  // role providing the candidates
  int32_t flow;  // 1: +-radius in v; 0: +-disp_tolerance (stereo search)
  int32_t slot;  // which of the 4 result tables of the stream receives this pass
};

struct VhMatchArgs {
  VhPass pass[4];
  int32_t npass;
  int32_t pair_cur;  // ring slots: current frame | previous frame << 8
  int32_t S;
  int32_t radius, disp_tol;
  int32_t wide_keys;  // test hook (VH_FLOW_WIDE_KEYS): 1 = never the 16-bit position keys, 2 = always the 64-bit keys
  int32_t prior;      // quad with a motion prior (kernels_prior.hip): pass 1 is not searched by match_kernel, and its table is
                      // indexed by the driving feature i1p instead of by the query i2p
  int32_t rows;       // rows (streams) the searches, chains and prior cover: S in group mode, the chunk's frames in sequence mode
  // Sequence mode (vh_sequence_*, vh_row_set): the rows of a slot are consecutive frames of ONE camera.  -1: group mode;
  // otherwise the row of the previous slot that holds the predecessor of row 0 (the last frame of the previous chunk).
  int32_t seq_prev_last = -1;
  int32_t seq_lo;     // sequence mode: rows [seq_lo, rows) are frame pairs (seq_lo = 1 on the first chunk: row 0 has no predecessor)
  int32_t seq_void;   // sequence mode: set id of the (left) empty set that the other rows read -- zeroed once, never written
};

__host__ __device__ inline int32_t vh_set_id(int32_t S, int32_t pair, int32_t stream, int32_t cam) {
  return pair * (2 * S) + stream * 2 + cam;
}
// role: 0=1p 1=2p 2=1c 3=2c
__host__ __device__ inline int32_t vh_role_set(int32_t S, int32_t pairs, int32_t stream, int32_t role) {
  const int32_t pair = (role >= 2) ? (pairs & 0xFF) : (pairs >> 8);
  return vh_set_id(S, pair, stream, role & 1);
}
// The set of `role` for row `row` of a match launch, both modes (every kernel and host getter goes through this).
//   group:    the stream's own slots, vh_role_set (row = stream).
//   sequence: current roles (pair_cur, row, cam); previous roles (pair_cur, row - 1, cam) for row >= 1 and
//             (pair_prev, seq_prev_last, cam) for row 0.  Rows outside [seq_lo, rows) read the empty set seq_void.
__host__ __device__ inline int32_t vh_row_set(const VhMatchArgs &a, int32_t row, int32_t role) {
  if (a.seq_prev_last < 0) return vh_role_set(a.S, a.pair_cur, row, role);
  const int32_t cam = role & 1;
  if (row < a.seq_lo || row >= a.rows) return a.seq_void + cam;
  if (role >= 2) return vh_set_id(a.S, a.pair_cur & 0xFF, row, cam);
  return row > 0 ? vh_set_id(a.S, a.pair_cur & 0xFF, row - 1, cam) : vh_set_id(a.S, a.pair_cur >> 8, a.seq_prev_last, cam);
}

struct VhImages {
  const uint8_t *base[2];  // left / right image of stream 0
  int64_t stride;          // bytes between consecutive streams
  int32_t ncam;            // 1 (mono / flow) or 2 (stereo)
  int32_t S;               // streams covered by this launch (a sub-batch of the group)
  int32_t pair_cur;        // ring slot the new features are written to
  int32_t S_total, s0;     // streams of the group / first stream of this launch (base[] already point at it)
};
// image id = stream*ncam + cam
__host__ __device__ inline const uint8_t *vh_image_ptr(const VhImages &im, int32_t id) {
  const int32_t s = id / im.ncam, cam = id % im.ncam;
  return im.base[cam] + (int64_t)s * im.stride;
}
__host__ __device__ inline int32_t vh_image_set(const VhImages &im, int32_t id) {
  return vh_set_id(im.S_total, im.pair_cur, im.s0 + id / im.ncam, id % im.ncam);
}

// Refinement (kernels_refine.hip): full-resolution du/dv planes, one pair per feature set
// (indexed like the sets; vh_refine_matches: one per role 1p, 2p, 1c, 2c), and the recorded Gauss-Jordan steps of the
// sub-pixel fit's constant normal matrix.
struct VhRefine {
  uint8_t *du, *dv;   // [set][H][pitch]
  int64_t plane;      // bytes per plane: pitch * H
  int32_t pitch;      // W rounded up to 16
  int32_t W, H, bpl;  // full-resolution dims of the pushed images
  int32_t mode;       // 1: pixel (relocateMinimum), 2: sub-pixel (parabolicFitting)
  int32_t gj_row[6], gj_col[6];
  double gj_pivinv[6], gj_dum[6][6];
};

// ---- launchers (defined in the kernels_*.hip files) ------------------------
void vh_launch_half_res(const VhImages &src, uint8_t *dst, const VhGeom &g, hipStream_t st);
void vh_launch_detect_nms(const VhImages &im, const VhGeom &g, uint64_t *rec, int32_t *chunk_count,
                          hipStream_t st);
void vh_launch_emit_features(const VhImages &im, const VhGeom &g, const uint64_t *rec,
                             const int32_t *chunk_count, const VhSets &s, hipStream_t st);
void vh_launch_planes(const uint8_t *img, int32_t bpl, int32_t H, uint8_t *du, uint8_t *dv,
                      int16_t *f1, int16_t *f2, hipStream_t st);

void vh_launch_zero_counters(const VhSets &s, int32_t set0, int32_t nsets, int32_t *extra, int64_t n_extra, hipStream_t st);
void vh_launch_bin_hist(const VhSets &s, int32_t set0, int32_t nsets, hipStream_t st);
void vh_launch_bin_scan(const VhSets &s, int32_t set0, int32_t nsets, hipStream_t st);
void vh_launch_bin_fill(const VhSets &s, int32_t set0, int32_t nsets, hipStream_t st);
void vh_launch_bin_sort(const VhSets &s, int32_t set0, int32_t nsets, int32_t staged, hipStream_t st);
void vh_launch_ref_index(const VhSets &s, int32_t set, int32_t *bin_start_ref, int32_t *list_ref,
                         hipStream_t st);

// findMatch with one prediction for every query of pass 0 (kernels_prior.hip)
void vh_launch_match_prior(const VhSets &s, const VhMatchArgs &a, double u_, double v_, int32_t *best,
                           hipStream_t st);
// (kernels_match.hip) grid_x: workgroups per (pass, stream) row (<= 0: one per 4 tiles of the capacity-sized tile list); lds_bytes: LDS a workgroup
// is to occupy, static part included (<= 0: the static part only) -- see the launcher for what both are for
void vh_launch_match(const VhSets &s, const VhMatchArgs &a, int32_t *best, int32_t *redo, int32_t speculative, int32_t grid_x,
                     int32_t lds_bytes, hipStream_t st);
void vh_launch_quad_prior(const VhSets &s, const VhMatchArgs &a, const double *tr, double f, double cu, double cv, double base, int32_t *best,
                          hipStream_t st);
// (kernels_chain.hip) chain: [stream][cap][2] int4 = {i1p,i2p,i1c,i2c} (z = -2: no match), {uv1p,uv2p,uv1c,uv2c}
void vh_launch_chain(const VhSets &s, const VhMatchArgs &a, int32_t method, const int32_t *best,
                     int4 *chain, uint32_t *mask, uint32_t epoch, int32_t *mchunk, hipStream_t st);
// the flow method's second half of the chain step (first-writer pixel mask): what vh_launch_chain ends with
void vh_launch_flow_keep(const VhSets &s, const VhMatchArgs &a, int4 *chain, const uint32_t *mask, uint32_t epoch, int32_t *mchunk,
                         hipStream_t st);
// pass 2 of multi-stage matching (kernels_chain.hip): the whole circle per driving feature inside the ranges of the
// driver's statistics bin, ranges [row][ubn * vbn][4 stages]{u_min, u_max, v_min, v_max}; writes what vh_launch_chain's
// first kernel writes (flow: vh_launch_flow_keep follows)
void vh_launch_ranged_circle(const VhSets &s, const VhMatchArgs &a, int32_t method, const int32_t *ranges, int4 *chain, uint32_t *mask,
                             uint32_t epoch, int32_t *mchunk, hipStream_t st);
// The motion prior of quad matching: tr [rows][16] row-major 4x4 per row of the launch, and the intrinsics of vh_set_intrinsics
struct VhPriorArgs {
  const double *tr;
  double f, cu, cv, base;
};
// the quad circle of pass 2 with the prior's distance term on its second hop (vh_prior.h); writes what vh_launch_ranged_circle writes
void vh_launch_ranged_circle_prior(const VhSets &s, const VhMatchArgs &a, const int32_t *ranges, const VhPriorArgs &pa, int4 *chain, int32_t *mchunk,
                                   hipStream_t st);
// ref: refined coordinates of the step (vh_launch_refine), or null: the chain's own
void vh_launch_emit_matches(const VhSets &s, const VhMatchArgs &a, int32_t method, const int4 *chain,
                            void *matches, int32_t mcap, int32_t *match_count, int32_t *overflow,
                            const int32_t *mchunk, int32_t *redo, int32_t *mchunk_next, void *host_out, void *host_matches,
                            const float4 *ref, hipStream_t st);

// computePriorStatistics of multi-stage matching on the device (kernels_stats.hip): one workgroup per list.
#define VH_STATS_LDS_MAX 65536  // bytes of LDS the key table [bins][16] may take; larger grids keep their keys in `out`
struct vh_p_match;
struct VhStatsArgs {
  const vh_p_match *pm;   // list l: pm + l * pm_stride, min(counts[l * count_stride], count_cap) records
  int64_t pm_stride;
  const int32_t *counts;  // (a plain array with count_stride = 1, or a field of an array of structures)
  const int32_t *status;  // null, or VH_VOTE_* of list l at status[l * count_stride]: a refused list reads as empty
  int32_t count_stride, count_cap;
  int32_t n_lists, method;
  int32_t ubn, vbn;       // the bin grid of `matching` (matcher.cpp:282-283)
  float bs, R;            // match_binsize, match_radius
  void *out;              // [n_lists][ubn * vbn][4 stages]{u_min, u_max, v_min, v_max}: float, or the int32 windows of vh_launch_ranged_circle
  int32_t *err;           // null, or [n_lists]: set to 1 for a list with a non-finite reference point or delta (zeroed by the caller)
};
void vh_launch_prior_stats(const VhStatsArgs &a, int32_t windows, hipStream_t st);

void vh_refine_setup(VhRefine &rf);  // fills gj_* (host, once per handle)
void vh_launch_refine_planes(const VhImages &im, const VhRefine &rf, hipStream_t st);
// ref: [row][cap][2] float4 {u1p, v1p, u2p, v2p}, {u1c, v1c, u2c, v2c}, written for the kept entries
void vh_launch_refine(const VhSets &s, const VhMatchArgs &a, int32_t method, const VhRefine &rf, int4 *chain, float4 *ref,
                      int32_t *mchunk, hipStream_t st);
// planes of role r (0 = 1p .. 3 = 2c) at rf.du/dv + r * rf.plane; keep[i] = 0 for a dropped record
void vh_launch_refine_records(const VhRefine &rf, int32_t method, struct vh_p_match *pm, int32_t n, int32_t *keep, hipStream_t st);

// Feature tracks (kernels_track.hip).  Lists live in the rows of a launch; tables and track
// records live in SLOTS, so that a list which is final already (the previous step of a group, the carry of a sequence)
// can be looked up beside the rows being linked.
#define VH_TRACK_POS_BITS 24  // table entry: epoch << 24 | (2^24 - 1 - position); a list holds at most 2^24 - 1 records
#define VH_TRACK_POS_MASK ((1u << VH_TRACK_POS_BITS) - 1u)
#define VH_TRACK_EPOCH_MAX ((1u << (32 - VH_TRACK_POS_BITS)) - 1u)
struct vh_track;
struct vh_p_match;
struct VhTrackArgs {
  const vh_p_match *pm;   // list of row r: pm + r * pm_stride, min(counts[r], count_cap) records
  int64_t pm_stride;
  const int32_t *counts;
  int32_t count_cap;
  int32_t rows, n_index;  // rows of the launch; feature indices outside [0, n_index) never link
  uint32_t *tab_c;        // [slots][n_index] lowest position holding the feature as i1c (what the next list looks up)
  uint32_t *tab_p;        // [rows][n_index]  lowest position holding the feature as i1p (this launch only)
  vh_track *trk;          // [slots][trk_stride]
  int64_t trk_stride;
  int32_t *slot_count;    // [slots] records of the list in each slot
  int32_t slot0;          // slot of row 0; row r lives in slot0 + r
  int32_t pred0;          // slot of the predecessor outside the launch, -1: none (see vh_track_pred)
  int32_t chain;          // 1: the rows are consecutive pairs of one camera, row r continues row r - 1; 0: independent streams
  uint32_t epoch, pred_epoch;  // of this launch's bids / of the bids in the predecessor outside the launch
  int64_t serial0;        // serial of row 0's frame B (chain: row r's is serial0 + r)
  uint32_t *check;        // VH_CHECK builds: VhSets::check
};
// The slot that holds the predecessor list of row `row`, -1 if it has none; *in_launch: that list is row - 1 of this launch
// (not final yet: track_rank walks into it).  The counterpart of vh_row_set for lists.
//   chain (sequence handle, vh_link_tracks): row r >= 1 -> row r - 1; row 0 -> the carry slot pred0.
//   group / lone matcher: row r -> slot pred0 + r, the same stream's list of the previous step.
__host__ __device__ inline int32_t vh_track_pred(const VhTrackArgs &t, int32_t row, bool *in_launch) {
  *in_launch = t.chain && row > 0;
  if (*in_launch) return t.slot0 + row - 1;
  return t.pred0 < 0 ? -1 : t.pred0 + (t.chain ? 0 : row);
}
void vh_launch_track_scatter(const VhTrackArgs &t, hipStream_t st);
void vh_launch_track_link(const VhTrackArgs &t, hipStream_t st);
void vh_launch_track_rank(const VhTrackArgs &t, hipStream_t st);
void vh_launch_track_copy(const VhTrackArgs &t, int32_t src, int32_t dst, hipStream_t st);
void vh_launch_track_retag(uint32_t *tab, int64_t n_index, int64_t n_slots, int64_t keep0, int64_t keep1, uint32_t live, hipStream_t st);

// Reconstruction from the lists of a handle or of vh_reconstruct_lists (kernels_recon_gather.hip).
// The ring keeps, per list of the last `ring_slots` frames, one 32-byte record per match record: the list of frame f (the
// pair f - 1 -> f) lives in slot f % ring_slots.  Both halves of a record are aligned 16-byte vectors; a step of the
// gather's walk reads one record, and recon_tails reads only the second half.
// The list axis (section 4.9): a frame holds lists_per_frame lists, one per camera stream (1: a sequence handle,
// vh_reconstruct_lists; S: a group); the list of (frame f, stream s) lives in slot (f % ring_slots) * lists_per_frame + s.
struct VhReconRec {
  float u1p, v1p, u1c, v1c;  // the left camera's pixels in frames f - 1 and f
  int32_t prev;              // vh_track::prev: position of the continued record in the list of frame f - 1, -1: a head
  int32_t age;               // vh_track::age: records of the track up to this one
  int32_t birth_pos;         // vh_track::birth_pos (the birth frame is f - age + 1)
  int32_t cont;              // 1: a record of the list of frame f + 1 continues this one
};
// one lost track, appended by recon_tails (solved tracks from the front of the array, VH_RECON_HISTORY ones from its end)
struct VhReconTail {
  int32_t lost_off, birth_off;  // lost_frame, birth_frame as offsets from the call's window0 (birth_off < 0: only beyond the history)
  int32_t birth_pos, frames;    // frames = age + 1
  int32_t pos;                  // of the track's last record, in its stream's list of frame lost_frame - 1
  int32_t px_off;               // first of its `frames` pixels in the gathered array; -1: older than the history, not gathered
  int32_t stream, reserved;     // the list axis: 0 on a sequence handle; reserved = 0
};
struct VhReconGatherArgs {
  // recon_store: the lists of rows [row_lo, rows) of a launch and their tracks, addressed as VhTrackArgs does; row r is frame0 + r.
  // The list of (row r, stream s) is list r + s * stream_stride of pm / counts / trk.
  int32_t lists_per_frame;
  int64_t stream_stride;
  const vh_p_match *pm;
  int64_t pm_stride;
  const int32_t *counts;
  int32_t count_cap;
  const vh_track *trk;       // list l at trk + l * trk_stride
  int64_t trk_stride;
  int32_t row_lo, rows;
  int64_t frame0;
  int32_t pred_valid;        // 0: the list of row_lo has no predecessor in the ring -- its records are stored as heads
  VhReconRec *ring;          // [ring_slots][lists_per_frame][ring_cap]
  int32_t *ring_count;       // [ring_slots][lists_per_frame]
  int32_t ring_slots, ring_cap, history;
  // recon_tails: the lists of frames [tail_lo, tail_hi) have a successor now; totals = {solved tracks, their pixels,
  // history tracks} of the counting mode, then {solved tracks << 40 | pixels, history tracks} of the appending mode
  int64_t tail_lo, tail_hi;
  unsigned long long *totals;
  VhReconTail *tails;        // [n_tails]
  int32_t n_tails, n_solved;
  int64_t n_pixels;
  // recon_gather: the arrays recon_kernel reads (vh_recon.h); the frame table holds `window` frames from frame `window0`
  // per stream, stream after stream, and first_frame indexes the concatenation
  int64_t window0;
  int32_t window;
  int32_t *first_frame, *offsets, *order;
  float *pixels;
  uint32_t *check;           // VH_CHECK builds: {violations, code, value, bound}
};
void vh_launch_recon_store(const VhReconGatherArgs &a, hipStream_t st);                // the copy, then the continued marks
void vh_launch_recon_tails(const VhReconGatherArgs &a, int32_t append, hipStream_t st);
void vh_launch_recon_gather(const VhReconGatherArgs &a, hipStream_t st);

// n lists of match records, the one view every whole-list stage and both estimators address their input through
// (DESIGN.md section 4.0): slices of one concatenated array (offsets, n_lists + 1 entries: `packed`) or fixed-stride slots
// whose counts live on the device (counts, clamped to count_cap: `slots`).
struct VhLists {
  const vh_p_match *pm;
  int64_t pm_stride;
  const int32_t *offsets, *counts;
  int32_t count_cap, n_lists;
  static VhLists packed(const vh_p_match *pm, const int32_t *offsets, int32_t n) { return VhLists{pm, 0, offsets, nullptr, 0, n}; }
  static VhLists slots(const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t cap, int32_t n) {
    return VhLists{pm, stride, nullptr, counts, cap, n};
  }
};
// list s of them
struct VhList {
  const vh_p_match *pm;
  int32_t n;
};
__device__ __forceinline__ VhList vh_list(const VhLists &l, int32_t s) {
  VhList L;
  L.pm = l.offsets ? l.pm + l.offsets[s] : l.pm + (int64_t)s * l.pm_stride;
  L.n = l.offsets ? l.offsets[s + 1] - l.offsets[s] : min(l.counts[s], l.count_cap);
  return L;
}

struct vh_ego_params;
void vh_launch_ego(const vh_ego_params &e, VhLists lists, const int32_t *rand3, double *xyz, int64_t xyz_stride, double *tr, int32_t *ok,
                   int32_t *ninl, int32_t *inl, int64_t inl_stride, hipStream_t st);

// Motion inliers of whole lists (kernels_inlier.hip).  The lists are addressed as vh_list does;
// flags, out and src_pos of list s begin at offsets[s] (concatenated lists) or at s * out_stride (fixed-stride slots).
#define VH_INLIER_TILE 1024  // records per workgroup
struct VhInlierArgs {
  vh_ego_params e;          // f, cu, cv, base, inlier_threshold (ransac_iters and reweighting are not read)
  VhLists lists;
  int32_t tiles_per_list;  // tiles_per_list >= ceil(longest list / VH_INLIER_TILE)
  const double *tr;         // [n_lists][6]
  const int32_t *ok;        // [n_lists]; 0: the list has no inliers (tr is not read)
  int64_t out_stride;
  uint8_t *flags;
  int32_t *tile_cnt;        // [n_lists][tiles_per_list] inliers per tile, then (after the scan) inliers before the tile
  int32_t *n_inl;           // [n_lists]
  vh_p_match *out;          // the inlier records in list order
  int32_t *src_pos;         // position of each in its list
  // inlier_flag_mono (it reads these in the place of e and tr)
  const vh_mono_model *model;  // [n_lists]; not read where ok = 0
  double mono_threshold;       // vh_mono_params::inlier_threshold
};
void vh_launch_inlier_flag(const VhInlierArgs &a, hipStream_t st);
void vh_launch_inlier_flag_mono(const VhInlierArgs &a, hipStream_t st);
void vh_launch_inlier_compact(const VhInlierArgs &a, hipStream_t st);  // the scan of the tile counts, then the scatter

// The stereo motion refined on whole lists (kernels_refit.hip): the Gauss-Newton loop of
// src/viso_stereo.cpp:126-139 on every record of each list, one workgroup of VH_REFIT_THREADS lanes per list.  The lists
// are a VhLists.
#ifndef VH_REFIT_THREADS
#define VH_REFIT_THREADS 256
#endif
struct VhRefitArgs {
  vh_ego_params e;          // f, cu, cv, base, reweighting (ransac_iters and inlier_threshold are not read)
  VhLists lists;
  const double *tr_in;      // [n_lists][6] the start; not read where ok_in = 0 or the list has fewer than 6 records
  const int32_t *ok_in;     // [n_lists]
  double *tr_out;           // [n_lists][6]; zero where ok_out = 0
  int32_t *ok_out;          // [n_lists]
  int32_t *n_updates;       // [n_lists] updateParameters calls made: 0 (not started), 1 .. 102
};
void vh_launch_refit(const VhRefitArgs &a, hipStream_t st);

// The covariance of a stereo motion over whole lists (kernels_cov.hip): one accumulation pass at
// a fixed tr, sigma^2 (J^T J)^-1, one workgroup of VH_REFIT_THREADS lanes per list.  The lists are addressed as vh_list does.
struct VhCovArgs {
  vh_ego_params e;          // f, cu, cv, base, reweighting (ransac_iters and inlier_threshold are not read)
  VhLists lists;
  const double *tr;         // [n_lists][6]; not read where ok = 0 or the list has fewer than 6 records
  const int32_t *ok;        // [n_lists]
  double *cov;              // [n_lists][36] row-major, exactly symmetric; zero where ok_out = 0
  double *ssr;              // [n_lists] the sum of the 4 N squared weighted residuals; zero where ok_out = 0
  int32_t *ok_out;          // [n_lists]
};
void vh_launch_motion_cov(const VhCovArgs &a, hipStream_t st);

// The epipolar model refitted on whole lists (kernels_mono_refit.hip): fundamentalMatrix over every
// record of a list in the frame of the incoming model, one workgroup of VH_REFIT_THREADS lanes per list.  The lists are
// addressed as vh_list does.
struct VhMonoRefitArgs {
  VhLists lists;
  const vh_mono_model *model_in;  // [n_lists]; not read where ok_in = 0 or the list has fewer than 10 records
  const int32_t *ok_in;           // [n_lists]
  vh_mono_model *model_out;       // [n_lists]; c, s copied, F refitted, valid = 1; the zero record where ok_out = 0
  int32_t *ok_out;                // [n_lists]
  double *w_out;                  // [n_lists][2] the two smallest singular values of M: w[8], w[7]; zero where ok_out = 0
};
void vh_launch_mono_refit(const VhMonoRefitArgs &a, hipStream_t st);

// The pose tail of the mono estimator on whole lists (kernels_mono_pose.hip): E, the four (R, t)
// candidates, the chirality count of every record, the points in front under the winner, their median distance, the
// ground-plane vote, tr.  The lists are addressed as vh_list does; dist and d of list s begin at offsets[s]
// (concatenated lists) or at s * slot_stride (fixed-stride slots).
#define VH_MONO_POSE_TILE 512  // elements of a list staged in LDS per trip of the rank and vote kernels
#define VH_MONO_POSE_HDR 96    // doubles per list: Ra[9] Rb[9] t0[3] | P1[12] | P2[4][12] | median | int32: counts[4], reason, winner, np
// the header of a list (doubles): kernels_mono_pose.hip writes and reads it, kernels_mono_pose_refine.hip rewrites the winner's slot
#define MP_H_RT 0     /* Ra[9], Rb[9], t0[3] */
#define MP_H_P1 21    /* [K | 0], [12] */
#define MP_H_P2 33    /* P2 of the four candidates, [4][12] */
#define MP_H_MED 81   /* the median (mono_pose_rank) */
#define MP_H_INT 82   /* int32 from here: counts[4], reason, winner, np */
#define MP_I_REASON 4
#define MP_I_BEST 5
#define MP_I_NP 6
static_assert(MP_H_INT * 8 + 7 * 4 <= VH_MONO_POSE_HDR * 8, "mono pose header");
struct VhMonoPoseArgs {
  vh_mono_params e;         // f, cu, cv, height, pitch, motion_threshold (ransac_iters and inlier_threshold are not read)
  VhLists lists;
  int64_t cap;              // >= the longest list: the grids of the per-record kernels are sized by it
  int64_t slot_stride;
  const vh_mono_model *model;  // [n_lists]; not read where ok_in = 0
  const int32_t *ok_in;        // [n_lists]
  double *hdr;              // [n_lists][VH_MONO_POSE_HDR]
  double *dist, *d;         // per record slot: the L1 distance (later the vote's sum) and the ground-plane coordinate of the points in front
  double *tr;               // [n_lists][6]
  int32_t *ok;              // [n_lists]
  vh_mono_pose *pose;       // [n_lists]
};
// launch k of the six, in this order on one stream: 0 head, 1 tri, 2 front, 3 rank, 4 vote, 5 finish (a launch each, so
// that a handle can time every kernel under a scope of its own: vh_mono_pose_scope(k))
#define VH_MONO_POSE_STAGES 6
void vh_launch_mono_pose_stage(const VhMonoPoseArgs &a, int32_t k, hipStream_t st);
const char *vh_mono_pose_scope(int32_t k);
// The pose refined between launches 1 and 2 (kernels_mono_pose_refine.hip): Gauss-Newton on the
// Sampson distance of every record from the winner of the chirality counts, one workgroup of VH_REFIT_THREADS lanes per
// list; where it converges, the refined R, t and projection matrix replace the winner's in the list's header, which the
// launches 2..5 then read as they always do.  refine: [n_lists].  grid: a.n_lists workgroups.
void vh_launch_mono_pose_refine(const VhMonoPoseArgs &a, vh_mono_refine *refine, hipStream_t st);

// The 3-d points of whole lists, compacted in list order (kernels_scene.hip).  The lists are
// addressed as vh_list does; out (and src, where given) of list s begin at offsets[s] (concatenated lists) or at
// s * out_stride (fixed-stride slots).
#define VH_SCENE_TILE 256  // records per workgroup, one per lane
struct VhSceneArgs {
  vh_ego_params e;          // stereo: f, cu, cv, base
  vh_mono_params m;         // mono: f, cu, cv
  vh_scene_params sp;
  VhLists lists;
  int32_t tiles_per_list;  // tiles_per_list >= ceil(longest list / VH_SCENE_TILE)
  const double *tr;         // stereo: [n_lists][6]; not read where ok = 0
  const vh_mono_pose *pose; // mono: [n_lists]; R, t, scale are read, and not where ok = 0
  const int32_t *ok;        // [n_lists]; 0: the list has no points
  const double *Tw;         // null, or [n_lists][16] row-major
  const int32_t *src;       // null (a record's src_pos is its position in the list), or indexed like out: the value to store
  int64_t out_stride;
  int32_t *tile_cnt;        // [n_lists][tiles_per_list] survivors per tile, then (after the scan) survivors before the tile
  int32_t *n_out;           // [n_lists]
  vh_scene_point *out;      // the points in list order
};
void vh_launch_scene_points(const VhSceneArgs &a, bool mono, hipStream_t st);  // flag, scan, store
void vh_launch_scene_scan(const VhSceneArgs &a, hipStream_t st);                // the scan alone: lists (lengths only), ok, tile_cnt, n_out

// Landmarks: the scene points of a step fused along the feature tracks (kernels_landmark.hip).
// Three families of lists, each either slices of one concatenated array (offsets, n_lists + 1 entries) or fixed-stride
// slots whose counts live on the device (counts, clamped to the stride): the records (trk, and state_out / out / obs
// indexed like it), their scene points, and the predecessor lists' states (prev null: no list has a predecessor).
struct VhLandmarkArgs {
  vh_landmark_params lp;
  int32_t n_lists;
  int32_t tiles_per_list;          // >= ceil(longest record list / VH_SCENE_TILE)
  const vh_track *trk;
  const int32_t *rec_offsets, *rec_counts;
  int64_t rec_stride;
  const vh_scene_point *pts;
  const int32_t *pt_offsets, *pt_counts;
  int64_t pt_stride;
  const int32_t *ok;               // [n_lists] the scan's ok: non-zero where the list has points (0: count 0, its tile counts are not read)
  const vh_landmark_state *prev;
  const int32_t *prev_offsets, *prev_counts;
  int64_t prev_stride;
  vh_landmark_state *state_out;
  vh_landmark *out;                // list s compacted at its first record's position
  int32_t *obs;                    // per record: the position of its scene point, -1: none; after landmark_fuse: of the emitted ones only
  int32_t *tile_cnt;               // [n_lists][tiles_per_list] emitted per tile, then (after the scan) emitted before the tile
  int32_t *n_out;                  // [n_lists]
};
// the memset of obs, then index, fuse, scan, store on one stream; obs_elems: the elements of obs the lists span.
// The caller keeps n_lists * tiles_per_list below 2^30.  -> the memset's code
hipError_t vh_launch_landmarks(const VhLandmarkArgs &a, int64_t obs_elems, hipStream_t st);
// its index, scan and store launches alone (what the chain form shares)
void vh_launch_landmark_index(const VhLandmarkArgs &a, hipStream_t st);
void vh_launch_landmark_scan(const VhLandmarkArgs &a, hipStream_t st);
void vh_launch_landmark_store(const VhLandmarkArgs &a, hipStream_t st);

// Landmarks of lists that are the rows of one chain (kernels_landmark_chain.hip): list s's
// predecessor is list s - 1 of the same call, list 0's the carry.  a.prev* are not read.
struct VhLandmarkChainArgs {
  VhLandmarkArgs a;
  int32_t *next;                   // indexed like a.obs, and the array right behind it: the record of the next list that continues this one, -1: none
  const vh_landmark_state *carry;  // null: list 0 has no predecessor
  const int32_t *carry_count;      // the carry's length on the device (clamped to [0, carry_cap]); null: n_carry
  int32_t n_carry, carry_cap;
  uint32_t *check;                 // VH_CHECK builds: {violations, code, value, bound}
};
// the memset of obs and next (obs_elems each), then launch k of the six, in this order on one stream: 0 index, 1 link,
// 2 chain, 3 count, 4 scan, 5 store (a launch each, so that a handle can time every kernel under a scope of its own).
// The caller keeps n_lists * tiles_per_list below 2^30.
#define VH_LANDMARK_CHAIN_STAGES 6
hipError_t vh_launch_landmarks_chain_clear(const VhLandmarkChainArgs &c, int64_t obs_elems, hipStream_t st);
void vh_launch_landmarks_chain_stage(const VhLandmarkChainArgs &c, int32_t k, hipStream_t st);
const char *vh_landmark_chain_scope(int32_t k);

// The motion refit on the landmarks (kernels_lmk_refit.hip): refit_prior writes every record's
// point (vh_refit_prior.h), refit_prior_fit is the loop of VhRefitArgs over those points.  The lists are a VhLists; prior
// of list s begins where its records do (offsets[s], or s * pm_stride).  A record's position in the predecessor list:
// prev_pos (indexed like the records), or -- where it is null -- trk[src_pos[i]].prev with src_pos indexed like the
// records and list s's tracked records the first min(trk_counts[s], slot_stride) of trk + s * slot_stride.  The
// predecessor lists' states: slices of one array (prev_offsets) or slots of prev_stride whose counts live on the device
// (prev_counts, clamped to the stride); prev null: no list has a predecessor.
struct VhLmkRefitArgs {
  vh_ego_params e;                 // f, cu, cv, base, reweighting
  vh_lmk_refit_params rp;
  VhLists lists;
  int32_t tiles_per_list;          // >= ceil(longest list / VH_SCENE_TILE)
  const int32_t *prev_pos;
  const int32_t *src_pos;
  const vh_track *trk;
  const int32_t *trk_counts;
  int64_t slot_stride;
  const vh_landmark_state *prev;
  const int32_t *prev_offsets, *prev_counts;
  int64_t prev_stride;
  const double *Tw;                // [n_lists][16] row-major, the previous camera to the world
  vh_refit_prior *prior;
  int32_t *n_used;                 // [n_lists], zeroed by the launch function: records with source == 1
  const double *tr_in;             // the fit's arguments: VhRefitArgs'
  const int32_t *ok_in;
  double *tr_out;
  int32_t *ok_out;
  int32_t *n_updates;
};
// the memset of n_used and the refit_prior launch on one stream -> the memset's code.  The caller keeps
// n_lists * tiles_per_list below 2^30.
hipError_t vh_launch_refit_prior(const VhLmkRefitArgs &a, hipStream_t st);
// behind it on the same stream; grid: a.lists.n_lists workgroups (the caller keeps it below 2^24)
void vh_launch_refit_prior_fit(const VhLmkRefitArgs &a, hipStream_t st);

// The trajectory (kernels_trajectory.hip): n_chains chains of rows, a workgroup each.  Chain c is
// the rows [offsets[c], offsets[c + 1]), or without offsets the rows [c * rows_per_chain, (c + 1) * rows_per_chain).
struct VhTrajArgs {
  vh_traj_params p;
  int32_t n_chains;
  const int32_t *offsets;          // null: rows_per_chain rows each
  int32_t rows_per_chain;
  int32_t pair_lo, pair_hi;        // row k of a chain (counted from its first row) holds a pair iff pair_lo <= k < pair_hi
  const double *tr;                // [rows][6]
  const int32_t *ok;               // [rows]; < 0: the row holds no pair
  const double *T0;                // [n_chains][16], null: the unit matrix; not read where carry_in is given
  const vh_traj_carry *carry_in;   // [n_chains], nullable
  vh_traj_pose *out;               // [rows]
  vh_traj_carry *carry_out;        // [n_chains], nullable (may be carry_in: a chain reads its carry before it writes it)
};
void vh_launch_trajectory(const VhTrajArgs &a, hipStream_t st);

// The pose covariance along the same chains (kernels_trajectory_cov.hip): chains, rows and pairs
// as VhTrajArgs'.
struct VhTrajCovArgs {
  vh_traj_params p;
  double fill_scale;
  int32_t n_chains;
  const int32_t *offsets;               // null: rows_per_chain rows each
  int32_t rows_per_chain;
  int32_t pair_lo, pair_hi;
  const double *tr;                     // [rows][6]
  const int32_t *ok;                    // [rows]; < 0: the row holds no pair
  const double *cov;                    // [rows][36] the motions' covariances
  const int32_t *ok_cov;                // [rows]
  const double *Sigma0;                 // [n_chains][36], null: zero; not read where carry_in is given
  const vh_traj_cov_carry *carry_in;    // [n_chains], nullable
  vh_traj_cov *out;                     // [rows]
  vh_traj_cov_carry *carry_out;         // [n_chains], nullable (may be carry_in)
};
void vh_launch_trajectory_cov(const VhTrajCovArgs &a, hipStream_t st);

// The camera gain over index lists into match lists (kernels_gain.hip).  The lists are addressed
// as vh_list does, and so are the index lists: slices of one concatenated array (idx_offsets) or slots of idx_stride
// entries whose counts live on the device (idx_counts, clamped to idx_cap); the ratio of an entry lies where the entry does.
// The images are u8 planes of `pitch` bytes per row (a multiple of 4, the base 4-byte aligned), `plane` bytes apart.
#define VH_GAIN_TILE 256  // index entries per workgroup of gain_ratio
struct VhGainArgs {
  VhLists lists;
  const int32_t *idx;
  int64_t idx_stride;
  const int32_t *idx_offsets, *idx_counts;
  int32_t idx_cap;
  const int32_t *ok;        // null, or [n_lists]; 0: the list reads as one without index entries
  int32_t tiles_per_list;   // tiles_per_list >= ceil(longest index list / VH_GAIN_TILE)
  const uint8_t *planes_prev, *planes_cur;
  int64_t plane;
  int32_t pitch, W, H;
  // by_set = 0: list l reads plane l of planes_prev / planes_cur.  1 (a handle): the plane of its previous / current left
  // set under m (vh_row_set(m, l, 0 / 2) >> 1: the planes are indexed by ring slot and row); a sequence row outside
  // [seq_lo, rows) reads as a list without index entries
  int32_t by_set;
  VhMatchArgs m;
  float *ratio;
  float *gain;              // [n_lists]
  int32_t *num;             // [n_lists]
  uint32_t *check;          // VH_CHECK builds: {violations, code, value, bound}
};
void vh_launch_gain_copy(const uint8_t *src, int64_t stride, int32_t bpl, int32_t W, int32_t H, int32_t n_images, uint8_t *dst, int64_t plane,
                         int32_t pitch, hipStream_t st);
void vh_launch_gain_ratio(const VhGainArgs &a, hipStream_t st);
void vh_launch_gain_sum(const VhGainArgs &a, hipStream_t st);  // behind gain_ratio on the same stream

struct vh_mono_params;
int64_t vh_mono_scratch_bytes(int32_t n_sets, int64_t cap, int32_t ransac_iters);
// model (nullable): [n_sets] the normalisation and the refit F of every list (vh_mono_model), written by mono_final_a
void vh_launch_mono(const vh_mono_params &e, VhLists lists, const int32_t *rand8, uint8_t *scratch, int64_t cap, double *tr, int32_t *ok,
                    int32_t *ninl, int32_t *inl, int64_t inl_stride, vh_mono_model *model, hipStream_t st);

#endif
