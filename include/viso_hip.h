/*
 * viso_hip.h -- C ABI of libviso_hip.so: the MI355X (gfx950) implementation of
 * the libviso2-style feature detection + matching hot path of
 * Chang-Tun-Yu/HLS-final-Visual-Odometry.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types.  Each entry point names the reference interface it replaces
 * (file:line relative to the reference tree).  include/viso_hip_matcher.hpp
 * wraps these calls in a C++ `Matcher` class with the reference's public
 * method set, so src/viso_stereo.cpp / src/viso_mono.cpp compile against it
 * unchanged.
 *
 * All compute runs in hand-written HIP kernels; there is no CPU fallback.
 * Every call returns VH_OK (0) or a negative VH_ERR_* code; nothing throws.
 *
 * Threading: a handle is not re-entrant (neither is the reference's Matcher);
 * use one handle per camera stream and one host thread per handle.
 */
#ifndef VISO_HIP_H
#define VISO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VH_ABI_VERSION 1

/* ---- error codes ------------------------------------------------------- */
#define VH_OK 0
#define VH_ERR_INVALID_ARG (-1)  /* null pointer, bad dims (reference: cerr "Image dimension mismatch", src/matcher.cpp:59-62) */
#define VH_ERR_NO_DEVICE (-2)    /* no HIP device / kernel image for this GPU: the product path never falls back to the CPU */
#define VH_ERR_HIP (-3)          /* a HIP runtime call failed; see vh_last_error() */
#define VH_ERR_CAPACITY (-4)     /* more features/matches than the capacity given (the reference overruns POINT_L silently, src/matcher.cpp:332) */
#define VH_ERR_UNSUPPORTED (-5)  /* parameter outside the supported envelope (see vh_create) */
#define VH_ERR_STATE (-6)        /* e.g. match before two frames were pushed */

/* ---- types --------------------------------------------------------------- */

/* POD mirror of Matcher::parameters, field for field (src/matcher.h:45-72). */
typedef struct vh_params {
  int32_t nms_n;                  /* non-max-suppression: min. distance between maxima (pixels) */
  int32_t nms_tau;                /* non-max-suppression: interest point peakiness threshold */
  int32_t match_binsize;          /* matching bin width/height */
  int32_t match_radius;           /* matching radius (du/dv in pixels) */
  int32_t match_disp_tolerance;   /* dv tolerance for stereo matches (pixels) */
  int32_t outlier_disp_tolerance; /* disparity tolerance of the outlier vote under VH_VOTE_STOCK (vh_set_vote_rule); not read under the default rule, as in the reference */
  int32_t outlier_flow_tolerance; /* flow tolerance of the outlier vote under VH_VOTE_STOCK; not read under the default rule (the reference's literal 5) */
  int32_t multi_stage;            /* 1 = also extract the sparse feature set (max1) */
  int32_t half_resolution;        /* 1 = detect at half resolution, coordinates x2 */
  int32_t refinement;             /* 0 = none, 1 = pixel, 2 = sub-pixel relocation of the matches (stock libviso2;
                                     absent from the reference): see vh_refine_matches */
  double f, cu, cv, base;         /* calibration (only for match prediction; unused) */
} vh_params;

/* Mirror of Matcher::p_match (src/matcher.h:89-104): 48 bytes, unused slots = -1. */
typedef struct vh_p_match {
  float u1p, v1p; int32_t i1p; /* previous left  */
  float u2p, v2p; int32_t i2p; /* previous right */
  float u1c, v1c; int32_t i1c; /* current  left  */
  float u2c, v2c; int32_t i2c; /* current  right */
} vh_p_match;

/* Feature records are int32[12] = {u, v, 0, class, d1..d8} exactly as
 * Matcher::computeFeatures packs them (src/matcher.cpp:663-671). */
#define VH_FEATURE_WORDS 12

/* Which ring-buffer feature set (vh_get_features). */
#define VH_SET_1P 0 /* previous left  */
#define VH_SET_2P 1 /* previous right */
#define VH_SET_1C 2 /* current  left  */
#define VH_SET_2C 3 /* current  right */

/* Matching method (Matcher::matchFeatures, src/matcher.h:124-128). */
#define VH_METHOD_FLOW 0
#define VH_METHOD_STEREO 1
#define VH_METHOD_QUAD 2

typedef struct vh_matcher vh_matcher; /* one camera stream (== one Matcher)      */
typedef struct vh_group vh_group;     /* S independent streams stepped together  */

/* ---- library ------------------------------------------------------------- */
int32_t vh_abi_version(void);
/* Number of visible HIP devices, or VH_ERR_NO_DEVICE. */
int32_t vh_device_count(void);
const char *vh_error_string(int32_t code);
/* Text of the last failing HIP call on this thread ("" if none). */
const char *vh_last_error(void);
/* Matcher::parameters() defaults (src/matcher.h:60-71). */
void vh_default_params(vh_params *p);

/* ---- one stream: the Matcher surface ----------------------------------- */

/* Matcher::Matcher(parameters) (src/matcher.cpp:32-41) on HIP device `device`.
 * Envelope (VH_ERR_UNSUPPORTED outside): 1 <= nms_n <= 32, match_binsize >= 1,
 * 0 <= match_radius <= 16384, 0 <= match_disp_tolerance <= 16384, nms_tau >= 0,
 * images up to 16384 x 16384 with a row pitch dims[2] < 2^24 bytes and dims[2]*dims[1] <= 2^28
 * bytes.  max_features/max_matches = 0 select the
 * worst-case capacity for the pushed image size (4 per NMS block), clamped to
 * 16 777 215 features per image.
 * When a pushed image yields more features than the capacity, the records
 * beyond it are dropped, matching runs on the truncated sets, and
 * vh_get_matches / vh_group_get_matches(_all) / vh_group_wait_download return
 * VH_ERR_CAPACITY (vh_get_features reports the true count). */
int32_t vh_create(const vh_params *p, int32_t device, vh_matcher **out);
int32_t vh_create_ex(const vh_params *p, int32_t device, int32_t max_features,
                     int32_t max_matches, vh_matcher **out);
/* Matcher::~Matcher (src/matcher.cpp:44-49). */
void vh_destroy(vh_matcher *m);
/* Matcher::setIntrinsics (src/matcher.h:81-86). */
int32_t vh_set_intrinsics(vh_matcher *m, double f, double cu, double cv, double base);

/* Matcher::pushBack(I1,I2,dims,replace) (src/matcher.h:116, src/matcher.cpp:51-91)
 * with the stock computeFeatures behind it (src/matcher.cpp:585-672).
 * I1/I2: host images, row-major u8, stride dims[2] >= dims[0]; I2 may be NULL
 * (mono/flow).  The images are borrowed for the duration of the call.
 * A call whose dims differ from the previous one's starts a new sequence: the
 * ring buffer is emptied (the reference keeps the old pair and would match
 * across image sizes, src/matcher.cpp:64-84; no caller does that). */
int32_t vh_push_back(vh_matcher *m, const uint8_t *I1, const uint8_t *I2,
                     const int32_t dims[3], int32_t replace);
/* Same, images already resident in device memory (e.g. a torch tensor's
 * data_ptr); asynchronous (the images must stay valid until vh_synchronize or
 * the next vh_get_*). */
int32_t vh_push_back_device(vh_matcher *m, const void *dI1, const void *dI2,
                            const int32_t dims[3], int32_t replace);

/* Page-locked host memory for image buffers handed to vh_push_back /
 * vh_group_push_back.  The reference's callers read frames into malloc'd
 * buffers (src/demo.cpp:107-110) and lend them to pushBack for the call
 * (src/matcher.cpp:51-91); any host pointer works here too, but uploads from
 * page-locked memory run at PCIe rate instead of through the driver's bounce
 * buffer.  Needs a device (VH_ERR_NO_DEVICE otherwise). */
int32_t vh_host_alloc(int32_t device, size_t bytes, void **out);
int32_t vh_host_free(void *ptr);

/* Matcher::matchFeatures(method, Tr_delta) (src/matcher.h:128,
 * src/matcher.cpp:93-111) with the stock Matcher::matching behind it
 * (src/matcher.cpp:274-344).  Tr_delta16 = NULL: no motion prior -- what the
 * reference's matchFeatures does with ANY Tr_delta (it ignores the argument),
 * and what the C++ shim passes.  Tr_delta16 != NULL (row-major 4x4) with
 * method 2 after vh_set_intrinsics: stock libviso2's prior
 * [upstream-recollection; absent from the reference tree] -- the hop previous
 * right -> current right of the quad circle is searched with findMatch's
 * prediction term (src/matcher.cpp:257-262, pinned) around the position that
 * Tr_delta predicts for the 3-d point of the (1p, 2p) pair
 * (csrc/kernels_prior.hip).  VH_ERR_STATE without intrinsics (f, base > 0).  The reference's matchFeatures goes on to
 * call removeOutliers (src/matcher.cpp:108); here that is the separate
 * vh_remove_outliers below, which the C++ shim calls for you. */
int32_t vh_match_features(vh_matcher *m, int32_t method, const double *Tr_delta16);

/* removeOutliers (src/remove_outliers.cpp:4-94 over src/delaunator.cpp:183-407):
 * Delaunay-neighbour flow-consistency vote on the current matches, host side
 * (a sequential float triangulation whose result depends on its
 * visiting order -- see csrc/outliers.cpp).  Filters flow and quad matches;
 * stereo matches (no previous-frame position) are left as they are.  Under
 * VH_VOTE_STOCK (vh_set_vote_rule, below) the vote uses the last match call's
 * method and the handle's two tolerances, and stereo matches are voted too.
 * VH_ERR_STATE before the first vh_match_features. */
int32_t vh_remove_outliers(vh_matcher *m);
/* The same on caller-owned records, in place, order preserved; *n_out = count
 * kept.  Pure host function: needs no device. */
int32_t vh_remove_outliers_pm(vh_p_match *pm, int32_t n, int32_t *n_out);
/* The same on the DEVICE for n_lists lists at once (csrc/kernels_vote.hip): list l = pm[l * stride .. + counts[l]).
 * The triangulation under the vote stays the sequential chain it is (csrc/sweep_hull.h, the code the host form
 * runs): one list per GPU lane, lanes_per_wave (1..64) lists per wavefront -- latency per list is tens of
 * milliseconds, the throughput comes from the number of lists in flight (see vh_group_post_begin_device).
 * max_features < 1: removeOutliers only, out[l * out_cap ..] receives list l's survivors in order;
 * max_features >= 1: followed by Matcher::bucketFeatures(max_features, bucket_width, bucket_height)
 * (src/matcher.cpp:140-187), out receives the bucketed lists.  out_counts[l]: records of list l in out;
 * n_triangles (nullable): triangles of each list's triangulation; sweep_ms (nullable): device time of the
 * sweep kernel.  VH_ERR_CAPACITY if a list does not fit out_cap; VH_ERR_UNSUPPORTED for lists the sweep
 * refuses (NaN / infinite / negative coordinates, more than 31 flips pending in one legalisation -- the reference's
 * stack has 13 slots and is undefined beyond; such a list's sweep stops at the flip that does not fit, nothing of it is
 * delivered, out_counts[l] = 0, and the other lists of the call are delivered as usual). */
int32_t vh_remove_outliers_device(int32_t device, int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts,
                                  int32_t lanes_per_wave, int32_t max_features, float bucket_width, float bucket_height,
                                  vh_p_match *out, int32_t out_cap, int32_t *out_counts, int32_t *n_triangles, float *sweep_ms);

/* ---- the rule of the vote ---------------------------------------------------
 * VH_VOTE_REFERENCE (the default everywhere): the reference's cut-down vote (src/remove_outliers.cpp:34-90) -- the flow
 * term under the literal 5, no method; method and the tolerances are not read, and on a handle a stereo list is not voted.
 * VH_VOTE_STOCK: stock libviso2's Matcher::removeOutliers(p_matched, method) [upstream-recollection; absent from the
 * reference tree, parity unpinned] as this project defines it, in single precision, for a list of method M:
 *     fu(i) = u1c - u1p,  fv(i) = v1c - v1p,  d(i) = u1c - u2c
 *     F(a,b) = fabsf(fu(a) - fu(b)) + fabsf(fv(a) - fv(b)) < flow_tolerance
 *     D(a,b) = fabsf(d(a) - d(b)) < disp_tolerance
 *     agree(a,b) = M == 0 ? F : M == 1 ? D : (D && F)
 * Everything else is the vote as it is: n <= 3 returns the list, the points are (u1c, v1c) under the same triangulation
 * (csrc/sweep_hull.h), a triangle gives each corner one vote per agreeing edge it lies on, a record survives with at
 * least 4 votes, in list order.  The compares are strict: a NaN term disagrees, a tolerance <= 0 agrees with nothing
 * (every record of a list longer than 3 is dropped).  STOCK with method 0 and flow_tolerance 5 is REFERENCE bit for bit.
 * Any other rule, or a method outside 0..2 under VH_VOTE_STOCK, is VH_ERR_INVALID_ARG.  A NULL rule is VH_VOTE_REFERENCE. */
#define VH_VOTE_REFERENCE 0
#define VH_VOTE_STOCK 1
typedef struct vh_vote_rule {
  int32_t rule;          /* VH_VOTE_REFERENCE or VH_VOTE_STOCK */
  int32_t method;        /* VH_METHOD_* of the list (STOCK only) */
  float flow_tolerance;  /* STOCK only */
  float disp_tolerance;  /* STOCK only */
} vh_vote_rule;
typedef char vh_vote_rule_is_16_bytes[sizeof(vh_vote_rule) == 16 ? 1 : -1]; /* (a static assertion that C99 and C++11 both take) */
/* vh_remove_outliers_pm / vh_remove_outliers_device under a rule (the plain entries are these with rule = NULL); the
 * refusals and the envelope of the device form are unchanged. */
int32_t vh_remove_outliers_pm_rule(vh_p_match *pm, int32_t n, const vh_vote_rule *rule, int32_t *n_out);
int32_t vh_remove_outliers_device_rule(int32_t device, int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts,
                                       int32_t lanes_per_wave, int32_t max_features, float bucket_width, float bucket_height,
                                       vh_p_match *out, int32_t out_cap, int32_t *out_counts, int32_t *n_triangles, float *sweep_ms,
                                       const vh_vote_rule *rule);
/* The rule of a handle (lone matcher, group or sequence handle): rule = VH_VOTE_REFERENCE or VH_VOTE_STOCK, before the
 * first push only (VH_ERR_STATE afterwards).  Under VH_VOTE_STOCK every vote of the handle -- vh_remove_outliers,
 * vh_group_remove_outliers, the host and device post chains, pass 1 of multi-stage matching in host and device mode and
 * so what vh_(group_)get_sparse_matches returns -- uses the method of the list it votes (stereo lists are voted too) and
 * the tolerances (float)outlier_flow_tolerance / (float)outlier_disp_tolerance of the vh_params given at creation.  With
 * the default rule nothing is allocated, launched or decided differently; no rule needs more device memory. */
int32_t vh_set_vote_rule(vh_matcher *m, int32_t rule);
int32_t vh_group_set_vote_rule(vh_group *g, int32_t rule);

/* Matcher::bucketFeatures (src/matcher.h:132, src/matcher.cpp:140-187):
 * host-side post-processing of the current matches, LFSR shuffle included. */
int32_t vh_bucket_features(vh_matcher *m, int32_t max_features, float bucket_width,
                           float bucket_height);

/* Matcher::getMatches (src/matcher.h:138-143).  *n receives the true count;
 * at most cap records are written (VH_ERR_CAPACITY if n > cap). */
int32_t vh_get_matches(vh_matcher *m, vh_p_match *out, int32_t cap, int32_t *n);
/* The ring buffer's feature records (max2p/max2c in the reference,
 * src/matcher.h:252): the parity contract includes descriptors. */
int32_t vh_get_features(vh_matcher *m, int32_t which, int32_t *out12, int32_t cap, int32_t *n);
/* Block until everything queued on the handle's stream has finished. */
int32_t vh_synchronize(vh_matcher *m);
/* Order this handle's work after a caller-owned hipStream_t (e.g. the stream
 * that produces the device images, torch's current stream): every pushBack
 * first waits for what that stream has been given so far.  The work itself runs
 * on the handle's internal (non-blocking) streams -- detection of frame t+1
 * overlaps matching of frame t -- and results are complete after
 * vh_synchronize / vh_get_*.  The handle 0 (NULL) is the legacy default
 * stream and is ordered after like any other stream; without a set stream
 * (the initial state, or after vh_clear_stream) a pushBack is ordered after
 * nothing, and images produced on ANY stream, the default one included, must
 * be complete (hipStreamSynchronize) before vh_push_back_device. */
int32_t vh_set_stream(vh_matcher *m, void *hip_stream);
int32_t vh_clear_stream(vh_matcher *m);
/* The reverse ordering: make `hip_stream` wait (on the device, without
 * blocking the host) until the images handed to the last vh_push_back_device
 * have been consumed, so that work queued on it afterwards may overwrite them. */
int32_t vh_stream_wait_images(vh_matcher *m, void *hip_stream);

/* ---- stateless primitives (private members of the reference's Matcher) -- */

/* Matcher::computeFeatures (src/matcher.h:209, src/matcher.cpp:585-672).
 * max1/num1 (sparse set, multi_stage only), du/dv (matching-resolution
 * gradient planes, stride dims_matching[2]) may be NULL.  num1/num2 return
 * the true counts. */
int32_t vh_compute_features(const vh_params *p, int32_t device, const uint8_t *I,
                            const int32_t dims[3], int32_t *max1, int32_t cap1,
                            int32_t *num1, int32_t *max2, int32_t cap2, int32_t *num2,
                            uint8_t *du, uint8_t *dv);
/* filter::sobel5x5 / blob5x5 / checkerboard5x5 (src/filter.h:80-96) on the
 * valid interior; pixels outside it are 0.  Any output may be NULL. */
int32_t vh_filters(int32_t device, const uint8_t *I, int32_t bpl, int32_t H, uint8_t *du,
                   uint8_t *dv, int16_t *f1, int16_t *f2);
/* Matcher::createIndexVector (src/matcher.cpp:194-214) flattened to CSR in the
 * reference's bin numbering (c*v_bin_num+v_bin)*u_bin_num+u_bin:
 * bin_start[4*ubn*vbn+1], list[n]. */
int32_t vh_create_index(const vh_params *p, int32_t device, const int32_t dims[3],
                        const int32_t *m, int32_t n, int32_t *bin_start, int32_t *list);
/* Matcher::findMatch (src/matcher.cpp:216-272) for every query of set 1
 * against set 2: best[i1] = min_ind.  flow=0 narrows v to
 * +-match_disp_tolerance (stock libviso2 stereo search). */
int32_t vh_match_all(const vh_params *p, int32_t device, const int32_t dims[3],
                     const int32_t *m1, int32_t n1, const int32_t *m2, int32_t n2,
                     int32_t flow, int32_t *best);
/* Matcher::findMatch with its optional match-prediction term
 * (src/matcher.cpp:257-262): cost = SAD + 4*||(u2,v2)-(u_,v_)|| evaluated and
 * compared in double, as the reference does.  No caller in the reference passes
 * u_,v_ (they default to -1 = off); provided so that the whole primitive is
 * covered.  Not on the throughput path (one lane per query, double math). */
int32_t vh_match_all_prior(const vh_params *p, int32_t device, const int32_t dims[3],
                           const int32_t *m1, int32_t n1, const int32_t *m2, int32_t n2,
                           int32_t flow, double u_, double v_, int32_t *best);
/* Matcher::matching (src/matcher.h:218, src/matcher.cpp:274-344) on
 * caller-supplied feature arrays. Unused sets: NULL/0.  There are no images
 * here: the list is never refined, whatever p->refinement says. */
int32_t vh_match(const vh_params *p, int32_t device, const int32_t dims[3], int32_t method,
                 const int32_t *m1p, int32_t n1p, const int32_t *m2p, int32_t n2p,
                 const int32_t *m1c, int32_t n1c, const int32_t *m2c, int32_t n2c,
                 vh_p_match *out, int32_t cap, int32_t *n);

/* ---- multi-stage matching (stock libviso2's multi_stage = 1) [upstream-recollection; DESIGN.md section 6 (f-3) is the
 * specification; the reference tree keeps struct range / struct delta, src/matcher.h:163-178, and the stat_bin, stage
 * and use_prior arguments of findMatch and matching, src/matcher.cpp:216-218, 274-276, with nothing behind them] ----
 * With the switch on, every push also detects the sparse set of each image (src/matcher.cpp:621-628) and every
 * vh_match_features / vh_group_match_features runs two passes: (1) the method's matching on the sparse sets, unranged,
 * followed by removeOutliers (flow and quad lists); (2) the statistics of the surviving sparse matches give every
 * statistics bin a search range per stage of the circle (vh_prior_statistics), and the dense sets are matched inside
 * the range of the DRIVING feature's bin (vh_match_ranged; csrc/kernels_ranged.hip).  The dense list of pass 2 is the
 * handle's match list: refinement, every getter and download, vh_remove_outliers, the post chains and the estimators
 * see it.  Off (the default), nothing is allocated or launched and p.multi_stage keeps its only other meaning
 * (vh_compute_features hands out the sparse set).
 * Before the first push only (VH_ERR_STATE afterwards); on = 1 needs p.multi_stage = 1 (VH_ERR_INVALID_ARG);
 * a sequence handle (vh_sequence_create) has its own entry, vh_sequence_set_multi_stage, and answers these two with
 * VH_ERR_UNSUPPORTED.  The motion prior combines with the mode through vh_(group_)set_multi_stage_prior only: without
 * it vh_match_features / vh_group_match_features_prior with Tr_delta16 != NULL return VH_ERR_UNSUPPORTED.
 * The vote between the passes runs on the host: a match call waits for pass 1 (DESIGN.md section 6 has the cost),
 * unless vh_set_multi_stage_device moves it to the device. */
int32_t vh_set_multi_stage_matching(vh_matcher *m, int32_t on);
int32_t vh_group_set_multi_stage_matching(vh_group *g, int32_t on);
/* Both steps between the passes on the device: the vote (csrc/kernels_vote.hip, as vh_remove_outliers_device with
 * max_features = 0) and the statistics (csrc/kernels_stats.hip, as vh_prior_statistics_device) are queued behind pass 1,
 * pass 2 behind them.  A match call then only queues work, like every other match call of the library: no wait, no
 * transfer of lists, no host threads.  Lists and ranges equal the host form's (off, the default: that form, unchanged).
 * Before the first push only (VH_ERR_STATE afterwards); on = 1 needs multi-stage matching switched on already
 * (VH_ERR_STATE); a sequence handle: VH_ERR_UNSUPPORTED (vh_sequence_set_multi_stage, mode 2).  Switching multi-stage
 * matching off clears it.
 * A sparse list the device vote refuses (truncated, above 65 535 records, more pending flips than its stack holds) gets
 * +-match_radius in every bin, for which pass 2 is single-stage matching: the match call returns VH_OK, and
 * vh_(group_)get_sparse_matches returns the refusal's code for that stream (VH_ERR_CAPACITY / VH_ERR_UNSUPPORTED) with
 * *n = 0.  The first match call allocates the vote buffer (176 bytes per record slot of the sparse lists; counted by
 * vh_group_device_bytes); when that fails the call returns VH_ERR_HIP and the handle keeps working. */
int32_t vh_set_multi_stage_device(vh_matcher *m, int32_t on);
int32_t vh_group_set_multi_stage_device(vh_group *g, int32_t on);
/* The sparse list of pass 1 after the vote, of the last match step (*n = 0 before it); VH_ERR_STATE with the switch off.
 * In device mode the list comes from the vote buffer, and the call waits for the vote. */
int32_t vh_get_sparse_matches(vh_matcher *m, vh_p_match *out, int32_t cap, int32_t *n);
int32_t vh_group_get_sparse_matches(vh_group *g, int32_t stream, vh_p_match *out, int32_t cap, int32_t *n);
/* Multi-stage matching on a sequence handle (vh_sequence_create).  mode 0: off; 1: the vote and the statistics between
 * the passes on the host (as vh_group_set_multi_stage_matching); 2: both on the device (as vh_group_set_multi_stage_device
 * on top of it).  Row r of a chunk pushed at position F holds the pair F + r - 1 -> F + r, and its list is the list of a
 * lone matcher with vh_set_multi_stage_matching on that was pushed frame F + r - 1, then frame F + r, byte for byte, for
 * every method.  The sparse sets live in a sequence handle of their own that takes the same chunks: row 0 links to the
 * last row of the previous chunk in the sparse pass as in the dense one (a chunk that was pushed and never matched
 * included), and a frame's sparse set is detected once.  Rows that hold no pair (row 0 of the first chunk, rows >=
 * n_frames) have an empty sparse list, ranges of +-match_radius and an empty list.  Every reader of the lists sees the
 * list of pass 2, as on a group; vh_group_get_sparse_matches(g, row, ...) returns the voted pass-1 list of the row (mode
 * 2: the refusal's code with *n = 0 for a list the device vote refused, whose row was matched over the full window).
 * vh_group_device_bytes counts the sparse handle's arrays and, in mode 2, the vote buffer of max_frames lists.
 * Before the first push only (VH_ERR_STATE afterwards); mode outside 0..2: VH_ERR_INVALID_ARG; mode > 0 needs
 * p.multi_stage = 1 (VH_ERR_INVALID_ARG); a group or a lone matcher: VH_ERR_UNSUPPORTED (they keep their own entries). */
int32_t vh_sequence_set_multi_stage(vh_group *g, int32_t mode);
/* The motion prior together with multi-stage matching [upstream-recollection: stock matchFeatures hands Tr_delta to both
 * passes].  On, vh_match_features(m, 2, Tr), vh_group_match_features_prior and its sequence form (one Tr per row) are
 * honoured for the quad method: pass 1 is the prior's quad matching on the sparse sets, and pass 2 adds the term to the
 * second hop of the circle (previous right -> current right) -- the accept window stays query + range[bin of the
 * driver][stage 1], the cost becomes SAD + 4 * sqrt(du * du + dv * dv) in double around the prediction of the DRIVING
 * feature (csrc/vh_prior.h), added only when both of its coordinates are >= 0, first strict minimum below 10000000 in the
 * reference's visiting order, min_ind = 0 when nothing is accepted (src/matcher.cpp:221-264).  Flow and stereo ignore the
 * estimate, as single-stage matching does.  VH_ERR_STATE from the match call without intrinsics (f, base > 0).
 * Off (the default): such a call returns VH_ERR_UNSUPPORTED, as before.  Lone matchers, groups and sequence handles;
 * before the first push only and after multi-stage matching was switched on (VH_ERR_STATE otherwise); switching
 * multi-stage matching off clears it. */
int32_t vh_set_multi_stage_prior(vh_matcher *m, int32_t on);
int32_t vh_group_set_multi_stage_prior(vh_group *g, int32_t on);
/* computePriorStatistics on caller-owned records (host function, needs no device): ranges[nb][4][4] float, nb = ubn * vbn
 * statistics bins of matching's grid for dims (src/matcher.cpp:282-283), bin = v_bin * ubn + u_bin, then stage 0..3, then
 * u_min, u_max, v_min, v_max relative to the query of the stage.  Each match contributes its displacement per stage
 * (flow: 1c->1p, 1p->1c; stereo: 1c->2c, 2c->1c, v = 0; quad: 1p->2p, 2p->2c, 2c->1c, 1c->1p, v = 0 in the stereo
 * stages) to the 3 x 3 bins, clamped to the grid, around the bin of its reference point ((u1c, v1c); quad: (u1p, v1p)).
 * A bin without observations gets +-match_radius; otherwise min / max of the observations, an axis narrower than 20 is
 * widened by ceil((20 - d) / 2) on both sides.  Stages the method does not have (2, 3 of flow and stereo) read
 * +-match_radius.  Coordinates must be finite (VH_ERR_INVALID_ARG). */
int32_t vh_prior_statistics(const vh_params *p, const int32_t dims[3], int32_t method, const vh_p_match *pm, int32_t n,
                            float *ranges);
/* The same for n_lists lists in one launch on the device (csrc/kernels_stats.hip; host pointers): list l is
 * pm[l * stride .. + counts[l]), its table ranges[l][nb][4][4].  Every value equals vh_prior_statistics' (a zero may
 * carry the other sign).  counts[l] = 0 gives the +-match_radius table.  VH_ERR_INVALID_ARG for n_lists < 1, null
 * pointers, a bad method, counts[l] outside [0, stride], or a list that holds a non-finite value (ranges is then
 * left unwritten); VH_ERR_UNSUPPORTED for a grid of more than 2^27 - 1 bins. */
int32_t vh_prior_statistics_device(const vh_params *p, int32_t device, const int32_t dims[3], int32_t method, int32_t n_lists,
                                   const vh_p_match *pm, int64_t stride, const int32_t *counts, float *ranges);
/* vh_match with use_prior = true: every stage of a circle searches query + ranges[stat_bin][stage], stat_bin the bin of
 * the circle's driving feature (1c; quad: 1p; src/matcher.cpp:314-317); 1-d stages (stereo, quad stages 0 and 2) take
 * v = query +- match_disp_tolerance whatever the range says.  Everything else is vh_match: unrefined.  Range values must
 * be finite (VH_ERR_INVALID_ARG); they are used as the integer window ceil(min) .. floor(max), clamped to +-2^20. */
int32_t vh_match_ranged(const vh_params *p, int32_t device, const int32_t dims[3], int32_t method,
                        const int32_t *m1p, int32_t n1p, const int32_t *m2p, int32_t n2p,
                        const int32_t *m1c, int32_t n1c, const int32_t *m2c, int32_t n2c,
                        const float *ranges, vh_p_match *out, int32_t cap, int32_t *n);

/* Stock libviso2's match refinement [upstream-recollection; absent from the reference tree, built on its
 * computeSmallDescriptor, src/matcher.cpp:516-543, and Matrix::solve, src/matrix.cpp:417-504; DESIGN.md section 6
 * (f-3) is the specification] on caller-owned records, in place, order preserved; *n_out = records kept.
 * p->refinement <= 0: nothing changes (*n_out = n, nothing is launched); 2: sub-pixel (a 7x7 window of 16-byte SADs,
 * a quadratic fit around the minimum; matches whose fit fails are dropped); any other positive value: pixel (the
 * minimum of a 5x5 window).  Each record is refined hop by hop from the anchor (u1c, v1c) on image I1c, which never
 * moves: flow 1c -> 1p, stereo 1c -> 2c, quad 1c -> 1p, 1c -> 2c, 1c -> 2p; indices are kept.  The images are host
 * images at full resolution (dims = W, H, bytes per line, as pushed; also with half_resolution, whose coordinates are
 * full-resolution already); NULL where the method does not read one (flow: I1p, I1c; stereo: I1c, I2c; quad: all
 * four).  Hops outside the bounds (anchor 4 <= u <= W-5, 4 <= v <= H-5; target the same, narrowed by the window
 * radius) are left as they are in pixel mode and dropped in sub-pixel mode.
 * The stateful calls refine with the handle's p.refinement after every match step, before anything reads the list:
 * vh_get_matches, every vh_group_* getter and download, vh_remove_outliers, the post chains (host and device) and
 * vh_group_estimate_motion(_mono) all see the refined list and its count. */
int32_t vh_refine_matches(const vh_params *p, int32_t device, int32_t method, const int32_t dims[3], const uint8_t *I1p,
                          const uint8_t *I2p, const uint8_t *I1c, const uint8_t *I2c, vh_p_match *pm, int32_t n,
                          int32_t *n_out);

/* ---- S independent camera streams stepped together ---------------------- */
/* The multi-stream configuration (one sequence per stream, no exchange
 * between streams): every kernel launch covers all S streams, which is what
 * fills an MI355X at KITTI image size.  Stream s of a group behaves exactly
 * like its own vh_matcher. */
int32_t vh_group_create(const vh_params *p, int32_t device, int32_t n_streams,
                        int32_t max_features, int32_t max_matches, vh_group **out);
void vh_group_destroy(vh_group *g);
int32_t vh_group_streams(const vh_group *g);
/* Device memory the group currently holds (allocated at the first push_back for
 * the image size and capacities in use): for sizing S against the HBM of a GPU. */
int64_t vh_group_device_bytes(const vh_group *g);
/* Device-resident images: stream s reads dI1 + s*stride_bytes (and dI2 + ...;
 * dI2 may be NULL).  Asynchronous: returns once the work is queued; the images
 * must stay valid until the detection has run (vh_group_synchronize, or the
 * next vh_group_get_*). */
int32_t vh_group_push_back_device(vh_group *g, const void *dI1, const void *dI2,
                                  int64_t stride_bytes, const int32_t dims[3],
                                  int32_t replace);
/* Host images, same addressing. */
int32_t vh_group_push_back(vh_group *g, const uint8_t *I1, const uint8_t *I2,
                           int64_t stride_bytes, const int32_t dims[3], int32_t replace);
int32_t vh_group_match_features(vh_group *g, int32_t method);
/* ... with a motion prior per stream, Tr_delta16[S][16] (see vh_match_features); NULL: none */
int32_t vh_group_match_features_prior(vh_group *g, int32_t method, const double *Tr_delta16);
/* vh_remove_outliers for every stream of the group, `host_threads` workers
 * (<= 0: one per hardware thread).  Host-bound: a few ms per stream. */
int32_t vh_group_remove_outliers(vh_group *g, int32_t host_threads);
int32_t vh_group_get_matches(vh_group *g, int32_t stream, vh_p_match *out, int32_t cap,
                             int32_t *n);
/* Every stream's matches with one wait: stream s's records go to
 * out[s * cap_per_stream ...], its true count to counts[s] (VH_ERR_CAPACITY if
 * any count exceeds cap_per_stream; the records that fit are still written).
 * `out` in page-locked memory (vh_host_alloc) makes the transfers run at PCIe rate. */
int32_t vh_group_get_matches_all(vh_group *g, vh_p_match *out, int32_t cap_per_stream, int32_t *counts);
/* The same without waiting: starts one strided device->host transfer of the first
 * cap_per_stream records of every stream (whatever their counts; records beyond
 * counts[s] are stale) plus the S counts, ordered after the last
 * vh_group_match_features, and returns.  The next step can be issued at once; its
 * emission waits for this download on the device.  `out` and `counts` must be
 * page-locked (vh_host_alloc) and stay untouched until vh_group_wait_download
 * (or vh_group_synchronize) returns.  Host-side post-processing
 * (vh_group_remove_outliers) is not reflected: these are the device lists. */
int32_t vh_group_download_matches_async(vh_group *g, vh_p_match *out, int32_t cap_per_stream, int32_t *counts);
int32_t vh_group_wait_download(vh_group *g);
int32_t vh_group_get_features(vh_group *g, int32_t stream, int32_t which, int32_t *out12,
                              int32_t cap, int32_t *n);
/* Per-stream counts of the last step without copying records:
 * n_features[4*S] (1p,2p,1c,2c per stream), n_matches[S]. Either may be NULL. */
int32_t vh_group_get_counts(vh_group *g, int32_t *n_features, int32_t *n_matches);
int32_t vh_group_synchronize(vh_group *g);
int32_t vh_group_set_stream(vh_group *g, void *hip_stream);
int32_t vh_group_clear_stream(vh_group *g);
int32_t vh_group_stream_wait_images(vh_group *g, void *hip_stream);

/* ---- consecutive frames of ONE camera in one launch ---------------------- */
/* A sequence handle is a vh_group whose rows ("streams") hold consecutive frames of one camera (stereo or mono), so
 * that one sequence -- an offline replay, one sequence per GPU -- fills the GPU as a group of max_frames cameras does.
 * Each push brings a chunk of n frames (1 <= n <= max_frames); with F frames pushed before it in the current sequence:
 *   - row r < n holds the pair frame F+r-1 -> frame F+r: after vh_group_match_features(_prior) its match list is exactly
 *     what a lone vh_matcher returns after pushing those two frames and matching with the same method, and its four
 *     feature sets (vh_group_get_features: 1p/2p = frame F+r-1, 1c/2c = frame F+r) are that matcher's;
 *   - row 0 links to the last frame of the previous chunk, so chunk boundaries lose no pair;
 *   - on the first chunk of a sequence (F = 0) row 0 has no predecessor: it is an empty row -- 0 matches and 0 features
 *     in every role -- and matching returns VH_OK;
 *   - rows r >= n of a short chunk are empty rows too;
 *   - a chunk whose dims differ from the previous chunk's starts a new sequence (F = 0), as vh_push_back does.
 * Every frame is detected once.  The ring rotates one slot per chunk: detection of chunk k+1 overlaps matching of
 * chunk k exactly as for a group.  Every vh_group_* call below works on a sequence handle with "stream s" read as
 * "row s": vh_group_match_features, vh_group_match_features_prior (Tr_delta16[n][16], one motion per row of the last
 * chunk), vh_group_get_matches(_all), vh_group_download_matches_async, vh_group_get_features, vh_group_get_counts,
 * vh_group_streams (= max_frames), the post chains (vh_group_post_begin/_finish(_mono), vh_group_post_begin_device /
 * vh_group_post_finish_device: empty rows come out as ok = 0 with no error) and vh_group_estimate_motion(_mono).
 * vh_group_push_back(_device) on a sequence handle, and vh_sequence_push_back(_device) on a plain group, return
 * VH_ERR_STATE; n_frames outside [1, max_frames] returns VH_ERR_INVALID_ARG.  Destroy with vh_group_destroy. */
int32_t vh_sequence_create(const vh_params *p, int32_t device, int32_t max_frames, int32_t max_features,
                           int32_t max_matches, vh_group **out);
/* Frame F+r of the chunk at dI1 + r*stride_bytes (and dI2 + ..., NULL for mono), device memory, asynchronous as
 * vh_group_push_back_device. */
int32_t vh_sequence_push_back_device(vh_group *g, const void *dI1, const void *dI2, int64_t stride_bytes,
                                     const int32_t dims[3], int32_t n_frames);
/* Host images, same addressing (only the n_frames images are read). */
int32_t vh_sequence_push_back(vh_group *g, const uint8_t *I1, const uint8_t *I2, int64_t stride_bytes,
                              const int32_t dims[3], int32_t n_frames);
/* *first_frame = F, the index within the sequence of row 0's current frame, and *n_frames = n, the rows valid in the
 * last push (both 0 before the first push); both pointers are required. */
int32_t vh_sequence_position(const vh_group *g, int64_t *first_frame, int32_t *n_frames);

/* ---- feature tracks: the match lists of consecutive frame pairs linked on the GPU -------------------------------------
 * Every p_match carries the feature indices i1p / i1c "for tracking" (src/matcher.h:92-98): a record of pair (Z -> A)
 * with i1c = k and a record of pair (A -> B) with i1p = k are the same left-image feature of frame A.  With the switch on,
 * every match call also links its lists to their predecessors (csrc/kernels_track.hip) and keeps
 * one vh_track per match record, same order and count as the list.
 *   Tracked list: the match list of a handle row as the getters return it right after the match call (after refinement
 *   if set; host-side post-processing -- vh_remove_outliers, vh_bucket_features -- is not reflected: the tracks describe
 *   the device list) for a pair of pushed frames (A -> B).  Every push gives its frame a serial number: 0 for the first
 *   frame of a sequence, + 1 per push; a replace push keeps the serial of the frame it replaces; a change of dims starts
 *   a new sequence at 0.  On a sequence handle the serial is the frame's index (vh_sequence_position).
 *   Predecessor of the list of (A -> B): the most recent tracked list of the same camera for a pair (Z -> A) with the
 *   same frame A -- sequence handle: row r - 1 of the same match call, for row 0 the last row of the last match call
 *   on the previous chunk; group / lone matcher: the same stream's list of the previous step.  None if no match call
 *   was made for (Z -> A), if dims changed in between, or if A was replaced after (Z -> A) was matched.  Matching the same
 *   pair again replaces its tracked list and keeps the predecessor.  Empty rows of a sequence handle hold empty lists.
 *   Link: record j continues record q of the predecessor iff i1p(j) >= 0 and i1c(q) == i1p(j); of several q the lowest;
 *   a predecessor record is continued by the lowest such j only.  Every other record starts a new track (age 1), as do
 *   records whose index lies outside the table (the feature capacity; n_index of vh_link_tracks). */
typedef struct vh_track {
  int64_t birth_frame; /* serial of frame B of the pair whose list holds the track's first record */
  int32_t birth_pos;   /* that record's position in its list: (birth_frame, birth_pos) names the track */
  int32_t age;         /* records in the track up to and including this one, >= 1 */
  int32_t prev;        /* position of the continued record in the predecessor list, -1 if none */
  int32_t reserved;    /* 0 */
} vh_track;
/* Before the first push only (VH_ERR_STATE afterwards).  Works on sequence handles and together with refinement, the
 * motion prior and multi-stage matching.  Off (the default): nothing is allocated or launched.  On: two tables of
 * 4 * max_features bytes and 24 * max_matches bytes of records per list kept -- S rows and one carry list for a sequence
 * handle, two lists per stream for a group -- allocated by the first match call and counted by vh_group_device_bytes.
 * A table entry keeps a list position in 24 bits: with max_matches above 16 777 215 the match calls return
 * VH_ERR_UNSUPPORTED while the switch is on. */
int32_t vh_set_track_linking(vh_matcher *m, int32_t on);
int32_t vh_group_set_track_linking(vh_group *g, int32_t on);
/* The tracks of the last match call's list(s): capacity and error rules of vh_get_matches / vh_group_get_matches(_all);
 * VH_ERR_STATE with the switch off or before a match call. */
int32_t vh_get_tracks(vh_matcher *m, vh_track *out, int32_t cap, int32_t *n);
int32_t vh_group_get_tracks(vh_group *g, int32_t stream, vh_track *out, int32_t cap, int32_t *n);
int32_t vh_group_get_tracks_all(vh_group *g, vh_track *out, int32_t cap_per_stream, int32_t *counts);
/* The device array those getters copy from: stream s's records at *d_tracks + s * *stride (in records), complete once
 * the work queued by the match call has run (vh_group_synchronize), valid until the next match call. */
int32_t vh_group_tracks_device(vh_group *g, const vh_track **d_tracks, int64_t *stride);
/* The same linking for caller-owned lists (host pointers, as vh_remove_outliers_device): list l = pm[l * stride ..
 * + counts[l]), its predecessor is list l - 1, list 0's the last list of the call that produced carry_in (NULL: none).
 * This is how lists the handle never sees again -- voted, bucketed -- are linked.  out[l * stride ..] receives list l's
 * tracks.  n_index >= 1 bounds the feature indices (the table size); birth frames count on from the carry (from 0
 * without one).  *carry_out (nullable pointer) receives a new carry, to be released with vh_track_carry_free; carry_in
 * is not consumed.  Lists of more than 16 777 215 records: VH_ERR_UNSUPPORTED.
 * A convenience entry, not a throughput path: every call allocates and clears two tables of (n_lists + 1) * n_index
 * words and moves every list with a transfer of its own, so its cost grows with n_lists * n_index. */
typedef struct vh_track_carry vh_track_carry;
int32_t vh_link_tracks(int32_t device, int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t n_index,
                       const vh_track_carry *carry_in, vh_track_carry **carry_out, vh_track *out);
void vh_track_carry_free(vh_track_carry *c);

/* ---- stereo egomotion ------------------------------------- */

/* VisualOdometryStereo::parameters and the calibration it reads
 * (src/viso_stereo.h:31-43, src/viso.h:41-50). */
typedef struct vh_ego_params {
  int32_t ransac_iters;     /* number of RANSAC iterations (200) */
  int32_t reweighting;      /* 1 = lower border weights (src/viso_stereo.cpp:280-282) */
  double inlier_threshold;  /* reprojection error bound in pixels (2.0) */
  double f, cu, cv, base;   /* focal length, principal point (pixels), baseline (meters) */
} vh_ego_params;
/* VisualOdometryStereo::parameters() defaults; f = 1, cu = cv = 0, base = 1 as VisualOdometry::calibration(). */
void vh_default_ego_params(vh_ego_params *e);

/* VisualOdometryStereo::estimateMotion (src/viso_stereo.cpp:54-157) for n_sets independent
 * match lists in one launch (one workgroup per list; RANSAC hypotheses in parallel, double
 * precision): pm = the lists back to back, list s = pm[offsets[s] .. offsets[s+1]).
 * rand3[n_sets][ransac_iters][3] = the values rand() returns while
 * VisualOdometry::getRandomSample(N,3) draws each hypothesis' sample (src/viso.cpp:86-106;
 * the reference seeds srand(0) in its constructor, src/viso.cpp:35) -- the caller owns the
 * random stream, so the result is a function of the inputs.
 * Outputs per list: tr[6] = (rx,ry,rz,tx,ty,tz) and ok = 1, or ok = 0 (and tr = 0) where the
 * reference returns an empty vector (fewer than 6 matches / inliers, refinement not
 * converged); n_inliers and, if inliers != NULL, the ascending inlier indices of the best
 * hypothesis at inliers[offsets[s] ..] (VisualOdometry::getInlierIndices).
 * Each hypothesis follows the reference's operation order exactly; the refinement sums the
 * normal equations in parallel, so tr agrees with the reference to rounding (1e-9 relative
 * is what tests/ assert), the inlier sets exactly.
 * The two stateless estimators (this and vh_estimate_motion_mono) keep one device work buffer per
 * device between calls (grow-only, requests above 1 GiB are not kept, released with the process)
 * and run one at a time per process. */
int32_t vh_estimate_motion_stereo(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm,
                                  const int32_t *offsets, const int32_t *rand3, double *tr, int32_t *ok,
                                  int32_t *n_inliers, int32_t *inliers);
/* The same on the device-resident match lists of the group's last vh_group_match_features
 * (flow matches carry no disparity: VH_METHOD_QUAD only, VH_ERR_STATE otherwise): nothing
 * but rand3 [S][ransac_iters][3] goes up and S x (tr, ok, n_inliers) comes back. */
int32_t vh_group_estimate_motion(vh_group *g, const vh_ego_params *e, const int32_t *rand3, double *tr, int32_t *ok,
                                 int32_t *n_inliers);

/* ---- motion inliers: which records of whole lists agree with a motion ------------------------------- */
/* VisualOdometryStereo::getInlier (src/viso_stereo.cpp:159-177) for any quad list and any tr[6] = (rx,ry,rz,tx,ty,tz):
 * the 3-d point of the previous pair with float df = max(u1p - u2p, 0.0001f) (:83-86), the rotation (:244-250), the
 * four predicted coordinates (:274-276, :317-321) and the test  sum of the four squared differences to
 * (u1c, v1c, u2c, v2c) < inlier_threshold^2  -- strict, in double, added left to right, unweighted (`reweighting` and
 * `ransac_iters` are not read).  A sum that is NaN or infinite (NaN coordinates, Z1c = 0) is "not an inlier", never
 * an error; a list with ok = 0 has no inliers and its tr is not read; a list of one record is classified like any
 * other (the N < 6 return belongs to estimateMotion).  The estimators' n_inliers / inliers refer to the (bucketed)
 * lists they ran on; this classifies the dense lists under the motion they found.
 * Only sin / cos come from the device library: with a non-zero rotation a record whose sum lies within rounding of
 * the threshold may be classified differently from a host restatement using libm.
 *
 * Stateless: n_sets lists laid out as for vh_estimate_motion_stereo, tr[n_sets][6], ok[n_sets].  flags (one byte
 * per record, 1 = inlier, indexed like pm, i.e. sized offsets[n_sets]) and n_inliers[n_sets] are written; if not
 * NULL, inlier_pm and src_pos (both indexed like pm) receive at [offsets[s], offsets[s] + n_inliers[s]) the inlier
 * records of list s in list order and the position of each in list s -- the rest of each slice is not written.
 * n_sets == 0 or no records at all: VH_OK, nothing is launched and no device is needed.  VH_ERR_UNSUPPORTED for a
 * list of more than 2^24 - 1 records or n_sets * ceil(longest / 1024) >= 2^24. */
int32_t vh_motion_inliers(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                          const double *tr, const int32_t *ok, uint8_t *flags, int32_t *n_inliers, vh_p_match *inlier_pm,
                          int32_t *src_pos);
/* The same on the device-resident lists of the handle's last match call -- exactly the lists vh_group_get_matches
 * returns (refined where refinement is on, pass 2 under multi-stage matching): tr[S][6], ok[S] go up, counts[S]
 * (inliers per stream) comes back; synchronous.  Quad lists only (VH_ERR_STATE otherwise, and before any match, as
 * vh_group_estimate_motion).  Once vh_remove_outliers / vh_group_remove_outliers / vh_bucket_features replaced a list
 * on the host, the replaced list -- what the getters return -- is the one classified, from a device copy made by the
 * call (a second block of 48 bytes per record slot and 4 per stream, allocated when that first happens).  Legal from the return of a match call until the next push or match; a further call with another tr replaces
 * the result.  Plain groups, sequence handles (rows without a pair: count 0, their tr is not read) and lone matchers.
 * VH_ERR_CAPACITY when a list or a feature set was truncated (the classification of the truncated list is kept).
 * The first call allocates 1 + 48 + 4 bytes per record slot (S x max_matches slots), 4 bytes per tile of 1024 slots
 * and 56 bytes per stream, counted by vh_group_device_bytes; a handle that never calls this allocates and launches
 * nothing for it.  A failed allocation is VH_ERR_HIP before anything is launched, and the call may be repeated.
 * Profile scopes: "inlier_flag", "inlier_compact". */
int32_t vh_group_motion_inliers(vh_group *g, const vh_ego_params *e, const double *tr, const int32_t *ok, int32_t *counts);
int32_t vh_match_inliers(vh_matcher *m, const vh_ego_params *e, const double *tr, int32_t ok, int32_t *count);
/* The results of that call, valid until the next match call (VH_ERR_STATE before a classification of the current
 * lists), under the getters' capacity rule: *n is the full number, at most cap elements are written, VH_ERR_CAPACITY
 * when there are more.  Flags: one byte per record of the list.  Inlier matches: the inlier records in list order,
 * and (src_pos_out, nullable) the position of each in the list, so pm_out[k] == list[src_pos_out[k]].  The _all form
 * writes stream s at [s * cap_per_stream ..] and counts[S]. */
int32_t vh_group_get_inlier_flags(vh_group *g, int32_t stream, uint8_t *out, int32_t cap, int32_t *n);
int32_t vh_group_get_inlier_matches(vh_group *g, int32_t stream, vh_p_match *pm_out, int32_t *src_pos_out, int32_t cap, int32_t *n);
int32_t vh_group_get_inlier_matches_all(vh_group *g, vh_p_match *pm_out, int32_t *src_pos_out, int32_t cap_per_stream, int32_t *counts);
int32_t vh_get_inlier_matches(vh_matcher *m, vh_p_match *pm_out, int32_t *src_pos_out, int32_t cap, int32_t *n);
/* The device arrays themselves, stream s at [s * *stride ..] (elements), valid until the next match call; the
 * compacted lists are ordinary lists: vh_reconstruct_lists and vh_link_tracks take them once downloaded. */
int32_t vh_group_inliers_device(vh_group *g, const uint8_t **d_flags, const vh_p_match **d_matches, const int32_t **d_src_pos,
                                int64_t *stride);

/* ---- the stereo motion refined on whole lists (csrc/kernels_refit.hip) ---------------------------------
 * The "final optimization" of VisualOdometryStereo::estimateMotion (reference src/viso_stereo.cpp:126-139) on any quad
 * list, EVERY record of it active (pass an inlier list), from a start tr_in[6]: updateParameters(.., 1, 1e-8) until it
 * reports CONVERGED, at most 102 times.  Double precision; `reweighting` is read, inlier_threshold and ransac_iters
 * are not.  Per list:
 *   ok_in == 0 or fewer than 6 records: ok_out = 0, tr_out = 0, n_updates = 0 (tr_in is not read);
 *   CONVERGED: ok_out = 1, tr_out = the refined motion; Matrix::solve refuses, or still not converged after 102
 *   updates: ok_out = 0, tr_out = 0.  n_updates = updateParameters calls made (1 .. 102).
 * The normal equations are summed in parallel in an order that depends on the list's length alone: tr_out agrees with
 * a sequential evaluation to rounding (not bit for bit), is the same from run to run, and does not depend on the other
 * lists of the call.  Non-finite records are not an error: they propagate as they do in the reference's arithmetic.
 *
 * Stateless: lists laid out as for vh_motion_inliers, tr_in[n_sets][6], ok_in[n_sets] -> tr_out[n_sets][6],
 * ok_out[n_sets], n_updates[n_sets].  n_sets == 0 or no records at all: VH_OK (outputs zero), nothing is launched and
 * no device is needed.  Length limits as vh_motion_inliers. */
int32_t vh_refit_motion(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                        const double *tr_in, const int32_t *ok_in, double *tr_out, int32_t *ok_out, int32_t *n_updates);
/* The same on the compacted inlier lists of the handle's current STEREO classification (vh_group_motion_inliers /
 * vh_match_inliers), from the tr / ok that classification was made under -- both are on the device already: nothing
 * goes up, tr_out[S][6], ok_out[S], n_updates[S] and counts[S] come back; the call is synchronous.  VH_ERR_STATE
 * before any classification of the current lists, after the next push or match, and when the current result is a
 * mono classification.  Rows without a pair have ok_out = 0.
 *   reclassify == 0: the classification is untouched, counts are its counts.
 *   reclassify != 0: the lists are classified again under tr_out / ok_out with e->inlier_threshold, queued behind the
 *   refit on the same stream (the host does not wait in between); the getters and vh_group_inliers_device then return
 *   the refined motion's inliers and counts are theirs (VH_ERR_CAPACITY as vh_group_motion_inliers).  Should that
 *   classification fail with another error, tr_out / ok_out / n_updates are still delivered and the handle is left
 *   without a classification (VH_ERR_STATE from the getters) until vh_group_motion_inliers is called again.
 * Plain groups, sequence handles and lone matchers.  The first call adds one block of 56 bytes per stream (each of
 * its three arrays rounded up to 256 bytes), counted by vh_group_device_bytes; a handle that never calls it allocates
 * and launches nothing.  A refused allocation is VH_ERR_HIP before any launch and leaves the handle as it was; the
 * call may be repeated.  Profile scope: "motion_refit". */
int32_t vh_group_refit_motion(vh_group *g, const vh_ego_params *e, int32_t reclassify, double *tr_out, int32_t *ok_out,
                              int32_t *n_updates, int32_t *counts);
int32_t vh_match_refit_motion(vh_matcher *m, const vh_ego_params *e, int32_t reclassify, double *tr_out, int32_t *ok_out,
                              int32_t *n_updates, int32_t *count);

/* ---- the covariance of a stereo motion over whole lists (csrc/kernels_cov.hip) --------------------------
 * How well a quad list of N records determines the motion tr[6] = (rx,ry,rz,tx,ty,tz): the 6x6 covariance of the least
 * squares estimate, in the order of tr.  The reference and stock libviso2 have no counterpart; every term is theirs:
 *   J (4N x 6), r (4N): the rows computeResidualsAndJacobian (src/viso_stereo.cpp:274-330) forms per record AT tr, every
 *     record active, in the order u1c, v1c, u2c, v2c, both weighted by 1 / (|u1c - cu| / |cu| + 0.05) under `reweighting`;
 *   A = J^T J;  ssr = sum r^2 (the 4N weighted squared residuals);  dof = 4N - 6;  sigma2 = ssr / dof;
 *   cov = sigma2 * A^-1, A^-1 by Matrix::solve (src/matrix.cpp:417-504) on the six unit right-hand sides; the upper
 *     triangle m <= n is computed and mirrored: cov is exactly symmetric, row-major.
 * One pass at a fixed tr, no update: pass the motion the list was fitted to (vh_refit_motion's tr_out on its own list).
 * Double precision; f, cu, cv, base, reweighting are read, inlier_threshold and ransac_iters are not.  Per list, never
 * an error of the call:
 *   ok_out = 0, cov = 0, ssr = 0 where ok == 0 (tr is then not read), where N < 6, where Matrix::solve refuses
 *   (a pivot below 1e-20), and where ssr or an entry of cov is not finite (non-finite records propagate and end here);
 *   ok_out = 1 otherwise.
 * The sums run in parallel in an order that depends on N alone: cov agrees with a sequential evaluation to rounding, is
 * the same from run to run, does not depend on the other lists of the call, and is the same bytes from the stateless
 * and the handle forms on the same records and tr.
 *
 * Stateless: lists laid out as for vh_refit_motion, tr[n_sets][6], ok[n_sets] -> cov[n_sets][36], ssr[n_sets],
 * ok_out[n_sets].  n_sets == 0 or no records at all: VH_OK (outputs zero), nothing is launched and no device is needed.
 * Length limits as vh_motion_inliers. */
int32_t vh_motion_covariance(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                             const double *tr, const int32_t *ok, double *cov, double *ssr, int32_t *ok_out);
/* The same on the compacted inlier lists of the handle's current STEREO classification -> cov[S][36], ssr[S], ok_out[S]
 * and counts[S] (the lists' lengths); the call is synchronous.
 *   tr == NULL (then ok == NULL): under the tr / ok that classification was made under, which are on the device already
 *   -- after vh_group_refit_motion(reclassify = 1) the refined motion and its inliers.  Nothing is uploaded.
 *   tr != NULL (then ok != NULL; one without the other is VH_ERR_INVALID_ARG): tr[S][6], ok[S] go up, the caller's motion
 *   on the same lists -- after reclassify = 0, where the refit's tr_out belongs to the lists it was fitted on.
 * VH_ERR_STATE where vh_group_refit_motion returns it: before any classification of the current lists, after the next
 * push or match, and when the current result is a mono classification.  Rows without a pair have ok_out = 0.  Plain
 * groups, sequence handles and lone matchers.  The first call adds one block of 352 bytes per stream (288 + 8 + 4 and the
 * 48 + 4 a caller's tr / ok go up into; each of the five arrays rounded up to 256 bytes), counted by vh_group_device_bytes; a handle that never calls it allocates and launches
 * nothing.  A refused allocation is VH_ERR_HIP before any launch and leaves the handle as it was; the call may be
 * repeated.  Profile scope: "motion_cov". */
int32_t vh_group_motion_covariance(vh_group *g, const vh_ego_params *e, const double *tr, const int32_t *ok, double *cov, double *ssr,
                                   int32_t *ok_out, int32_t *counts);
int32_t vh_match_motion_covariance(vh_matcher *m, const vh_ego_params *e, const double *tr, const int32_t *ok, double *cov, double *ssr,
                                   int32_t *ok_out, int32_t *count);

/* ---- the camera gain over motion inliers (csrc/kernels_gain.hip) -----------------------------------------
 * Matcher::getGain (reference src/matcher.h:145-148, src/viso.h:104: "given a vector of inliers computes gain factor
 * between the current and the previous frame"; the reference keeps the body commented out and its helper
 * Matcher::mean, src/matcher.cpp:347-354, compiled -- the loop is stock libviso2's, parity unpinned; the helper is
 * pinned by tests/golden/gain_reference.npz).  For one list pm[0, n), index entries idx[0, k) and the previous / current
 * LEFT images at full resolution (dims = {W, H, bpl}; also under half_resolution: match coordinates are full-resolution):
 *   gain = 0; num = 0
 *   for every entry i = idx[j], in order:  skipped if i < 0 or i >= n, or if one of u1p, v1p, u1c, v1c is not finite or
 *       has a magnitude >= 2^24;
 *     (up, vp) = the truncated (u1p, v1p); u_min = min(max(up - 3, 0), W - 1), u_max = min(max(up + 3, 0), W - 1), v alike
 *     mean_prev = Matcher::mean(I_prev, window), mean_curr likewise around (u1c, v1c) in I_cur
 *     if (mean_prev > 10) { gain += mean_curr / mean_prev; num++; }
 *   gain = num > 0 ? gain / num : 1
 * Single precision throughout; the sum runs in the order of idx, and that order is part of the result: gain and num are
 * bit-identical to the sequential evaluation (the numpy restatement under tests/).  Two rules are tighter than stock, which reads
 * outside its arguments there: windows are clamped to W - 1 / H - 1 (stock: W / H, one column or row past the image; the
 * matcher's own coordinates lie 7 px inside, where the rules agree), and stock tests only i < n and no coordinate.
 *
 * Stateless (replaces src/matcher.h:148 for n_sets lists in one call): all pointers are host pointers; list s is
 * pm[offsets[s] .. offsets[s+1]) with the index entries idx[idx_offsets[s] .. idx_offsets[s+1]) and its own image pair at
 * I_prev / I_cur + s * image_stride_bytes -> gain[n_sets], num[n_sets] (1, 0 for a list without a counted entry).
 * n_sets == 0 or no index entries at all: VH_OK, nothing is launched and no device is needed.  VH_ERR_UNSUPPORTED: an
 * image beyond 16384 x 16384, a list of 2^24 or more records, or a launch grid beyond the device's. */
int32_t vh_gain(int32_t device, int32_t n_sets, const int32_t dims[3], const uint8_t *I_prev, const uint8_t *I_cur, int64_t image_stride_bytes,
                const vh_p_match *pm, const int32_t *offsets, const int32_t *idx, const int32_t *idx_offsets, float *gain, int32_t *num);
/* The images of a handle (the state behind src/matcher.h:148; the reference's Matcher keeps no images either): with
 * the switch on, every push also copies the pushed full-resolution left image of every row into a u8 plane of the ring
 * (pitch: W rounded up to 16; VH_RING x streams planes, allocated with the ring at the first push and counted by
 * vh_group_device_bytes; profile scope "gain_copy", on the detect stream, per sub-batch).  Before the first push only:
 * VH_ERR_STATE afterwards.  Plain groups, sequence handles and lone matchers.  Off (the default): nothing is allocated,
 * launched or changed. */
int32_t vh_group_set_gain(vh_group *g, int32_t on);
int32_t vh_set_gain(vh_matcher *m, int32_t on);
/* getGain (src/matcher.h:148) on the lists of the handle's last FLOW or QUAD match call -- exactly those
 * vh_group_get_matches returns -- over the inlier positions of its current classification (vh_group_motion_inliers,
 * _mono, or the reclassification of vh_group_refit_motion): lists and positions are on the device already, nothing is
 * uploaded -> gain[S], num[S]; the call waits once, for that download.  gain = 1, num = 0 for a stream classified with
 * ok = 0, an empty list, a sequence row without a pair and a list without a counted entry.  VH_ERR_STATE with the switch
 * off, before a classification of the current lists, after the next push or match, and on stereo lists (they hold no
 * previous frame).  The first call adds S * (max_matches + 2) floats, counted by vh_group_device_bytes; a refused
 * allocation is VH_ERR_HIP before any launch and leaves the handle as it was.  Profile scopes: "gain_ratio", "gain_sum". */
int32_t vh_group_gain(vh_group *g, float *gain, int32_t *num);
int32_t vh_match_gain(vh_matcher *m, float *gain, int32_t *num);
/* The same (src/matcher.h:148) over the caller's index lists, which are uploaded: stream s takes
 * idx[idx_offsets[s] .. idx_offsets[s+1]), positions into the list vh_group_get_matches returns for it (also where that
 * list was replaced on the host by vh_remove_outliers / vh_bucket_features: the lists then go up as well).  The form for
 * bucketed or voted index sets and the one Matcher::getGain of viso_hip_matcher.hpp uses.  VH_ERR_STATE with the switch
 * off, before a match call, after the next push, and on stereo lists. */
int32_t vh_group_gain_indices(vh_group *g, const int32_t *idx, const int32_t *idx_offsets, float *gain, int32_t *num);
int32_t vh_match_gain_indices(vh_matcher *m, const int32_t *idx, int32_t k, float *gain, int32_t *num);

/* ---- the steps after matching, pipelined ------------------------------------------------------------- */
/* What the reference's loop runs between Matcher::matching and the pose -- removeOutliers (the tail of
 * matchFeatures, src/matcher.cpp:108), bucketFeatures (src/viso_stereo.cpp:41-43 -> src/matcher.cpp:140-187)
 * and VisualOdometryStereo::estimateMotion (src/viso_stereo.cpp:49-51) -- for every stream of a group,
 * arranged so that the host part of step t runs beside the GPU work of step t+1:
 *   vh_group_post_begin   after vh_group_match_features: starts the download of the step's match lists (the
 *                         first cap_per_stream records of every stream) into one of two internal page-locked
 *                         slots and returns at once.
 *   vh_group_post_finish  age 0: the step begun last, 1: the one before.  Waits for that download, runs the
 *                         Delaunay vote (flow and quad lists) and the bucketing of every stream on host_threads
 *                         host threads (<= 0: one per hardware thread), copies the bucketed lists to
 *                         bucketed[s * cap_per_stream ..] / counts[s] (either may be NULL), and -- if e != NULL
 *                         (quad lists only) -- uploads them (a few hundred records per stream) and runs the
 *                         batched egomotion kernel: tr[S][6], ok[S], n_inliers[S] as vh_group_estimate_motion,
 *                         rand3[S][ransac_iters][3].  *host_ms (nullable) = wall time of the host part.
 * VH_ERR_CAPACITY when a list was longer than the slot or a feature set was truncated.  The lists
 * vh_group_get_matches returns are not changed by these calls. */
int32_t vh_group_post_begin(vh_group *g, int32_t cap_per_stream);
int32_t vh_group_post_finish(vh_group *g, int32_t age, int32_t max_features, float bucket_width, float bucket_height,
                             int32_t host_threads, const vh_ego_params *e, const int32_t *rand3, double *tr, int32_t *ok,
                             int32_t *n_inliers, vh_p_match *bucketed, int32_t cap_per_stream, int32_t *counts,
                             double *host_ms);

/* ---- monocular egomotion (mono half) ---------------------------- */

/* VisualOdometryMono::parameters and the calibration it reads (src/viso_mono.h:32-46, src/viso.h:41-50). */
typedef struct vh_mono_params {
  int32_t ransac_iters;     /* number of RANSAC iterations (2000) */
  int32_t reserved_;        /* 0 */
  double inlier_threshold;  /* fundamental-matrix (Sampson distance) inlier threshold (0.00001) */
  double motion_threshold;  /* median depth above which the motion counts as too small (100.0) */
  double height, pitch;     /* camera height above ground (m), pitch (rad, negative = pointing down) */
  double f, cu, cv;         /* focal length and principal point (pixels) */
} vh_mono_params;
/* VisualOdometryMono::parameters() defaults; f = 1, cu = cv = 0 as VisualOdometry::calibration(). */
void vh_default_mono_params(vh_mono_params *e);

/* VisualOdometryMono::estimateMotion (src/viso_mono.cpp:41-160) for n_sets independent lists of flow
 * matches (u1p,v1p -> u1c,v1c; the other fields are not read): 8-point RANSAC on normalised points,
 * F from all inliers of the best hypothesis, E, the four (R,t) candidates with the chirality vote,
 * scale from the ground plane.  Same layout as vh_estimate_motion_stereo; rand8[n_sets][ransac_iters][8]
 * = the values rand() returns while getRandomSample(N,8) draws each hypothesis' sample
 * (src/viso.cpp:86-106).  ok = 0 (tr = 0) where the reference returns an empty vector (fewer than
 * 10 matches / inliers / points in front of the cameras, median depth above motion_threshold) --
 * and where it would call exit(0) (no chirality solution, division by a vanishing plane distance).
 * Every hypothesis, the refit and the triangulation follow the reference's operation order exactly
 * (Matrix::svd restated, src/matrix.cpp:579-802), so the inlier sets are equal to the reference's;
 * the ground-plane vote uses the device's exp and the angles its asin/cos, so tr agrees to rounding
 * (tests assert 1e-9 relative). */
int32_t vh_estimate_motion_mono(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm,
                                const int32_t *offsets, const int32_t *rand8, double *tr, int32_t *ok,
                                int32_t *n_inliers, int32_t *inliers);
/* The same on the device-resident match lists of the group's last vh_group_match_features
 * (VH_METHOD_FLOW or VH_METHOD_QUAD: both carry the left camera's flow). */
int32_t vh_group_estimate_motion_mono(vh_group *g, const vh_mono_params *e, const int32_t *rand8, double *tr,
                                      int32_t *ok, int32_t *n_inliers);

/* The epipolar model the estimator arrived at, in its own normalised frame: what is needed to apply its inlier test
 * (getInlier, src/viso_mono.cpp:268-315) to any other list.  inlier_threshold only has a meaning in this frame, and
 * F cannot be rebuilt from tr.  16 doubles, 128 bytes. */
typedef struct vh_mono_model {
  double c[4];   /* cpu, cpv, ccu, ccv: the centroids normalizeFeaturePoints subtracts (src/viso_mono.cpp:190-200) */
  double s[2];   /* sp, sc: its two scales (:216-217) */
  double F[9];   /* the refit F of :80 in the normalised frame, after fundamentalMatrix's rank-2 step, row-major */
  double valid;  /* 1.0: the estimator reached the refit (>= 10 inliers of the best hypothesis); 0.0: everything above is 0 */
} vh_mono_model;
/* vh_estimate_motion_mono / vh_group_estimate_motion_mono with one more output, model[n_sets] / model[S]; tr, ok,
 * n_inliers and inliers are bit for bit those of the plain entries on the same inputs (the plain entries are these
 * with model = NULL inside; here NULL is VH_ERR_INVALID_ARG).  valid does not depend on ok: a list that fails after
 * the refit (too few points in front, median depth above motion_threshold, no chirality solution) has valid = 1 and
 * a meaningful F; valid = 0 and a zeroed record for fewer than 10 matches, a degenerate scale, or a best hypothesis
 * with fewer than 10 inliers.  The sign of F is the refit's (Matrix::svd's sign normalisation of the N x 9 system);
 * the Sampson test is the same for F and -F bit for bit.
 * The first vh_group_estimate_motion_mono_model call of a handle allocates one block of 128 bytes per stream for this
 * output, counted by vh_group_device_bytes (beside what vh_group_estimate_motion_mono allocates; the plain entry never
 * allocates it).
 * The pipelined post chains (vh_group_post_finish_mono, vh_group_post_begin_device / _finish_device) have no model
 * output: take the bucketed lists they return through vh_estimate_motion_mono_model -- or set a dense mode
 * (vh_group_post_device_dense) and take it from vh_group_post_finish_device_dense. */
int32_t vh_estimate_motion_mono_model(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm,
                                      const int32_t *offsets, const int32_t *rand8, double *tr, int32_t *ok,
                                      int32_t *n_inliers, int32_t *inliers, vh_mono_model *model);
int32_t vh_group_estimate_motion_mono_model(vh_group *g, const vh_mono_params *e, const int32_t *rand8, double *tr,
                                            int32_t *ok, int32_t *n_inliers, vh_mono_model *model);

/* ---- motion inliers, monocular: which records of whole lists agree with an epipolar model ------------ */
/* VisualOdometryMono::getInlier (src/viso_mono.cpp:268-315) for any flow or quad list under a vh_mono_model: a record's
 * (u1p, v1p) is normalised with c[0], c[1], s[0] and its (u1c, v1c) with c[2], c[3], s[1] as normalizeFeaturePoints
 * does -- q = (float)((double)u - c), then (float)((double)q * s), each rounded to float once -- and the test is
 * |Sampson distance under F| < inlier_threshold: strict, in double, one division, no transcendental function, so the
 * flags equal a host restatement byte for byte on every input.  A quotient that is NaN or infinite (NaN coordinates,
 * a zero denominator, 0/0 under F = 0) is "not an inlier", never an error; a list with ok = 0 has no inliers and its
 * model is not read (`valid` is never read: pass ok = (int32_t)valid, or the estimator's ok); a list of one record
 * is classified like any other.  Only inlier_threshold of vh_mono_params is read; the other fields of a record are
 * not read.
 *
 * Stateless: as vh_motion_inliers with model[n_sets] in the place of tr -- same outputs, same limits, and n_sets == 0
 * or no records at all is VH_OK without a device. */
int32_t vh_motion_inliers_mono(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm,
                               const int32_t *offsets, const vh_mono_model *model, const int32_t *ok, uint8_t *flags,
                               int32_t *n_inliers, vh_p_match *inlier_pm, int32_t *src_pos);
/* The same on the device-resident lists of the handle's last match call, as vh_group_motion_inliers / vh_match_inliers:
 * model[S], ok[S] go up, counts[S] comes back.  Flow and quad lists (VH_ERR_STATE for stereo lists and before any
 * match).  Plain groups, sequence handles and lone matchers; refined, multi-stage and host-replaced lists as there.
 * A handle has ONE result: the getters above (vh_group_get_inlier_flags / _matches / _matches_all,
 * vh_get_inlier_matches, vh_group_inliers_device) return the last classification of either kind, and a mono
 * classification replaces a stereo one and the other way round.  The first classification of either kind allocates
 * the block described at vh_group_motion_inliers; the first mono classification adds one block of 128 bytes per
 * stream for the models (its own: not the one vh_group_estimate_motion_mono_model keeps for its output).  Both are counted by vh_group_device_bytes; a refused allocation is VH_ERR_HIP before
 * anything is launched, leaves nothing behind, and the call may be repeated.
 * Profile scopes: "inlier_flag_mono", "inlier_compact". */
int32_t vh_group_motion_inliers_mono(vh_group *g, const vh_mono_params *e, const vh_mono_model *model, const int32_t *ok,
                                     int32_t *counts);
int32_t vh_match_inliers_mono(vh_matcher *m, const vh_mono_params *e, const vh_mono_model *model, int32_t ok, int32_t *count);

/* ---- the epipolar model refitted on whole lists (csrc/kernels_mono_refit.hip) ----------------------------
 * The estimator's F comes from the inliers of its best hypothesis in a bucketed list (the refit of src/viso_mono.cpp:80,
 * a few hundred rows).  This is the same fundamentalMatrix (:235-266) over EVERY record of any flow or quad list (pass
 * an inlier list), in the normalised frame of the model the list was classified under.  The reference has no
 * counterpart (its estimator stops at :80); every term is its own:
 *   1. normalisation: the incoming model's.  c[4] and s[2] are copied to the output unchanged (bit for bit), not
 *      recomputed over the list; a record is normalised as vh_motion_inliers_mono does -- (float)((double)u - c), then
 *      (float)((double)q * s), one rounding to float per step;
 *   2. rows: the nine entries of :244-252 as the estimator's own refit forms them -- u1c*u1p, u1c*v1p, u1c, v1c*u1p,
 *      v1c*v1p, v1c, u1p, v1p, 1: float products of the normalised float fields, then widened to double;
 *   3. moments: M = sum a a^T in double, the 45 sums of the upper triangle mirrored.  The sums run in parallel in an
 *      order that depends on the list's length alone: the result agrees with a sequential evaluation to rounding, is the
 *      same bytes from run to run, alone or among other lists, and from the stateless and the handle forms;
 *   4. null direction: f = the right singular vector of M for its smallest singular value -- Matrix::svd
 *      (src/matrix.cpp:579-802, restated) on the 9 x 9 M, the column of V its descending sort puts last (M is symmetric
 *      positive semi-definite: the right singular vectors of the N x 9 system the reference decomposes).  Matrix::svd's
 *      sign normalisation is not applied; instead f is negated when its dot product with model_in's F (nine terms,
 *      row-major order, in double) is negative -- a zero or NaN product leaves it as it is -- so that the refined F is
 *      comparable entry by entry with the F it refines.  w_out[.][0] = w[8] and w_out[.][1] = w[7], the two smallest
 *      singular values of M (squares of the system's): w[8] / w[7] near 1 is a degenerate fit (pure rotation, a plane);
 *   5. rank 2: the 3 x 3 step of :262-265 on f.
 *   6. per list, never an error of the call: ok_out = 0, a zeroed model_out and w_out = 0 where ok_in == 0 (model_in is
 *      then not read), where the list has fewer than 10 records (the reference's floor at :76), and where an entry of
 *      F, w[8] or w[7] is not finite (non-finite records propagate and end here); otherwise ok_out = 1, valid = 1.0.
 * Double precision; vh_mono_params is not read by the refit itself (inlier_threshold by the reclassification below).
 *
 * Stateless: lists laid out as for vh_motion_inliers_mono, model_in[n_sets], ok_in[n_sets] -> model_out[n_sets],
 * ok_out[n_sets], w_out[n_sets][2].  n_sets == 0 or no records at all: VH_OK (outputs zero), nothing is launched and no
 * device is needed.  Length limits as vh_motion_inliers. */
int32_t vh_refit_model_mono(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                            const vh_mono_model *model_in, const int32_t *ok_in, vh_mono_model *model_out, int32_t *ok_out,
                            double *w_out /* [n_sets][2] */);
/* The same on the compacted inlier lists of the handle's current MONO classification (vh_group_motion_inliers_mono /
 * vh_match_inliers_mono), from the model / ok that classification was made under -- both are on the device already:
 * nothing goes up, model_out[S], ok_out[S], w_out[S][2] and counts[S] come back; the call is synchronous.  VH_ERR_STATE
 * before any classification of the current lists, after the next push or match, and when the current result is a
 * stereo classification.  Rows without a pair have ok_out = 0.
 *   reclassify == 0: the classification is untouched, counts are its counts.
 *   reclassify != 0: the lists are classified again under model_out / ok_out with e->inlier_threshold, queued behind
 *   the refit on the same stream (the host does not wait in between); the refined model becomes the model the
 *   classification was made under, so a second call refits again with nothing uploaded; the getters and
 *   vh_group_inliers_device then return the refined model's inliers and counts are theirs (VH_ERR_CAPACITY as
 *   vh_group_motion_inliers).  Should that classification fail with another error, model_out / ok_out / w_out are still
 *   delivered and the handle is left without a classification (VH_ERR_STATE from the getters) until
 *   vh_group_motion_inliers_mono is called again.
 * Plain groups, sequence handles and lone matchers.  The first call adds one block of 148 bytes per stream (128 + 16 +
 * 4, each of its three arrays rounded up to 256 bytes), counted by vh_group_device_bytes; a handle that never calls it
 * allocates and launches nothing.  A refused allocation is VH_ERR_HIP before any launch and leaves the handle as it
 * was; the call may be repeated.  Profile scope: "mono_refit". */
int32_t vh_group_refit_model_mono(vh_group *g, const vh_mono_params *e, int32_t reclassify, vh_mono_model *model_out,
                                  int32_t *ok_out, double *w_out, int32_t *counts);
int32_t vh_match_refit_model_mono(vh_matcher *m, const vh_mono_params *e, int32_t reclassify, vh_mono_model *model_out,
                                  int32_t *ok_out, double *w_out, int32_t *count);

/* ---- the mono pose on whole lists: R|t, chirality and scale (csrc/kernels_mono_pose.hip) -----------------
 * The rest of VisualOdometryMono::estimateMotion after the refit (src/viso_mono.cpp:83-158) for any flow or quad list
 * (pass an inlier list) under a vh_mono_model: the six motion parameters, and what they were formed from.  The scale
 * comes from where the reference takes it, the ground-plane vote of :116-143, over the triangulated points of the list
 * the pose is computed on.  Per list:
 *   1. F out of the model's frame: Tp = {sp,0,-sp*cpu, 0,sp,-sp*cpv, 0,0,1}, Tc likewise from c[2], c[3], s[1]
 *      (:226-227); F = ~Tc*F*Tp, E = ~K*F*K, the rank-2 step on E (:83-94);
 *   2. EtoRt (:317-348): Matrix::svd of E, the four candidates (Ra,t), (Ra,-t), (Rb,t), (Rb,-t), the projection
 *      matrices of :370-375;
 *   3. triangulateChieral (:380-397) per record and candidate on the raw u1p, v1p, u1c, v1c; the winner is the first
 *      candidate with the strictly largest count;
 *   4. under the winner X / X(3,:) (a zero w gives the zero point), the points with z > 0 in list order, their
 *      dist = |x|+|y|+|z| and d = cos(-pitch)*y + sin(-pitch)*z;
 *   5. median: the element of rank np/2 of dist, by counting, ties broken by position (smallerThanMedian);
 *   6. the ground-plane vote (:124-142): for every i with d[i] > median/motion_threshold the sum over all j, ascending
 *      from 0, of exp(-(d[j]-d[i])^2 * weight); the first i with the largest sum wins, plane = d[i];
 *   7. tr as :143-158: the angles of R, t * height / plane.
 * Double precision, every product and sum rounded on its own, every sum in an order fixed by the list's length alone:
 * the same bytes from run to run, alone or among other lists, and from the stateless and the handle forms.  exp, asin,
 * cos and sin are the device library's.  On a bucketed list with the model vh_estimate_motion_mono_model returned for
 * it, tr, ok and the winner are that call's.
 * f, cu, cv, height, pitch and motion_threshold of vh_mono_params are read; ransac_iters and inlier_threshold are not. */
typedef struct vh_mono_pose {   /* 152 bytes */
  double R[9];        /* the winning rotation, row-major */
  double t[3];        /* the winning translation, unit length as EtoRt leaves it (sign applied) */
  double scale;       /* height / plane: tr[3..5] = t * height / plane, formed as the estimator forms it */
  double median;      /* smallerThanMedian's median of the L1 distances of the points in front */
  double plane;       /* d[best_idx] of the ground-plane vote */
  int32_t chirality[4];  /* triangulateChieral's count per candidate (Ra,t), (Ra,-t), (Rb,t), (Rb,-t) */
  int32_t candidate;  /* the winner 0..3, -1 if none */
  int32_t n_front;    /* points with z > 0 under the winner */
  int32_t reason;     /* 0 ok; see below */
  int32_t reserved_;  /* 0 */
} vh_mono_pose;
/* reason: the first of these that applies; each gives ok = 0, tr = 0 and zeros for the fields not yet determined, never
 * an error of the call:
 *   1  ok_in == 0 (the model is not read)            2  fewer than 10 records (:45)
 *   3  no candidate has a positive chirality count   4  fewer than 10 points in front (:105)
 *   5  median > motion_threshold (:113)              6  fabs(plane) < 1e-20
 *   7  a non-finite value in R, t, median, plane or tr (the fields stay as computed; tr = 0)
 * A record with a NaN coordinate is in front of no camera (every comparison with NaN is false): it counts for no
 * candidate and is not among the points in front.
 *
 * Stateless: lists laid out and validated as for vh_refit_model_mono; model[n_sets], ok_in[n_sets] -> tr[n_sets][6],
 * ok[n_sets], pose[n_sets] (pose may be NULL).  n_sets == 0 or no records at all: VH_OK (outputs zero, reason 1 or 2 per
 * list), nothing is launched and no device is needed. */
int32_t vh_pose_mono(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                     const vh_mono_model *model, const int32_t *ok_in, double *tr, int32_t *ok, vh_mono_pose *pose);
/* The same on the compacted inlier lists of the handle's current MONO classification, under the model / ok that
 * classification was made under (after vh_group_refit_model_mono(reclassify = 1): the refined model with its inliers);
 * nothing goes up, tr[S][6], ok[S], pose[S] (nullable) and counts[S] (nullable: the lists' lengths) come back; the call
 * is synchronous.  VH_ERR_STATE before any classification of the current lists, after the next push or match, and when
 * the current result is a stereo classification.  Plain groups, sequence handles and lone matchers.  The first call adds
 * one block: 16 bytes per record slot (dist, d: 8 + 8, S * max_matches slots) and 972 bytes per stream (a header of 768,
 * tr 48, ok 4, pose 152; each of the six arrays rounded up to 256 bytes), counted by vh_group_device_bytes; a handle that never calls
 * it allocates and launches nothing.  A refused allocation is VH_ERR_HIP before any launch and leaves the handle as it
 * was; the call may be repeated.  Profile scopes: "mono_pose_head", "mono_pose_tri", "mono_pose_front",
 * "mono_pose_rank", "mono_pose_vote", "mono_pose_finish". */
int32_t vh_group_pose_mono(vh_group *g, const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose, int32_t *counts);
int32_t vh_match_pose_mono(vh_matcher *m, const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose);

/* ---- the mono pose refined on whole lists: Gauss-Newton on R|t, covariance (csrc/kernels_mono_pose_refine.hip) ----
 * vh_pose_mono decomposes an algebraic F; here the winning (R, unit t) is refined by Gauss-Newton on the signed Sampson
 * distance of EVERY record of the list, the scale tail then runs under the refined pose, and the 5 x 5 covariance of the
 * refined pose is returned.  Neither the reference nor stock libviso2 has a counterpart: the contract is this text.
 * Per list, every record active, double precision, every product and sum rounded on its own, K = {f, cu, cv}:
 *   1. Start: steps 1-3 of vh_pose_mono unchanged; the start is the winner's R and signed unit t.  With pose reasons 1, 2
 *      or 3 there is nothing to refine: status = 1, everything else is vh_pose_mono's result for the list.
 *   2. Residual of a record: xp = (((double)u1p - cu) / f, ((double)v1p - cv) / f, 1), xc likewise from u1c, v1c;
 *      E = [t]x R; n = xc^T E xp; a = E xp; b = E^T xc; s = a0^2 + a1^2 + b0^2 + b1^2; r = f * n / sqrt(s), the signed
 *      Sampson distance in pixels.  Nothing is clamped: s = 0 or a NaN coordinate propagates and ends in status = 4.
 *   3. Parameters delta = (w0, w1, w2, tau0, tau1): w a left rotation, R <- Exp([w]x) * R by Rodrigues (I + [w]x below
 *      |w| = 1e-12); tau in the tangent plane of the unit sphere at t: m the first index of the smallest |t_m|,
 *      b0 = normalise(e_m - (e_m . t) t), b1 = t x b0, t <- normalise(t + tau0 b0 + tau1 b1); the basis is rebuilt at
 *      every update.
 *   4. Jacobian, analytic and complete: E_k = [t]x [e_k]x R for w_k, E_k = [b_k]x R for tau_k; dn = xc^T E_k xp,
 *      da = E_k xp, db = E_k^T xc, ds = 2 (a0 da0 + a1 da1 + b0 db0 + b1 db1),
 *      J_k = f * (dn / sqrt(s) - n * ds / (2 s sqrt(s))).
 *   5. Update: A = sum J^T J (15 sums, the upper triangle mirrored), g = sum J^T r, ssr = sum r^2; delta = -A^-1 g by
 *      Matrix::solve (src/matrix.cpp:417-504); step size 1.  The update that reports max |delta_k| < 1e-8 is applied
 *      and ends the loop as converged; at most 102 updates.
 *   6. Covariance: one more accumulation at the converged pose gives A and ssr; cov = ssr / (N - 5) * A^-1 by
 *      Matrix::solve on the five unit right-hand sides, the upper triangle computed and mirrored, in the order of delta.
 *      B = (b0, b1) at the converged t maps the two translation coordinates to 3-D: dt = tau0 b0 + tau1 b1.
 *   7. Tail: steps 4-7 of vh_pose_mono under the refined R, t with their own reasons 4-7.  The sign of t is the
 *      winner's; the chirality vote is not repeated.
 *   8. A refused refinement is not a refused pose: for status != 0 the tail runs under the unrefined winner; tr, ok and
 *      the vh_mono_pose are byte for byte those of vh_pose_mono on that list; cov, B, ssr, moved_R, moved_t are zero,
 *      ssr_start is kept where it was finite.  Never an error of the call.
 *   9. Sums run in an order fixed by the list's length alone, no atomics: the same bytes from run to run, alone or
 *      among other lists, and from the stateless and the handle forms.  sin and asin are the device library's. */
typedef struct vh_mono_refine {   /* 288 bytes */
  double B[6];        /* b0[3], b1[3]: the tangent basis at the refined t */
  double cov[25];     /* row-major, exactly symmetric, in the order (w0, w1, w2, tau0, tau1): rad^2 */
  double ssr_start;   /* sum r^2 at the winner (px^2) */
  double ssr;         /* sum r^2 at the refined pose */
  double moved_R;     /* angle between the start and the refined rotation: 2 asin(|R1 - R0|_F / (2 sqrt 2)), rad */
  double moved_t;     /* angle between the start and the refined direction: 2 asin(|t1 - t0| / 2), rad */
  int32_t status;     /* 0 refined; see below */
  int32_t n_updates;  /* updates applied: 0 .. 102 */
} vh_mono_refine;
/* status: 0  converged, the pose is the refined one
 *         1  nothing to refine (pose reason 1, 2 or 3)      2  Matrix::solve refused (a pivot below 1e-20)
 *         3  not converged after 102 updates                4  a sum, R, t or a covariance entry is not finite
 *
 * Stateless: layout, validation and empty-input behaviour are vh_pose_mono's; refine[n_sets] (nullable; status 1 where
 * nothing is launched). */
int32_t vh_pose_mono_refined(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                             const vh_mono_model *model, const int32_t *ok_in, double *tr, int32_t *ok, vh_mono_pose *pose,
                             vh_mono_refine *refine);
/* The same on the compacted inlier lists of the handle's current MONO classification: state rules, outputs and the
 * arena block are vh_group_pose_mono's (the two share the block); refine[S] is nullable.  The first call adds one array
 * of 288 bytes per stream, rounded up to 256 bytes, counted by vh_group_device_bytes; a handle that never calls these
 * entries allocates and launches nothing for them.  A refused allocation is VH_ERR_HIP before any launch and leaves the
 * handle as it was; the call may be repeated.  Profile scope: "mono_pose_refine", between "mono_pose_tri" and
 * "mono_pose_front". */
int32_t vh_group_pose_mono_refined(vh_group *g, const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose,
                                   vh_mono_refine *refine, int32_t *counts);
int32_t vh_match_pose_mono_refined(vh_matcher *m, const vh_mono_params *e, double *tr, int32_t *ok, vh_mono_pose *pose,
                                   vh_mono_refine *refine);
/* ---- scene points: the 3-d point of every record of whole lists, stereo and mono (csrc/kernels_scene.hip) ----
 * One point per record of a list (pass an inlier list), compacted in list order: the per-step cloud beside the pose.
 * Double precision, every product and sum rounded on its own, one rounding to float at the store.
 * Stereo, a quad list under tr[6] (vh_ego_params: f, cu, cv, base are read):
 *   the point of the previous pair as getInlier forms it (src/viso_stereo.cpp:80-86), float df = max(u1p - u2p, 0.0001f):
 *   X = (u1p - cu) * base / df, Y = (v1p - cv) * base / df, Z = f * base / df;  frame 0: (X, Y, Z);  frame 1: the point
 *   moved by tr, X1c = r00 X + r01 Y + r02 Z + tx and so on (:274-276);  err = sqrt of the sum of the four squared
 *   differences between (u1c, v1c, u2c, v2c) and the prediction (:317-321) -- the sum vh_motion_inliers compares -- for
 *   either frame;  sigma_z = z * z / (f * base) of the point in the frame asked for.
 * Mono, a flow or quad list under a vh_mono_pose (vh_mono_params: f, cu, cv are read):
 *   P1 = K [I | 0], P2 = K [R | t] from the pose's R and unit t; the record triangulated as triangulateChieral does
 *   (src/viso_mono.cpp:378-387); X / X(3,:), a zero w giving the zero point (:100);  frame 0: that point times
 *   pose.scale;  frame 1: (R X + t) times pose.scale;  err = sqrt of the sum of the four squared differences between
 *   (u1p, v1p), (u1c, v1c) and the projections of X by P1, P2;  sigma_z = 0.
 * A record is dropped, never an error: in a list with ok = 0 (count 0; tr / pose is not read); where x, y, z or err is
 * not finite (also: not finite as a float); where z <= 0;  stereo: where min_disp > 0 and the float u1p - u2p <
 * min_disp;  where max_depth > 0 and z > max_depth;  where max_err > 0 and err > max_err -- strict compares in double on
 * the values in the frame asked for, before Tw.  Tw (nullable; [n][16], a row-major 4x4 per list of which the top three
 * rows are read) is applied last: x' = Tw[0] x + Tw[1] y + Tw[2] z + Tw[3], added left to right.
 * Survivors keep list order; the same bytes from run to run, alone or among other lists, and from the stateless and the
 * handle forms.  The stereo rotation's sin / cos are the device library's. */
typedef struct vh_scene_point {   /* 32 bytes */
  float   x, y, z;      /* metres, in the frame asked for, after Tw if given */
  float   sigma_z;      /* stereo: z * z / (f * base), depth std-dev per pixel of disparity error, of the camera-frame
                         * point before Tw; mono: 0 */
  float   err;          /* reprojection error in pixels */
  int32_t src_pos;      /* position of the record in the list the classification ran on (stateless: in the list given) */
  int32_t i1p, i1c;     /* copied from the record: joins vh_track / features */
} vh_scene_point;
typedef struct vh_scene_params {
  int32_t frame;        /* 0: previous left camera, 1: current left camera */
  float   min_disp;     /* stereo: drop records with u1p - u2p < min_disp (0: keep all) */
  double  max_depth;    /* drop camera-frame z > max_depth (<= 0: no limit) */
  double  max_err;      /* drop err > max_err (<= 0: no limit) */
} vh_scene_params;
void vh_default_scene_params(vh_scene_params *sp);   /* frame 1, 0, 0, 0 */
/* Stateless: lists laid out and validated as for vh_motion_inliers (the same length limits); tr[n_sets][6] (mono:
 * pose[n_sets]), ok[n_sets], Tw NULL or [n_sets][16] -> out (indexed like pm: list s compacted at [offsets[s],
 * offsets[s] + counts[s]), the rest of each slice not written) and counts[n_sets].  sp->frame outside 0..1 is
 * VH_ERR_INVALID_ARG.  n_sets == 0 or no records at all: VH_OK with zero counts, nothing is launched and no device is needed. */
int32_t vh_scene_points_stereo(const vh_ego_params *e, const vh_scene_params *sp, int32_t device, int32_t n_sets, const vh_p_match *pm,
                               const int32_t *offsets, const double *tr, const int32_t *ok, const double *Tw, vh_scene_point *out,
                               int32_t *counts);
int32_t vh_scene_points_mono(const vh_mono_params *e, const vh_scene_params *sp, int32_t device, int32_t n_sets, const vh_p_match *pm,
                             const int32_t *offsets, const vh_mono_pose *pose, const int32_t *ok, const double *Tw, vh_scene_point *out,
                             int32_t *counts);
/* The same on the compacted inlier lists of the handle's current classification, the motion / pose taken from the
 * device: nothing goes up but Tw (nullable, [S][16]); counts[S] comes back; synchronous.  src_pos is the position in the
 * list the classification ran on (vh_group_get_inlier_matches' src_pos_out of the record).
 *   _stereo: under the tr / ok the STEREO classification was made under (after vh_group_refit_motion(reclassify = 1)
 *     the refined motion); VH_ERR_STATE wherever vh_group_motion_covariance returns it.
 *   _mono: under the pose the last vh_group_pose_mono / _refined left on the device for the current MONO classification
 *     (R, t, scale, ok); VH_ERR_STATE without one, after the next push, match or classification, and on a stereo
 *     classification.
 * Plain groups, sequence handles (rows without a pair: count 0) and lone matchers.  The first call adds one block: 32
 * bytes per record slot (S x max_matches slots), 4 bytes per tile of 256 slots (S x ceil(max_matches / 256)) and 128 + 4
 * bytes per stream (Tw, counts), each of the four arrays rounded up to 256 bytes, counted by vh_group_device_bytes; a
 * handle that never calls these allocates and launches nothing.  A refused allocation is VH_ERR_HIP before any launch
 * and leaves the handle as it was; the call may be repeated.  Profile scope: "scene_points". */
int32_t vh_group_scene_points_stereo(vh_group *g, const vh_ego_params *e, const vh_scene_params *sp, const double *Tw, int32_t *counts);
int32_t vh_match_scene_points_stereo(vh_matcher *m, const vh_ego_params *e, const vh_scene_params *sp, const double *Tw, int32_t *count);
int32_t vh_group_scene_points_mono(vh_group *g, const vh_mono_params *e, const vh_scene_params *sp, const double *Tw, int32_t *counts);
int32_t vh_match_scene_points_mono(vh_matcher *m, const vh_mono_params *e, const vh_scene_params *sp, const double *Tw, int32_t *count);
/* The points of the last such call, valid until the next match call (VH_ERR_STATE before one on the current lists),
 * under the getters' capacity rule: *n is the full number, at most cap records are written, VH_ERR_CAPACITY when there
 * are more.  The _all form writes stream s at [s * cap_per_stream ..] and counts[S].  _device: the array itself, stream
 * s at [s * *stride ..] (records). */
int32_t vh_group_get_scene_points(vh_group *g, int32_t stream, vh_scene_point *out, int32_t cap, int32_t *n);
int32_t vh_group_get_scene_points_all(vh_group *g, vh_scene_point *out, int32_t cap_per_stream, int32_t *counts);
int32_t vh_get_scene_points(vh_matcher *m, vh_scene_point *out, int32_t cap, int32_t *n);
int32_t vh_group_scene_points_device(vh_group *g, const vh_scene_point **d_points, int64_t *stride);

/* ---- landmarks: the scene points of a step fused along the feature tracks (csrc/kernels_landmark.hip) ----
 * One landmark per live track that was observed in this step: its position averaged, weighted by 1 / sigma_z^2, over
 * every step that saw it, with the uncertainty of that mean and the number of observations.  The join of vh_track
 * (prev: the record continued in the predecessor list) and vh_scene_point (src_pos: the record a point belongs to) is a
 * gather, one lane per record; the per-track state travels from list to list in vh_landmark_state.
 * THE CALLER'S DUTY: the points of every step must lie in ONE COMMON FRAME -- call vh_group_scene_points_* (or the
 * stateless forms) with a Tw that takes the camera of sp.frame to the world.  The entries cannot check it: points given
 * in the moving camera's frame are averaged all the same (or restart at the gate).
 * Record j of a list, in this order; all arithmetic in double, every product and sum rounded on its own, sums added
 * left to right:
 *   1. carry: st = prev_state[trk[j].prev] where a predecessor state exists and 0 <= trk[j].prev < n_prev, else all
 *      zeros (a prev outside the predecessor list is never dereferenced).
 *   2. the observation is the scene point k with pts[k].src_pos == j (at most one).  Without one: if st.n_obs > 0 then
 *      st.n_missed += 1, and if max_missed >= 0 && st.n_missed > max_missed st becomes zeros; nothing is emitted.
 *   3. with one, (x, y, z, s = sigma_z) widened to double: w = s > 0 ? 1.0 / (s * s) : 1.0 (mono: sigma_z = 0).  The
 *      gate, only if st.n_obs > 0 and T = max_dist + gate_sigma * s is > 0: dx = x - st.swx / st.sw, likewise dy, dz; if
 *      dx*dx + dy*dy + dz*dz > T*T, st becomes zeros (the landmark restarts from this observation).  Then st.sw += w;
 *      st.swx += w*x; st.swy += w*y; st.swz += w*z; st.n_obs += 1; st.n_missed = 0.  If the new sw, swx, swy or swz is
 *      not finite, st becomes zeros and nothing is emitted.
 *   4. state_out[j] = st.
 *   5. the record emits a vh_landmark iff it had an observation and st.n_obs >= min_obs.
 * Survivors are compacted in list order; the same bytes from run to run, alone or among other lists, and from the
 * stateless and the handle forms. */
typedef struct vh_landmark_state {   /* 48 bytes, one per record of a tracked list */
  double  sw, swx, swy, swz;         /* sum of w, w*x, w*y, w*z over the accepted observations */
  int32_t n_obs;                     /* accepted observations; 0: no state, every field 0 */
  int32_t n_missed;                  /* consecutive records of the track without an observation since the last one */
  int32_t reserved[2];               /* 0 */
} vh_landmark_state;
typedef struct vh_landmark {         /* 48 bytes */
  float   x, y, z;                   /* swx / sw, swy / sw, swz / sw: double quotients, one rounding to float */
  float   sigma;                     /* sqrt(1.0 / sw) in double, rounded once */
  int32_t n_obs;
  int32_t age;                       /* vh_track.age of the record */
  int64_t birth_frame;               /* the track id, */
  int32_t birth_pos;                 /*   copied from vh_track */
  int32_t src_pos;                   /* position of the record in the tracked list */
  int32_t i1c;                       /* copied from the scene point */
  int32_t point_pos;                 /* position of this step's scene point in its list */
} vh_landmark;
typedef struct vh_landmark_params {
  int32_t min_obs;                   /* emit only landmarks with n_obs >= min_obs; >= 1 */
  int32_t max_missed;                /* < 0: a track keeps its state through any gap; else the state is dropped once n_missed > max_missed */
  double  max_dist;                  /* the gate: T = max_dist + gate_sigma * sigma_z, applied where T > 0; both <= 0: no gate */
  double  gate_sigma;
} vh_landmark_params;
void vh_default_landmark_params(vh_landmark_params *lp);   /* 2, 3, 0, 0 */
/* Stateless: one step for n_sets independent lists, host pointers.  The three families of lists are laid out and
 * validated as for vh_motion_inliers / vh_scene_points_* (the same offsets convention and length limits): trk behind
 * rec_offsets, pts behind pt_offsets (src_pos numbering the records of the same list), prev behind prev_offsets (both
 * NULL: no list has a predecessor).  state_out and out are indexed like trk: list s's landmarks compacted at
 * [rec_offsets[s], rec_offsets[s] + counts[s]), the rest of each slice of out not written.
 * VH_ERR_INVALID_ARG: min_obs < 1; a list whose src_pos values are not strictly increasing and inside [0, n_rec) -- checked
 * on the host before anything is launched -- or that holds more points than records; only one of prev / prev_offsets given;
 * null pointers.  n_sets == 0 or no records at all: VH_OK with zero counts, nothing is launched and no device is needed. */
int32_t vh_landmarks_update(const vh_landmark_params *lp, int32_t device, int32_t n_sets,
                            const vh_track *trk, const int32_t *rec_offsets,
                            const vh_scene_point *pts, const int32_t *pt_offsets,
                            const vh_landmark_state *prev, const int32_t *prev_offsets,
                            vh_landmark_state *state_out, vh_landmark *out, int32_t *counts);
/* The same on a handle: the current tracked lists (vh_group_set_track_linking) and the scene points of the last
 * vh_group_scene_points_* call, both on the device; nothing goes up but the params; counts[S] comes back; synchronous.
 * The predecessor state is what the last vh_group_landmarks call wrote for the predecessor list as it stands (the list
 * vh_track.prev indexes): no call for that list, a list matched again after the call, or no predecessor at all, and every
 * record starts without state (prev = NULL of the stateless form).  A repeated call in one step reads the same
 * predecessor state and gives the same bytes; after matching the same pair again the next call recomputes the current
 * state from the predecessor's, which is kept.
 * VH_ERR_STATE with track linking off, without a tracked list for the current pair (before a match call, after the next
 * push), without scene points of the current lists, and where the classification read lists replaced on the host
 * (vh_remove_outliers / vh_bucket_features: their positions are not the tracked list's).  VH_ERR_UNSUPPORTED on a
 * sequence handle without vh_sequence_set_landmarks (below; checked before the state), where the predecessor of row r is
 * row r - 1 of the same call: a chain, not a gather.
 * Plain groups and lone matchers.  The first call adds one block: 2 x 48 bytes of state, 48 bytes of output and 4 bytes
 * of observation index per record slot (S x max_matches slots), 4 bytes per tile of 256 slots and 4 bytes per stream,
 * each of the five arrays rounded up to 256 bytes, counted by vh_group_device_bytes; a handle that never calls these
 * allocates and launches nothing.  A refused allocation is VH_ERR_HIP before any launch and leaves the handle as it was;
 * the call may be repeated.  Profile scope: "landmarks". */
int32_t vh_group_landmarks(vh_group *g, const vh_landmark_params *lp, int32_t *counts);
int32_t vh_match_landmarks(vh_matcher *m, const vh_landmark_params *lp, int32_t *count);
/* The landmarks of the last such call, valid until the next match call (VH_ERR_STATE before one on the current lists),
 * under the getters' capacity rule, as vh_group_get_scene_points.  _device: the array itself, stream s at
 * [s * *stride ..] (records). */
int32_t vh_group_get_landmarks(vh_group *g, int32_t stream, vh_landmark *out, int32_t cap, int32_t *n);
int32_t vh_group_get_landmarks_all(vh_group *g, vh_landmark *out, int32_t cap_per_stream, int32_t *counts);
int32_t vh_get_landmarks(vh_matcher *m, vh_landmark *out, int32_t cap, int32_t *n);
int32_t vh_group_landmarks_device(vh_group *g, const vh_landmark **d_out, int64_t *stride);

/* ---- landmarks along the rows of one chain (csrc/kernels_landmark_chain.hip) ----
 * The lists of a call are the rows 0 .. n_sets - 1 of one chain, as vh_link_tracks links them: list s's predecessor is
 * list s - 1 OF THE SAME CALL, so vh_track.prev of list s indexes list s - 1 and the predecessor state of a record is the
 * state_out this very call computes for it.  List 0's predecessor is the carry: n_carry states (carry NULL, n_carry 0:
 * none), for instance the last list's slice of state_out of the call before.  Every record follows the rule above, steps
 * 1 - 5, with "predecessor state" read so: step 1 for record j of list s > 0 is st = state_out[list s - 1][trk[j].prev]
 * where 0 <= trk[j].prev < n_rec[s - 1], for list 0 st = carry[trk[j].prev] where 0 <= trk[j].prev < n_carry, else zeros
 * (a prev outside is never dereferenced; an empty list ends every chain).  The result is the bytes of n_sets
 * vh_landmarks_update calls, one list at a time, each fed the state_out of the one before -- in one call: the device walks
 * every track from its first record in the call to its last, the 48-byte state in registers, the same arithmetic in the
 * same order.  Lists, points, outputs, refusals and the n_sets == 0 / no-records shortcuts are vh_landmarks_update's.
 * One refusal more, made on the host before any device work: two records of one list with the same prev inside their
 * predecessor list (list 0: inside the carry) are VH_ERR_INVALID_ARG -- a record is continued at most once (the link
 * rule of vh_link_tracks), and the walk relies on it.  n_carry < 0, or n_carry > 0 without carry: VH_ERR_INVALID_ARG. */
int32_t vh_landmarks_chain(const vh_landmark_params *lp, int32_t device, int32_t n_sets,
                           const vh_track *trk, const int32_t *rec_offsets,
                           const vh_scene_point *pts, const int32_t *pt_offsets,
                           const vh_landmark_state *carry, int32_t n_carry,
                           vh_landmark_state *state_out, vh_landmark *out, int32_t *counts);
/* Sequence handles.  on = 1, before the first push only (VH_ERR_STATE afterwards; VH_ERR_UNSUPPORTED on a plain group or
 * a lone matcher; as vh_sequence_set_multi_stage): vh_group_landmarks(g, lp, counts[S]) then runs the chain form over the
 * rows of the current chunk's tracked lists and the points of the last vh_group_scene_points_* call, both on the device;
 * only the params go up.  Its VH_ERR_STATE conditions are the group's; rows without a pair (row 0 of the first chunk, the
 * rows behind a short chunk) give count 0; vh_group_get_landmarks(_all) and vh_group_landmarks_device serve rows as they
 * serve streams.  Off (the default): everything as before, VH_ERR_UNSUPPORTED from vh_group_landmarks included.
 * The carry: row 0 continues the last row of the previous chunk.  The rows' states stay on the device; the last row's
 * are copied aside when the first landmarks call of the next chunk is queued (the rule of the track carry), and used iff
 * the track carry is valid, the last landmarks call on the previous chunk came after that chunk's last match call, and no
 * chunk went without a call in between; otherwise every record of row 0 starts without state.  A repeated call gives the
 * same bytes; matching the chunk again and repeating scene points and landmarks recomputes the rows from the same carry;
 * a match call that failed half way voids the carry with the track carry.
 * The first call adds one block, counted by vh_group_device_bytes: 48 bytes of state, 48 of output and 8 of observation
 * index and forward link per record slot (S x max_matches slots), 48 bytes per carry slot (max_matches), 4 bytes per tile
 * of 256 slots and 4 per row, each of the six arrays rounded up to 256 bytes.  A refused allocation is VH_ERR_HIP before
 * any launch and leaves the handle as it was.  Profile scope: "landmarks" (and one per launch inside it: "landmark_index",
 * "landmark_link", "landmark_chain", "landmark_count", "landmark_scan", "landmark_store"). */
int32_t vh_sequence_set_landmarks(vh_group *g, int32_t on);

/* ---- trajectory: the camera's pose in the world, accumulated from the motions (csrc/kernels_trajectory.hip) ----
 * The reference's demo loop, pose = pose * Matrix::inv(viso.getMotion()) (src/demo.cpp), one row at a time along a chain
 * of rows, strictly left to right.  The rule has one copy, csrc/vh_trajectory.h; all arithmetic in double, every product
 * and sum rounded on its own.  One row with motion tr[6] and ok, the running pose P (row-major 4x4):
 *   1. T = transformationVectorToMatrix(tr) (src/viso.cpp:59-84): the rotation of the estimators, the translation column
 *      tr[3..5], the last row 0 0 0 1.
 *   2. Tinv = Matrix::inv(T): the general Gauss-Jordan elimination of Matrix::solve on the unit matrix, not the rigid
 *      shortcut.
 *   3. status: 4 where the row holds no pair (ok < 0 in the stateless form; on a sequence handle row 0 of the first chunk
 *      and the rows behind a short chunk), else 1 where ok == 0, else 2 where a value of tr is not finite, else 3 where
 *      the elimination refuses (a pivot below 1e-20), else 2 where a value of Tinv is not finite, else 0: accepted.
 *   4. accepted: P' = P * Tinv in Matrix::operator*'s order (c = 0; c += P[i][k] * Tinv[k][j], k ascending), step += 1,
 *      and Tinv becomes the chain's last accepted one.  Not accepted is never an error of the call: under VH_TRAJ_HOLD the
 *      pose stays (demo.cpp when process() fails); under VH_TRAJ_REPEAT a row of status 1..3 multiplies by the last
 *      accepted Tinv of the chain once more (constant velocity; before any accepted row it holds).  Status 4 always holds.
 *   5. the row's record: Tw_prev = P (the world pose of the previous camera), Tw_cur = P', status, step.
 * What a chain carries from call to call is vh_traj_carry: the last Tw_cur, the last accepted Tinv and step.  The same
 * bytes from run to run, for a chain alone or among others, and from the stateless and the handle forms. */
#define VH_TRAJ_HOLD   0
#define VH_TRAJ_REPEAT 1
#define VH_TRAJ_STEREO 0
#define VH_TRAJ_MONO   1
typedef struct vh_traj_params {
  int32_t on_fail;                   /* VH_TRAJ_HOLD / VH_TRAJ_REPEAT */
  int32_t reserved;                  /* 0 */
} vh_traj_params;
typedef struct vh_traj_pose {        /* 272 bytes, one per row */
  double  Tw_prev[16];               /* the pose before the row, row-major */
  double  Tw_cur[16];                /* the pose after it */
  int32_t status;                    /* 0 accepted, 1 ok == 0, 2 not finite, 3 elimination refused, 4 row without a pair */
  int32_t step;                      /* accepted rows of the chain so far, this one included */
  int32_t reserved[2];               /* 0 */
} vh_traj_pose;
typedef struct vh_traj_carry {       /* 272 bytes, one per chain */
  double  Tw[16];                    /* the last Tw_cur */
  double  Tinv[16];                  /* the last accepted Tinv (zeros while has_tinv == 0) */
  int32_t step;
  int32_t has_tinv;                  /* 0: no row of the chain was accepted yet */
  int32_t reserved[2];               /* 0 */
} vh_traj_carry;
void vh_default_traj_params(vh_traj_params *tp);   /* VH_TRAJ_HOLD */
/* Stateless, host pointers: n_chains chains, chain c the rows [offsets[c], offsets[c + 1]) of tr[.][6], ok[.] and out[.]
 * (offsets as vh_motion_inliers': offsets[0] >= 0, not decreasing; an empty chain is allowed and only copies its start to
 * carry_out).  A chain starts from carry_in[c] where carry_in is given (T0 is then not read), else from T0[c] (NULL: the
 * unit matrix) with step 0 and no accepted Tinv.  carry_out (nullable) [n_chains].  One workgroup walks a chain in rounds
 * of VH_TRAJ_ROUND rows (csrc/vh_trajectory.h).  VH_ERR_INVALID_ARG: null tp / offsets / (with rows) tr, ok, out;
 * on_fail outside the two policies; n_chains < 0.  VH_ERR_UNSUPPORTED: more than 2^24 chains.  n_chains == 0: VH_OK;
 * no rows at all: VH_OK, carry_out filled on the host; neither launches anything nor needs a device. */
int32_t vh_trajectory(const vh_traj_params *tp, int32_t device, int32_t n_chains, const int32_t *offsets, const double *tr,
                      const int32_t *ok, const double *T0, const vh_traj_carry *carry_in, vh_traj_pose *out,
                      vh_traj_carry *carry_out);
/* Handles, opt-in, before the first push only (VH_ERR_STATE afterwards); tp == NULL switches the feature off.  T0: the
 * start pose of every stream [S][16] (a sequence handle and a lone matcher: one, [16]; NULL: the unit matrix).  A plain
 * group is S chains that advance one row per pair; a sequence handle is ONE chain over the rows of its chunks
 * (vh_sequence_set_trajectory; VH_ERR_UNSUPPORTED from vh_group_set_trajectory on it and the reverse).  Off (the default):
 * nothing is allocated or launched and vh_group_device_bytes is unchanged.  On: the first vh_group_trajectory adds one
 * block, counted by vh_group_device_bytes: 272 bytes per stream / row of poses and 2 x 272 bytes per chain of carries
 * (base and current), each of the three arrays rounded up to 256 bytes. */
int32_t vh_group_set_trajectory(vh_group *g, const vh_traj_params *tp, const double *T0);
int32_t vh_sequence_set_trajectory(vh_group *g, const vh_traj_params *tp, const double *T0);
int32_t vh_set_trajectory(vh_matcher *m, const vh_traj_params *tp, const double *T0);
/* One step of every chain under the motion the device holds for the current classification; nothing goes up; out
 * (nullable) [S] comes back; synchronous.
 *   VH_TRAJ_STEREO: the tr / ok the current STEREO classification was made under (after
 *     vh_group_refit_motion(reclassify = 1) the refined motion); VH_ERR_STATE wherever vh_group_scene_points_stereo
 *     returns it.
 *   VH_TRAJ_MONO: the tr / ok the last vh_group_pose_mono / _refined left on the device for the current MONO
 *     classification; VH_ERR_STATE wherever vh_group_scene_points_mono returns it.
 * The step belongs to the pushed pair and is idempotent: the first call behind a push latches base = current, and every
 * call computes current = step(base) -- a repeated call, e.g. after a refit or after matching the pair again, recomputes
 * the step instead of stepping twice.  A replace push undoes the step of the pair it replaces (current = base).  On a
 * sequence handle one call walks the rows of the chunk as one chain: row 0 continues the previous chunk's last row, rows
 * without a pair get status 4.  VH_ERR_STATE with the switch off; source outside the two: VH_ERR_INVALID_ARG.  A refused
 * allocation is VH_ERR_HIP before any launch and leaves the handle as it was.  Profile scope: "trajectory". */
int32_t vh_group_trajectory(vh_group *g, int32_t source, vh_traj_pose *out);
int32_t vh_match_trajectory(vh_matcher *m, int32_t source, vh_traj_pose *out);
/* The records of the last vh_group_trajectory call (a sequence handle: one per row), valid until the next push or
 * vh_group_set_pose (VH_ERR_STATE otherwise, and with the switch off).  _device: the array itself, *stride in records. */
int32_t vh_group_get_poses(vh_group *g, vh_traj_pose *out);
int32_t vh_get_pose(vh_matcher *m, vh_traj_pose *out);
int32_t vh_group_poses_device(vh_group *g, const vh_traj_pose **d_poses, int64_t *stride);
/* Re-anchoring: the chain of `stream` (a sequence handle: 0) continues from T[16] with step 0 and no accepted Tinv; base
 * and current are both set, the records of the last call become stale.  VH_ERR_STATE with the switch off. */
int32_t vh_group_set_pose(vh_group *g, int32_t stream, const double *T);
/* vh_group_scene_points_stereo / _mono with Tw taken from the trajectory's poses on the device: Tw_prev where
 * sp->frame == 0, Tw_cur where it is 1 (a device-to-device copy of the chosen matrices; nothing goes up).
 * VH_ERR_STATE unless vh_group_trajectory ran behind the current match call, under the current classification and from
 * the source of the same kind (a classification made after the step -- another vh_group_motion_inliers, a refit with
 * reclassify -- makes the poses stale: step again); otherwise everything as the plain entries, and vh_group_landmarks
 * works unchanged behind them. */
int32_t vh_group_scene_points_stereo_world(vh_group *g, const vh_ego_params *e, const vh_scene_params *sp, int32_t *counts);
int32_t vh_group_scene_points_mono_world(vh_group *g, const vh_mono_params *e, const vh_scene_params *sp, int32_t *counts);
int32_t vh_match_scene_points_stereo_world(vh_matcher *m, const vh_ego_params *e, const vh_scene_params *sp, int32_t *count);
int32_t vh_match_scene_points_mono_world(vh_matcher *m, const vh_mono_params *e, const vh_scene_params *sp, int32_t *count);

/* ---- pose covariance: the uncertainty of the trajectory's pose, propagated along the chains (csrc/kernels_trajectory_cov.hip) ----
 * Stereo source only.  The uncertainty of a pose P is a right (camera-frame) perturbation, P_true = P * Exp(xi),
 * xi = (phi_x, phi_y, phi_z, rho_x, rho_y, rho_z), Sigma = E[xi xi^T], 6x6 row-major.  The rule has one copy,
 * csrc/vh_trajectory_cov.h; all arithmetic in double, every product and sum rounded on its own.  One accepted row with tr,
 * R = the estimators' rotation of tr, t = tr[3..5] and the motion's covariance C (vh_motion_covariance's, in the order of tr):
 *   1. G (6x6) maps a change of tr to the right perturbation of T(tr): column k of the upper-left 3x3 block is
 *      vee(R^T dR_k) with dR_k the derivative of R by tr[k] and vee(W) = (W[2][1], W[0][2], W[1][0]); the lower-right block
 *      is R^T; the rest is zero.
 *   2. Q = G C G^T: W = G C in full (c = 0; c += G[i][k] * C[k][j], k = 0..5), Q[i][j] = sum_k W[i][k] * G[j][k] for i <= j,
 *      mirrored.
 *   3. Ad = [[R, 0], [[t]x R, R]], [t]x the cross-product matrix.
 *   4. S = Sigma + Q; U = Ad S (k = 0..5, all six terms); Sigma'[i][j] = sum_k U[i][k] * Ad[j][k] for i <= j, mirrored:
 *      Sigma' = Ad (Sigma + Q) Ad^T, which is what P' = P * inv(T) does to a right perturbation.
 * Which rows step is the pose chain's: status and step of a record equal the pose record's.  A row that holds keeps Sigma.
 * A step without a covariance of its own -- a row repeated under VH_TRAJ_REPEAT, or an accepted row whose ok_cov is 0 or
 * whose C or Q holds a value that is not finite -- steps with the Ad it steps with (its own; repeated: the last accepted
 * one), adds fill_scale * Q_last, Q_last being the Q of the chain's last step that had its own (zero before any), and
 * counts in n_filled: n_filled > 0 reads "this covariance is a lower bound". */
typedef struct vh_traj_cov_params {
  double  fill_scale;                /* finite, >= 0 */
  int32_t reserved[2];               /* 0 */
} vh_traj_cov_params;
typedef struct vh_traj_cov {         /* 304 bytes, one per row */
  double  cov[36];                   /* Sigma behind the row, row-major, exactly symmetric */
  int32_t status;                    /* the pose record's */
  int32_t step;                      /* the pose record's */
  int32_t n_filled;                  /* steps of the chain so far without a covariance of their own */
  int32_t reserved;                  /* 0 */
} vh_traj_cov;
typedef struct vh_traj_cov_carry {   /* 880 bytes, one per chain */
  double  cov[36];                   /* the last Sigma */
  double  Ad_last[36];               /* Ad of the last accepted row (zeros while has_ad == 0) */
  double  Q_last[36];                /* Q of the last step that had its own (zeros while has_q == 0) */
  int32_t n_filled;
  int32_t has_ad;                    /* the pose carry's has_tinv */
  int32_t has_q;
  int32_t step;                      /* the pose carry's step: what the records' step goes on from */
} vh_traj_cov_carry;
void vh_default_traj_cov_params(vh_traj_cov_params *tcp);   /* fill_scale 1.0 */
/* Stateless, host pointers: chains as vh_trajectory's; cov[rows][36] and ok_cov[rows] are the rows' motion covariances
 * (vh_motion_covariance's cov and ok_out).  A chain starts from carry_in[c] where given, else from Sigma0[c] (NULL: zero)
 * with n_filled 0, step 0 and neither Ad_last nor Q_last.  carry_out (nullable) [n_chains].  One workgroup walks a chain in rounds
 * of VH_TRAJ_COV_ROUND rows (csrc/vh_trajectory_cov.h).  VH_ERR_INVALID_ARG: null tp / tcp / offsets / (with rows) tr, ok,
 * cov, ok_cov, out; on_fail outside the two policies; fill_scale negative or not finite; n_chains < 0.
 * VH_ERR_UNSUPPORTED: more than 2^24 chains.  n_chains == 0: VH_OK; no rows at all: VH_OK, carry_out filled on the host;
 * neither launches anything nor needs a device. */
int32_t vh_trajectory_cov(const vh_traj_params *tp, const vh_traj_cov_params *tcp, int32_t device, int32_t n_chains,
                          const int32_t *offsets, const double *tr, const int32_t *ok, const double *cov, const int32_t *ok_cov,
                          const double *Sigma0, const vh_traj_cov_carry *carry_in, vh_traj_cov *out, vh_traj_cov_carry *carry_out);
/* Handles, opt-in, before the first push only and only with the trajectory on (VH_ERR_STATE otherwise); tcp == NULL
 * switches it off.  Sigma0: the start covariance of every chain [chains][36] (NULL: zero), finite.  Off (the default):
 * nothing is allocated or launched.  On: vh_group_trajectory / vh_match_trajectory run both kernels in the one call.
 * VH_TRAJ_MONO is then VH_ERR_UNSUPPORTED, and VH_TRAJ_STEREO needs the motion covariance of the current classification
 * on the device -- vh_group_motion_covariance(tr = NULL) behind the current match call and the current classification
 * -- else VH_ERR_STATE before any launch or latch, the handle as it was.  The covariance carries latch, step and go
 * stale with the pose carries.  The first call adds one block, counted by vh_group_device_bytes: 304 bytes per stream /
 * row of records and 2 x 880 bytes per chain of carries, each of the three arrays rounded up to 256 bytes; a refused
 * allocation is VH_ERR_HIP before any launch and leaves the poses' state as it was.  Profile scope: "trajectory_cov". */
int32_t vh_group_set_trajectory_covariance(vh_group *g, const vh_traj_cov_params *tcp, const double *Sigma0);
int32_t vh_sequence_set_trajectory_covariance(vh_group *g, const vh_traj_cov_params *tcp, const double *Sigma0);
int32_t vh_set_trajectory_covariance(vh_matcher *m, const vh_traj_cov_params *tcp, const double *Sigma0);
/* The records of the last vh_group_trajectory call: VH_ERR_STATE where vh_group_get_poses returns it, or with the
 * covariance off.  _device: the array itself, *stride in records. */
int32_t vh_group_get_pose_covariances(vh_group *g, vh_traj_cov *out);
int32_t vh_get_pose_covariance(vh_matcher *m, vh_traj_cov *out);
int32_t vh_group_pose_covariances_device(vh_group *g, const vh_traj_cov **d_cov, int64_t *stride);
/* The chain of `stream` continues from Sigma[36] (finite) with n_filled 0; Ad_last and Q_last stay.  Base and current are
 * both set, the records of the last call become stale.  (vh_group_set_pose also resets the chain's covariance: zero, and
 * neither Ad_last nor Q_last.)  VH_ERR_STATE with the covariance off. */
int32_t vh_group_set_pose_covariance(vh_group *g, int32_t stream, const double *Sigma);

/* ---- the same chain ON THE DEVICE: no host work between matching and the pose (csrc/kernels_vote.hip) ----
 * removeOutliers' Delaunay triangulation is a sequential chain per match list (csrc/sweep_hull.h); on the GPU a list
 * takes tens of milliseconds as one lane, and the throughput comes from the lists in flight:
 *   vh_group_post_device_config  steps_per_batch (1..256) steps are voted on by one kernel sequence (steps_per_batch * S
 *                         lists, at most 65 535: beyond that vh_group_post_begin_device returns VH_ERR_UNSUPPORTED), up to `batches` (1..64) such batches are in flight on low-priority streams beside the
 *                         matcher's own kernels; lanes_per_wave (1..64) lists share a wavefront.  Default 64, 3, 16 (a batch takes
 *                         0.4-0.5 s whatever its size: the rate is steps in flight over that latency).
 *                         VH_ERR_STATE while steps are in flight.
 *                         Device memory of the ring: batches * steps_per_batch * S lists, each 176 bytes per record slot
 *                         (cap_per_stream slots: the record, its point, votes, order, a 16-byte hull node, six 16-byte
 *                         half-edge records) + 48 bytes per bucketed output record + the estimator's scratch -- 2.0 MB per
 *                         KITTI list of 11 363 slots.  The first vh_group_post_begin_device sizes the ring against the
 *                         device's free memory: steps_per_batch is halved until the ring fits 80 % of it, and
 *                         VH_ERR_CAPACITY is returned -- before anything has moved -- if one step per batch does not.
 *   vh_group_post_begin_device   after vh_group_match_features: the step's S lists leave the matcher's buffer for the
 *                         current batch (a device-to-device move; the matcher can go on at once); a full batch is launched:
 *                         vote -> Matcher::bucketFeatures(max_features, bucket_width, bucket_height) (bucket sides >= 1 px)
 *                         -> the stereo estimator (e, rand3[S][ransac_iters][3]) or the monocular one (mono,
 *                         rand8[S][ransac_iters][8]) or neither.  want_lists: keep the bucketed lists for the finish call.
 *                         All steps of a batch share one configuration (a different one closes the batch early).
 *   vh_group_post_finish_device  the step begun `age` begins ago (0: the last): waits for its batch (launching it first if it
 *                         is not full yet), then tr[S][6], ok[S], n_inliers[S] (with an estimator), counts[S] (nullable) and
 *                         bucketed[S][cap_per_stream] (nullable; needs want_lists) as vh_group_post_finish.  A caller that
 *                         finishes step t - steps_per_batch * (batches - 1) after beginning step t never waits for the vote.
 *                         Every step begun must be finished before the ring of steps_per_batch * batches steps comes
 *                         round (VH_ERR_STATE from the begin call otherwise).  A stream whose list was refused
 *                         (truncated: VH_ERR_CAPACITY; NaN / negative coordinates or an exhausted flip stack:
 *                         VH_ERR_UNSUPPORTED) reports ok = 0, n_inliers = 0, tr = 0, counts = -1; the other streams of
 *                         the step are delivered as usual and the call returns the error code.
 * Results per stream are those of vh_group_post_finish: lists and flags bit for bit, tr to rounding. */
int32_t vh_group_post_device_config(vh_group *g, int32_t steps_per_batch, int32_t batches, int32_t lanes_per_wave);
int32_t vh_group_post_begin_device(vh_group *g, int32_t cap_per_stream, int32_t max_features, float bucket_width, float bucket_height,
                                   const vh_ego_params *e, const int32_t *rand3, const vh_mono_params *mono, const int32_t *rand8,
                                   int32_t want_lists);
int32_t vh_group_post_finish_device(vh_group *g, int32_t age, double *tr, int32_t *ok, int32_t *n_inliers, vh_p_match *bucketed,
                                    int32_t cap_per_stream, int32_t *counts);

/* ---- dense inliers and the motion refit as stages of the device post chain ----
 * vh_group_motion_inliers(_mono) and vh_group_refit_motion work on the lists of the handle's last match call; in the
 * device post chain a step's lists leave the matcher's buffer at once and its motion arrives steps_per_batch * batches
 * steps later.  With a dense mode set, the batch itself classifies the VOTED list of every stream (what vote_select
 * leaves compacted in the batch: the list removeOutliers returns, before bucketFeatures) under the motion its
 * estimator found, behind the estimator on the batch's own stream: no host round trip, no upload.
 *   vh_group_post_device_dense   mode 0: off (the default: every call allocates, launches and returns what it did
 *                         without this entry); 1: classify every voted list under the batch's motion -- tr / ok of
 *                         the stereo estimator (getInlier, as vh_motion_inliers), or the model / ok of the monocular
 *                         one (as vh_motion_inliers_mono; the estimator's vh_mono_model becomes an output of the
 *                         batch); 2: mode 1, then the refit of vh_refit_motion on the compacted inliers from the
 *                         batch's tr / ok; 3: mode 2, then the classification again under tr_refit / ok_refit (as
 *                         reclassify = 1 of vh_group_refit_motion).  VH_ERR_INVALID_ARG outside 0..3; VH_ERR_STATE
 *                         while steps are in flight; a change of mode releases the ring (as
 *                         vh_group_post_device_config), and the next begin call sizes it again.
 *                         With mode >= 1 vh_group_post_begin_device returns VH_ERR_INVALID_ARG when no estimator is
 *                         given and, with mode >= 2, when the estimator is the monocular one (the reference has no
 *                         mono refit); VH_ERR_UNSUPPORTED when steps_per_batch * S lists of cap_per_stream records
 *                         exceed the classification's launch grid (2^24 tiles of 1 024 records).  The mode is part
 *                         of a batch's configuration.
 *                         Device memory: per batch 53 bytes per record slot (flag, compacted record, position),
 *                         4 bytes per tile of 1 024 slots and about 100 bytes per list (+ 128 per list for the mono
 *                         model), in a block beside the batch's own; it is part of the ring the first begin call
 *                         sizes against 80 % of the free memory, counted by vh_group_device_bytes, allocated before
 *                         the batch's first launch (a refusal is VH_ERR_HIP, nothing has moved, the begin call can
 *                         be repeated) and released with the ring.
 *                         Profile scopes (on the batch's stream): "inlier_flag" / "inlier_flag_mono",
 *                         "inlier_compact", "motion_refit", "post_dense_gate".
 *   vh_group_post_finish_device_dense   vh_group_post_finish_device with one more argument; d = NULL, or a struct of
 *                         NULLs, is that call.  tr, ok, n_inliers, bucketed, counts and the return value are those
 *                         of vh_group_post_finish_device in every mode, bit for bit.
 * vh_post_dense: nullable output pointers, each for this step's S streams.  Ten pointers in the order below: 80 bytes,
 * member k at offset 8 k. */
typedef struct vh_post_dense {
  /* with the batch's results (a few bytes per list) */
  int32_t *voted_counts;    /* [S] records of the voted list; mode >= 1 */
  int32_t *inlier_counts;   /* [S] inliers (mode 3: of the second classification); mode >= 1 */
  double *tr_refit;         /* [S][6]; mode >= 2; zero where ok_refit = 0 */
  int32_t *ok_refit;        /* [S]; mode >= 2; 0: ok = 0, fewer than six inliers, or the refit failed */
  int32_t *n_updates;       /* [S]; mode >= 2 */
  vh_mono_model *model;     /* [S]; mode >= 1 with the monocular estimator */
  /* per record: copied for this step's lists out of the batch's buffers when the call is made (they stay valid until
   * the ring comes round to the batch); [S][cap_per_stream], list s at s * cap_per_stream; mode >= 1 */
  vh_p_match *voted_pm;     /* the voted lists */
  uint8_t *flags;           /* one byte per voted record (mode 3: of the second classification) */
  vh_p_match *inlier_pm;    /* the inliers in list order */
  int32_t *src_pos;        /* the position of each inlier in its voted list */
} vh_post_dense;
/* VH_ERR_STATE when d asks for an output the step's mode did not produce (checked first: the step stays open and
 * can be finished again); VH_ERR_INVALID_ARG for a per-record output with cap_per_stream < 1.
 * A voted list (voted_pm, flags) or an inlier list (inlier_pm, src_pos) longer than cap_per_stream: that stream's
 * voted_counts and inlier_counts are -1, nothing of it is copied, the other streams are delivered and the call
 * returns VH_ERR_CAPACITY.  A stream whose list the vote refused takes part in nothing: voted_counts = inlier_counts
 * = -1, ok_refit = 0, tr_refit = 0, n_updates = 0, a zeroed model, and the call returns the refusal's code as
 * vh_group_post_finish_device does.  A list with ok = 0 has no inliers (its tr / model is not read), and fewer than
 * six inliers give ok_refit = 0: the stateless contracts.  Sequence handles as vh_group_post_begin_device. */
int32_t vh_group_post_device_dense(vh_group *g, int32_t mode);
int32_t vh_group_post_finish_device_dense(vh_group *g, int32_t age, double *tr, int32_t *ok, int32_t *n_inliers, vh_p_match *bucketed,
                                          int32_t cap_per_stream, int32_t *counts, const vh_post_dense *d);

/* ---- the covariance, the mono refit and the mono pose as stages of the device post chain ----
 * vh_group_motion_covariance, vh_group_refit_model_mono, vh_group_pose_mono and vh_group_pose_mono_refined work on the
 * lists of the handle's last match call, which the pipelined chain has overwritten long before a batch's motion arrives.
 * With a tail mask set the batch runs the same kernels over its own inlier lists, on its vote stream behind the dense
 * stages and before the small downloads: no new stream, no event, no host wait, no upload.
 *   vh_group_post_device_tail    stages: a mask of the bits below; 0 is the default, and with it every call allocates,
 *                         launches and returns what it did without this entry.
 *                           VH_POST_TAIL_COV          stereo estimator, dense mode >= 1: the covariance of
 *                               vh_motion_covariance over the batch's final inlier lists under the batch's final motion --
 *                               mode 1: tr / ok of the estimator over the classification's inliers; mode 2: tr_refit /
 *                               ok_refit over the FIRST classification's inliers (the reclassify = 0 pairing of
 *                               vh_group_refit_motion + vh_group_motion_covariance); mode 3: tr_refit / ok_refit over
 *                               the second classification's.
 *                           VH_POST_TAIL_MONO_REFIT   mono estimator, dense mode 1: vh_refit_model_mono on the compacted
 *                               inliers from the estimator's model / ok, then the classification again under the
 *                               refitted model / its ok (reclassify = 1 of vh_group_refit_model_mono).  The counts,
 *                               flags, records and positions vh_post_dense hands out are then the second
 *                               classification's; vh_post_dense::model stays the estimator's.
 *                           VH_POST_TAIL_MONO_POSE    mono estimator, dense mode 1: vh_pose_mono over the final inlier
 *                               lists under the model they were classified under (the refitted one with
 *                               VH_POST_TAIL_MONO_REFIT, else the estimator's).
 *                           VH_POST_TAIL_MONO_REFINE  with VH_POST_TAIL_MONO_POSE: the pose is vh_pose_mono_refined's.
 *                         VH_ERR_INVALID_ARG for an unknown bit or REFINE without POSE; VH_ERR_STATE while steps are in
 *                         flight; a change of the mask releases the ring (as vh_group_post_device_dense), and the next
 *                         begin call sizes it again.  The mask is part of a batch's configuration.
 *                         With a mask set vh_group_post_begin_device returns VH_ERR_INVALID_ARG when the dense mode is
 *                         0, when COV is set without the stereo estimator, and when any other bit is set without the
 *                         mono estimator; VH_ERR_UNSUPPORTED when POSE is set and steps_per_batch * S lists of
 *                         ceil(cap_per_stream / 64) workgroups reach 2^30 (the pose's per-record launches) -- a limit
 *                         the dense mode's own (2^24 tiles of 1 024 records, above) is reached long before, so today
 *                         the dense mode's refusal is the one a caller meets.
 *                         Device memory, per batch, in a block beside the dense stages': per list 300 bytes (COV), 148
 *                         (MONO_REFIT), 972 (MONO_POSE: tr, ok, vh_mono_pose and the 768-byte header) and 288
 *                         (MONO_REFINE), each array rounded up to 256 bytes, and with MONO_POSE 16 bytes per record
 *                         slot.  It is part of the ring the first begin call sizes against 80 % of the free memory,
 *                         counted by vh_group_device_bytes, allocated before the batch's first launch (a refusal is
 *                         VH_ERR_HIP, nothing has moved, the begin call can be repeated) and released with the ring.
 *                         Profile scopes (on the batch's stream): "motion_cov", "mono_refit", "mono_pose_head" ..
 *                         "mono_pose_finish", "mono_pose_refine", and the classification's once more with MONO_REFIT.
 *   vh_group_post_device_shape   the ring's shape in effect: the steps per batch and the batches of
 *                         vh_group_post_device_config, the steps per batch as the first begin call of a ring left
 *                         them.  The configured value is an upper bound -- that call halves it until the ring fits
 *                         80 % of the free device memory, and the tail's block makes that likelier; before it, this
 *                         returns the configured shape.  A caller sizes its lead (steps_per_batch * (batches - 1)) by it.
 *   vh_group_post_finish_device_tail   vh_group_post_finish_device_dense with one more argument; t = NULL, or a struct
 *                         whose pointers are all NULL, is that call: tr, ok, n_inliers, bucketed, counts, every output
 *                         of d and the return value are the same bits under any mask (with MONO_REFIT the
 *                         classification d hands out is the second one, see above).
 * vh_post_tail: nullable output pointers, each for this step's S streams, behind the size the caller compiled:
 * 88 bytes, pointer k at offset 8 + 8 k.  Members beyond `size` are not read, so a later, longer struct stays compatible. */
#define VH_POST_TAIL_COV 1u
#define VH_POST_TAIL_MONO_REFIT 2u
#define VH_POST_TAIL_MONO_POSE 4u
#define VH_POST_TAIL_MONO_REFINE 8u
#define VH_POST_TAIL_ALL 15u
typedef struct vh_post_tail {
  uint32_t size;            /* sizeof(vh_post_tail) as the caller compiled it; members beyond it are not read */
  uint32_t reserved;        /* 0 */
  double *cov;              /* [S][36]  VH_POST_TAIL_COV; row-major, zero where ok_cov = 0 */
  double *ssr;              /* [S]      VH_POST_TAIL_COV */
  int32_t *ok_cov;          /* [S]      VH_POST_TAIL_COV */
  vh_mono_model *model_refit; /* [S]    VH_POST_TAIL_MONO_REFIT; the zero record where ok_model = 0 */
  int32_t *ok_model;        /* [S]      VH_POST_TAIL_MONO_REFIT */
  double *w;                /* [S][2]   VH_POST_TAIL_MONO_REFIT */
  double *tr_pose;          /* [S][6]   VH_POST_TAIL_MONO_POSE */
  int32_t *ok_pose;         /* [S]      VH_POST_TAIL_MONO_POSE */
  vh_mono_pose *pose;       /* [S]      VH_POST_TAIL_MONO_POSE */
  vh_mono_refine *refine;   /* [S]      VH_POST_TAIL_MONO_REFINE */
} vh_post_tail;
/* VH_ERR_INVALID_ARG for a size below 8 or not 8 + a multiple of 8.  VH_ERR_STATE when t asks for an output the step's
 * mask did not produce (checked first, with d's: the step stays open and can be finished again).  Every output came
 * down with the batch's results: nothing is copied per record.  A refused refinement is not a refused pose (as
 * vh_pose_mono_refined: refine[s].status says why, and the pose is the plain one).  A stream whose list the vote
 * refused takes part in nothing: its tail outputs are the zero records with ok = 0, and the call returns the
 * refusal's code as vh_group_post_finish_device does.  Sequence handles as vh_group_post_begin_device. */
int32_t vh_group_post_device_tail(vh_group *g, uint32_t stages);
int32_t vh_group_post_device_shape(vh_group *g, int32_t *steps_per_batch, int32_t *batches);
int32_t vh_group_post_finish_device_tail(vh_group *g, int32_t age, double *tr, int32_t *ok, int32_t *n_inliers, vh_p_match *bucketed,
                                         int32_t cap_per_stream, int32_t *counts, const vh_post_dense *d, const vh_post_tail *t);

/* vh_group_post_finish with the MONOCULAR estimator as its last stage: what VisualOdometryMono::process runs
 * after the matching (src/viso_mono.cpp:34-37: bucketFeatures, then estimateMotion on the bucketed list; the
 * Delaunay vote before them is the tail of matchFeatures) for every stream of a group, flow or quad lists,
 * rand8[S][ransac_iters][8].  Everything else as vh_group_post_finish. */
int32_t vh_group_post_finish_mono(vh_group *g, int32_t age, int32_t max_features, float bucket_width, float bucket_height,
                                  int32_t host_threads, const vh_mono_params *e, const int32_t *rand8, double *tr,
                                  int32_t *ok, int32_t *n_inliers, vh_p_match *bucketed, int32_t cap_per_stream,
                                  int32_t *counts, double *host_ms);

/* ---- reconstruction: 3-d points from lost feature tracks (csrc/kernels_recon.hip) ----------------- */

/* Reconstruction's calibration and the four thresholds of Reconstruction::update (src/reconstruction.h:55, :66). */
typedef struct vh_recon_params {
  double f, cu, cv;          /* setCalibration: focal length, principal point (pixels) */
  int32_t point_type;        /* 0 = everything, 1 = road and above, 2 = only above the road */
  int32_t min_track_length;  /* frames a feature must have been tracked for; negative: every track is SHORT (the reference
                                compares it with pixels.size() unsigned, src/reconstruction.cpp:131) */
  double max_dist;           /* largest distance from the camera of the track's middle frame (meters) */
  double min_angle;          /* smallest angle between the first and the last ray (degrees) */
} vh_recon_params;
/* f = 1, cu = cv = 0 (the constructor's K = eye(3)); 1, 2, 30, 2 (src/reconstruction.h:66). */
void vh_default_recon_params(vh_recon_params *r);

/* What became of a track, in the order Reconstruction::update tests (src/reconstruction.cpp:131-141). */
#define VH_RECON_ACCEPTED 0
#define VH_RECON_SHORT 1         /* fewer than min_track_length frames */
#define VH_RECON_INFINITY 2      /* initPoint false: |w| < 1e-10 */
#define VH_RECON_TYPE 3          /* pointType < point_type (-1: not more than 1 m in front of the first or the last camera) */
#define VH_RECON_NOT_REFINED 4   /* refinePoint false: a projection with c*c < 1e-10, a singular system, no convergence in 22 updates */
#define VH_RECON_FAR_OR_NARROW 5 /* pointDistance >= max_dist or rayAngle <= min_angle */

/* What Reconstruction::update computes for every lost track (src/reconstruction.cpp:131-142: initPoint, pointType,
 * refinePoint, pointDistance, rayAngle), for n_tracks tracks of one drive in ONE launch, one GPU lane per track.
 * The drive has frames 0 .. n_frames-1; Tr[k] (row-major 4x4) is the Tr handed to update number k, the motion frame
 * k -> k+1 (src/viso.h:80-86).  The per-frame tables Tr_total, Tr_inv_total, P_total are built on the host from r and
 * Tr exactly as the constructor, setCalibration and update build them (src/reconstruction.cpp:27-70).  A singular Tr
 * is not an error: Matrix::inv hands out what its elimination left, and the tracks that read it fail the kernel's tests.
 * Track t was seen in frames first_frame[t] .. first_frame[t] + len - 1, len = offsets[t+1] - offsets[t], at
 * pixels[offsets[t] ..][2] = (u, v) per frame.  Association (which match extends which track) stays with the caller:
 * include/viso_hip_reconstruction.hpp and the Python package restate Reconstruction::update's.
 * Outputs, in input order: status[t] = VH_RECON_*; points[t][3] = the point as the reference's `p` stood when the track's
 * fate was decided (ACCEPTED, FAR_OR_NARROW: refined; NOT_REFINED: after the last update; TYPE: initPoint's; SHORT,
 * INFINITY: 0); metrics[t][2] (nullable) = (pointDistance, rayAngle) for ACCEPTED and FAR_OR_NARROW, else 0.
 * points and metrics[.][0] equal the reference's bit for bit; the ray angle uses the device's acos and agrees to rounding,
 * so a track whose angle lies within rounding of min_angle may be classified differently.
 * VH_ERR_INVALID_ARG: null pointers, n_frames < 1, n_tracks < 0, offsets[0] < 0, a track with len < 1, first_frame < 0 or
 * first_frame + len > n_frames.  n_tracks == 0: VH_OK, nothing is launched and no device is needed.
 * Stateless: device buffers live for the call, and the tables of ALL n_frames frames are rebuilt on the host on every
 * call -- two 4x4 Gauss-Jordan inversions and two products per frame, a third of a microsecond -- and uploaded (256 bytes per
 * frame).  A caller that runs one call per update of a drive of N updates pays O(N^2) of that in total (N = 10 000:
 * some twenty seconds over the drive); one call per chunk of k updates (updateMany of the classes) divides it by k. */
int32_t vh_reconstruct_tracks(const vh_recon_params *r, int32_t device, int32_t n_frames, const double *Tr, int32_t n_tracks,
                              const int32_t *first_frame, const int32_t *offsets, const float *pixels, float *points, int32_t *status,
                              double *metrics);
/* Device time in milliseconds of the kernel of this thread's last successful vh_reconstruct_tracks (HIP events around the
 * launch; transfers excluded), -1 before the first.  A permanent part of the ABI, the counterpart of sweep_ms of
 * vh_remove_outliers_device and of vh_group_profile_read for the handles: the entry is synchronous and owns its buffers,
 * so a caller's own events could only time the whole call, transfers included.  Its price is two events per call
 * (microseconds beside the call's seven transfers) and one thread-local double; tools/reconstruct_rate.py reads it. */
double vh_reconstruct_last_kernel_ms(void);

/* ---- reconstruction on a sequence handle: lost tracks gathered on the device (csrc/kernels_recon_gather.hip, DESIGN.md
 * section 4.8).  The handle already holds the match lists and their vh_track chains on the device; with this switch it
 * also keeps a ring of compact records (32 bytes per match record: the four left-camera floats, prev, age, birth_pos and
 * a "continued" mark) for the lists of the last history_frames + max_frames frames, and vh_sequence_reconstruct turns
 * every track that ended into one vh_recon_track without moving a list to the host.
 *   Contract: THE LINK RULE of vh_track above decides which record continues which.  Reconstruction::update
 *   (src/reconstruction.cpp:75-145) extends a track when a match's i1p equals the track's last_idx: the first match in
 *   list order with a given i1p continues the track, a second one starts a new track, and of two tracks ending in the
 *   same feature the later one in track order wins.  Track order is (birth update, position in that list), so lost tracks
 *   leave an update in ascending (birth_frame, birth_pos).  The link rule agrees on the first point and on the order; it
 *   differs only when a predecessor list holds the same i1c twice (the link rule takes the lowest position, the reference
 *   the later track).  The result equals Reconstruction::update point for point whenever every list's i1c values are
 *   distinct.
 *   Frames: reconstruction frame k is frame k of the sequence (vh_sequence_position).  The list of row r of a chunk pushed
 *   at position F is the list of the update whose current_frame is F + r, and Tr[r] is that update's Tr, the motion
 *   F+r-1 -> F+r.  A track whose last record sits in the list of frame c-1 and is continued by no record of the list of
 *   frame c is lost at frame c; it was seen in frames birth_frame-1 (the head's u1p, v1p) .. c-1, age + 1 frames.  The
 *   last list of a chunk stays pending until the next chunk's row 0 shows what it continues; tracks alive at the end of
 *   a drive are never emitted, as in the reference.
 *   History: a lost track with age > history_frames is not solved: status VH_RECON_HISTORY, zeros for point and metrics.
 *   Breaks: the reconstruction starts again, as a new Reconstruction constructed at the frame before the chunk's first
 *   list, when the chunk's dims differ, when a chunk in between was never matched, after a failed match call, when the
 *   previous chunk was matched but not reconstructed, and when a chunk is matched again after it was reconstructed.
 *   Pending tracks and the history are dropped, not solved.  A break also takes the predecessor away from the track
 *   linking: with reconstruction on, vh_track's birth and age start again wherever the reconstruction does.  Matching a
 *   chunk again BEFORE its reconstruct call only replaces its lists. */
#define VH_RECON_HISTORY 6       /* older than history_frames: not solved */
typedef struct vh_recon_track {  /* 56 bytes */
  int64_t birth_frame;           /* (birth_frame, birth_pos): the vh_track id */
  int32_t birth_pos;
  int32_t frames;                /* age + 1 */
  int64_t lost_frame;
  int32_t status;                /* VH_RECON_* */
  float point[3];                /* as points of vh_reconstruct_tracks */
  double distance, angle;        /* as metrics of vh_reconstruct_tracks */
} vh_recon_track;
/* Before the first push only (VH_ERR_STATE afterwards); sequence handles only (VH_ERR_UNSUPPORTED on a plain group).
 * r == NULL switches the feature off; otherwise history_frames < 1 is VH_ERR_INVALID_ARG (there is no default).  It
 * switches track linking on; vh_group_set_track_linking(g, 0) returns VH_ERR_STATE while reconstruction is on.
 * Off (the default): nothing is allocated or launched.  On: 32 * max_matches bytes per ring slot, history_frames +
 * max_frames slots, plus the gather buffers (they grow with the lost tracks of a call), allocated by the first
 * vh_sequence_reconstruct and counted by vh_group_device_bytes. */
int32_t vh_sequence_set_reconstruction(vh_group *g, const vh_recon_params *r, int32_t history_frames);
/* The lost tracks of the chunk of the last match call: legal once per matched chunk, from the return of that match call
 * until the next match call -- also after the next chunk has been pushed, so that its detection runs beside this call;
 * otherwise VH_ERR_STATE.  Tr[rows][16]: one row-major motion per row of that chunk (rows that hold no pair are not read).
 * Synchronous: waits for the match and the linking, runs recon_store, recon_tails, recon_gather and recon_kernel, and keeps
 * the records, sorted by (lost_frame, birth_frame, birth_pos), until the next call.  *n_tracks = records, *n_accepted =
 * those with VH_RECON_ACCEPTED: their points, in order, are what the reference appends to `points` over the same updates.
 * A failed allocation returns VH_ERR_HIP and changes nothing: the call may be made again. */
int32_t vh_sequence_reconstruct(vh_group *g, const double *Tr, int32_t *n_tracks, int32_t *n_accepted);
/* The records of the last vh_sequence_reconstruct under the getters' capacity rule: VH_ERR_CAPACITY with the true count
 * in *n and the first cap records written. */
int32_t vh_sequence_get_recon_tracks(vh_group *g, vh_recon_track *out, int32_t cap, int32_t *n);
/* The same kernels on caller-owned lists (host pointers, laid out as for vh_link_tracks): a whole fresh drive in one call,
 * list l is update l of a new Reconstruction (the list of frame l + 1) and Tr[l] its Tr.  The history is n_lists deep, so
 * no record is VH_RECON_HISTORY; there is no carry.  The path for voted or bucketed lists.  Argument errors as
 * vh_link_tracks and vh_reconstruct_tracks; n_lists == 0: VH_OK, *n = 0, no device needed; capacity rule as above. */
int32_t vh_reconstruct_lists(const vh_recon_params *r, int32_t device, int32_t n_lists, const vh_p_match *pm, int64_t stride,
                             const int32_t *counts, int32_t n_index, const double *Tr, vh_recon_track *out, int32_t cap, int32_t *n);

/* ---- reconstruction on a group: S cameras stepped together, 3-d points per camera and step ----------
 * The sequence form above with a second axis: a step of the group is one frame of each of its S cameras, the ring keeps
 * history_steps + 1 steps of S lists, and ONE store, tails, gather and solve sequence per step serves all S streams.
 * Streams never interact: stream s's records over a drive are what the sequence form gives for stream s's own lists and
 * motions (the link rule, as stated above).
 *   Frames: frame k of stream s is the frame with push serial k (the serial vh_track.birth_frame counts in).  Stream s's
 *   list of a step is the update whose current_frame is that serial, and Tr[s] is its motion.  A track whose last record
 *   lies in the stream's previous list and that no record of this step's list continues is lost at this step: the previous
 *   step's lists are the pending ones.  The step of the first push holds no pair: its call reads no Tr and returns nothing.
 *   History: a lost track with age > history_steps is not solved (VH_RECON_HISTORY, zeros).
 *   Breaks are per group, as match calls are: the reconstruction of EVERY stream starts again -- pending tracks and the
 *   history dropped, not solved, and vh_track's birth and age starting again with it -- when dims change, when a step was
 *   pushed but never matched, after a failed match call, when a step was matched but not reconstructed, and when a step is
 *   matched again after it was reconstructed.  Matching a step again BEFORE its reconstruct call only replaces the lists.
 *   A replace push is a break as well: the linking contract gives the lists of a replaced frame no predecessor, and a push
 *   covers all S streams, so it breaks every stream of the group.
 * vh_group_set_reconstruction: plain groups only (VH_ERR_UNSUPPORTED on a sequence handle, which keeps its own entry);
 * before the first push only (VH_ERR_STATE afterwards); r == NULL switches the feature off; otherwise history_steps < 1 is
 * VH_ERR_INVALID_ARG.  It switches track linking on; vh_group_set_track_linking(g, 0) returns VH_ERR_STATE while it is on.
 * Off (the default): nothing is allocated or launched.  On: a ring of 32 * max_matches * S * (history_steps + 1) bytes and
 * a count per slot, allocated by the first vh_group_reconstruct, plus the gather buffers, which only grow; all counted by
 * vh_group_device_bytes. */
int32_t vh_group_set_reconstruction(vh_group *g, const vh_recon_params *r, int32_t history_steps);
/* The lost tracks of the step of the last match call, all streams: legal once per match call, from its return until the
 * next match call -- also after the next push; otherwise VH_ERR_STATE.  Tr[S][16]: one row-major motion per stream.
 * Synchronous.  *n_tracks / *n_accepted: the sums over the streams.  A failed allocation returns VH_ERR_HIP before any
 * host state changed: the call may be made again. */
int32_t vh_group_reconstruct(vh_group *g, const double *Tr, int32_t *n_tracks, int32_t *n_accepted);
/* Stream `stream`'s records of the last vh_group_reconstruct, sorted by (lost_frame, birth_frame, birth_pos), under the
 * getters' capacity rule: VH_ERR_CAPACITY with the true count in *n and the first cap records written. */
int32_t vh_group_get_recon_tracks(vh_group *g, int32_t stream, vh_recon_track *out, int32_t cap, int32_t *n);
/* Per stream the records and the accepted ones of the last vh_group_reconstruct ([S] each; either may be NULL). */
int32_t vh_group_get_recon_counts(vh_group *g, int32_t *n_tracks, int32_t *n_accepted);

/* Which form of the search loops the group currently runs and the last observed share of
 * queries the speculative form had to search again (-1 before the first report).  The
 * searches are exact either way; the library switches between a speculative loop (no accept
 * test per candidate, the winner verified afterwards) and the literal tested loop on that share
 * (DESIGN.md section 4.1).  VH_FLOW_TESTED=1 / 0 in the environment pins the choice. */
int32_t vh_group_search_stats(vh_group *g, int32_t *speculative, double *research_rate);

/* Test hook: the next device allocation the group makes fails (VH_ERR_HIP), once.  Lets the suite drive the error
 * paths of lazily allocated buffers (the flow method's pixel mask). */
int32_t vh_group_debug_fail_next_alloc(vh_group *g);
/* The same after `skip` (>= 0) more allocations have succeeded: a failure in the middle of a call that allocates several
 * buffers (the track tables, then the range tables of multi-stage matching). */
int32_t vh_group_debug_fail_alloc_after(vh_group *g, int32_t skip);
/* Test hook: the group form of the reconstruction kernels on caller-owned lists (host pointers), as vh_reconstruct_lists
 * is their sequence form.  n_streams cameras of n_lists lists each, stream s's list l at pm[(s * n_lists + l) * stride ..
 * + counts[s * n_lists + l]) with the motion Tr[s * n_lists + l]; every stream is a fresh drive of its own, and all of them
 * go through one store, tails, gather and solve sequence.  out receives the records stream after stream, each sorted;
 * n[n_streams] the counts; VH_ERR_CAPACITY if their sum exceeds cap (nothing is written then). */
int32_t vh_group_debug_reconstruct_lists(const vh_recon_params *r, int32_t device, int32_t n_streams, int32_t n_lists, const vh_p_match *pm,
                                         int64_t stride, const int32_t *counts, int32_t n_index, const double *Tr, vh_recon_track *out,
                                         int32_t cap, int32_t *n);
/* Test hook: flip-stack entries the device vote's sweep may hold per list (1..31; 0 restores the default, 31), process-wide.
 * With a small value ordinary match lists take the refusal path (VH_ERR_UNSUPPORTED for that list, see
 * vh_remove_outliers_device). */
int32_t vh_debug_vote_stack_slots(int32_t slots);
/* Kernel timing (HIP events recorded on the group's stream around every
 * kernel launch while enabled).  vh_group_profile_read returns the
 * accumulated milliseconds and launch count of kernel `name`
 * ("detect_nms", "emit_features", "bin_hist", "bin_scan", "bin_fill",
 *  "bin_sort", "match", "chain", "emit_matches"; with refinement > 0 also "refine_planes", "refine";
 *  with track linking "track_scatter", "track_link", "track_rank" and, once per chunk of a sequence handle, "track_carry";
 *  with reconstruction on a sequence handle "recon_store", "recon_tails", "recon_gather", "recon_solve", per vh_sequence_reconstruct,
 *  and the same four on a group, per vh_group_reconstruct;
 *  with multi-stage matching "ranged" (pass 2), the same names with the prefix "sparse_" for the sparse sets'
 *  detection and pass 1, and the host steps "sparse_vote_host", "statistics_host": wall-clock milliseconds;
 *  in its device mode those two record nothing and "sparse_vote" (the vote's kernels together), "prior_stats" take their place;
 *  "ego_kernel" per vh_group_estimate_motion, "inlier_flag" / "inlier_flag_mono" and "inlier_compact" per classification,
 *  "motion_refit" per vh_group_refit_motion, "motion_cov" per vh_group_motion_covariance, "mono_refit" per
 *  vh_group_refit_model_mono, "mono_pose_head", "mono_pose_tri", "mono_pose_front", "mono_pose_rank", "mono_pose_vote"
 *  and "mono_pose_finish" per vh_group_pose_mono, with "mono_pose_refine" per vh_group_pose_mono_refined;
 *  with vh_group_set_gain "gain_copy" per sub-batch of a push, and "gain_ratio", "gain_sum" per vh_group_gain(_indices))
 *  since the last reset. */
int32_t vh_group_profile_enable(vh_group *g, int32_t on);
int32_t vh_group_profile_read(vh_group *g, const char *name, double *ms, int64_t *launches);
int32_t vh_group_profile_reset(vh_group *g);

#ifdef __cplusplus
}
#endif
#endif /* VISO_HIP_H */
