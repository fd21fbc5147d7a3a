// engine_api.hip -- the extern "C" ABI declared in include/viso_hip.h, and the stateless primitives (engine.h).
#include "engine.h"

#include <mutex>
#include <thread>

namespace vh_engine {

struct Temp {  // transient one-stream group for the stateless entry points
  Group *gq = nullptr;
  ~Temp() { if (gq) { (void)gq->sync_all(); delete gq; } }
};
// A transient group never refines: none of the stateless entry points that use one has the images of a pair (vh_match
// matches caller-supplied features and must return the unrefined list, whatever p->refinement says), so refinement is
// cleared and no planes or refined-coordinate buffers are allocated or written.
int32_t temp_new(const vh_params *p, int32_t device, int32_t mf, int32_t mm, Temp &t) {
  if (!p) return VH_ERR_INVALID_ARG;
  vh_params q = *p;
  q.refinement = 0;
  return group_new(&q, device, 1, mf, mm, &t.gq);
}
// The set-up of the entries that search caller-supplied features: a transient group sized for the longest set (with
// room for as many matches, or none), allocated for dims with a line at least as long as the width, the sets loaded in order.
struct FeatureLoad { int32_t role; const int32_t *m; int32_t n; };
static int32_t temp_with_features(const vh_params *p, int32_t device, const int32_t dims[3], bool matches, std::initializer_list<FeatureLoad> sets, Temp &t) {
  int32_t rc, nmax = 64;
  for (const FeatureLoad &f : sets) nmax = std::max(nmax, f.n);
  if ((rc = temp_new(p, device, nmax, matches ? nmax : 1, t))) return rc;
  const int32_t d[3] = {dims[0], dims[1], std::max(dims[2], dims[0])};
  if ((rc = t.gq->ensure(d))) return rc;
  for (const FeatureLoad &f : sets)
    if ((rc = t.gq->load_features(f.role, f.m, f.n))) return rc;
  return VH_OK;
}

// host_threads < 1: one worker per hardware thread
static int32_t default_threads(int32_t host_threads) {
  return host_threads < 1 ? (int32_t)std::max(1u, std::thread::hardware_concurrency()) : host_threads;
}

// Device work buffer of the stateless estimators: one per device, grow-only, kept between calls (an allocation and its
// release cost more than the kernels of a bucketed batch).  Requests above 1 GiB are not kept.  The lock is held for the
// whole call: stateless estimates on one device run one at a time.  To a call its `need` bytes are a fresh buffer: with
// VH_POISON=1 (vh_poison.h) every take fills them, kept or not, so that nothing of the call before it can come back.
struct EgoWork {
  std::mutex mu;
  uint8_t *buf[16] = {};
  size_t bytes[16] = {};
};
static EgoWork g_ego_work;
struct EgoWorkLease {
  std::unique_lock<std::mutex> lock;
  uint8_t *d = nullptr;
  bool kept = false;
  hipError_t take(int32_t device, size_t need) {
    lock = std::unique_lock<std::mutex>(g_ego_work.mu);
    if (device >= 0 && device < 16 && need <= ((size_t)1 << 30)) {
      kept = true;
      if (g_ego_work.bytes[device] < need) {
        if (g_ego_work.buf[device]) (void)hipFree(g_ego_work.buf[device]);
        g_ego_work.buf[device] = nullptr; g_ego_work.bytes[device] = 0;
        const size_t want = need + need / 4;
        const hipError_t er = hipMalloc((void **)&g_ego_work.buf[device], want);
        if (er != hipSuccess) return er;
        g_ego_work.bytes[device] = want;
      }
      d = g_ego_work.buf[device];
      return vh_poison_device(d, need);
    }
    const hipError_t er = hipMalloc((void **)&d, need);
    if (er != hipSuccess) { d = nullptr; return er; }
    return vh_poison_device(d, need);
  }
  ~EgoWorkLease() { if (d && !kept) (void)hipFree(d); }
};

// The stateless estimators: validation, one device block (matches | offsets | random draws | ok,ninl | inliers | tr |
// scratch of scratch_bytes(longest list)), the uploads, the kernels through `launch`, the downloads.  unsupported: the
// verdict of the entry point's own limits, reported once the arguments are known to be valid.
// extra / extra_bytes (nullable / 0): one more output of the call (the mono models), behind the scratch; `launch` receives its
// device address as its last argument and the bytes come back with the other results.
template <class Bytes, class Launch>
static int32_t estimate_stateless(int32_t device, int32_t n_sets, int32_t ransac_iters, int32_t draws, bool unsupported, const vh_p_match *pm,
                                  const int32_t *offsets, const int32_t *rnd, double *tr, int32_t *ok, int32_t *n_inliers, int32_t *inliers,
                                  Bytes scratch_bytes, Launch launch, void *extra = nullptr, size_t extra_bytes = 0) {
  ListSpan sp;
  if (n_sets < 1 || !rnd || !tr || !ok || !n_inliers || ransac_iters < 1 || check_offsets(offsets, n_sets, sp)) return VH_ERR_INVALID_ARG;
  const int64_t total = sp.end, cap = std::max<int64_t>(sp.longest, 1);  // (the records go up from record 0)
  if (total > 0 && !pm) return VH_ERR_INVALID_ARG;
  if (unsupported) return VH_ERR_UNSUPPORTED;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets, slots = (size_t)std::max<int64_t>(total, 1);
  const size_t b_off = sizeof(int32_t) * (lists + 1), b_r = sizeof(int32_t) * lists * ransac_iters * draws, b_tr = sizeof(double) * 6 * lists;
  Carver c;
  const size_t o_pm = c.take<vh_p_match>(slots), o_off = c.take<int32_t>(lists + 1), o_r = c.take<int32_t>(lists * ransac_iters * draws);
  const size_t o_ok = c.take<int32_t>(2 * lists), o_inl = c.take<int32_t>(slots), o_tr = c.take<double>(6 * lists);
  const size_t o_scr = c.take<uint8_t>(scratch_bytes(cap)), o_extra = extra ? c.take<uint8_t>(extra_bytes) : 0;
  EgoWorkLease lease;
  VH_HIP(lease.take(device, c.tight()));
  uint8_t *d = lease.d;
  hipError_t er = hipSuccess;
  if (total) er = hipMemcpy(d + o_pm, pm, sizeof(vh_p_match) * (size_t)total, hipMemcpyHostToDevice);
  if (er == hipSuccess) er = hipMemcpy(d + o_off, offsets, b_off, hipMemcpyHostToDevice);
  if (er == hipSuccess) er = hipMemcpy(d + o_r, rnd, b_r, hipMemcpyHostToDevice);
  if (er == hipSuccess) {
    launch((const vh_p_match *)(d + o_pm), (const int32_t *)(d + o_off), (const int32_t *)(d + o_r), d + o_scr, cap, (double *)(d + o_tr), (int32_t *)(d + o_ok),
           (int32_t *)(d + o_inl), extra ? d + o_extra : nullptr);
    er = hipGetLastError();  // (a rejected launch is not reported by the synchronisation)
    if (er == hipSuccess) er = hipDeviceSynchronize();
  }
  if (er == hipSuccess) er = hipMemcpy(tr, d + o_tr, b_tr, hipMemcpyDeviceToHost);
  if (er == hipSuccess) er = hipMemcpy(ok, d + o_ok, sizeof(int32_t) * (size_t)n_sets, hipMemcpyDeviceToHost);
  if (er == hipSuccess) er = hipMemcpy(n_inliers, d + o_ok + sizeof(int32_t) * (size_t)n_sets, sizeof(int32_t) * (size_t)n_sets, hipMemcpyDeviceToHost);
  if (er == hipSuccess && inliers && total) er = hipMemcpy(inliers, d + o_inl, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost);
  if (er == hipSuccess && extra) er = hipMemcpy(extra, d + o_extra, extra_bytes, hipMemcpyDeviceToHost);
  if (er != hipSuccess) { t_last_error = hipGetErrorString(er); return VH_ERR_HIP; }
  return VH_OK;
}

// (arguments validated and the device selected by the caller)
int32_t link_lists_device(int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t n_index, const vh_p_match *carry_pm,
                          const vh_track *carry_trk, int32_t ccnt, int64_t carry_serial, bool has_carry, LinkedLists &out) {
  const int32_t cmax = n_lists > 0 ? *std::max_element(counts, counts + n_lists) : 0;
  const int32_t lcap = std::max(std::max(cmax, ccnt), 1), slots = n_lists + 1, cslot = n_lists;
  std::vector<DeviceBlock> &blocks = out.blocks;
  const auto alloc = [&](void **ptr, size_t bytes) { blocks.emplace_back(); const hipError_t e = blocks.back().alloc(bytes); *ptr = blocks.back().p; return e; };
  vh_p_match *d_pm = nullptr; vh_track *d_trk = nullptr; uint32_t *d_tc = nullptr, *d_tp = nullptr, *d_check = nullptr; int32_t *d_cnt = nullptr, *d_scnt = nullptr;
  VH_HIP(alloc((void **)&d_pm, sizeof(vh_p_match) * (size_t)slots * lcap));
  VH_HIP(alloc((void **)&d_trk, sizeof(vh_track) * (size_t)slots * lcap));
  VH_HIP(alloc((void **)&d_tc, sizeof(uint32_t) * (size_t)slots * n_index));
  VH_HIP(alloc((void **)&d_tp, sizeof(uint32_t) * (size_t)slots * n_index));
  VH_HIP(alloc((void **)&d_cnt, sizeof(int32_t) * (size_t)slots));
  VH_HIP(alloc((void **)&d_scnt, sizeof(int32_t) * (size_t)slots));
  VH_HIP(alloc((void **)&d_check, sizeof(uint32_t) * 4));
  VH_HIP(hipMemset(d_tc, 0, sizeof(uint32_t) * (size_t)slots * n_index));
  VH_HIP(hipMemset(d_tp, 0, sizeof(uint32_t) * (size_t)slots * n_index));
  VH_HIP(hipMemset(d_scnt, 0, sizeof(int32_t) * (size_t)slots));
  VH_HIP(hipMemset(d_check, 0, sizeof(uint32_t) * 4));
  std::vector<int32_t> hc(counts, counts + n_lists);
  hc.push_back(ccnt);
  VH_HIP(hipMemcpy(d_cnt, hc.data(), sizeof(int32_t) * (size_t)slots, hipMemcpyHostToDevice));
  int32_t rc = upload_strided_lists(d_pm, lcap, pm, stride, counts, n_lists);
  if (rc) return rc;
  VhTrackArgs t{};
  t.pm = d_pm; t.pm_stride = lcap; t.counts = d_cnt; t.count_cap = lcap; t.n_index = n_index;
  t.tab_c = d_tc; t.tab_p = d_tp; t.trk = d_trk; t.trk_stride = lcap; t.slot_count = d_scnt; t.check = d_check;
  t.chain = 1; t.epoch = 1; t.pred_epoch = 1; t.pred0 = -1;
  if (has_carry) {  // the carry's list bids for its table in the slot behind the lists; its tracks are final
    if (ccnt) {
      VH_HIP(hipMemcpy(d_pm + (size_t)cslot * lcap, carry_pm, sizeof(vh_p_match) * (size_t)ccnt, hipMemcpyHostToDevice));
    }
    VhTrackArgs c = t;
    c.pm = d_pm + (size_t)cslot * lcap; c.counts = d_cnt + cslot; c.rows = 1; c.slot0 = cslot; c.tab_p = d_tp + (size_t)cslot * n_index;
    vh_launch_track_scatter(c, nullptr);
    if (ccnt) VH_HIP(hipMemcpyAsync(d_trk + (size_t)cslot * lcap, carry_trk, sizeof(vh_track) * (size_t)ccnt, hipMemcpyHostToDevice, nullptr));
    t.pred0 = cslot;
  }
  t.rows = n_lists; t.slot0 = 0; t.serial0 = has_carry ? carry_serial : 0;
  vh_launch_track_scatter(t, nullptr);
  vh_launch_track_link(t, nullptr);
  vh_launch_track_rank(t, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  if ((rc = report_violation(d_check))) return rc;
  out.d_pm = d_pm; out.d_trk = d_trk; out.d_cnt = d_cnt; out.d_check = d_check; out.lcap = lcap; out.serial0 = t.serial0;
  return VH_OK;
}

// one search of m1's features among m2's; launch(gq, a) queues it on the transient group's stream, its result in mt.d_best
template <class Launch>
static int32_t match_all(const vh_params *p, int32_t device, const int32_t dims[3], const int32_t *m1, int32_t n1, const int32_t *m2, int32_t n2,
                         int32_t flow, int32_t *best, Launch launch) {
  if (!p || !dims || (n1 > 0 && !best)) return VH_ERR_INVALID_ARG;
  Temp t;
  int32_t rc;
  if ((rc = temp_with_features(p, device, dims, false, {{VH_SET_1C, m1, n1}, {VH_SET_1P, m2, n2}}, t))) return rc;
  Group *gq = t.gq;
  VhMatchArgs a = gq->match_args(VH_METHOD_FLOW);
  a.npass = 1; a.pass[0] = {VH_SET_1C, VH_SET_1P, flow ? 1 : 0, 0};
  launch(gq, a);
  VH_HIP(hipGetLastError());
  if (n1) VH_HIP(hipMemcpyAsync(best, gq->mt.d_best, sizeof(int32_t) * (size_t)n1, hipMemcpyDeviceToHost, gq->stream));
  VH_HIP(hipStreamSynchronize(gq->stream));
  return VH_OK;
}

// Matcher::matching on caller-supplied features; ranges (nullable): with use_prior = true inside them (kernels_ranged.hip)
static int32_t match_stateless(const vh_params *p, int32_t device, const int32_t dims[3], int32_t method, const int32_t *m1p, int32_t n1p,
                               const int32_t *m2p, int32_t n2p, const int32_t *m1c, int32_t n1c, const int32_t *m2c, int32_t n2c,
                               const float *ranges, vh_p_match *out, int32_t cap, int32_t *n) {
  if (!p || !dims || !n) return VH_ERR_INVALID_ARG;
  if (method < 0 || method > 2) return VH_ERR_INVALID_ARG;
  Temp t;
  int32_t rc;
  if ((rc = temp_with_features(p, device, dims, true, {{VH_SET_1P, m1p, n1p}, {VH_SET_2P, m2p, n2p}, {VH_SET_1C, m1c, n1c}, {VH_SET_2C, m2c, n2c}}, t))) return rc;
  Group *gq = t.gq;
  if (ranges && (rc = gq->load_ranges(ranges))) return rc;
  if ((rc = gq->match(method, nullptr, ranges != nullptr))) return rc;
  return gq->get_matches(0, out, cap, n);
}

}  // namespace vh_engine

using namespace vh_engine;

// vh_group / vh_matcher are opaque aliases of Group (a matcher is a group of one stream).

extern "C" {

int32_t vh_abi_version(void) { return VH_ABI_VERSION; }

int32_t vh_device_count(void) {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return VH_ERR_NO_DEVICE;
  return cnt;
}

const char *vh_error_string(int32_t code) {
  switch (code) {
    case VH_OK: return "ok";
    case VH_ERR_INVALID_ARG: return "invalid argument (image dimension mismatch / null pointer)";
    case VH_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case VH_ERR_HIP: return "HIP runtime error";
    case VH_ERR_CAPACITY: return "capacity exceeded";
    case VH_ERR_UNSUPPORTED: return "parameter outside the supported envelope";
    case VH_ERR_STATE: return "call sequence error";
    default: return "unknown error";
  }
}

const char *vh_last_error(void) { return t_last_error.c_str(); }

void vh_default_params(vh_params *p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->nms_n = 2; p->nms_tau = 50; p->match_binsize = 50; p->match_radius = 200;
  p->match_disp_tolerance = 2; p->outlier_disp_tolerance = 5; p->outlier_flow_tolerance = 5;
}

// ---- group -----------------------------------------------------------------
int32_t vh_group_create(const vh_params *p, int32_t device, int32_t n_streams, int32_t max_features,
                        int32_t max_matches, vh_group **out) {
  return group_new(p, device, n_streams, max_features, max_matches, (Group **)out);
}
void vh_group_destroy(vh_group *g) {
  if (!g) return;
  Group *gq = (Group *)g;
  (void)hipSetDevice(gq->device);
  (void)gq->sync_all();
  gq->prof_collect();
  delete gq;
}
int32_t vh_group_streams(const vh_group *g) { return g ? ((const Group *)g)->S : VH_ERR_INVALID_ARG; }
int64_t vh_group_device_bytes(const vh_group *g) {  // (the matcher's arrays and, once begun, the post stage's ring of batches)
  if (!g) return (int64_t)VH_ERR_INVALID_ARG;
  const Group *gq = (const Group *)g;
  int64_t b = (int64_t)gq->device_bytes;
  if (gq->sparse) b += vh_group_device_bytes((const vh_group *)gq->sparse.get());  // the sparse sets of multi-stage matching
  b += (int64_t)gq->ms_vb.bytes;                                             // and the voted sparse lists of its device mode
  for (const auto &vb : gq->vbatch) b += (int64_t)vb.vb.bytes + (int64_t)vb.block_bytes + (int64_t)vb.dn.bytes + (int64_t)vb.tl.bytes;  // (dn, tl: the dense and the tail stages' blocks)
  b += gq->rh.bytes;                                                         // the ring and the gather buffers of reconstruction
  return b;
}
int32_t vh_group_push_back_device(vh_group *g, const void *dI1, const void *dI2, int64_t stride_bytes,
                                  const int32_t dims[3], int32_t replace) {
  Group *gq = (Group *)g; ENTER(gq);
  if (gq->seq) return VH_ERR_STATE;  // a sequence handle takes chunks (vh_sequence_push_back_device)
  return gq->push_device(dI1, dI2, stride_bytes, dims, replace);
}
int32_t vh_group_push_back(vh_group *g, const uint8_t *I1, const uint8_t *I2, int64_t stride_bytes,
                           const int32_t dims[3], int32_t replace) {
  Group *gq = (Group *)g; ENTER(gq);
  if (gq->seq) return VH_ERR_STATE;
  return gq->push_host(I1, I2, stride_bytes, dims, replace);
}

// ---- sequence --------------------------------------------------------------
int32_t vh_sequence_create(const vh_params *p, int32_t device, int32_t max_frames, int32_t max_features, int32_t max_matches,
                           vh_group **out) {
  if (!out) return VH_ERR_INVALID_ARG;
  *out = nullptr;
  Group *gq = nullptr;
  const int32_t rc = group_new(p, device, max_frames, max_features, max_matches, &gq);
  if (rc) return rc;
  gq->seq = true;  // (before the first push: the feature sets are allocated there, with the empty pair of a sequence)
  *out = (vh_group *)gq;
  return VH_OK;
}
int32_t vh_sequence_push_back_device(vh_group *g, const void *dI1, const void *dI2, int64_t stride_bytes, const int32_t dims[3],
                                     int32_t n_frames) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!gq->seq) return VH_ERR_STATE;
  if (n_frames < 1 || n_frames > gq->S) return VH_ERR_INVALID_ARG;
  return gq->push_device(dI1, dI2, stride_bytes, dims, 0, n_frames);
}
int32_t vh_sequence_push_back(vh_group *g, const uint8_t *I1, const uint8_t *I2, int64_t stride_bytes, const int32_t dims[3],
                              int32_t n_frames) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!gq->seq) return VH_ERR_STATE;
  if (n_frames < 1 || n_frames > gq->S) return VH_ERR_INVALID_ARG;
  return gq->push_host(I1, I2, stride_bytes, dims, 0, n_frames);
}
int32_t vh_sequence_position(const vh_group *g, int64_t *first_frame, int32_t *n_frames) {
  if (!g || !first_frame || !n_frames) return VH_ERR_INVALID_ARG;
  const Group *gq = (const Group *)g;
  if (!gq->seq) return VH_ERR_STATE;
  *first_frame = gq->seq_first;
  *n_frames = gq->seq_n;
  return VH_OK;
}
// the sparse group of multi-stage matching: the same rows (a sequence handle's: a sequence group), the sparse NMS distance
static int32_t make_sparse(Group *gq) {
  if (gq->sparse) return VH_OK;
  vh_params q = gq->p;
  q.nms_n = gq->p.nms_n * 4;  // matcher.cpp:621-623
  if (q.nms_n > 10) q.nms_n = std::max(gq->p.nms_n, 10);
  q.multi_stage = 0; q.refinement = 0;
  Group *sp = nullptr;
  const int32_t rc = group_new(&q, gq->device, gq->S, 0, 0, &sp);
  if (rc) return rc;
  sp->stream = gq->stream;  // (its own detect stream stays idle, or carries its searches in a small group)
  sp->seq = gq->seq;
  gq->sparse.reset(sp);
  return VH_OK;
}
static void drop_sparse(Group *gq) { gq->sparse.reset(); gq->ms_device = gq->ms_prior = false; }
int32_t vh_group_set_multi_stage_matching(vh_group *g, int32_t on) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->allocated) return VH_ERR_STATE;  // before the first push only: the sparse sets belong to every frame of the ring
  if (on && !gq->p.multi_stage) return VH_ERR_INVALID_ARG;
  if (gq->seq) return VH_ERR_UNSUPPORTED;  // (vh_sequence_set_multi_stage)
  if (!on) { drop_sparse(gq); return VH_OK; }
  return make_sparse(gq);
}
int32_t vh_sequence_set_multi_stage(vh_group *g, int32_t mode) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (!gq->seq) return VH_ERR_UNSUPPORTED;  // a group or a lone matcher keeps its own entries
  if (mode < 0 || mode > 2) return VH_ERR_INVALID_ARG;
  if (gq->allocated) return VH_ERR_STATE;
  if (mode && !gq->p.multi_stage) return VH_ERR_INVALID_ARG;
  if (!mode) { drop_sparse(gq); return VH_OK; }
  const int32_t rc = make_sparse(gq);
  if (rc) return rc;
  gq->ms_device = mode == 2;
  return VH_OK;
}
int32_t vh_group_set_multi_stage_prior(vh_group *g, int32_t on) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->allocated) return VH_ERR_STATE;      // before the first push only, like the mode it belongs to
  if (on && !gq->sparse) return VH_ERR_STATE;  // multi-stage matching first
  gq->ms_prior = on != 0;
  return VH_OK;
}
int32_t vh_set_multi_stage_prior(vh_matcher *m, int32_t on) { return vh_group_set_multi_stage_prior((vh_group *)m, on); }
int32_t vh_set_multi_stage_matching(vh_matcher *m, int32_t on) { return vh_group_set_multi_stage_matching((vh_group *)m, on); }
int32_t vh_group_get_sparse_matches(vh_group *g, int32_t stream, vh_p_match *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!gq->sparse) return VH_ERR_STATE;
  if (gq->ms_device) return gq->get_sparse_device(stream, out, cap, n);
  return gq->sparse->get_matches(stream, out, cap, n);
}
int32_t vh_group_set_multi_stage_device(vh_group *g, int32_t on) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->seq) return VH_ERR_UNSUPPORTED;
  if (gq->allocated) return VH_ERR_STATE;   // before the first push only, like the mode it belongs to
  if (on && !gq->sparse) return VH_ERR_STATE;  // multi-stage matching first
  gq->ms_device = on != 0;
  return VH_OK;
}
int32_t vh_set_multi_stage_device(vh_matcher *m, int32_t on) { return vh_group_set_multi_stage_device((vh_group *)m, on); }
int32_t vh_get_sparse_matches(vh_matcher *m, vh_p_match *out, int32_t cap, int32_t *n) {
  return vh_group_get_sparse_matches((vh_group *)m, 0, out, cap, n);
}
int32_t vh_prior_statistics(const vh_params *p, const int32_t dims[3], int32_t method, const vh_p_match *pm, int32_t n, float *ranges) {
  if (!p || !dims || !ranges || n < 0 || (n > 0 && !pm) || method < 0 || method > 2) return VH_ERR_INVALID_ARG;
  int32_t rc = check_params(p);
  if (rc) return rc;
  if ((rc = check_dims(dims, false))) return rc;
  return prior_statistics(*p, dims, method, pm, n, ranges);
}
// The statistics of n_lists lists at once on the device (kernels_stats.hip), list l = pm[l * stride .. + counts[l]):
// value for value what vh_prior_statistics gives for each list.  The handle's device mode is the throughput path; this
// entry exists for tests and timing.
int32_t vh_prior_statistics_device(const vh_params *p, int32_t device, const int32_t dims[3], int32_t method, int32_t n_lists, const vh_p_match *pm,
                                   int64_t stride, const int32_t *counts, float *ranges) {
  if (!p || !dims || !ranges || !counts || n_lists < 1 || stride < 0 || method < 0 || method > 2) return VH_ERR_INVALID_ARG;
  int32_t rc = check_params(p);
  if (rc) return rc;
  if ((rc = check_dims(dims, false))) return rc;
  int32_t cap = 0;
  if (check_counts(counts, n_lists, stride, cap) || (cap > 0 && !pm)) return VH_ERR_INVALID_ARG;
  cap = std::max(cap, 1);
  if ((rc = select_device(device))) return rc;
  const float bs = (float)p->match_binsize;
  VhStatsArgs sa{};
  sa.ubn = (int32_t)ceilf((float)dims[0] / bs); sa.vbn = (int32_t)ceilf((float)dims[1] / bs);  // matcher.cpp:282-283
  if ((int64_t)sa.ubn * sa.vbn > INT32_MAX / 16) return VH_ERR_UNSUPPORTED;  // (the kernel indexes a list's table with 32 bits)
  const size_t per = (size_t)sa.ubn * sa.vbn * 16;
  DeviceBlock b_src, b_cnt, b_out;
  VH_HIP(b_src.alloc(sizeof(vh_p_match) * (size_t)n_lists * cap));
  VH_HIP(b_cnt.alloc(sizeof(int32_t) * 2 * (size_t)n_lists));  // counts, then the error flags
  VH_HIP(b_out.alloc(sizeof(float) * per * (size_t)n_lists));
  struct { vh_p_match *src; int32_t *cnt; float *out; } gd{b_src.as<vh_p_match>(), b_cnt.as<int32_t>(), b_out.as<float>()};
  if ((rc = upload_strided_lists(gd.src, cap, pm, stride, counts, n_lists))) return rc;
  VH_HIP(hipMemcpy(gd.cnt, counts, sizeof(int32_t) * (size_t)n_lists, hipMemcpyHostToDevice));
  VH_HIP(hipMemset(gd.cnt + n_lists, 0, sizeof(int32_t) * (size_t)n_lists));
  sa.pm = gd.src; sa.pm_stride = cap; sa.counts = gd.cnt; sa.status = nullptr; sa.count_stride = 1; sa.count_cap = cap;
  sa.n_lists = n_lists; sa.method = method; sa.bs = bs; sa.R = (float)p->match_radius;
  sa.out = gd.out; sa.err = gd.cnt + n_lists;
  vh_launch_prior_stats(sa, 0, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  std::vector<int32_t> err((size_t)n_lists);
  VH_HIP(hipMemcpy(err.data(), gd.cnt + n_lists, sizeof(int32_t) * (size_t)n_lists, hipMemcpyDeviceToHost));
  for (int32_t l = 0; l < n_lists; l++) if (err[(size_t)l]) return VH_ERR_INVALID_ARG;
  VH_HIP(hipMemcpy(ranges, gd.out, sizeof(float) * per * (size_t)n_lists, hipMemcpyDeviceToHost));
  return VH_OK;
}
// ---- feature tracks ----------------------------------------------------------
int32_t vh_group_set_track_linking(vh_group *g, int32_t on) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->allocated) return VH_ERR_STATE;  // before the first push only: every list since the first frame has its place in the chain
  if (!on && gq->rh.on) return VH_ERR_STATE;  // reconstruction reads the tracks (vh_sequence_set_reconstruction)
  gq->trk_on = on != 0;
  return VH_OK;
}
int32_t vh_set_track_linking(vh_matcher *m, int32_t on) { return vh_group_set_track_linking((vh_group *)m, on); }
// ---- the rule of the outlier vote ----------------------------------------------
int32_t vh_group_set_vote_rule(vh_group *g, int32_t rule) {
  Group *gq = (Group *)g;
  if (!gq || (rule != VH_VOTE_REFERENCE && rule != VH_VOTE_STOCK)) return VH_ERR_INVALID_ARG;
  if (gq->allocated) return VH_ERR_STATE;  // before the first push only: no step in flight is voted under two rules
  gq->vote_rule = rule;
  return VH_OK;
}
int32_t vh_set_vote_rule(vh_matcher *m, int32_t rule) { return vh_group_set_vote_rule((vh_group *)m, rule); }
int32_t vh_group_get_tracks(vh_group *g, int32_t stream, vh_track *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_tracks(stream, out, cap, n);
}
int32_t vh_get_tracks(vh_matcher *m, vh_track *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)m; ENTER(gq);
  return gq->get_tracks(0, out, cap, n);
}
int32_t vh_group_get_tracks_all(vh_group *g, vh_track *out, int32_t cap_per_stream, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_tracks_all(out, cap_per_stream, counts);
}
int32_t vh_group_tracks_device(vh_group *g, const vh_track **d_tracks, int64_t *stride) {
  Group *gq = (Group *)g;
  if (!gq || !d_tracks || !stride) return VH_ERR_INVALID_ARG;
  *d_tracks = nullptr; *stride = 0;
  if (!gq->trk_on || !gq->allocated || gq->last_method < 0 || !gq->trk_cur_valid) return VH_ERR_STATE;
  *d_tracks = gq->tk.d_trk + (size_t)(gq->seq ? 0 : gq->trk_cur * gq->S) * gq->mcap;
  *stride = gq->mcap;
  return VH_OK;
}

// The stateless form: the lists of one call are the rows of a chain (row l continues row l - 1), the carry of an earlier
// call -- its last list and that list's tracks, kept on the host -- is bid for again in the slot behind them.
struct vh_track_carry {
  int64_t next_serial = 0;
  std::vector<vh_p_match> pm;
  std::vector<vh_track> trk;
};
void vh_track_carry_free(vh_track_carry *c) { delete c; }
int32_t vh_link_tracks(int32_t device, int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t n_index,
                       const vh_track_carry *carry_in, vh_track_carry **carry_out, vh_track *out) {
  if (carry_out) *carry_out = nullptr;
  int32_t cmax = 0;
  if (n_lists < 1 || stride < 0 || n_index < 1 || check_counts(counts, n_lists, stride, cmax)) return VH_ERR_INVALID_ARG;
  if (cmax > 0 && (!pm || !out)) return VH_ERR_INVALID_ARG;
  if (cmax > (int32_t)VH_TRACK_POS_MASK || (int64_t)n_lists + 1 > (1 << 16)) return VH_ERR_UNSUPPORTED;  // (positions share a table entry with the epoch; rows are a grid dimension)
  const int32_t rc = select_device(device);
  if (rc) return rc;
  LinkedLists ll;
  const int32_t rl = link_lists_device(n_lists, pm, stride, counts, n_index, carry_in ? carry_in->pm.data() : nullptr, carry_in ? carry_in->trk.data() : nullptr,
                                       carry_in ? (int32_t)carry_in->pm.size() : 0, carry_in ? carry_in->next_serial : 0, carry_in != nullptr, ll);
  if (rl) return rl;
  for (int32_t l = 0; l < n_lists; l++)
    if (counts[l]) VH_HIP(hipMemcpy(out + (size_t)l * stride, ll.d_trk + (size_t)l * ll.lcap, sizeof(vh_track) * (size_t)counts[l], hipMemcpyDeviceToHost));
  if (carry_out) {
    vh_track_carry *c = new vh_track_carry();
    const int32_t last = n_lists - 1;
    c->next_serial = ll.serial0 + n_lists;
    if (counts[last]) {
      c->pm.assign(pm + (size_t)last * stride, pm + (size_t)last * stride + counts[last]);
      c->trk.assign(out + (size_t)last * stride, out + (size_t)last * stride + counts[last]);
    }
    *carry_out = c;
  }
  return VH_OK;
}
int32_t vh_group_match_features(vh_group *g, int32_t method) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->match(method);
}
int32_t vh_group_match_features_prior(vh_group *g, int32_t method, const double *Tr_delta16) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->match(method, Tr_delta16);
}
int32_t vh_group_get_matches(vh_group *g, int32_t stream, vh_p_match *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_matches(stream, out, cap, n);
}
int32_t vh_group_get_matches_all(vh_group *g, vh_p_match *out, int32_t cap_per_stream, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_matches_all(out, cap_per_stream, counts);
}
int32_t vh_group_download_matches_async(vh_group *g, vh_p_match *out, int32_t cap_per_stream, int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->download_async(out, cap_per_stream, counts);
}
int32_t vh_group_wait_download(vh_group *g) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->wait_download();
}
int32_t vh_group_get_features(vh_group *g, int32_t stream, int32_t which, int32_t *out12, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_features(stream, which, out12, cap, n);
}
int32_t vh_group_get_counts(vh_group *g, int32_t *n_features, int32_t *n_matches) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_counts(n_features, n_matches);
}
int32_t vh_group_synchronize(vh_group *g) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->sync_all();
}
int32_t vh_group_set_stream(vh_group *g, void *hip_stream) {
  Group *gq = (Group *)g; ENTER(gq);
  int32_t rc = gq->sync_all();
  if (rc) return rc;
  gq->user_stream = (hipStream_t)hip_stream;  // handle 0 is the legacy default stream, a stream like any other
  gq->user_stream_set = true;
  return VH_OK;
}
int32_t vh_group_clear_stream(vh_group *g) {
  Group *gq = (Group *)g; ENTER(gq);
  int32_t rc = gq->sync_all();
  if (rc) return rc;
  gq->user_stream = nullptr; gq->user_stream_set = false;
  return VH_OK;
}
int32_t vh_group_stream_wait_images(vh_group *g, void *hip_stream) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!gq->allocated) return VH_OK;  // nothing pushed yet: nothing reads any image
  // the detection (and indexing) of the last pushed frame is the last reader of its images
  VH_HIP(hipStreamWaitEvent((hipStream_t)hip_stream, gq->ev_det[gq->pair_cur], 0));
  return VH_OK;
}
int32_t vh_group_search_stats(vh_group *g, int32_t *speculative, double *research_rate) {
  Group *gq = (Group *)g; ENTER(gq);
  if (speculative) *speculative = gq->force_mode >= 0 ? gq->force_mode : (gq->spec_mode ? 1 : 0);
  if (research_rate) *research_rate = gq->last_redo_rate;
  return VH_OK;
}
int32_t vh_group_debug_fail_next_alloc(vh_group *g) {
  Group *gq = (Group *)g; ENTER(gq);
  gq->fail_next_alloc = true; gq->fail_alloc_skip = 0;
  return VH_OK;
}
int32_t vh_group_debug_fail_alloc_after(vh_group *g, int32_t skip) {
  Group *gq = (Group *)g; ENTER(gq);
  if (skip < 0) return VH_ERR_INVALID_ARG;
  gq->fail_next_alloc = true; gq->fail_alloc_skip = skip;
  return VH_OK;
}
int32_t vh_group_profile_enable(vh_group *g, int32_t on) {
  Group *gq = (Group *)g; ENTER(gq);
  gq->prof = on != 0;
  if (gq->sparse) gq->sparse->prof = gq->prof;
  return VH_OK;
}
int32_t vh_group_profile_read(vh_group *g, const char *name, double *ms, int64_t *launches) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!name) return VH_ERR_INVALID_ARG;
  if (gq->sparse && !strncmp(name, "sparse_", 7) && strcmp(name, "sparse_vote_host") && strcmp(name, "sparse_vote")) {  // the sparse group's kernels
    gq = gq->sparse.get(); name += 7;
  }
  gq->prof_collect();
  auto it = gq->prof_entries.find(name);
  if (ms) *ms = it == gq->prof_entries.end() ? 0.0 : it->second.ms;
  if (launches) *launches = it == gq->prof_entries.end() ? 0 : it->second.launches;
  return VH_OK;
}
int32_t vh_group_profile_reset(vh_group *g) {
  Group *gq = (Group *)g; ENTER(gq);
  gq->prof_collect();
  gq->prof_entries.clear();
  if (gq->sparse) { gq->sparse->prof_collect(); gq->sparse->prof_entries.clear(); }
  return VH_OK;
}

// ---- one stream ------------------------------------------------------------
int32_t vh_create_ex(const vh_params *p, int32_t device, int32_t max_features, int32_t max_matches,
                     vh_matcher **out) {
  return group_new(p, device, 1, max_features, max_matches, (Group **)out);
}
int32_t vh_create(const vh_params *p, int32_t device, vh_matcher **out) { return vh_create_ex(p, device, 0, 0, out); }
void vh_destroy(vh_matcher *m) { vh_group_destroy((vh_group *)m); }
int32_t vh_set_intrinsics(vh_matcher *m, double f, double cu, double cv, double base) {
  if (!m) return VH_ERR_INVALID_ARG;
  Group *gq = (Group *)m;
  gq->p.f = f; gq->p.cu = cu; gq->p.cv = cv; gq->p.base = base;
  return VH_OK;
}
int32_t vh_push_back(vh_matcher *m, const uint8_t *I1, const uint8_t *I2, const int32_t dims[3], int32_t replace) {
  Group *gq = (Group *)m; ENTER(gq);
  return gq->push_host(I1, I2, 0, dims, replace);
}
int32_t vh_push_back_device(vh_matcher *m, const void *dI1, const void *dI2, const int32_t dims[3], int32_t replace) {
  Group *gq = (Group *)m; ENTER(gq);
  return gq->push_device(dI1, dI2, 0, dims, replace);
}
int32_t vh_match_features(vh_matcher *m, int32_t method, const double *Tr_delta16) {
  Group *gq = (Group *)m; ENTER(gq);
  return gq->match(method, Tr_delta16);  // (null: as the reference's Matcher::matchFeatures, which ignores its Tr_delta, matcher.cpp:93-111)
}
int32_t vh_bucket_features(vh_matcher *m, int32_t max_features, float bucket_width, float bucket_height) {
  Group *gq = (Group *)m; ENTER(gq);
  if (max_features < 1 || !(bucket_width > 0) || !(bucket_height > 0)) return VH_ERR_INVALID_ARG;
  // (a bucket grid beyond 2^24 cells -- bucket sides of a fraction of a pixel -- would overflow the reference's int arithmetic too)
  if (gq->allocated && ((double)gq->dims[0] / bucket_width + 1) * ((double)gq->dims[1] / bucket_height + 1) > (double)(1 << 24)) return VH_ERR_INVALID_ARG;
  const int32_t rc = gq->fetch_matches(0);
  if (rc) return rc == VH_ERR_STATE ? VH_OK : rc;  // nothing matched yet: nothing to bucket
  bucket_host(gq->host_matches[0], max_features, bucket_width, bucket_height);
  return VH_OK;
}
int32_t vh_remove_outliers(vh_matcher *m) {
  Group *gq = (Group *)m; ENTER(gq);
  return gq->remove_outliers(0, 1, 1);
}
int32_t vh_group_remove_outliers(vh_group *g, int32_t host_threads) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->remove_outliers(0, gq->S, default_threads(host_threads));
}
int32_t vh_get_matches(vh_matcher *m, vh_p_match *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)m; ENTER(gq);
  return gq->get_matches(0, out, cap, n);
}
int32_t vh_get_features(vh_matcher *m, int32_t which, int32_t *out12, int32_t cap, int32_t *n) {
  Group *gq = (Group *)m; ENTER(gq);
  return gq->get_features(0, which, out12, cap, n);
}
int32_t vh_host_alloc(int32_t device, size_t bytes, void **out) {
  if (!out || bytes == 0) return VH_ERR_INVALID_ARG;
  *out = nullptr;
  const int32_t rc = select_device(device);
  if (rc) return rc;
  VH_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));  // (the caller's own buffer: exempt from vh_poison.h's rule, the library reads nothing from it that the caller did not put there)
  return VH_OK;
}
int32_t vh_host_free(void *ptr) {
  if (!ptr) return VH_OK;
  VH_HIP(hipHostFree(ptr));
  return VH_OK;
}
int32_t vh_synchronize(vh_matcher *m) { return vh_group_synchronize((vh_group *)m); }
int32_t vh_set_stream(vh_matcher *m, void *hip_stream) { return vh_group_set_stream((vh_group *)m, hip_stream); }
int32_t vh_clear_stream(vh_matcher *m) { return vh_group_clear_stream((vh_group *)m); }
int32_t vh_stream_wait_images(vh_matcher *m, void *hip_stream) { return vh_group_stream_wait_images((vh_group *)m, hip_stream); }

#ifdef VH_DEBUG_ROWS
// debug build only: the (class, v) row index of one feature set
int32_t vh_debug_rows(vh_matcher *m, int32_t which, int32_t *row_start, int32_t *r_pos, int32_t *bin_start) {
  Group *gq = (Group *)m; ENTER(gq);
  const int32_t set = vh_role_set(gq->S, gq->pairs(), 0, which);
  const size_t nrow = 4 * (size_t)gq->dims[1];
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(hipMemcpy(row_start, gq->sets.row_start + (size_t)set * (nrow + 1), sizeof(int32_t) * (nrow + 1), hipMemcpyDeviceToHost));
  VH_HIP(hipMemcpy(r_pos, gq->sets.r_pos + (size_t)set * gq->cap, sizeof(int32_t) * gq->cap, hipMemcpyDeviceToHost));
  VH_HIP(hipMemcpy(bin_start, gq->sets.bin_start + (size_t)set * (gq->sets.nbins + 1), sizeof(int32_t) * (gq->sets.nbins + 1), hipMemcpyDeviceToHost));
  return gq->cap;
}
#endif

// ---- stereo egomotion ------------------------------------------
void vh_default_ego_params(vh_ego_params *e) {
  if (!e) return;
  memset(e, 0, sizeof(*e));
  e->ransac_iters = 200; e->reweighting = 1; e->inlier_threshold = 2.0;  // src/viso_stereo.h:39-41
  e->f = 1; e->cu = 0; e->cv = 0; e->base = 1;                            // src/viso.h:46-48, src/viso_stereo.h:38
}
int32_t vh_group_estimate_motion(vh_group *g, const vh_ego_params *e, const int32_t *rand3, double *tr, int32_t *ok,
                                 int32_t *n_inliers) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->estimate_motion(e, rand3, tr, ok, n_inliers);
}
int32_t vh_estimate_motion_stereo(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm,
                                  const int32_t *offsets, const int32_t *rand3, double *tr, int32_t *ok,
                                  int32_t *n_inliers, int32_t *inliers) {
  if (!e) return VH_ERR_INVALID_ARG;
  return estimate_stateless(device, n_sets, e->ransac_iters, 3, false, pm, offsets, rand3, tr, ok, n_inliers, inliers,
    [&](int64_t cap) { return sizeof(double) * 4 * (size_t)n_sets * (size_t)cap; },  // xyz + flags
    [&](const vh_p_match *d_pm, const int32_t *d_off, const int32_t *d_rand, uint8_t *d_scr, int64_t cap, double *d_tr, int32_t *d_ok, int32_t *d_inl, uint8_t *) {
      vh_launch_ego(*e, VhLists::packed(d_pm, d_off, n_sets), d_rand, (double *)d_scr, cap, d_tr, d_ok, d_ok + n_sets, d_inl, 0, nullptr);
    });
}

int32_t vh_group_post_begin(vh_group *g, int32_t cap_per_stream) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_begin(cap_per_stream);
}
int32_t vh_group_post_finish(vh_group *g, int32_t age, int32_t max_features, float bucket_width, float bucket_height, int32_t host_threads,
                             const vh_ego_params *e, const int32_t *rand3, double *tr, int32_t *ok, int32_t *n_inliers,
                             vh_p_match *bucketed, int32_t cap_per_stream, int32_t *counts, double *host_ms) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_finish(age, max_features, bucket_width, bucket_height, default_threads(host_threads), e, rand3, nullptr, nullptr, tr, ok, n_inliers, bucketed, cap_per_stream, counts, host_ms);
}
int32_t vh_group_post_finish_mono(vh_group *g, int32_t age, int32_t max_features, float bucket_width, float bucket_height, int32_t host_threads,
                                  const vh_mono_params *e, const int32_t *rand8, double *tr, int32_t *ok, int32_t *n_inliers,
                                  vh_p_match *bucketed, int32_t cap_per_stream, int32_t *counts, double *host_ms) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_finish(age, max_features, bucket_width, bucket_height, default_threads(host_threads), nullptr, nullptr, e, rand8, tr, ok, n_inliers, bucketed, cap_per_stream, counts, host_ms);
}

int32_t vh_group_post_device_config(vh_group *g, int32_t steps_per_batch, int32_t batches, int32_t lanes_per_wave) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_device_config(steps_per_batch, batches, lanes_per_wave);
}
int32_t vh_group_post_begin_device(vh_group *g, int32_t cap_per_stream, int32_t max_features, float bucket_width, float bucket_height,
                                   const vh_ego_params *e, const int32_t *rand3, const vh_mono_params *mono, const int32_t *rand8, int32_t want_lists) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_begin_device(cap_per_stream, max_features, bucket_width, bucket_height, e, rand3, mono, rand8, want_lists);
}
int32_t vh_group_post_finish_device(vh_group *g, int32_t age, double *tr, int32_t *ok, int32_t *n_inliers, vh_p_match *bucketed, int32_t cap_per_stream,
                                    int32_t *counts) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_finish_device(age, tr, ok, n_inliers, bucketed, cap_per_stream, counts);
}
int32_t vh_group_post_device_dense(vh_group *g, int32_t mode) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_device_dense(mode);
}
int32_t vh_group_post_finish_device_dense(vh_group *g, int32_t age, double *tr, int32_t *ok, int32_t *n_inliers, vh_p_match *bucketed,
                                          int32_t cap_per_stream, int32_t *counts, const vh_post_dense *d) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_finish_device(age, tr, ok, n_inliers, bucketed, cap_per_stream, counts, d);
}
int32_t vh_group_post_device_tail(vh_group *g, uint32_t stages) {
  // the mask first, and with a message of its own: it can be judged without a device, and a caller (or a test) can tell it from the handle's refusal
  if ((stages & ~(uint32_t)VH_POST_TAIL_ALL) || ((stages & VH_POST_TAIL_MONO_REFINE) && !(stages & VH_POST_TAIL_MONO_POSE))) {
    t_last_error = "vh_group_post_device_tail: unknown VH_POST_TAIL bits, or VH_POST_TAIL_MONO_REFINE without VH_POST_TAIL_MONO_POSE";
    return VH_ERR_INVALID_ARG;
  }
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_device_tail(stages);
}
int32_t vh_group_post_device_shape(vh_group *g, int32_t *steps_per_batch, int32_t *batches) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_device_shape(steps_per_batch, batches);
}
int32_t vh_group_post_finish_device_tail(vh_group *g, int32_t age, double *tr, int32_t *ok, int32_t *n_inliers, vh_p_match *bucketed,
                                         int32_t cap_per_stream, int32_t *counts, const vh_post_dense *d, const vh_post_tail *t) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->post_finish_device(age, tr, ok, n_inliers, bucketed, cap_per_stream, counts, d, t);
}

// ---- monocular egomotion -----------------------------------------
void vh_default_mono_params(vh_mono_params *e) {
  if (!e) return;
  memset(e, 0, sizeof(*e));
  e->ransac_iters = 2000; e->inlier_threshold = 0.00001; e->motion_threshold = 100.0;  // src/viso_mono.h:39-45
  e->height = 1.0; e->pitch = 0.0; e->f = 1; e->cu = 0; e->cv = 0;                      // src/viso.h:46-48
}
int32_t vh_group_estimate_motion_mono(vh_group *g, const vh_mono_params *e, const int32_t *rand8, double *tr, int32_t *ok,
                                      int32_t *n_inliers) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->estimate_motion_mono(e, rand8, tr, ok, n_inliers, nullptr);
}
int32_t vh_group_estimate_motion_mono_model(vh_group *g, const vh_mono_params *e, const int32_t *rand8, double *tr, int32_t *ok,
                                            int32_t *n_inliers, vh_mono_model *model) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!model) return VH_ERR_INVALID_ARG;
  return gq->estimate_motion_mono(e, rand8, tr, ok, n_inliers, model);
}
// model (nullable): the models come back too
static int32_t estimate_mono_stateless(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets,
                                       const int32_t *rand8, double *tr, int32_t *ok, int32_t *n_inliers, int32_t *inliers, vh_mono_model *model) {
  if (!e) return VH_ERR_INVALID_ARG;
  // (the hypothesis and triangulation kernels put the list on grid.y)
  const bool unsupported = (int64_t)n_sets * e->ransac_iters > (int64_t)1 << 31 || n_sets > 65535;
  return estimate_stateless(device, n_sets, e->ransac_iters, 8, unsupported, pm, offsets, rand8, tr, ok, n_inliers, inliers,
    [&](int64_t cap) { return (size_t)vh_mono_scratch_bytes(n_sets, cap, e->ransac_iters); },  // per-list scratch
    [&](const vh_p_match *d_pm, const int32_t *d_off, const int32_t *d_rand, uint8_t *d_scr, int64_t cap, double *d_tr, int32_t *d_ok, int32_t *d_inl, uint8_t *d_model) {
      vh_launch_mono(*e, VhLists::packed(d_pm, d_off, n_sets), d_rand, d_scr, cap, d_tr, d_ok, d_ok + n_sets, d_inl, 0, (vh_mono_model *)d_model, nullptr);
    }, model, model ? sizeof(vh_mono_model) * (size_t)std::max(n_sets, 0) : 0);
}
int32_t vh_estimate_motion_mono(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm,
                                const int32_t *offsets, const int32_t *rand8, double *tr, int32_t *ok, int32_t *n_inliers,
                                int32_t *inliers) {
  return estimate_mono_stateless(e, device, n_sets, pm, offsets, rand8, tr, ok, n_inliers, inliers, nullptr);
}
int32_t vh_estimate_motion_mono_model(const vh_mono_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm,
                                      const int32_t *offsets, const int32_t *rand8, double *tr, int32_t *ok, int32_t *n_inliers,
                                      int32_t *inliers, vh_mono_model *model) {
  if (!model) return VH_ERR_INVALID_ARG;
  return estimate_mono_stateless(e, device, n_sets, pm, offsets, rand8, tr, ok, n_inliers, inliers, model);
}

// ---- stateless primitives ----------------------------------------------------
int32_t vh_filters(int32_t device, const uint8_t *I, int32_t bpl, int32_t H, uint8_t *du, uint8_t *dv,
                   int16_t *f1, int16_t *f2) {
  if (!I || bpl < 5 || H < 5) return VH_ERR_INVALID_ARG;
  int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t n = (size_t)bpl * H;
  DeviceBlock blk;
  VH_HIP(blk.alloc(n * 7));
  uint8_t *d = blk.as<uint8_t>(), *dI = d, *ddu = d + n, *ddv = d + 2 * n;
  int16_t *df1 = (int16_t *)(d + 3 * n), *df2 = (int16_t *)(d + 5 * n);
  VH_HIP(hipMemcpy(dI, I, n, hipMemcpyHostToDevice));
  vh_launch_planes(dI, bpl, H, ddu, ddv, df1, df2, nullptr);
  VH_HIP(hipDeviceSynchronize());
  if (du) VH_HIP(hipMemcpy(du, ddu, n, hipMemcpyDeviceToHost));
  if (dv) VH_HIP(hipMemcpy(dv, ddv, n, hipMemcpyDeviceToHost));
  if (f1) VH_HIP(hipMemcpy(f1, df1, 2 * n, hipMemcpyDeviceToHost));
  if (f2) VH_HIP(hipMemcpy(f2, df2, 2 * n, hipMemcpyDeviceToHost));
  return VH_OK;
}

int32_t vh_compute_features(const vh_params *p, int32_t device, const uint8_t *I, const int32_t dims[3],
                            int32_t *max1, int32_t cap1, int32_t *num1, int32_t *max2, int32_t cap2,
                            int32_t *num2, uint8_t *du, uint8_t *dv) {
  if (!p || !I || !dims) return VH_ERR_INVALID_ARG;
  if (num1) *num1 = 0;
  if (num2) *num2 = 0;
  int32_t rc, overflow = VH_OK;
  {  // dense set (matcher.cpp:634-635)
    Temp t;
    if ((rc = temp_new(p, device, 0, 0, t))) return rc;
    if ((rc = t.gq->push_host(I, nullptr, 0, dims, 0))) return rc;
    int32_t n = 0;
    rc = t.gq->get_features(0, VH_SET_1C, max2, max2 ? cap2 : 0, &n);
    if (num2) *num2 = n;
    if (rc == VH_ERR_CAPACITY) overflow = rc; else if (rc) return rc;
    if (du || dv) {  // I_du / I_dv at matching resolution (matcher.cpp:596-600, :606-612)
      const VhGeom &g = t.gq->g;
      const size_t np = (size_t)g.bplm * g.Hm;
      DeviceBlock blk;
      VH_HIP(blk.alloc(2 * np));
      uint8_t *d = blk.as<uint8_t>();
      const uint8_t *src = p->half_resolution ? t.gq->det.d_half : t.gq->stg.d_stage[0];
      vh_launch_planes(src, g.bplm, g.Hm, d, d + np, nullptr, nullptr, t.gq->stream);
      VH_HIP(hipStreamSynchronize(t.gq->stream));
      if (du) VH_HIP(hipMemcpy(du, d, np, hipMemcpyDeviceToHost));
      if (dv) VH_HIP(hipMemcpy(dv, d + np, np, hipMemcpyDeviceToHost));
    }
  }
  if (p->multi_stage) {  // sparse set (matcher.cpp:621-628)
    vh_params ps = *p;
    int32_t ns = p->nms_n * 4;
    if (ns > 10) ns = std::max(p->nms_n, 10);
    ps.nms_n = ns;
    Temp t;
    if ((rc = temp_new(&ps, device, 0, 0, t))) return rc;
    if ((rc = t.gq->push_host(I, nullptr, 0, dims, 0))) return rc;
    int32_t n = 0;
    rc = t.gq->get_features(0, VH_SET_1C, max1, max1 ? cap1 : 0, &n);
    if (num1) *num1 = n;
    if (rc == VH_ERR_CAPACITY) overflow = rc; else if (rc) return rc;
  }
  return overflow;
}

int32_t vh_create_index(const vh_params *p, int32_t device, const int32_t dims[3], const int32_t *m,
                        int32_t n, int32_t *bin_start, int32_t *list) {
  if (!p || !dims || !bin_start || (n > 0 && !list)) return VH_ERR_INVALID_ARG;
  Temp t;
  int32_t rc;
  if ((rc = temp_with_features(p, device, dims, false, {{VH_SET_1C, m, n}}, t))) return rc;
  Group *gq = t.gq;
  int32_t *d_bs = nullptr, *d_list = nullptr;
  if ((rc = gq->dmalloc(&d_bs, (size_t)gq->sets.nbins + 1, false))) return rc;
  if ((rc = gq->dmalloc(&d_list, (size_t)std::max(n, 1), false))) return rc;
  vh_launch_ref_index(gq->sets, vh_role_set(1, gq->pairs(), 0, VH_SET_1C), d_bs, d_list, gq->stream);
  VH_HIP(hipMemcpyAsync(bin_start, d_bs, sizeof(int32_t) * ((size_t)gq->sets.nbins + 1), hipMemcpyDeviceToHost, gq->stream));
  if (n) VH_HIP(hipMemcpyAsync(list, d_list, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, gq->stream));
  VH_HIP(hipStreamSynchronize(gq->stream));
  return VH_OK;
}

int32_t vh_match_all(const vh_params *p, int32_t device, const int32_t dims[3], const int32_t *m1, int32_t n1,
                     const int32_t *m2, int32_t n2, int32_t flow, int32_t *best) {
  return match_all(p, device, dims, m1, n1, m2, n2, flow, best, [](Group *gq, const VhMatchArgs &a) {
    vh_launch_match(gq->sets, a, gq->mt.d_best, gq->mt.d_redo, gq->force_mode == 0 ? 0 : 1, 0, 0, gq->stream); });
}
int32_t vh_match_all_prior(const vh_params *p, int32_t device, const int32_t dims[3], const int32_t *m1, int32_t n1,
                           const int32_t *m2, int32_t n2, int32_t flow, double u_, double v_, int32_t *best) {
  return match_all(p, device, dims, m1, n1, m2, n2, flow, best, [&](Group *gq, const VhMatchArgs &a) {
    vh_launch_match_prior(gq->sets, a, u_, v_, gq->mt.d_best, gq->stream); });
}

int32_t vh_match(const vh_params *p, int32_t device, const int32_t dims[3], int32_t method, const int32_t *m1p,
                 int32_t n1p, const int32_t *m2p, int32_t n2p, const int32_t *m1c, int32_t n1c,
                 const int32_t *m2c, int32_t n2c, vh_p_match *out, int32_t cap, int32_t *n) {
  return match_stateless(p, device, dims, method, m1p, n1p, m2p, n2p, m1c, n1c, m2c, n2c, nullptr, out, cap, n);
}
int32_t vh_match_ranged(const vh_params *p, int32_t device, const int32_t dims[3], int32_t method, const int32_t *m1p,
                        int32_t n1p, const int32_t *m2p, int32_t n2p, const int32_t *m1c, int32_t n1c,
                        const int32_t *m2c, int32_t n2c, const float *ranges, vh_p_match *out, int32_t cap, int32_t *n) {
  if (!ranges) return VH_ERR_INVALID_ARG;
  return match_stateless(p, device, dims, method, m1p, n1p, m2p, n2p, m1c, n1c, m2c, n2c, ranges, out, cap, n);
}

// Matcher::refinement on caller-owned records (kernels_refine.hip: the hops of the stateful path, same device code)
int32_t vh_refine_matches(const vh_params *p, int32_t device, int32_t method, const int32_t dims[3], const uint8_t *I1p,
                          const uint8_t *I2p, const uint8_t *I1c, const uint8_t *I2c, vh_p_match *pm, int32_t n, int32_t *n_out) {
  if (!p || !dims || !n_out || n < 0 || (n > 0 && !pm) || method < 0 || method > 2) return VH_ERR_INVALID_ARG;
  int32_t rc = check_params(p);
  if (rc) return rc;
  if ((rc = check_dims(dims, true))) return rc;
  const uint8_t *img[4] = {I1p, I2p, I1c, I2c};
  const bool need[4] = {method != VH_METHOD_STEREO, method == VH_METHOD_QUAD, true, method != VH_METHOD_FLOW};
  for (int k = 0; k < 4; k++) if (need[k] && !img[k]) return VH_ERR_INVALID_ARG;
  *n_out = n;
  if (p->refinement <= 0 || n == 0) return VH_OK;  // nothing to do: nothing is launched
  if ((rc = select_device(device))) return rc;
  VhRefine rf{};
  vh_refine_setup(rf);
  rf.W = dims[0]; rf.H = dims[1]; rf.bpl = dims[2];
  rf.pitch = round_up(dims[0], 16);
  rf.plane = (int64_t)rf.pitch * dims[1];
  rf.mode = p->refinement == 2 ? 2 : 1;
  const size_t isz = (size_t)dims[2] * dims[1];
  Carver c;  // the four images | du | dv (four planes each) | the records | their keep flags
  size_t o_img[4];
  for (int k = 0; k < 4; k++) o_img[k] = c.take<uint8_t>(isz);
  const size_t o_du = c.take<uint8_t>(4 * (size_t)rf.plane), o_dv = c.take<uint8_t>(4 * (size_t)rf.plane);
  const size_t o_pm = c.take<vh_p_match>((size_t)n), o_keep = c.take<int32_t>((size_t)n);
  DeviceBlock blk;
  VH_HIP(blk.alloc(c.bytes()));
  uint8_t *d = blk.as<uint8_t>();
  rf.du = d + o_du; rf.dv = d + o_dv;
  vh_p_match *dpm = (vh_p_match *)(d + o_pm);
  int32_t *dkeep = (int32_t *)(d + o_keep);
  for (int k = 0; k < 4; k++) {
    if (!need[k]) continue;
    VH_HIP(hipMemcpy(d + o_img[k], img[k], isz, hipMemcpyHostToDevice));
    VhImages im{};
    im.base[0] = d + o_img[k]; im.stride = (int64_t)isz; im.ncam = 1; im.S = 1; im.S_total = 1;
    VhRefine rk = rf;  // planes of role k: set 0 of this launch
    rk.du += k * rf.plane; rk.dv += k * rf.plane;
    vh_launch_refine_planes(im, rk, nullptr);
    VH_HIP(hipGetLastError());
  }
  VH_HIP(hipMemcpy(dpm, pm, sizeof(vh_p_match) * (size_t)n, hipMemcpyHostToDevice));
  vh_launch_refine_records(rf, method, dpm, n, dkeep, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  std::vector<vh_p_match> out((size_t)n);
  std::vector<int32_t> keep((size_t)n);
  VH_HIP(hipMemcpy(out.data(), dpm, sizeof(vh_p_match) * (size_t)n, hipMemcpyDeviceToHost));
  VH_HIP(hipMemcpy(keep.data(), dkeep, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  int32_t k = 0;
  for (int32_t i = 0; i < n; i++) if (keep[i]) pm[k++] = out[i];
  *n_out = k;
  return VH_OK;
}

// ---- removeOutliers (+ bucketFeatures) on the device, stateless form ------------
// n_lists match lists, list l = pm[l * stride .. + counts[l]).  max_features < 1: the vote only, out[l * out_cap ..] receives
// the survivors; otherwise the survivors are bucketed as Matcher::bucketFeatures(max_features, bw, bh) does and out receives
// the bucketed lists.  The group form (vh_group_post_begin_device) is the throughput path; this one exists for tests and timing.
int32_t vh_remove_outliers_device(int32_t device, int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t lanes_per_wave,
                                  int32_t max_features, float bw, float bh, vh_p_match *out, int32_t out_cap, int32_t *out_counts,
                                  int32_t *n_triangles, float *sweep_ms) {
  return vh_remove_outliers_device_rule(device, n_lists, pm, stride, counts, lanes_per_wave, max_features, bw, bh, out, out_cap, out_counts, n_triangles,
                                        sweep_ms, nullptr);
}
// rule: NULL or VH_VOTE_REFERENCE -- the reference's vote; VH_VOTE_STOCK -- the per-method rule (include/viso_hip.h: vh_vote_rule)
int32_t vh_remove_outliers_device_rule(int32_t device, int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts, int32_t lanes_per_wave,
                                       int32_t max_features, float bw, float bh, vh_p_match *out, int32_t out_cap, int32_t *out_counts,
                                       int32_t *n_triangles, float *sweep_ms, const vh_vote_rule *rule) {
  if (rule && rule->rule != VH_VOTE_REFERENCE && (rule->rule != VH_VOTE_STOCK || rule->method < 0 || rule->method > 2)) return VH_ERR_INVALID_ARG;
  if (n_lists < 1 || !counts || !out_counts || out_cap < 0 || (out_cap > 0 && !out) || stride < 0) return VH_ERR_INVALID_ARG;
  if (max_features >= 1 && (!(bw >= 1) || !(bh >= 1))) return VH_ERR_INVALID_ARG;
  int32_t cap = 0;
  if (check_counts(counts, n_lists, stride, cap) || !pm) return VH_ERR_INVALID_ARG;
  cap = std::max(cap, 4);
  if (cap > VH_VOTE_LIST_MAX) return VH_ERR_UNSUPPORTED;  // (16-bit hull links; the sweep's angular hash has VH_VOTE_HASH_MAX slots in LDS)
  const int32_t rc = select_device(device);
  if (rc) return rc;
  VoteBuffers vb;
  DeviceBlock b_src, b_cnt;
  Event ev0, ev1;
  // the bucket grid these lists can need (matcher.cpp:150-151: floor(u_max / bw) + 1 columns, floor(v_max / bh) + 1 rows)
  int64_t grid = 1;
  if (max_features >= 1) {
    float u_max = 0, v_max = 0;
    for (int32_t l = 0; l < n_lists; l++)
      for (int32_t i = 0; i < counts[l]; i++) {
        const vh_p_match &q = pm[(size_t)l * stride + i];
        if (q.u1c > u_max) u_max = q.u1c;
        if (q.v1c > v_max) v_max = q.v1c;
      }
    grid = ((int64_t)floorf(u_max / bw) + 1) * ((int64_t)floorf(v_max / bh) + 1);
    if (!(grid >= 1) || grid > (1 << 20)) return VH_ERR_UNSUPPORTED;
  }
  VH_HIP(vb.alloc(n_lists, cap, std::max(out_cap, 1), (int32_t)grid));
  VH_HIP(vb.upload_lfsr());
  VH_HIP(b_src.alloc(sizeof(vh_p_match) * (size_t)n_lists * cap));
  VH_HIP(b_cnt.alloc(sizeof(int32_t) * (size_t)n_lists));
  vh_p_match *src = b_src.as<vh_p_match>();
  const int32_t ru = upload_strided_lists(src, cap, pm, stride, counts, n_lists);
  if (ru) return ru;
  VH_HIP(hipMemcpy(b_cnt.p, counts, sizeof(int32_t) * (size_t)n_lists, hipMemcpyHostToDevice));
  VH_HIP(ev0.create(hipEventDefault)); VH_HIP(ev1.create(hipEventDefault));
  hipEvent_t ev[2] = {ev0, ev1};
  vh_launch_vote_prep(vb.v, 0, n_lists, src, cap, b_cnt.as<int32_t>(), cap, nullptr, 1, nullptr);
  vh_launch_vote(vb.v, VhVoteRule::of(rule), lanes_per_wave, max_features, bw, bh, vb.lfsr, vb.lfsr_n, vb.out, vb.out_cap, vb.out_count, ev, nullptr, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  if (sweep_ms) VH_HIP(hipEventElapsedTime(sweep_ms, ev0, ev1));
  std::vector<VhVoteMeta> meta((size_t)n_lists);
  VH_HIP(hipMemcpy(meta.data(), vb.v.meta, sizeof(VhVoteMeta) * (size_t)n_lists, hipMemcpyDeviceToHost));
  int32_t ret = VH_OK;
  for (int32_t l = 0; l < n_lists; l++) {
    const VhVoteMeta &m = meta[(size_t)l];
    if (n_triangles) n_triangles[l] = m.ntri;
    if (m.status == VH_VOTE_TRUNCATED) { out_counts[l] = max_features >= 1 ? m.out : m.kept; ret = VH_ERR_CAPACITY; continue; }
    if (m.status != VH_VOTE_OK && m.status != VH_VOTE_SKIP) { out_counts[l] = 0; if (ret == VH_OK) ret = VH_ERR_UNSUPPORTED; continue; }
    const int32_t k = max_features >= 1 ? m.out : m.kept;
    out_counts[l] = k;
    if (k > out_cap) { ret = VH_ERR_CAPACITY; continue; }
    if (k > 0) VH_HIP(hipMemcpy(out + (size_t)l * out_cap, max_features >= 1 ? vb.out + (size_t)l * vb.out_cap : vb.v.pm + (size_t)l * cap,
                                sizeof(vh_p_match) * (size_t)k, hipMemcpyDeviceToHost));
  }
  return ret;
}

}  // extern "C"
