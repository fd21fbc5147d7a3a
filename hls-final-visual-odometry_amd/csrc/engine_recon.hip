// engine_recon.hip -- the host half of reconstruction (include/viso_hip.h): the per-frame tables of Reconstruction
// (reference src/reconstruction.cpp:27-70), vh_reconstruct_tracks and its transfers around kernels_recon.hip, and
// reconstruction from tracked lists -- a sequence handle's (vh_sequence_reconstruct) or the caller's
// (vh_reconstruct_lists) -- through kernels_recon_gather.hip, and the same for the S streams of
// a group stepped together (vh_group_reconstruct, section 4.9): one store, tails, gather and solve sequence per step.
// Built with -ffp-contract=off: the tables are part of the bit-for-bit contract.
#include "engine.h"

#include <numeric>
#include <optional>

using namespace vh_engine;

namespace {

// Matrix::solve (src/matrix.cpp:417-504) on an n x n system with nb right-hand sides, row-major, in place; on a singular
// pivot it returns false and leaves both where the elimination stood -- Matrix::inv hands that state out
// (src/matrix.cpp:378-387), so a singular Tr gives the tables the reference would have.
bool matrix_solve(double *A, double *B, int32_t n, int32_t nb) {
  int32_t ipiv[4] = {0, 0, 0, 0}, irow = 0, icol = 0;
  for (int32_t i = 0; i < n; i++) {
    double big = 0.0;
    for (int32_t j = 0; j < n; j++)
      if (ipiv[j] != 1)
        for (int32_t k = 0; k < n; k++)
          if (ipiv[k] == 0 && fabs(A[j * n + k]) >= big) { big = fabs(A[j * n + k]); irow = j; icol = k; }
    ++ipiv[icol];
    if (irow != icol) {
      for (int32_t l = 0; l < n; l++) std::swap(A[irow * n + l], A[icol * n + l]);
      for (int32_t l = 0; l < nb; l++) std::swap(B[irow * nb + l], B[icol * nb + l]);
    }
    if (fabs(A[icol * n + icol]) < 1e-20) return false;
    const double pivinv = 1.0 / A[icol * n + icol];
    A[icol * n + icol] = 1.0;
    for (int32_t l = 0; l < n; l++) A[icol * n + l] *= pivinv;
    for (int32_t l = 0; l < nb; l++) B[icol * nb + l] *= pivinv;
    for (int32_t ll = 0; ll < n; ll++)
      if (ll != icol) {
        const double dum = A[ll * n + icol];
        A[ll * n + icol] = 0.0;
        for (int32_t l = 0; l < n; l++) A[ll * n + l] -= A[icol * n + l] * dum;
        for (int32_t l = 0; l < nb; l++) B[ll * nb + l] -= B[icol * nb + l] * dum;
      }
  }
  return true;
}

// Matrix::inv(M) for 4 x 4 (src/matrix.cpp:378-387)
void matrix_inv4(const double M[16], double out[16]) {
  double A[16];
  memcpy(A, M, sizeof(A));
  for (int32_t i = 0; i < 16; i++) out[i] = i % 5 == 0 ? 1.0 : 0.0;
  (void)matrix_solve(A, out, 4, 4);
}

// Matrix::operator* (src/matrix.cpp:263-277): C = 0, C[i][j] += A[i][k] * B[k][j] with k ascending; B's rows are ldb apart
void matrix_mul(const double *A, const double *B, int32_t m, int32_t kk, int32_t n, int32_t ldb, double *C) {
  for (int32_t i = 0; i < m; i++)
    for (int32_t j = 0; j < n; j++) {
      double c = 0.0;
      for (int32_t k = 0; k < kk; k++) c += A[i * kk + k] * B[k * ldb + j];
      C[i * n + j] = c;
    }
}

thread_local double t_recon_kernel_ms = -1.0;

// The tables of the constructor, setCalibration and update (src/reconstruction.cpp:27-70) for one more frame: Tr == null
// starts the drive (frame `origin`: Tr_total[0] = Tr_inv_total[0] = eye(4)), otherwise Tr is the motion from the last frame.
void recon_table_push(const vh_recon_params &r, ReconTable &t, const double *Tr, int64_t origin = 0) {
  const double K[9] = {r.f, 0, r.cu, 0, r.f, r.cv, 0, 0, 1};
  double *total = t.total, *inv = t.inv;
  if (!Tr) {
    t.frames.clear(); t.first = origin;
    for (int32_t i = 0; i < 16; i++) total[i] = inv[i] = i % 5 == 0 ? 1.0 : 0.0;
  } else {
    double ti[16], cur[16];
    matrix_inv4(Tr, ti);
    matrix_mul(total, ti, 4, 4, 4, 4, cur);  // Tr_total.back() * Matrix::inv(Tr)
    memcpy(total, cur, sizeof(t.total));
    matrix_inv4(total, inv);                 // Tr_inv_total; the same inverse again is what P_total takes its rows from
  }
  t.frames.resize(t.frames.size() + VH_RECON_FRAME_DOUBLES, 0.0);
  double *f = t.frames.data() + t.frames.size() - VH_RECON_FRAME_DOUBLES;
  matrix_mul(K, inv, 3, 3, 4, 4, f + VH_RECON_P);  // K * (.).getMat(0,0,2,3): rows 0..2 of the 4 x 4
  memcpy(f + VH_RECON_TINV, inv, sizeof(t.inv));
  for (int32_t i = 0; i < 3; i++) f[VH_RECON_C + i] = total[4 * i + 3];
}

// row 1 of Tr_cam_road (src/reconstruction.cpp:43-53)
void recon_road(double road[4]) {
  const double cam_pitch = -0.08, cam_height = 1.6;
  road[0] = 0.0; road[1] = +cos(cam_pitch); road[2] = -sin(cam_pitch); road[3] = -cam_height;
}

// ---- reconstruction from tracked lists ------------------------------------------------------------------------------
// gq: the handle (profile scopes, the allocation test hook), or null for vh_reconstruct_lists
bool recon_refused(Group *gq) { return gq && gq->alloc_refused(); }

int32_t recon_grow(ReconHistory &h, Group *gq, ReconHistory::Grown &g, size_t need) {
  if (g.bytes >= need && g.b.p) return VH_OK;
  if (recon_refused(gq)) return VH_ERR_HIP;
  DeviceBlock nb;
  const size_t want = need + need / 4 + 256;
  VH_HIP(nb.alloc(want));
  h.bytes += (int64_t)want - (int64_t)g.bytes;
  g.b = std::move(nb);  // (the old block goes with nb: its readers finished with the last call, which was synchronous)
  g.bytes = want;
  return VH_OK;
}

// slots frames of `lists` lists of cap records
int32_t recon_ensure_ring(ReconHistory &h, Group *gq, int32_t slots, int32_t lists, int32_t cap) {
  if (h.b_ring.p) return VH_OK;
  const size_t b_ring = sizeof(VhReconRec) * (size_t)slots * lists * cap, b_count = sizeof(int32_t) * (size_t)slots * lists, b_tot = sizeof(unsigned long long) * 5;
  DeviceBlock ring, count, totals;
  if (recon_refused(gq)) return VH_ERR_HIP;
  VH_HIP(ring.alloc(b_ring));
  if (recon_refused(gq)) return VH_ERR_HIP;
  VH_HIP(count.alloc(b_count));
  if (recon_refused(gq)) return VH_ERR_HIP;
  VH_HIP(totals.alloc(b_tot));
  VH_HIP(hipMemset(count.p, 0, b_count));
  h.b_ring = std::move(ring); h.b_count = std::move(count); h.b_totals = std::move(totals);
  h.ring_slots = slots; h.ring_lists = lists; h.ring_cap = cap;
  h.bytes += (int64_t)(b_ring + b_count + b_tot);
  return VH_OK;
}

// store -> tails (count) -> grow -> tails (append) -> gather -> solve -> the sorted records.  `a` names the lists, the
// tail range and `check`; nothing of `h` but its buffers changes, so a failed call can simply be made again.
// tabs: one table per stream (h.ring_lists of them), all over the same frames.  out: stream after stream, stream s's
// records at [off[s], off[s + 1]), each sorted by (lost_frame, birth_frame, birth_pos); accepted: per stream.
int32_t recon_run(ReconHistory &h, Group *gq, hipStream_t st, VhReconGatherArgs a, const ReconTable *tabs, const vh_recon_params &r,
                  std::vector<vh_recon_track> &out, std::vector<int32_t> &off, std::vector<int32_t> &accepted) {
  const int32_t L = h.ring_lists;
  const ReconTable &tab = tabs[0];
  a.ring = h.b_ring.as<VhReconRec>(); a.ring_count = h.b_count.as<int32_t>(); a.ring_slots = h.ring_slots; a.ring_cap = h.ring_cap;
  a.lists_per_frame = L;
  a.totals = h.b_totals.as<unsigned long long>();
  out.clear(); off.assign((size_t)L + 1, 0); accepted.assign((size_t)L, 0);
  VH_HIP(hipMemsetAsync(a.totals, 0, sizeof(unsigned long long) * 5, st));
  { std::optional<Scope> sc; if (gq) sc.emplace(gq, "recon_store", st); vh_launch_recon_store(a, st); }
  { std::optional<Scope> sc; if (gq) sc.emplace(gq, "recon_tails", st); vh_launch_recon_tails(a, 0, st); }
  VH_HIP(hipGetLastError());
  unsigned long long tot[5] = {0, 0, 0, 0, 0};
  VH_HIP(hipMemcpyAsync(tot, a.totals, sizeof(unsigned long long) * 3, hipMemcpyDeviceToHost, st));
  VH_HIP(hipStreamSynchronize(st));
  if (tot[0] >= (1ull << 24) || tot[2] >= (1ull << 24) || tot[1] > (unsigned long long)INT32_MAX) return VH_ERR_UNSUPPORTED;  // (the appending atomic packs both; offsets are 32 bits)
  const int32_t ns = (int32_t)tot[0], nt = ns + (int32_t)tot[2];
  const size_t n_px = (size_t)tot[1];
  a.n_solved = ns; a.n_tails = nt; a.n_pixels = (int64_t)n_px;
  // the window of the tables the tracks can reach: a track of a list since tail_lo began at most `history` frames before it
  a.window0 = std::max(tab.first, a.tail_lo - a.history);
  a.window = (int32_t)(tab.first + tab.count() - a.window0);
  const size_t w_one = (size_t)a.window * VH_RECON_FRAME_DOUBLES, w_doubles = w_one * (size_t)L;  // a window per stream, stream after stream
  int32_t rc;
  if ((rc = recon_grow(h, gq, h.g_tails, sizeof(VhReconTail) * (size_t)nt))) return rc;
  if ((rc = recon_grow(h, gq, h.g_first, sizeof(int32_t) * (size_t)ns))) return rc;
  if ((rc = recon_grow(h, gq, h.g_off, sizeof(int32_t) * ((size_t)ns + 1)))) return rc;
  if ((rc = recon_grow(h, gq, h.g_order, sizeof(int32_t) * (size_t)ns))) return rc;
  if ((rc = recon_grow(h, gq, h.g_px, sizeof(float) * 2 * n_px))) return rc;
  if ((rc = recon_grow(h, gq, h.g_pts, sizeof(float) * 3 * (size_t)ns))) return rc;
  if ((rc = recon_grow(h, gq, h.g_st, sizeof(int32_t) * (size_t)ns))) return rc;
  if ((rc = recon_grow(h, gq, h.g_met, sizeof(double) * 2 * (size_t)ns))) return rc;
  if ((rc = recon_grow(h, gq, h.g_frames, sizeof(double) * w_doubles))) return rc;
  if (nt == 0) return VH_OK;
  a.tails = h.g_tails.b.as<VhReconTail>(); a.first_frame = h.g_first.b.as<int32_t>(); a.offsets = h.g_off.b.as<int32_t>();
  a.order = h.g_order.b.as<int32_t>(); a.pixels = h.g_px.b.as<float>();
  const size_t w_skip = (size_t)(a.window0 - tab.first) * VH_RECON_FRAME_DOUBLES;
  std::vector<double> windows;  // (lives until the synchronisation below)
  const double *w_src = tab.frames.data() + w_skip;
  if (L > 1) {
    windows.resize(w_doubles);
    for (int32_t s = 0; s < L; s++) memcpy(windows.data() + w_one * (size_t)s, tabs[s].frames.data() + w_skip, sizeof(double) * w_one);
    w_src = windows.data();
  }
  VH_HIP(hipMemcpyAsync(h.g_frames.b.p, w_src, sizeof(double) * w_doubles, hipMemcpyHostToDevice, st));
  { std::optional<Scope> sc; if (gq) sc.emplace(gq, "recon_tails", st); vh_launch_recon_tails(a, 1, st); }
  { std::optional<Scope> sc; if (gq) sc.emplace(gq, "recon_gather", st); vh_launch_recon_gather(a, st); }
  double road[4];
  recon_road(road);
  {
    std::optional<Scope> sc; if (gq) sc.emplace(gq, "recon_solve", st);
    vh_launch_recon(r, road, h.g_frames.b.as<double>(), ns, a.order, a.first_frame, a.offsets, a.pixels, h.g_pts.b.as<float>(), h.g_st.b.as<int32_t>(),
                    h.g_met.b.as<double>(), st);
  }
  VH_HIP(hipGetLastError());
  std::vector<VhReconTail> tails((size_t)nt);
  std::vector<float> pts(3 * (size_t)ns);
  std::vector<int32_t> stat((size_t)ns);
  std::vector<double> met(2 * (size_t)ns);
  VH_HIP(hipMemcpyAsync(tails.data(), a.tails, sizeof(VhReconTail) * (size_t)nt, hipMemcpyDeviceToHost, st));
  if (ns) {
    VH_HIP(hipMemcpyAsync(pts.data(), h.g_pts.b.p, sizeof(float) * 3 * (size_t)ns, hipMemcpyDeviceToHost, st));
    VH_HIP(hipMemcpyAsync(stat.data(), h.g_st.b.p, sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, st));
    VH_HIP(hipMemcpyAsync(met.data(), h.g_met.b.p, sizeof(double) * 2 * (size_t)ns, hipMemcpyDeviceToHost, st));
  }
  VH_HIP(hipStreamSynchronize(st));
  if ((rc = report_violation(a.check))) return rc;
  std::vector<int32_t> order((size_t)nt);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
    const VhReconTail &p = tails[(size_t)x], &q = tails[(size_t)y];
    if (p.stream != q.stream) return p.stream < q.stream;
    if (p.lost_off != q.lost_off) return p.lost_off < q.lost_off;
    if (p.birth_off != q.birth_off) return p.birth_off < q.birth_off;
    return p.birth_pos < q.birth_pos;
  });
  out.resize((size_t)nt);
  for (int32_t k = 0; k < nt; k++) {
    const int32_t t = order[(size_t)k];
    vh_recon_track &o = out[(size_t)k];
    const VhReconTail &q = tails[(size_t)t];
    if (q.stream < 0 || q.stream >= L) { t_last_error = "recon_tails: a record of no stream"; return VH_ERR_HIP; }  // (never)
    off[(size_t)q.stream + 1]++;
    memset(&o, 0, sizeof(o));
    o.birth_frame = a.window0 + q.birth_off; o.birth_pos = q.birth_pos; o.frames = q.frames; o.lost_frame = a.window0 + q.lost_off;
    if (t >= ns) { o.status = VH_RECON_HISTORY; continue; }
    o.status = stat[(size_t)t];
    for (int32_t i = 0; i < 3; i++) o.point[i] = pts[3 * (size_t)t + i];
    o.distance = met[2 * (size_t)t]; o.angle = met[2 * (size_t)t + 1];
    accepted[(size_t)q.stream] += o.status == VH_RECON_ACCEPTED ? 1 : 0;
  }
  for (int32_t s = 0; s < L; s++) off[(size_t)s + 1] += off[(size_t)s];
  return VH_OK;
}

// the getters' capacity rule
int32_t recon_copy_out(const vh_recon_track *res, size_t count, vh_recon_track *out, int32_t cap, int32_t *n) {
  *n = (int32_t)count;
  const size_t k = std::min(count, (size_t)cap);
  if (k) memcpy(out, res, sizeof(vh_recon_track) * k);
  return count > (size_t)cap ? VH_ERR_CAPACITY : VH_OK;
}

}  // namespace

// ---- the handle's state (breaks) -------------------------------------------------------------
namespace vh_engine {

// a push has succeeded; first: the ring of feature sets starts again (first push, new dims)
// shifted: the push brought a new step (group: false for a replace push, which keeps the step and voids its lists)
void Group::recon_pushed(bool first, bool shifted) {
  if (!rh.on) return;
  if (first) { rh.drop_chain(); rh.m_valid = rh.m_done = false; rh.pushes_since_match = 0; rh.replaced = false; }
  if (!seq && !first && !shifted) { rh.replaced = true; return; }
  rh.pushes_since_match++;
}

// Before the lists of a match call are linked.  The chain goes on only if this is the first match call on the chunk
// pushed right after a chunk that was matched AND reconstructed; every other order is a break.  A break also takes the
// predecessor away from the track linking, so that vh_track's age and birth -- which the ring stores -- describe the
// same tracks as the reconstruction: both start again at this chunk.
void Group::recon_before_link() {
  if (!rh.on) return;
  const bool again = rh.pushes_since_match == 0;
  bool goes_on = again ? (rh.m_valid && !rh.m_done) : (rh.pushes_since_match == 1 && rh.m_valid && rh.m_done && rh.chain);
  // group: the linking contract gives the lists of a replaced frame no predecessor, and a push covers every stream
  if (rh.replaced) { goes_on = false; rh.replaced = false; }
  if (again && goes_on) return;  // the chunk's lists are replaced: the ring has none of them yet
  if (!goes_on) { rh.drop_chain(); trk_pred_valid = false; trk_carry_src = -1; }
}

void Group::recon_matched(const VhMatchArgs &a) {
  if (!rh.on) return;
  rh.m_valid = true; rh.m_done = false; rh.pushes_since_match = 0;
  if (seq) { rh.m_first = seq_first; rh.m_lo = a.seq_lo; rh.m_rows = a.rows; return; }
  // group: a chunk of one row, the step with push serial trk_serial; the first push's step holds no pair.  The buffer of
  // its tracks is recorded too: the next push may come before the reconstruct call, and it changes trk_cur
  rh.m_first = trk_serial; rh.m_lo = trk_serial == 0 ? 1 : 0; rh.m_rows = 1; rh.m_buf = trk_cur;
}

int32_t Group::reconstruct(const double *Tr, int32_t *n_tracks, int32_t *n_accepted) {
  if (!n_tracks || !n_accepted) return VH_ERR_INVALID_ARG;
  *n_tracks = *n_accepted = 0;
  if (!rh.on || !allocated || !rh.m_valid || rh.m_done) return VH_ERR_STATE;  // (a push since the match call changes nothing)
  const int64_t F = rh.m_first;
  const int32_t lo = rh.m_lo, rows = rh.m_rows;
  if (lo < rows && !Tr) return VH_ERR_INVALID_ARG;
  if (rh.chain && rh.last != F + lo - 1) rh.drop_chain();  // (cannot happen: recon_before_link keeps the two in step)
  // The list axis: a sequence handle holds one camera, its rows are frames; a group holds S cameras, its one row is the
  // step -- the list of (row r, stream s) is list r + s * stride of the handle's arrays, and its motion Tr[r + s * stride]
  const int32_t L = recon_lists();
  const int64_t stride = seq ? 0 : 1;
  int32_t rc = recon_ensure_ring(rh, this, seq ? rh.history + S : rh.history + 1, L, mcap);
  if (rc) return rc;
  std::vector<ReconTable> tabs;
  if (rh.chain) tabs = rh.tables;
  else { tabs.resize((size_t)L); for (ReconTable &t : tabs) recon_table_push(rh.params, t, nullptr, F + lo - 1); }
  for (int32_t s = 0; s < L; s++)
    for (int32_t r = lo; r < rows; r++) recon_table_push(rh.params, tabs[(size_t)s], Tr + 16 * (size_t)(r + s * stride));
  const bool pred = rh.chain && rh.has_pending;
  VhReconGatherArgs a{};
  a.pm = (const vh_p_match *)mt.d_matches; a.pm_stride = mcap; a.counts = mt.d_match_count; a.count_cap = mcap;
  a.trk = tk.d_trk + (seq ? 0 : (size_t)rh.m_buf * S * mcap); a.trk_stride = mcap; a.stream_stride = stride;
  a.row_lo = lo; a.rows = rows; a.frame0 = F; a.pred_valid = pred ? 1 : 0; a.history = rh.history;
  a.tail_lo = pred ? F + lo - 1 : F + lo; a.tail_hi = F + rows - 1;
  a.check = sets.check;
  if (lo < rows) {
    // behind the emission and the linking of the match call, on their stream
    if ((rc = recon_run(rh, this, post_stream, a, tabs.data(), rh.params, rh.result, rh.res_off, rh.accepted))) return rc;
  } else { rh.result.clear(); rh.res_off.assign((size_t)L + 1, 0); rh.accepted.assign((size_t)L, 0); }
  // the next call reaches back `history` frames from its first tail, the list of frame F + rows - 1
  for (ReconTable &tab : tabs) {
    const int64_t keep = std::max(tab.first, F + rows - 1 - rh.history - 1);
    tab.frames.erase(tab.frames.begin(), tab.frames.begin() + (size_t)(keep - tab.first) * VH_RECON_FRAME_DOUBLES);
    tab.first = keep;
  }
  rh.tables = std::move(tabs);
  rh.chain = true; rh.has_pending = lo < rows; rh.last = F + rows - 1; rh.m_done = true;
  *n_tracks = (int32_t)rh.result.size(); *n_accepted = std::accumulate(rh.accepted.begin(), rh.accepted.end(), 0);
  return VH_OK;
}

}  // namespace vh_engine

extern "C" {

void vh_default_recon_params(vh_recon_params *r) {
  if (!r) return;
  memset(r, 0, sizeof(*r));
  r->f = 1; r->cu = 0; r->cv = 0;                                                // K = eye(3), src/reconstruction.cpp:28
  r->point_type = 1; r->min_track_length = 2; r->max_dist = 30; r->min_angle = 2;  // src/reconstruction.h:66
}

double vh_reconstruct_last_kernel_ms(void) { return t_recon_kernel_ms; }

int32_t vh_reconstruct_tracks(const vh_recon_params *r, int32_t device, int32_t n_frames, const double *Tr, int32_t n_tracks,
                              const int32_t *first_frame, const int32_t *offsets, const float *pixels, float *points, int32_t *status,
                              double *metrics) {
  if (!r || n_frames < 1 || n_tracks < 0 || (n_frames > 1 && !Tr)) return VH_ERR_INVALID_ARG;
  if (n_tracks > 0 && (!first_frame || !offsets || !pixels || !points || !status)) return VH_ERR_INVALID_ARG;
  if (n_tracks > 0 && offsets[0] < 0) return VH_ERR_INVALID_ARG;
  for (int32_t t = 0; t < n_tracks; t++) {
    const int64_t len = (int64_t)offsets[t + 1] - offsets[t];
    if (len < 1 || first_frame[t] < 0 || first_frame[t] + len > n_frames) return VH_ERR_INVALID_ARG;
  }
  if (n_tracks == 0) return VH_OK;
  const int32_t rc = select_device(device);
  if (rc) return rc;

  // the tables of the constructor, setCalibration and update (src/reconstruction.cpp:27-70), frame by frame
  ReconTable tab;
  for (int32_t k = 0; k < n_frames; k++) recon_table_push(*r, tab, k ? Tr + (size_t)(k - 1) * 16 : nullptr);
  const std::vector<double> &frames = tab.frames;
  double road[4];
  recon_road(road);

  // longest tracks first, so that the lanes of a wave run the same number of frames; outputs go to the track's own index
  std::vector<int32_t> order((size_t)n_tracks);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b]; });

  const size_t n_px = (size_t)offsets[n_tracks];
  DeviceBlock b_frames, b_order, b_first, b_off, b_px, b_pts, b_st, b_met;
  VH_HIP(b_frames.alloc(sizeof(double) * frames.size()));
  VH_HIP(b_order.alloc(sizeof(int32_t) * (size_t)n_tracks));
  VH_HIP(b_first.alloc(sizeof(int32_t) * (size_t)n_tracks));
  VH_HIP(b_off.alloc(sizeof(int32_t) * ((size_t)n_tracks + 1)));
  VH_HIP(b_px.alloc(sizeof(float) * 2 * n_px));
  VH_HIP(b_pts.alloc(sizeof(float) * 3 * (size_t)n_tracks));
  VH_HIP(b_st.alloc(sizeof(int32_t) * (size_t)n_tracks));
  if (metrics) VH_HIP(b_met.alloc(sizeof(double) * 2 * (size_t)n_tracks));
  VH_HIP(hipMemcpy(b_frames.p, frames.data(), sizeof(double) * frames.size(), hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(b_order.p, order.data(), sizeof(int32_t) * (size_t)n_tracks, hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(b_first.p, first_frame, sizeof(int32_t) * (size_t)n_tracks, hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(b_off.p, offsets, sizeof(int32_t) * ((size_t)n_tracks + 1), hipMemcpyHostToDevice));
  VH_HIP(hipMemcpy(b_px.p, pixels, sizeof(float) * 2 * n_px, hipMemcpyHostToDevice));

  hipEvent_t ev[2] = {nullptr, nullptr};
  VH_HIP(hipEventCreate(&ev[0]));
  hipError_t e = hipEventCreate(&ev[1]);
  if (e == hipSuccess) e = hipEventRecord(ev[0], nullptr);
  if (e == hipSuccess) {
    vh_launch_recon(*r, road, b_frames.as<double>(), n_tracks, b_order.as<int32_t>(), b_first.as<int32_t>(), b_off.as<int32_t>(),
                    b_px.as<float>(), b_pts.as<float>(), b_st.as<int32_t>(), metrics ? b_met.as<double>() : nullptr, nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  if (ev[1]) (void)hipEventDestroy(ev[1]);
  if (e != hipSuccess) { t_last_error = std::string("vh_reconstruct_tracks: ") + hipGetErrorString(e); return VH_ERR_HIP; }
  t_recon_kernel_ms = ms;
  VH_HIP(hipMemcpy(points, b_pts.p, sizeof(float) * 3 * (size_t)n_tracks, hipMemcpyDeviceToHost));
  VH_HIP(hipMemcpy(status, b_st.p, sizeof(int32_t) * (size_t)n_tracks, hipMemcpyDeviceToHost));
  if (metrics) VH_HIP(hipMemcpy(metrics, b_met.p, sizeof(double) * 2 * (size_t)n_tracks, hipMemcpyDeviceToHost));
  return VH_OK;
}

int32_t vh_sequence_set_reconstruction(vh_group *g, const vh_recon_params *r, int32_t history_frames) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (!gq->seq) return VH_ERR_UNSUPPORTED;
  if (gq->allocated) return VH_ERR_STATE;  // before the first push only: every list since the first frame has its place in the ring
  if (!r) { gq->rh.on = false; return VH_OK; }
  if (history_frames < 1) return VH_ERR_INVALID_ARG;
  gq->rh.on = true; gq->rh.params = *r; gq->rh.history = history_frames;
  gq->trk_on = true;
  return VH_OK;
}

int32_t vh_sequence_reconstruct(vh_group *g, const double *Tr, int32_t *n_tracks, int32_t *n_accepted) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!gq->seq) { if (n_tracks) *n_tracks = 0; if (n_accepted) *n_accepted = 0; return n_tracks && n_accepted ? VH_ERR_STATE : VH_ERR_INVALID_ARG; }
  return gq->reconstruct(Tr, n_tracks, n_accepted);
}

int32_t vh_sequence_get_recon_tracks(vh_group *g, vh_recon_track *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g;
  if (!gq || !n || cap < 0 || (cap > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (!gq->seq || !gq->rh.on || !gq->rh.m_done) return VH_ERR_STATE;  // (a group's records come per stream: vh_group_get_recon_tracks)
  return recon_copy_out(gq->rh.result.data(), gq->rh.result.size(), out, cap, n);
}

int32_t vh_group_set_reconstruction(vh_group *g, const vh_recon_params *r, int32_t history_steps) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->seq) return VH_ERR_UNSUPPORTED;  // (a sequence handle keeps its own entry)
  if (gq->allocated) return VH_ERR_STATE;
  if (!r) { gq->rh.on = false; return VH_OK; }
  if (history_steps < 1) return VH_ERR_INVALID_ARG;
  gq->rh.on = true; gq->rh.params = *r; gq->rh.history = history_steps;
  gq->trk_on = true;
  return VH_OK;
}

int32_t vh_group_reconstruct(vh_group *g, const double *Tr, int32_t *n_tracks, int32_t *n_accepted) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->seq) return VH_ERR_UNSUPPORTED;
  ENTER(gq);
  return gq->reconstruct(Tr, n_tracks, n_accepted);
}

int32_t vh_group_get_recon_tracks(vh_group *g, int32_t stream, vh_recon_track *out, int32_t cap, int32_t *n) {
  Group *gq = (Group *)g;
  if (!gq || !n || cap < 0 || (cap > 0 && !out) || stream < 0 || stream >= gq->S) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (gq->seq) return VH_ERR_UNSUPPORTED;
  if (!gq->rh.on || !gq->rh.m_done) return VH_ERR_STATE;
  const int32_t lo = gq->rh.res_off[(size_t)stream], hi = gq->rh.res_off[(size_t)stream + 1];
  return recon_copy_out(gq->rh.result.data() + lo, (size_t)(hi - lo), out, cap, n);
}

int32_t vh_group_get_recon_counts(vh_group *g, int32_t *n_tracks, int32_t *n_accepted) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->seq) return VH_ERR_UNSUPPORTED;
  if (!gq->rh.on || !gq->rh.m_done) return VH_ERR_STATE;
  for (int32_t s = 0; s < gq->S; s++) {
    if (n_tracks) n_tracks[s] = gq->rh.res_off[(size_t)s + 1] - gq->rh.res_off[(size_t)s];
    if (n_accepted) n_accepted[s] = gq->rh.accepted[(size_t)s];
  }
  return VH_OK;
}

int32_t vh_reconstruct_lists(const vh_recon_params *r, int32_t device, int32_t n_lists, const vh_p_match *pm, int64_t stride, const int32_t *counts,
                             int32_t n_index, const double *Tr, vh_recon_track *out, int32_t cap, int32_t *n) {
  if (!r || !n || n_lists < 0 || cap < 0 || (cap > 0 && !out)) return VH_ERR_INVALID_ARG;
  *n = 0;
  if (n_lists == 0) return VH_OK;
  int32_t cmax = 0;
  if (!Tr || stride < 0 || n_index < 1 || check_counts(counts, n_lists, stride, cmax)) return VH_ERR_INVALID_ARG;
  if (cmax > 0 && !pm) return VH_ERR_INVALID_ARG;
  if (cmax > (int32_t)VH_TRACK_POS_MASK || (int64_t)n_lists + 1 > (1 << 16)) return VH_ERR_UNSUPPORTED;  // (as vh_link_tracks)
  int32_t rc = select_device(device);
  if (rc) return rc;
  LinkedLists ll;
  if ((rc = link_lists_device(n_lists, pm, stride, counts, n_index, nullptr, nullptr, 0, 0, false, ll))) return rc;
  ReconHistory h;  // a whole fresh drive: list l is the list of frame l + 1, nothing is older than the history
  if ((rc = recon_ensure_ring(h, nullptr, n_lists, 1, ll.lcap))) return rc;
  ReconTable tab;
  recon_table_push(*r, tab, nullptr);
  for (int32_t l = 0; l < n_lists; l++) recon_table_push(*r, tab, Tr + 16 * (size_t)l);
  VhReconGatherArgs a{};
  a.pm = ll.d_pm; a.pm_stride = ll.lcap; a.counts = ll.d_cnt; a.count_cap = ll.lcap; a.trk = ll.d_trk; a.trk_stride = ll.lcap;
  a.row_lo = 0; a.rows = n_lists; a.frame0 = 1; a.pred_valid = 0; a.history = n_lists;
  a.tail_lo = 1; a.tail_hi = n_lists;
  a.check = ll.d_check;
  std::vector<vh_recon_track> res;
  std::vector<int32_t> off, accepted;
  if ((rc = recon_run(h, nullptr, nullptr, a, &tab, *r, res, off, accepted))) return rc;
  return recon_copy_out(res.data(), res.size(), out, cap, n);
}

int32_t vh_group_debug_reconstruct_lists(const vh_recon_params *r, int32_t device, int32_t n_streams, int32_t n_lists, const vh_p_match *pm,
                                         int64_t stride, const int32_t *counts, int32_t n_index, const double *Tr, vh_recon_track *out,
                                         int32_t cap, int32_t *n) {
  if (!r || !n || n_streams < 1 || n_lists < 1 || cap < 0 || (cap > 0 && !out) || !counts || !Tr || stride < 0 || n_index < 1) return VH_ERR_INVALID_ARG;
  const int64_t per = (int64_t)n_lists + 1, total = per * n_streams;  // an empty list behind every stream's: no track crosses it
  if (total + 1 > (1 << 16)) return VH_ERR_UNSUPPORTED;
  std::vector<int32_t> cnt((size_t)total, 0);
  std::vector<vh_p_match> rows;
  int32_t cmax = 0;
  if (check_counts(counts, (int64_t)n_streams * n_lists, stride, cmax)) return VH_ERR_INVALID_ARG;
  if (cmax > 0 && !pm) return VH_ERR_INVALID_ARG;
  if (cmax > (int32_t)VH_TRACK_POS_MASK) return VH_ERR_UNSUPPORTED;
  const int64_t rs = std::max(cmax, 1);
  rows.resize((size_t)(total * rs));
  for (int32_t s = 0; s < n_streams; s++)
    for (int32_t l = 0; l < n_lists; l++) {
      const size_t k = (size_t)s * n_lists + l, d = (size_t)(s * per + l);
      cnt[d] = counts[k];
      if (counts[k]) memcpy(rows.data() + d * rs, pm + k * (size_t)stride, sizeof(vh_p_match) * (size_t)counts[k]);
    }
  int32_t rc = select_device(device);
  if (rc) return rc;
  LinkedLists ll;
  if ((rc = link_lists_device((int32_t)total, rows.data(), rs, cnt.data(), n_index, nullptr, nullptr, 0, 0, false, ll))) return rc;
  ReconHistory h;
  if ((rc = recon_ensure_ring(h, nullptr, n_lists, n_streams, ll.lcap))) return rc;
  std::vector<ReconTable> tabs((size_t)n_streams);
  for (int32_t s = 0; s < n_streams; s++) {
    recon_table_push(*r, tabs[(size_t)s], nullptr);
    for (int32_t l = 0; l < n_lists; l++) recon_table_push(*r, tabs[(size_t)s], Tr + 16 * ((size_t)s * n_lists + l));
  }
  VhReconGatherArgs a{};
  a.pm = ll.d_pm; a.pm_stride = ll.lcap; a.counts = ll.d_cnt; a.count_cap = ll.lcap; a.trk = ll.d_trk; a.trk_stride = ll.lcap;
  a.stream_stride = per;
  a.row_lo = 0; a.rows = n_lists; a.frame0 = 1; a.pred_valid = 0; a.history = n_lists;
  a.tail_lo = 1; a.tail_hi = n_lists;
  a.check = ll.d_check;
  std::vector<vh_recon_track> res;
  std::vector<int32_t> off, accepted;
  if ((rc = recon_run(h, nullptr, nullptr, a, tabs.data(), *r, res, off, accepted))) return rc;
  for (int32_t s = 0; s < n_streams; s++) n[s] = off[(size_t)s + 1] - off[(size_t)s];
  if (res.size() > (size_t)cap) return VH_ERR_CAPACITY;
  if (!res.empty()) memcpy(out, res.data(), sizeof(vh_recon_track) * res.size());
  return VH_OK;
}

}  // extern "C"
