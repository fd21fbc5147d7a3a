// engine_trajectory_cov.hip -- the covariance of the camera's pose propagated along the trajectory's chains
// (kernels_trajectory_cov.hip): on caller-owned chains of rows; on a handle, inside Group::trajectory
// (engine_trajectory.hip) from the motion and the motion covariance the device holds for the current classification; and
// its part of the ABI.
#include "engine.h"

namespace vh_engine {

static bool traj_params_ok(const vh_traj_params *tp) { return tp && (tp->on_fail == VH_TRAJ_HOLD || tp->on_fail == VH_TRAJ_REPEAT); }
static bool tcov_params_ok(const vh_traj_cov_params *tcp) { return tcp && std::isfinite(tcp->fill_scale) && tcp->fill_scale >= 0.0; }
static bool all_finite(const double *v, size_t n) {
  for (size_t q = 0; q < n; q++) if (!std::isfinite(v[q])) return false;
  return true;
}

static vh_traj_cov_carry tcov_start(const double *Sigma0) {
  vh_traj_cov_carry c{};
  if (Sigma0) std::copy(Sigma0, Sigma0 + 36, c.cov);
  return c;
}

int32_t Group::set_trajectory_covariance(const vh_traj_cov_params *tcp, const double *Sigma0) {
  if (allocated) return VH_ERR_STATE;  // before the first push only
  if (!tcp) { tcov_on = false; tcov_S0.clear(); return VH_OK; }
  if (!tcov_params_ok(tcp) || (Sigma0 && !all_finite(Sigma0, 36 * (size_t)traj_chains()))) return VH_ERR_INVALID_ARG;
  if (!traj_on) return VH_ERR_STATE;
  tcov_on = true; tcov_params = *tcp; tcov_params.reserved[0] = tcov_params.reserved[1] = 0;
  tcov_S0.clear();
  if (Sigma0) tcov_S0.assign(Sigma0, Sigma0 + 36 * (size_t)traj_chains());
  return VH_OK;
}

int32_t Group::tcov_alloc() {
  if (tcv.d_out) return VH_OK;
  const size_t chains = (size_t)traj_chains();
  const int32_t rc = dmalloc_carved(static_cast<TrajCovArrays &>(tcv), nullptr, false, (size_t)S, chains);
  if (rc) return rc;
  std::vector<vh_traj_cov_carry> start(chains);
  for (size_t c = 0; c < chains; c++) start[c] = tcov_start(tcov_S0.empty() ? nullptr : tcov_S0.data() + 36 * c);
  VH_HIP(hipMemcpy(tcv.d_cur, start.data(), sizeof(vh_traj_cov_carry) * chains, hipMemcpyHostToDevice));
  return VH_OK;
}

// behind trajectory_kernel on the post stream: the same rows, the same base
void Group::tcov_launch(const double *d_tr, const int32_t *d_ok, int32_t pair_lo, int32_t pair_hi) {
  VhTrajCovArgs a{};
  a.p = traj_params; a.fill_scale = tcov_params.fill_scale;
  a.n_chains = traj_chains(); a.rows_per_chain = seq ? S : 1;
  a.pair_lo = pair_lo; a.pair_hi = pair_hi;
  a.tr = d_tr; a.ok = d_ok; a.cov = cv.d_cov; a.ok_cov = cv.d_ok;
  a.carry_in = tcv.d_base; a.out = tcv.d_out; a.carry_out = tcv.d_cur;
  Scope sc(this, "trajectory_cov", post_stream);
  vh_launch_trajectory_cov(a, post_stream);
}

// restart (vh_group_set_pose): the chain starts again, from zero.  Otherwise (vh_group_set_pose_covariance): Sigma and
// n_filled 0 into both carries, the rest of them stays.
int32_t Group::tcov_set(int32_t s, const double *Sigma, bool restart) {
  if (!tcv.d_out) {  // nothing on the device yet: the chain's start
    if (tcov_S0.empty()) tcov_S0.assign(36 * (size_t)traj_chains(), 0.0);
    if (restart) std::fill_n(tcov_S0.begin() + 36 * (size_t)s, 36, 0.0);
    else std::copy(Sigma, Sigma + 36, tcov_S0.begin() + 36 * (size_t)s);
    return VH_OK;
  }
  VH_HIP(hipStreamSynchronize(post_stream));
  const vh_traj_cov_carry c = tcov_start(Sigma);
  for (vh_traj_cov_carry *d : {tcv.d_base + s, tcv.d_cur + s}) {
    if (restart) { VH_HIP(hipMemcpy(d, &c, sizeof c, hipMemcpyHostToDevice)); continue; }
    VH_HIP(hipMemcpy(d->cov, c.cov, sizeof c.cov, hipMemcpyHostToDevice));
    VH_HIP(hipMemcpy(&d->n_filled, &c.n_filled, sizeof c.n_filled, hipMemcpyHostToDevice));
  }
  trj.valid = false;
  return VH_OK;
}

int32_t Group::get_pose_covariances(vh_traj_cov *out) {
  if (!out) return VH_ERR_INVALID_ARG;
  if (!traj_on || !tcov_on || !trj.d_out || !tcv.d_out || !trj.valid) return VH_ERR_STATE;
  VH_HIP(hipMemcpy(out, tcv.d_out, sizeof(vh_traj_cov) * (size_t)S, hipMemcpyDeviceToHost));
  return VH_OK;
}

}  // namespace vh_engine

using namespace vh_engine;

extern "C" {

void vh_default_traj_cov_params(vh_traj_cov_params *tcp) {
  if (!tcp) return;
  tcp->fill_scale = 1.0; tcp->reserved[0] = tcp->reserved[1] = 0;
}

// One device block (offsets | tr | ok | cov | ok_cov | Sigma0 | carry in | records | carry out), one launch.
int32_t vh_trajectory_cov(const vh_traj_params *tp, const vh_traj_cov_params *tcp, int32_t device, int32_t n_chains, const int32_t *offsets,
                          const double *tr, const int32_t *ok, const double *cov, const int32_t *ok_cov, const double *Sigma0,
                          const vh_traj_cov_carry *carry_in, vh_traj_cov *out, vh_traj_cov_carry *carry_out) {
  if (!traj_params_ok(tp) || !tcov_params_ok(tcp) || n_chains < 0) return VH_ERR_INVALID_ARG;
  if (n_chains == 0) return VH_OK;
  ListSpan sp;
  if (check_offsets(offsets, n_chains, sp) || (sp.total > 0 && (!tr || !ok || !cov || !ok_cov || !out))) return VH_ERR_INVALID_ARG;
  if (n_chains > (1 << 24)) return VH_ERR_UNSUPPORTED;
  const size_t chains = (size_t)n_chains;
  if (sp.total == 0) {  // every chain ends where it starts
    if (carry_out) for (size_t c = 0; c < chains; c++) carry_out[c] = carry_in ? carry_in[c] : tcov_start(Sigma0 ? Sigma0 + 36 * c : nullptr);
    return VH_OK;
  }
  const int32_t rc = select_device(device);
  if (rc) return rc;
  int32_t *d_off = nullptr, *d_ok = nullptr, *d_okc = nullptr; double *d_tr = nullptr, *d_cov = nullptr, *d_S0 = nullptr;
  vh_traj_cov_carry *d_cin = nullptr, *d_cout = nullptr; vh_traj_cov *d_out = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    d_off = c.ptr<int32_t>(chains + 1); d_tr = c.ptr<double>(6 * (size_t)sp.end); d_ok = c.ptr<int32_t>((size_t)sp.end);
    d_cov = c.ptr<double>(36 * (size_t)sp.end); d_okc = c.ptr<int32_t>((size_t)sp.end);
    d_S0 = c.ptr<double>(Sigma0 && !carry_in ? 36 * chains : 0); d_cin = c.ptr<vh_traj_cov_carry>(carry_in ? chains : 0);
    d_out = c.ptr<vh_traj_cov>((size_t)sp.end); d_cout = c.ptr<vh_traj_cov_carry>(chains);
  }));
  VH_HIP(blk.up(d_off, offsets, chains + 1));
  VH_HIP(blk.up(d_tr + 6 * (size_t)sp.first, tr + 6 * (size_t)sp.first, 6 * (size_t)sp.total));
  VH_HIP(blk.up(d_ok + sp.first, ok + sp.first, (size_t)sp.total));
  VH_HIP(blk.up(d_cov + 36 * (size_t)sp.first, cov + 36 * (size_t)sp.first, 36 * (size_t)sp.total));
  VH_HIP(blk.up(d_okc + sp.first, ok_cov + sp.first, (size_t)sp.total));
  if (carry_in) VH_HIP(blk.up(d_cin, carry_in, chains));
  else if (Sigma0) VH_HIP(blk.up(d_S0, Sigma0, 36 * chains));
  VhTrajCovArgs a{};
  a.p = *tp; a.fill_scale = tcp->fill_scale;
  a.n_chains = n_chains; a.offsets = d_off;
  a.pair_lo = 0; a.pair_hi = INT32_MAX;
  a.tr = d_tr; a.ok = d_ok; a.cov = d_cov; a.ok_cov = d_okc;
  a.Sigma0 = carry_in ? nullptr : (Sigma0 ? d_S0 : nullptr); a.carry_in = carry_in ? d_cin : nullptr;
  a.out = d_out; a.carry_out = d_cout;
  vh_launch_trajectory_cov(a, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  VH_HIP(blk.down(out + sp.first, d_out + sp.first, (size_t)sp.total));
  if (carry_out) VH_HIP(blk.down(carry_out, d_cout, chains));
  return VH_OK;
}

int32_t vh_group_set_trajectory_covariance(vh_group *g, const vh_traj_cov_params *tcp, const double *Sigma0) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->seq) return VH_ERR_UNSUPPORTED;  // one chain over the rows: vh_sequence_set_trajectory_covariance
  return gq->set_trajectory_covariance(tcp, Sigma0);
}
int32_t vh_sequence_set_trajectory_covariance(vh_group *g, const vh_traj_cov_params *tcp, const double *Sigma0) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (!gq->seq) return VH_ERR_UNSUPPORTED;
  return gq->set_trajectory_covariance(tcp, Sigma0);
}
int32_t vh_set_trajectory_covariance(vh_matcher *m, const vh_traj_cov_params *tcp, const double *Sigma0) {
  Group *gq = (Group *)m;
  if (!gq || gq->S != 1 || gq->seq) return VH_ERR_INVALID_ARG;
  return gq->set_trajectory_covariance(tcp, Sigma0);
}
int32_t vh_group_get_pose_covariances(vh_group *g, vh_traj_cov *out) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->get_pose_covariances(out);
}
int32_t vh_get_pose_covariance(vh_matcher *m, vh_traj_cov *out) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->get_pose_covariances(out);
}
int32_t vh_group_pose_covariances_device(vh_group *g, const vh_traj_cov **d_cov, int64_t *stride) {
  Group *gq = (Group *)g;
  if (!gq || !d_cov || !stride) return VH_ERR_INVALID_ARG;
  if (!gq->traj_on || !gq->tcov_on || !gq->trj.d_out || !gq->tcv.d_out || !gq->trj.valid) return VH_ERR_STATE;
  *d_cov = gq->tcv.d_out; *stride = 1;
  return VH_OK;
}
int32_t vh_group_set_pose_covariance(vh_group *g, int32_t stream, const double *Sigma) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!Sigma || stream < 0 || stream >= gq->traj_chains() || !all_finite(Sigma, 36)) return VH_ERR_INVALID_ARG;
  if (!gq->traj_on || !gq->tcov_on) return VH_ERR_STATE;
  return gq->tcov_set(stream, Sigma, false);
}

}  // extern "C"
