// engine_recon.hip -- the host half of vh_reconstruct_tracks (include/viso_hip.h): argument checks, the per-frame
// tables of Reconstruction (reference src/reconstruction.cpp:27-70) and the transfers around kernels_recon.hip.
// Built with -ffp-contract=off: the tables are part of the bit-for-bit contract.
#include "engine.h"
#include "vh_recon.h"

#include <numeric>

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

}  // namespace

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
  std::vector<double> frames((size_t)n_frames * VH_RECON_FRAME_DOUBLES, 0.0);
  const double K[9] = {r->f, 0, r->cu, 0, r->f, r->cv, 0, 0, 1};
  double total[16], inv[16];
  for (int32_t i = 0; i < 16; i++) total[i] = inv[i] = i % 5 == 0 ? 1.0 : 0.0;  // Tr_total[0] = Tr_inv_total[0] = eye(4)
  for (int32_t k = 0; k < n_frames; k++) {
    if (k > 0) {
      double ti[16], cur[16];
      matrix_inv4(Tr + (size_t)(k - 1) * 16, ti);
      matrix_mul(total, ti, 4, 4, 4, 4, cur);  // Tr_total.back() * Matrix::inv(Tr)
      memcpy(total, cur, sizeof(total));
      matrix_inv4(total, inv);                 // Tr_inv_total; the same inverse again is what P_total takes its rows from
    }
    double *f = frames.data() + (size_t)k * VH_RECON_FRAME_DOUBLES;
    matrix_mul(K, inv, 3, 3, 4, 4, f + VH_RECON_P);  // K * (.).getMat(0,0,2,3): rows 0..2 of the 4 x 4
    memcpy(f + VH_RECON_TINV, inv, sizeof(inv));
    for (int32_t i = 0; i < 3; i++) f[VH_RECON_C + i] = total[4 * i + 3];
  }
  // row 1 of Tr_cam_road (src/reconstruction.cpp:43-53)
  const double cam_pitch = -0.08, cam_height = 1.6;
  const double road[4] = {0.0, +cos(cam_pitch), -sin(cam_pitch), -cam_height};

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

}  // extern "C"
