// shim_reconstruction.cpp -- include/viso_hip_reconstruction.hpp compiled as the reference's callers would (g++, C++11) and
// driven over recorded match lists with vh_reconstruct_tracks STUBBED: the stub writes down the tracks it is handed and
// accepts every second one, so that association, batching (update vs updateMany) and the order of getPoints() can be
// checked without a GPU (tests/test_reconstruction.py).
//   shim_reconstruction <drive.bin> <out.bin> <k>     k updates per updateMany call (1: update)
// drive.bin as tools/recon_ref_harness.cpp; out.bin: per call int32 n_frames, n_tracks, then first[n], offsets[n + 1],
// pixels[2 * offsets[n]] (float); at the end int32 -1, int32 n_points, points (float[3]).
#include <stdio.h>
#include <vector>

#include "viso_hip_reconstruction.hpp"

static FILE *g_out;

struct Mat { double val[4][4]; };  // stands for the reference's Matrix: update is a template over .val[i][j]

extern "C" {
void vh_default_recon_params(vh_recon_params *r) { r->f = 1; r->cu = r->cv = 0; r->point_type = 1; r->min_track_length = 2; r->max_dist = 30; r->min_angle = 2; }
const char *vh_error_string(int32_t) { return ""; }
const char *vh_last_error(void) { return ""; }
int32_t vh_reconstruct_tracks(const vh_recon_params *, int32_t, int32_t n_frames, const double *, int32_t n_tracks, const int32_t *first_frame,
                              const int32_t *offsets, const float *pixels, float *points, int32_t *status, double *) {
  fwrite(&n_frames, 4, 1, g_out); fwrite(&n_tracks, 4, 1, g_out);
  fwrite(first_frame, 4, n_tracks, g_out); fwrite(offsets, 4, n_tracks + 1, g_out); fwrite(pixels, 4, 2 * (size_t)offsets[n_tracks], g_out);
  for (int32_t t = 0; t < n_tracks; t++) {
    status[t] = t % 2 ? VH_RECON_TYPE : VH_RECON_ACCEPTED;
    points[3 * t] = (float)first_frame[t]; points[3 * t + 1] = pixels[2 * offsets[t]]; points[3 * t + 2] = pixels[2 * offsets[t + 1] - 1];
  }
  return VH_OK;
}
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *in = fopen(argv[1], "rb");
  g_out = fopen(argv[2], "wb");
  const int32_t k = atoi(argv[3]);
  if (!in || !g_out || k < 1) return 2;
  int32_t n_updates = 0;
  double cal[3];
  if (fread(&n_updates, 4, 1, in) != 1 || fread(cal, 8, 3, in) != 3) return 3;
  Reconstruction rec;
  rec.setCalibration(cal[0], cal[1], cal[2]);
  std::vector<std::vector<Matcher::p_match> > lists;
  std::vector<double> trs;
  for (int32_t u = 0; u < n_updates; u++) {
    double tr[16];
    int32_t n = 0;
    if (fread(tr, 8, 16, in) != 16 || fread(&n, 4, 1, in) != 1) return 3;
    std::vector<Matcher::p_match> pm(n);
    if (n && fread(&pm[0], 48, n, in) != (size_t)n) return 3;
    if (k == 1) {
      Mat M;
      for (int i = 0; i < 16; i++) M.val[i / 4][i % 4] = tr[i];
      if (u % 2) rec.update(pm, M); else rec.update(pm, tr);
    } else {
      lists.push_back(pm); trs.insert(trs.end(), tr, tr + 16);
      if ((int32_t)lists.size() == k || u == n_updates - 1) { rec.updateMany(lists, &trs[0]); lists.clear(); trs.clear(); }
    }
  }
  const std::vector<Reconstruction::point3d> pts = rec.getPoints();
  const int32_t end = -1, np = (int32_t)pts.size();
  fwrite(&end, 4, 1, g_out); fwrite(&np, 4, 1, g_out);
  for (int32_t i = 0; i < np; i++) { const float p[3] = {pts[i].x, pts[i].y, pts[i].z}; fwrite(p, 4, 3, g_out); }
  fclose(g_out);
  return 0;
}
