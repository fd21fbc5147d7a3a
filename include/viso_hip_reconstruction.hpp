// viso_hip_reconstruction.hpp -- drop-in C++ `Reconstruction` over vh_reconstruct_tracks of libviso_hip.so.
//
// Same public surface as the reference's class (src/reconstruction.h:35-110 of Chang-Tun-Yu/HLS-final-Visual-Odometry):
// point3d, setCalibration, update with its four defaulted thresholds, getPoints.  The association of matches to tracks is
// update's own, statement for statement (src/reconstruction.cpp:72-145), and stays on the host: integer work, O(matches).
// Everything numeric -- initPoint, pointType, refinePoint, pointDistance, rayAngle for every lost track -- runs in one
// batched HIP kernel (csrc/kernels_recon.hip).  On the include path AS "reconstruction.h"  the reference's
// callers compile unchanged; `update` is a template over the matrix type, so the reference's Matrix (anything with
// .val[i][j]) is accepted without being included here.
//
// Differences a maintainer should know about:
//  * the reference indexes its track table with i1p and last_idx unchecked (src/reconstruction.cpp:87, :93): a negative
//    index reads or writes before the array.  Here a match with i1p < 0 starts a new track and a track whose last_idx
//    is negative is not entered into the table;
//  * updateMany runs k consecutive updates with ONE launch for all their lost tracks (a chunk of a sequence handle's
//    getMatchesAll): points never feed back into the association, so the points equal those of k single updates;
//  * the GPU entry is stateless: every call rebuilds the per-frame tables of the whole drive so far on the host (two 4x4
//    inversions and two products per frame, a third of a microsecond) and uploads them, so one update() per frame costs O(N^2)
//    of that over N frames -- negligible for hundreds of frames, some twenty seconds in total at 10 000.  For long drives call
//    updateMany once per chunk;
//  * errors of the GPU call are reported on std::cerr and add no points.
#ifndef VISO_HIP_RECONSTRUCTION_HPP
#define VISO_HIP_RECONSTRUCTION_HPP

#include <stdint.h>
#include <iostream>
#include <type_traits>
#include <vector>

#include "viso_hip.h"
#include "viso_hip_matcher.hpp"

class Reconstruction {
 public:
  explicit Reconstruction(int32_t device = 0) : device(device) { vh_default_recon_params(&recon); }

  // a generic 3d point (src/reconstruction.h:46-50)
  struct point3d {
    float x, y, z;
    point3d() {}
    point3d(float x, float y, float z) : x(x), y(y), z(z) {}
  };

  // src/reconstruction.h:55
  void setCalibration(double f, double cu, double cv) { recon.f = f; recon.cu = cu; recon.cv = cv; }

  // src/reconstruction.h:66 with Tr as 16 doubles, row-major
  void update(const std::vector<Matcher::p_match> &p_matched, const double Tr[16], int32_t point_type = 1, int32_t min_track_length = 2,
              double max_dist = 30, double min_angle = 2) {
    const std::vector<Matcher::p_match> *lists[1] = {&p_matched};
    run(lists, Tr, 1, point_type, min_track_length, max_dist, min_angle);
  }
  // ... with the reference's Matrix, or any type with .val[i][j]
  template <class M, class = typename std::enable_if<std::is_class<M>::value>::type>
  void update(const std::vector<Matcher::p_match> &p_matched, const M &Tr, int32_t point_type = 1, int32_t min_track_length = 2,
              double max_dist = 30, double min_angle = 2) {
    double tr[16];
    for (int32_t i = 0; i < 4; i++)
      for (int32_t j = 0; j < 4; j++) tr[4 * i + j] = Tr.val[i][j];
    update(p_matched, tr, point_type, min_track_length, max_dist, min_angle);
  }
  // lists.size() consecutive updates, Trs = 16 doubles per update back to back, one launch
  void updateMany(const std::vector<std::vector<Matcher::p_match> > &lists, const double *Trs, int32_t point_type = 1,
                  int32_t min_track_length = 2, double max_dist = 30, double min_angle = 2) {
    std::vector<const std::vector<Matcher::p_match> *> ptr(lists.size());
    for (size_t k = 0; k < lists.size(); k++) ptr[k] = &lists[k];
    if (!ptr.empty()) run(&ptr[0], Trs, (int32_t)ptr.size(), point_type, min_track_length, max_dist, min_angle);
  }

  // return currently computed 3d points (finished tracks) (src/reconstruction.h:69)
  std::vector<point3d> getPoints() { return points; }

 private:
  struct track {
    std::vector<float> pixels;  // u, v per frame
    int32_t first_frame, last_frame, last_idx;
  };

  // src/reconstruction.cpp:72-145 for one list; the lost tracks are appended to the batch instead of being solved in place
  void associate(const std::vector<Matcher::p_match> &p_matched, int32_t current_frame) {
    int32_t track_idx_max = 0;
    for (size_t m = 0; m < p_matched.size(); m++)
      if (p_matched[m].i1p > track_idx_max) track_idx_max = p_matched[m].i1p;
    for (size_t t = 0; t < tracks.size(); t++)
      if (tracks[t].last_idx > track_idx_max) track_idx_max = tracks[t].last_idx;
    std::vector<int32_t> track_idx((size_t)track_idx_max + 1, -1);
    for (size_t i = 0; i < tracks.size(); i++)
      if (tracks[i].last_idx >= 0) track_idx[tracks[i].last_idx] = (int32_t)i;  // in track order: the later track wins
    for (size_t k = 0; k < p_matched.size(); k++) {
      const Matcher::p_match &m = p_matched[k];
      const int32_t idx = m.i1p >= 0 ? track_idx[m.i1p] : -1;
      if (idx >= 0 && tracks[idx].last_frame == current_frame - 1) {
        tracks[idx].pixels.push_back(m.u1c); tracks[idx].pixels.push_back(m.v1c);
        tracks[idx].last_frame = current_frame;
        tracks[idx].last_idx = m.i1c;
      } else {
        track t;
        t.pixels.push_back(m.u1p); t.pixels.push_back(m.v1p);
        t.pixels.push_back(m.u1c); t.pixels.push_back(m.v1c);
        t.first_frame = current_frame - 1;
        t.last_frame = current_frame;
        t.last_idx = m.i1c;
        tracks.push_back(t);
      }
    }
    std::vector<track> tracks_copy;
    tracks_copy.swap(tracks);
    for (size_t t = 0; t < tracks_copy.size(); t++) {
      if (tracks_copy[t].last_frame == current_frame) tracks.push_back(tracks_copy[t]);
      else {
        first.push_back(tracks_copy[t].first_frame);
        pixels.insert(pixels.end(), tracks_copy[t].pixels.begin(), tracks_copy[t].pixels.end());
        offsets.push_back((int32_t)(pixels.size() / 2));
      }
    }
  }

  void run(const std::vector<Matcher::p_match> *const *lists, const double *Trs, int32_t n, int32_t point_type, int32_t min_track_length,
           double max_dist, double min_angle) {
    first.clear(); pixels.clear(); offsets.assign(1, 0);
    for (int32_t k = 0; k < n; k++) {
      Tr_all.insert(Tr_all.end(), Trs + 16 * k, Trs + 16 * (k + 1));
      associate(*lists[k], (int32_t)(Tr_all.size() / 16));
    }
    if (first.empty()) return;
    recon.point_type = point_type; recon.min_track_length = min_track_length; recon.max_dist = max_dist; recon.min_angle = min_angle;
    std::vector<float> pts(3 * first.size());
    std::vector<int32_t> status(first.size());
    const int32_t rc = vh_reconstruct_tracks(&recon, device, (int32_t)(Tr_all.size() / 16) + 1, &Tr_all[0], (int32_t)first.size(), &first[0],
                                             &offsets[0], &pixels[0], &pts[0], &status[0], 0);
    if (rc != VH_OK) {
      std::cerr << "ERROR: viso_hip: Reconstruction: " << vh_error_string(rc) << " " << vh_last_error() << std::endl;
      return;
    }
    for (size_t t = 0; t < first.size(); t++)
      if (status[t] == VH_RECON_ACCEPTED) points.push_back(point3d(pts[3 * t], pts[3 * t + 1], pts[3 * t + 2]));
  }

  vh_recon_params recon;
  int32_t device;
  std::vector<track> tracks;
  std::vector<double> Tr_all;  // Tr of every update so far
  std::vector<point3d> points;
  std::vector<int32_t> first, offsets;  // the batch of lost tracks of the running call
  std::vector<float> pixels;
};

#endif  // VISO_HIP_RECONSTRUCTION_HPP
