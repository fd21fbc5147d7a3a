// mono_inlier_check.cpp -- csrc/vh_mono.h compiled for the host (-ffp-contract=off): the per-record test of the mono
// motion-inlier kernel (mono_center, mono_scale, sampson_inlier through mono_is_inlier) on records read from a file,
// flags written to another.
//   mono_inlier_check IN OUT     IN: vh_mono_model (16 doubles), double inlier_threshold, int64 n, n records of 48 bytes; OUT: n bytes
// tests/test_mono_inliers.py compares the flags with tests/mono_inlier_oracle.py byte for byte.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../hls-final-visual-odometry_amd/csrc/vh_mono.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return 2;
  static_assert(sizeof(vh_mono_model) == 128, "vh_mono_model");
  vh_mono_model model;
  double thr = 0;
  long long n = 0;
  if (fread(&model, sizeof(model), 1, in) != 1 || fread(&thr, sizeof(thr), 1, in) != 1 || fread(&n, sizeof(n), 1, in) != 1 || n < 0) return 2;
  std::vector<vh_p_match> pm((size_t)n);
  if (n && fread(pm.data(), sizeof(vh_p_match), (size_t)n, in) != (size_t)n) return 2;
  fclose(in);
  std::vector<unsigned char> flags((size_t)n);
  for (long long i = 0; i < n; i++) {
    const vh_p_match &m = pm[(size_t)i];
    flags[(size_t)i] = mono_is_inlier(model, m.u1p, m.v1p, m.u1c, m.v1c, thr) ? 1 : 0;
  }
  FILE *out = fopen(argv[2], "wb");
  if (!out || (n && fwrite(flags.data(), 1, (size_t)n, out) != (size_t)n)) return 2;
  fclose(out);
  return 0;
}
