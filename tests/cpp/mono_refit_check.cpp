// mono_refit_check.cpp -- csrc/vh_mono.h compiled for the host (-ffp-contract=off): the row builder of the mono model
// refit (mono_normalise, mono_row9: what mono_refit_kernel and mono_final_a_kernel form per record) on records read
// from a file, the N x 9 system written to another.
//   mono_refit_check IN OUT     IN: vh_mono_model (16 doubles), int64 n, n records of 48 bytes; OUT: n x 9 doubles
// tests/test_mono_refit.py compares the rows with tests/mono_refit_oracle.py byte for byte.
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
  long long n = 0;
  if (fread(&model, sizeof(model), 1, in) != 1 || fread(&n, sizeof(n), 1, in) != 1 || n < 0) return 2;
  std::vector<vh_p_match> pm((size_t)n);
  if (n && fread(pm.data(), sizeof(vh_p_match), (size_t)n, in) != (size_t)n) return 2;
  fclose(in);
  std::vector<double> rows((size_t)n * 9);
  for (long long i = 0; i < n; i++) {
    const vh_p_match &m = pm[(size_t)i];
    mono_row9(mono_normalise(model, m.u1p, m.v1p, m.u1c, m.v1c), rows.data() + 9 * (size_t)i);
  }
  FILE *out = fopen(argv[2], "wb");
  if (!out || (n && fwrite(rows.data(), sizeof(double), rows.size(), out) != rows.size())) return 2;
  fclose(out);
  return 0;
}
