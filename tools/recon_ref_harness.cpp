// recon_ref_harness.cpp -- drives the REFERENCE's own Reconstruction class over a recorded drive (test infrastructure;
// tools/gen_golden_reconstruction.py compiles it against the reference tree, where that lies, into oracle/_ref/).
//   recon_ref_harness <drive.bin> <points.bin>
// drive.bin:  int32 n_updates; double f, cu, cv; per update: double Tr[16] (row-major), int32 n, n p_match records (48 bytes)
// points.bin: per update: int32 n_points, n_points x float[3] -- getPoints() after that update
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "reconstruction.h"

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s drive.bin points.bin\n", argv[0]); return 2; }
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) { perror("open"); return 2; }
  static_assert(sizeof(Matcher::p_match) == 48, "p_match");
  int32_t n_updates = 0;
  double cal[3];
  if (fread(&n_updates, 4, 1, in) != 1 || fread(cal, 8, 3, in) != 3) return 3;
  Reconstruction rec;
  rec.setCalibration(cal[0], cal[1], cal[2]);
  for (int32_t k = 0; k < n_updates; k++) {
    double tr[16];
    int32_t n = 0;
    if (fread(tr, 8, 16, in) != 16 || fread(&n, 4, 1, in) != 1) return 3;
    std::vector<Matcher::p_match> pm(n);
    if (n && fread(pm.data(), 48, n, in) != (size_t)n) return 3;
    Matrix Tr(4, 4, tr);
    rec.update(pm, Tr);
    const std::vector<Reconstruction::point3d> pts = rec.getPoints();
    const int32_t np = (int32_t)pts.size();
    fwrite(&np, 4, 1, out);
    for (int32_t i = 0; i < np; i++) { const float p[3] = {pts[i].x, pts[i].y, pts[i].z}; fwrite(p, 4, 3, out); }
  }
  fclose(in); fclose(out);
  return 0;
}
