// gain_ref_harness.cpp -- calls the REFERENCE's own Matcher::mean (src/matcher.cpp:347-354, the helper of getGain) on
// recorded windows (test infrastructure; tools/gen_golden_gain.py compiles it against the reference tree, where that
// lies, into oracle/_ref/).  The member is private and declared inline, so the reference's matcher.cpp is compiled as
// part of this unit, behind the `#define private public` of SURVEY section 0.5.
//   gain_ref_harness <windows.bin> <means.bin>
// windows.bin: int32 W, H, bpl; bpl * H image bytes; int32 n; n x int32[4] {u_min, u_max, v_min, v_max}
// means.bin:   n x float
#include <stdint.h>
#include <stdio.h>
#include <vector>

#define private public
#include "matcher.h"
#undef private
#include "matcher.cpp"

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s windows.bin means.bin\n", argv[0]); return 2; }
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) { perror("open"); return 2; }
  int32_t d[3], n = 0;
  if (fread(d, 4, 3, in) != 3) return 3;
  std::vector<uint8_t> img((size_t)d[2] * d[1]);
  if (fread(img.data(), 1, img.size(), in) != img.size() || fread(&n, 4, 1, in) != 1) return 3;
  std::vector<int32_t> win(4 * (size_t)n);
  if (n && fread(win.data(), 4, win.size(), in) != win.size()) return 3;
  Matcher::parameters param;
  Matcher m(param);
  for (int32_t i = 0; i < n; i++) {
    const int32_t *w = &win[4 * (size_t)i];
    const float v = m.mean(img.data(), d[2], w[0], w[1], w[2], w[3]);
    fwrite(&v, 4, 1, out);
  }
  fclose(in); fclose(out);
  return 0;
}
