// engine_lists_check.cpp -- csrc/engine_lists.h alone, compiled by a plain host compiler (tests/test_stateless_validation.py
// builds it with -fsanitize=address,undefined where the compiler has the runtime): the offsets and counts checks at their
// edges, the dims check, and the carver against the offsets the classification's block has always had -- the literals below
// are the values of  o_out = up256(slots), o_src = o_out + up256(48 * slots), o_tiles = o_src + up256(4 * slots),
// o_ninl = o_tiles + up256(4 * lists * tiles), o_ok = o_ninl + up256(4 * lists), o_tr = o_ok + up256(4 * lists),
// bytes = o_tr + up256(48 * lists).  Exit status 0 and "ok" when everything holds, else the line of the first failure.
#include "../../hls-final-visual-odometry_amd/csrc/engine_lists.h"

#include <cstdio>
#include <vector>

using namespace vh_engine;

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static bool span_is(const ListSpan &s, int64_t first, int64_t end, int64_t total, int64_t longest) {
  return s.first == first && s.end == end && s.total == total && s.longest == longest;
}

int main() {
  ListSpan s;
  // offsets
  { const int32_t o[] = {0, 5}; CHECK(check_offsets(o, 1, s) == VH_OK && span_is(s, 0, 5, 5, 5)); }              // one list
  { const int32_t o[] = {2, 9, 9, 12}; CHECK(check_offsets(o, 3, s) == VH_OK && span_is(s, 2, 12, 10, 7)); }    // an empty list in the middle
  { const int32_t o[] = {7, 7, 7, 7}; CHECK(check_offsets(o, 3, s) == VH_OK && span_is(s, 7, 7, 0, 0)); }       // all empty, offsets[0] > 0
  { const int32_t o[] = {4}; CHECK(check_offsets(o, 0, s) == VH_OK && span_is(s, 4, 4, 0, 0)); }                // n = 0: offsets[0] alone
  { const int32_t o[] = {-1}; CHECK(check_offsets(o, 0, s) == VH_ERR_INVALID_ARG); }
  { const int32_t o[] = {-1, 3}; CHECK(check_offsets(o, 1, s) == VH_ERR_INVALID_ARG); }
  { const int32_t o[] = {0, 4, 3, 8}; CHECK(check_offsets(o, 3, s) == VH_ERR_INVALID_ARG); }                    // a decreasing pair
  { const int32_t o[] = {0, 4, 8, 7}; CHECK(check_offsets(o, 3, s) == VH_ERR_INVALID_ARG); }                    // ... the last one
  { const int32_t o[] = {0, INT32_MAX}; CHECK(check_offsets(o, 1, s) == VH_OK && span_is(s, 0, INT32_MAX, INT32_MAX, INT32_MAX)); }
  CHECK(check_offsets(nullptr, 3, s) == VH_ERR_INVALID_ARG && check_offsets(nullptr, 0, s) == VH_ERR_INVALID_ARG);
  // counts
  int32_t longest = -1;
  { const int32_t c[] = {5}; CHECK(check_counts(c, 1, 5, longest) == VH_OK && longest == 5); }                  // one list, as long as the stride
  { const int32_t c[] = {3, 0, 9}; CHECK(check_counts(c, 3, 10, longest) == VH_OK && longest == 9); }           // an empty list in the middle
  { const int32_t c[] = {0, 0, 0}; CHECK(check_counts(c, 3, 0, longest) == VH_OK && longest == 0); }            // all empty, stride 0
  { const int32_t c[] = {1}; CHECK(check_counts(c, 0, 0, longest) == VH_OK && longest == 0); }                  // n = 0: nothing is read
  { const int32_t c[] = {3, 11, 2}; CHECK(check_counts(c, 3, 10, longest) == VH_ERR_INVALID_ARG); }
  { const int32_t c[] = {3, 2, -1}; CHECK(check_counts(c, 3, 10, longest) == VH_ERR_INVALID_ARG); }
  { const int32_t c[] = {1}; CHECK(check_counts(c, 1, -1, longest) == VH_ERR_INVALID_ARG); }
  CHECK(check_counts(nullptr, 0, 4, longest) == VH_ERR_INVALID_ARG);
  { std::vector<int32_t> c(70000, 2); c[69999] = 6; CHECK(check_counts(c.data(), 70000, 6, longest) == VH_OK && longest == 6); }
  // dims
  { const int32_t d[] = {640, 480, 640}; CHECK(check_dims(d, true) == VH_OK && check_dims(d, false) == VH_OK); }
  { const int32_t d[] = {640, 480, 639}; CHECK(check_dims(d, true) == VH_ERR_INVALID_ARG && check_dims(d, false) == VH_OK); }
  { const int32_t d[] = {0, 480, 640}; CHECK(check_dims(d, false) == VH_ERR_INVALID_ARG); }
  { const int32_t d[] = {640, -1, 640}; CHECK(check_dims(d, true) == VH_ERR_INVALID_ARG); }
  { const int32_t d[] = {16384, 16384, 16384}; CHECK(check_dims(d, true) == VH_OK); }
  { const int32_t d[] = {16385, 4, 16385}; CHECK(check_dims(d, true) == VH_ERR_UNSUPPORTED); }
  { const int32_t d[] = {4, 16385, 4}; CHECK(check_dims(d, false) == VH_ERR_UNSUPPORTED); }
  { const int32_t d[] = {16385, 4, 4}; CHECK(check_dims(d, true) == VH_ERR_INVALID_ARG && check_dims(d, false) == VH_ERR_UNSUPPORTED); }  // invalid wins
  CHECK(check_dims(nullptr, false) == VH_ERR_INVALID_ARG);
  // the carver: offsets, both totals, the measuring pass
  {
    Carver c;
    CHECK(c.bytes() == 0 && c.tight() == 0);
    CHECK(c.take<uint8_t>(1) == 0 && c.bytes() == 256 && c.tight() == 1);
    CHECK(c.take<double>(32) == 256 && c.bytes() == 512 && c.tight() == 512);
    CHECK(c.take<int32_t>(0) == 512 && c.bytes() == 512 && c.tight() == 512);
    CHECK(c.take<int32_t>(65) == 512 && c.bytes() == 1024 && c.tight() == 772);
    CHECK(c.ptr<int32_t>(1) == nullptr && c.tight() == 1028);
  }
  // the classification's block for (lists, slots, tiles)
  static const size_t want[3][10] = {
      // lists, slots, tiles, o_out, o_src, o_tiles, o_ninl, o_ok, o_tr, bytes
      {1, 1, 1, 256, 512, 768, 1024, 1280, 1536, 1792},
      {3, 700, 3, 768, 34560, 37376, 37632, 37888, 38144, 38400},
      {5, 256, 1, 256, 12544, 13568, 13824, 14080, 14336, 14592},
  };
  for (const auto &w : want) {
    InlierArrays n;
    CHECK(n.carve(nullptr, w[0], w[1], w[2]).bytes() == w[9]);
    CHECK(!n.d_flags && !n.d_out && !n.d_src && !n.d_tiles && !n.d_ninl && !n.d_ok && !n.d_tr);
    std::vector<uint8_t> block(w[9]);
    uint8_t *d = block.data();
    InlierArrays a;
    Carver c = a.carve(d, w[0], w[1], w[2]);
    CHECK(c.bytes() == w[9] && c.tight() == w[8] + 48 * w[0]);
    CHECK(a.d_flags == d && (uint8_t *)a.d_out == d + w[3] && (uint8_t *)a.d_src == d + w[4] && (uint8_t *)a.d_tiles == d + w[5]);
    CHECK((uint8_t *)a.d_ninl == d + w[6] && (uint8_t *)a.d_ok == d + w[7] && (uint8_t *)a.d_tr == d + w[8]);
    CHECK(c.take<int32_t>(w[0]) == w[9]);  // what a caller takes next lies behind the arrays
    // every array lies inside the block: write its first and last element
    a.d_flags[0] = a.d_flags[w[1] - 1] = 1; a.d_out[0].i1c = a.d_out[w[1] - 1].i1c = 1; a.d_src[0] = a.d_src[w[1] - 1] = 1;
    a.d_tiles[0] = a.d_tiles[w[0] * w[2] - 1] = 1; a.d_ninl[w[0] - 1] = a.d_ok[w[0] - 1] = 1; a.d_tr[6 * w[0] - 1] = 1.0;
  }
  std::puts("ok");
  return 0;
}
