// engine_lists_check.cpp -- csrc/engine_lists.h alone, compiled by a plain host compiler (tests/test_stateless_validation.py
// builds it with -fsanitize=address,undefined where the compiler has the runtime): the offsets and counts checks at their
// edges, the dims check, and the carver against the offsets the classification's block has always had -- the literals below
// are the values of  o_out = up256(slots), o_src = o_out + up256(48 * slots), o_tiles = o_src + up256(4 * slots),
// o_ninl = o_tiles + up256(4 * lists * tiles), o_ok = o_ninl + up256(4 * lists), o_tr = o_ok + up256(4 * lists),
// bytes = o_tr + up256(48 * lists); the shared checks of a packed list (packed_args, packed_limit) at their edges; and the
// two-pass layout of every stage's block: the measuring pass gives null pointers, the binding pass the offsets each stage's
// block has always had -- the literals in `stages` are the running sums of up256(sizeof(T) * count) over the arrays in the
// order the stage took them, with sizeof(vh_p_match) = 48, vh_mono_model = 128, vh_mono_pose = 152, vh_scene_point = 32 and
// 96 doubles per mono pose header -- and the first and last element of every array lie inside the block.
// Exit status 0 and "ok" when everything holds, else the line of the first failure.
#include "../../hls-final-visual-odometry_amd/csrc/engine_lists.h"

#include <cstdio>
#include <vector>

using namespace vh_engine;

static_assert(sizeof(vh_p_match) == 48 && sizeof(vh_mono_model) == 128 && sizeof(vh_mono_pose) == 152 && sizeof(vh_scene_point) == 32, "record sizes");

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
  // the shared checks of a packed list: step 1 refuses what is invalid, step 2 what no launch takes
  {
    const vh_p_match *rec = (const vh_p_match *)&s;  // (never read: the checks look at the pointer alone)
    CHECK(packed_args(nullptr, 3, rec, s) == VH_ERR_INVALID_ARG);                                                  // null offsets
    { const int32_t o[] = {-1, 2, 2, 5}; CHECK(packed_args(o, 3, rec, s) == VH_ERR_INVALID_ARG); }                 // offsets[0] < 0
    { const int32_t o[] = {0, 3, 2, 5}; CHECK(packed_args(o, 3, rec, s) == VH_ERR_INVALID_ARG); }                  // a decreasing pair
    { const int32_t o[] = {3, 3, 3, 3}; CHECK(packed_args(o, 3, nullptr, s) == VH_OK && span_is(s, 3, 3, 0, 0) && packed_limit(s, 3) == VH_OK); }  // all empty behind offsets[0] > 0: no records needed
    { const int32_t o[] = {3, 3, 4, 4}; CHECK(packed_args(o, 3, nullptr, s) == VH_ERR_INVALID_ARG); }              // records claimed, none given
    { const int32_t o[] = {3, 3, 4, 4}; CHECK(packed_args(o, 3, rec, s) == VH_OK && span_is(s, 3, 4, 1, 1) && packed_limit(s, 3) == VH_OK); }
    const int32_t pos_max = (1 << 24) - 1;  // (1 << VH_TRACK_POS_BITS) - 1
    CHECK(kListMax == pos_max && kInlierTile == 1024);
    { const int32_t o[] = {0, 0, pos_max}; CHECK(packed_args(o, 2, rec, s) == VH_OK && s.longest == pos_max && packed_limit(s, 2) == VH_OK); }
    { const int32_t o[] = {0, 0, pos_max + 1}; CHECK(packed_args(o, 2, rec, s) == VH_OK && packed_limit(s, 2) == VH_ERR_UNSUPPORTED); }
    { const int32_t o[] = {5, pos_max + 6}; CHECK(packed_args(o, 1, rec, s) == VH_OK && packed_limit(s, 1) == VH_ERR_UNSUPPORTED); }  // the length counts, not the end
    { const int32_t o[] = {0, pos_max + 1, pos_max}; CHECK(packed_args(o, 2, rec, s) == VH_ERR_INVALID_ARG); }     // invalid wins: step 1 comes first
    // inlier_grid_ok: tiles <= 65535 and lists * tiles < 2^24
    CHECK(inlier_grid_ok(1, 65535) && !inlier_grid_ok(1, 65536));
    CHECK(inlier_grid_ok(256, 65535) && !inlier_grid_ok(257, 65535));  // 256 * 65535 = 2^24 - 256
    CHECK(inlier_grid_ok((1 << 24) - 1, 1) && !inlier_grid_ok(1 << 24, 1) && inlier_grid_ok(1 << 24, 0));
    {  // ... as packed_limit applies it: lists x ceil(longest / 1024) tiles
      std::vector<int32_t> o((size_t)(1 << 13) + 1, 0);
      for (size_t i = 1; i < o.size(); i++) o[i] = 2047;  // one list of 2047 records (2 tiles), the others empty
      CHECK(packed_args(o.data(), (1 << 13) - 1, rec, s) == VH_OK && packed_limit(s, (1 << 13) - 1) == VH_OK);   // 8191 lists x 2 tiles
      CHECK(packed_limit(s, 1 << 23) == VH_ERR_UNSUPPORTED && packed_limit(s, (1 << 23) - 1) == VH_OK);           // 2^23 lists x 2 tiles = 2^24: one too many
    }
    CHECK(mono_pose_grid_ok(1 << 14, 65535) && !mono_pose_grid_ok(1 << 20, 65536) && mono_pose_grid_ok((1 << 20) - 1, 65536));
  }
  // the two-pass layout of every stage's block for (lists, slots, tiles, index entries)
  struct Stage { size_t lists, slots, tiles, entries, refit[5], cov[7], mrefit[5], mpose[8], scene[6], gidx[5], packed[4]; };  // offsets.., bytes, tight
  static const Stage stages[3] = {
      {1, 1, 1, 1, {0, 256, 512, 768, 516}, {0, 512, 768, 1024, 1280, 1536, 1284}, {0, 256, 512, 768, 516},
       {0, 256, 512, 1280, 1536, 1792, 2048, 1796}, {0, 256, 512, 768, 1024, 772}, {0, 256, 512, 768, 520}, {0, 256, 512, 264}},
      {3, 2100, 9, 77, {0, 256, 512, 768, 524}, {0, 1024, 1280, 1536, 1792, 2048, 1804}, {0, 512, 768, 1024, 780},
       {0, 16896, 33792, 36096, 36352, 36864, 37120, 36876}, {0, 67328, 67584, 68096, 68352, 68108}, {0, 512, 1024, 1280, 1040},
       {0, 100864, 101120, 100880}},
      {70, 4480, 1, 3000, {0, 3584, 4096, 4608, 4376}, {0, 20224, 20992, 21504, 25088, 25600, 25368}, {0, 8960, 10240, 10752, 10520},
       {0, 35840, 71680, 125440, 129024, 139776, 140288, 140056}, {0, 143360, 143872, 152832, 153344, 153112}, {0, 12032, 24064, 24576, 24348},
       {0, 215040, 215552, 215324}},
  };
  for (const Stage &w : stages) {
    const size_t L = w.lists;
    auto at = [](const void *p, const uint8_t *d, size_t o) { return (const uint8_t *)p == d + o; };
    {  // RefitState: tr | ok | updates
      RefitState n; Carver m; n.carve(m, L);
      CHECK(m.bytes() == w.refit[3] && m.tight() == w.refit[4] && !n.d_tr && !n.d_ok && !n.d_nupd);
      std::vector<uint8_t> block(m.bytes()); uint8_t *d = block.data();
      RefitState a; Carver c(d); a.carve(c, L);
      CHECK(c.bytes() == m.bytes() && at(a.d_tr, d, w.refit[0]) && at(a.d_ok, d, w.refit[1]) && at(a.d_nupd, d, w.refit[2]));
      a.d_tr[0] = a.d_tr[6 * L - 1] = 1.0; a.d_ok[0] = a.d_ok[L - 1] = a.d_nupd[0] = a.d_nupd[L - 1] = 1;
    }
    {  // CovState: cov | ssr | ok | tr | ok in
      CovState n; Carver m; n.carve(m, L);
      CHECK(m.bytes() == w.cov[5] && m.tight() == w.cov[6] && !n.d_cov && !n.d_ssr && !n.d_ok && !n.d_tr && !n.d_okin);
      std::vector<uint8_t> block(m.bytes()); uint8_t *d = block.data();
      CovState a; Carver c(d); a.carve(c, L);
      CHECK(c.bytes() == m.bytes() && at(a.d_cov, d, w.cov[0]) && at(a.d_ssr, d, w.cov[1]) && at(a.d_ok, d, w.cov[2]) && at(a.d_tr, d, w.cov[3]) && at(a.d_okin, d, w.cov[4]));
      a.d_cov[0] = a.d_cov[36 * L - 1] = a.d_ssr[0] = a.d_ssr[L - 1] = a.d_tr[0] = a.d_tr[6 * L - 1] = 1.0; a.d_ok[0] = a.d_ok[L - 1] = a.d_okin[0] = a.d_okin[L - 1] = 1;
    }
    {  // MonoRefitState: model | w | ok
      MonoRefitState n; Carver m; n.carve(m, L);
      CHECK(m.bytes() == w.mrefit[3] && m.tight() == w.mrefit[4] && !n.d_model && !n.d_w && !n.d_ok);
      std::vector<uint8_t> block(m.bytes()); uint8_t *d = block.data();
      MonoRefitState a; Carver c(d); a.carve(c, L);
      CHECK(c.bytes() == m.bytes() && at(a.d_model, d, w.mrefit[0]) && at(a.d_w, d, w.mrefit[1]) && at(a.d_ok, d, w.mrefit[2]));
      a.d_model[0].valid = a.d_model[L - 1].valid = 1; a.d_w[0] = a.d_w[2 * L - 1] = 1.0; a.d_ok[0] = a.d_ok[L - 1] = 1;
    }
    {  // MonoPoseArrays: dist | d | headers | tr | pose | ok
      MonoPoseArrays n; Carver m; n.carve(m, L, w.slots, 96);
      CHECK(m.bytes() == w.mpose[6] && m.tight() == w.mpose[7] && !n.d_dist && !n.d_d && !n.d_hdr && !n.d_tr && !n.d_pose && !n.d_ok);
      std::vector<uint8_t> block(m.bytes()); uint8_t *d = block.data();
      MonoPoseArrays a; Carver c(d); a.carve(c, L, w.slots, 96);
      CHECK(c.bytes() == m.bytes() && at(a.d_dist, d, w.mpose[0]) && at(a.d_d, d, w.mpose[1]) && at(a.d_hdr, d, w.mpose[2]));
      CHECK(at(a.d_tr, d, w.mpose[3]) && at(a.d_pose, d, w.mpose[4]) && at(a.d_ok, d, w.mpose[5]));
      a.d_dist[0] = a.d_dist[w.slots - 1] = a.d_d[0] = a.d_d[w.slots - 1] = a.d_hdr[0] = a.d_hdr[96 * L - 1] = a.d_tr[0] = a.d_tr[6 * L - 1] = 1.0;
      a.d_pose[0].candidate = a.d_pose[L - 1].candidate = 1; a.d_ok[0] = a.d_ok[L - 1] = 1;
    }
    {  // SceneArrays: points | tile counts | Tw | counts
      SceneArrays n; Carver m; n.carve(m, L, w.slots, w.tiles);
      CHECK(m.bytes() == w.scene[4] && m.tight() == w.scene[5] && !n.d_out && !n.d_tiles && !n.d_Tw && !n.d_n);
      std::vector<uint8_t> block(m.bytes()); uint8_t *d = block.data();
      SceneArrays a; Carver c(d); a.carve(c, L, w.slots, w.tiles);
      CHECK(c.bytes() == m.bytes() && at(a.d_out, d, w.scene[0]) && at(a.d_tiles, d, w.scene[1]) && at(a.d_Tw, d, w.scene[2]) && at(a.d_n, d, w.scene[3]));
      a.d_out[0].src_pos = a.d_out[w.slots - 1].src_pos = 1; a.d_tiles[0] = a.d_tiles[L * w.tiles - 1] = 1; a.d_Tw[0] = a.d_Tw[16 * L - 1] = 1.0; a.d_n[0] = a.d_n[L - 1] = 1;
    }
    {  // GainIndexArrays: entries | ratios | offsets, in a block as long as tight() says
      GainIndexArrays n; Carver m; n.carve(m, w.entries, L);
      CHECK(m.bytes() == w.gidx[3] && m.tight() == w.gidx[4] && !n.d_idx && !n.d_idx_ratio && !n.d_idx_off);
      std::vector<uint8_t> block(m.tight()); uint8_t *d = block.data();
      GainIndexArrays a; Carver c(d); a.carve(c, w.entries, L);
      CHECK(c.tight() == m.tight() && at(a.d_idx, d, w.gidx[0]) && at(a.d_idx_ratio, d, w.gidx[1]) && at(a.d_idx_off, d, w.gidx[2]));
      a.d_idx[0] = a.d_idx[w.entries - 1] = 1; a.d_idx_ratio[0] = a.d_idx_ratio[w.entries - 1] = 1.0f; a.d_idx_off[0] = a.d_idx_off[L] = 1;
    }
    {  // PackedArrays: records up to offsets[n] | offsets
      ListSpan sp; sp.first = 0; sp.end = sp.total = sp.longest = (int64_t)w.slots;
      PackedArrays n; Carver m; n.carve(m, sp, L);
      CHECK(m.bytes() == w.packed[2] && m.tight() == w.packed[3] && !n.d_pm && !n.d_off);
      std::vector<uint8_t> block(m.bytes()); uint8_t *d = block.data();
      PackedArrays a; Carver c(d); a.carve(c, sp, L);
      CHECK(c.bytes() == m.bytes() && at(a.d_pm, d, w.packed[0]) && at(a.d_off, d, w.packed[1]));
      a.d_pm[0].i1c = a.d_pm[w.slots - 1].i1c = 1; a.d_off[0] = a.d_off[L] = 1;
    }
  }
  std::puts("ok");
  return 0;
}
