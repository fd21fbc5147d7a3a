// kernels_match.hip -- binned 32-byte SAD matching on gfx950.
//
// Replaces Matcher::findMatch (reference src/matcher.cpp:216-272) and the
// circle-match compositions of Matcher::matching (src/matcher.cpp:274-344).
//
// Restructuring relative to the reference (results identical):
//  * The reference calls findMatch on demand along each match chain.  findMatch
//    is a pure function of (query feature, candidate set), so here every pass
//    of a chain is evaluated for ALL features of its query set at once
//    (`match`), and the chains are then followed by table look-ups (`chain`).
//  * Mapping (flow_tile / rows_tile below): one wavefront per tile of <= 32 consecutive queries
//    of one class -- in SNAKE order over the (class, u-bin) columns for the flow passes
//    (kernels_bin.hip: make_tiles; the queries' order is free, only the candidates' positions carry
//    the tie-break), in (class, v) row order for the 1-d stereo passes.  The 64 lanes are
//    4 phases of 16 lanes, lane (phase, l) holds queries l and l+16, so every phase holds the
//    whole tile; the candidate region of the tile -- the union of its queries' bin ranges -- is
//    streamed through two wave-private LDS buffers of 64 candidates filled by LDS-DMA
//    (walk_region_lds), and the four phases take candidates j, j+1, j+2, j+3 of a buffer in the
//    same step: one candidate stream shared by all phases, every record read from LDS serves two
//    queries per lane, 8 v_sad_u8 / v_sad_hi_u8 per pair, the partial minima joined by two
//    row swaps per tile (join_phases).
//    Positions in bin order ARE the reference's visiting order, so its first-minimum tie-break
//    (strict `<`, src/matcher.cpp:264) is the minimum of the key (SAD << 19 | position) -- or
//    (SAD << 16 | position - class base), which the v_sad_hi_u8 chain produces by itself --
//    whatever order candidates arrive in.
//  * The accept test of src/matcher.cpp:249 is applied per pair only in the "tested" form of the
//    loops.  The default, speculative form applies none: every lane takes the minimum over the
//    whole region the wave walks, a superset of its own window, tests ONE candidate at the end --
//    its winner -- and the few queries whose winner lies outside their own window are searched
//    again exactly, in groups sharing one walk (finish_tile / RedoGroup).  Either way the result
//    is findMatch's; engine.hip picks the form per launch from the observed share of such queries.
#include "vh_findmatch.h"
#include "vh_wave.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#ifdef VH_FLOW_STATS
// debug build only (EXTRA=-DVH_FLOW_STATS): what the flow search executed --
// [0] tiles [1] chunks [2..4] trips without test / v test / full test [5] queries [6] columns [7] queries searched again
__device__ unsigned long long g_flow_stats[12];  // [8] stereo tiles [9] stereo trips [10] stereo queries searched again [11] stereo queries
extern "C" int32_t vh_debug_flow_stats(unsigned long long *out, int32_t reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_flow_stats), sizeof(g_flow_stats)) != hipSuccess) return -3;
  if (reset) { unsigned long long z[12] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_flow_stats), z, sizeof(z)) != hipSuccess) return -3; }
  return 0;
}
#define VH_STAT(k, n) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_flow_stats[k], (unsigned long long)(n)); } while (0)
#else
#define VH_STAT(k, n) do { } while (0)
#endif

// register budget of match_kernel: at least this many waves per SIMD must fit (the loop hides its LDS and L2
// round trips behind other waves; 99 registers / 4 waves measured 7 % slower than 68 / 7)
#ifndef VH_MATCH_WAVES
#define VH_MATCH_WAVES 7
#endif

namespace {

// All-reduce over each 16-lane row of the wave with DPP row rotations (no LDS, no
// bpermute): afterwards every lane holds the extremum of its row.
template <bool MAX>
__device__ __forceinline__ int32_t row16_allreduce(int32_t v) {
#define VH_ROW_STEP(CTRL)                                                                   \
  {                                                                                         \
    const int32_t t = __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);             \
    v = MAX ? max(v, t) : min(v, t);                                                        \
  }
  VH_ROW_STEP(0x128)  // row_ror:8
  VH_ROW_STEP(0x124)  // row_ror:4
  VH_ROW_STEP(0x122)  // row_ror:2
  VH_ROW_STEP(0x121)  // row_ror:1
#undef VH_ROW_STEP
  return v;
}

// Gathers of the tiles.  Every array base below is wave-uniform and every index is below 2^24, so a lane's address is
// a uniform base plus a 32-bit BYTE offset: the scalar-base form of the global loads and stores (base in two scalar
// registers, offset in one vector register) instead of a sign extension and a 64-bit shift-and-add per access.
template <class T>
__device__ __forceinline__ T ld_off(const T *base, uint32_t byte_off) { return *(const T *)((const char *)base + byte_off); }
template <class T>
__device__ __forceinline__ void st_off(T *base, uint32_t byte_off, T x) { *(T *)((char *)base + byte_off) = x; }
// A wave-uniform word of the index arrays (tile records, bin and row starts).  match_kernel only reads them -- earlier
// kernels of the stream wrote them -- but it also stores (the tables), so through a plain pointer the compiler has to
// assume they may change and emits a vector load plus v_readfirstlane.  Read through the constant address space the
// same access is one scalar load.
template <class T>
__device__ __forceinline__ T ld_uniform(const T *p) { return *(const __attribute__((address_space(4))) T *)(uintptr_t)p; }
__device__ __forceinline__ int32_t ld_uniform_i32(const int32_t *p) { return __builtin_amdgcn_readfirstlane(ld_uniform(p)); }

// The candidate stream of a tile of the flow search: every candidate of class c in
// the bins [UB0, UB1] x [VB0, VB1] (u-bin major, as Matcher::findMatch visits them,
// matcher.cpp:243-246), in chunks of <= 64 consecutive positions of one column.
// walk_columns is the part the two walkers below share: the column table (first/last
// position of up to 64 columns, one column per lane, one round trip per batch of
// columns) and the chunk cursor over it.  How a chunk's records travel is theirs:
//   first(pc, p1): start the first chunk [pc, min(pc+64, p1)) of a batch on its way
//   step(pc, p1, pa0, pa1, more, npc, np1): if `more`, start the next chunk [npc, ..)
//   of a column ending at np1, then wait for and consume chunk [pc, min(pc+64, p1)) of
//   a column ending at p1; [pa0, pa1) = its positions inside EVERY query's window
//   (TESTED only; pa0 > pa1 marks a column that is not inside every query's u window).
template <bool TESTED, class First, class Step>
__device__ __forceinline__ void walk_columns(const VhSets &s, const int32_t *__restrict__ cbs, int32_t c, int32_t UB0, int32_t UB1, int32_t VB0,
                                             int32_t VB1, int32_t ULO_MAX, int32_t UHI_MIN, int32_t VA0, int32_t VA1, First first, Step step) {
  const int32_t lane = threadIdx.x & 63;
  // When the v range covers every v-bin (2*radius >= H, as at KITTI size), the columns
  // [UB0, UB1] are one contiguous run of positions: walk it as a single column -- fewer,
  // fuller chunks and one rounding of the tail instead of one per column.
  const bool merged = !TESTED && VB0 == 0 && VB1 == s.vbn - 1;
  const int32_t UB1w = merged ? UB0 : UB1;
  for (int32_t cb = UB0; cb <= UB1w; cb += 64) {
    const int32_t ncb = min(64, UB1w - cb + 1);
    int32_t t_p0 = 0, t_p1 = 0, t_a0 = 0, t_a1 = 0;
    if (lane < ncb) {
      const int32_t row = (c * s.ubn + cb + lane) * s.vbn;
      t_p0 = ld_off(cbs, (uint32_t)(row + VB0) * 4u);
      t_p1 = ld_off(cbs, (uint32_t)(merged ? (c * s.ubn + UB1 + 1) * s.vbn : row + VB1 + 1) * 4u);
      if (TESTED) {
        const int32_t ubx = cb + lane;
        const bool in_ = ubx * s.binsize >= ULO_MAX && ubx * s.binsize + s.binsize - 1 <= UHI_MIN;
        // an interior column without untested bins has t_a0 == t_a1 == t_p1
        t_a0 = in_ ? ((VA0 <= VA1) ? cbs[row + VA0] : t_p1) : 1;
        t_a1 = in_ ? ((VA0 <= VA1) ? cbs[row + VA1 + 1] : t_p1) : 0;
      }
    }
    // chunk cursor: column ci of the batch, positions [pc, p1)
    int32_t ci = -1, pc = -64, p1 = 0;
    const auto advance = [&]() -> bool {  // to the next non-empty chunk; false past the last one (wave-uniform)
      pc += 64;
      while (pc >= p1) {
        if (++ci >= ncb) return false;
        pc = __builtin_amdgcn_readlane(t_p0, ci); p1 = __builtin_amdgcn_readlane(t_p1, ci);
      }
      return true;
    };
    if (!advance()) continue;
    first(pc, p1);
    for (;;) {
      const int32_t c_pc = pc, c_p1 = p1, c_ci = ci;
      const bool more = advance();
      int32_t pa0 = 1, pa1 = 0;
      if (TESTED) { pa0 = __builtin_amdgcn_readlane(t_a0, c_ci); pa1 = __builtin_amdgcn_readlane(t_a1, c_ci); }
      step(c_pc, c_p1, pa0, pa1, more, pc, p1);
      if (!more) break;
    }
  }
}

// The stream through registers, one record per lane (lane j: candidate min(pc+j, p1-1), so the lanes past the end
// of a column repeat its last candidate).  Software-pipelined: the records of chunk k+1 are in flight while
// `consume` works on chunk k.  With 16..32 queries per tile a chunk is only a few
// hundred cycles of work, less than one L2 round trip; unpipelined, those round
// trips (two per column for the table, one per chunk for the records) bounded
// small tiles.
//   consume(pc, p1, pa0, pa1, pl, gu, g0, g1): pl/gu/g0/g1 = this lane's candidate position, u|v<<16 (NEED_UV only)
//   and descriptor.
template <bool TESTED, bool NEED_UV, class Consume>
__device__ __forceinline__ void walk_region(const VhSets &s, const int32_t *__restrict__ cbs, const uint32_t *__restrict__ cuv,
                                            const uint4 *__restrict__ cdesc, int32_t c, int32_t UB0, int32_t UB1, int32_t VB0,
                                            int32_t VB1, int32_t ULO_MAX, int32_t UHI_MIN, int32_t VA0, int32_t VA1,
                                            Consume consume) {
  const int32_t lane = threadIdx.x & 63;
  int32_t pl = 0;
  uint32_t gu = 0;
  uint4 g0, g1;
  const auto load = [&](int32_t pc, int32_t p1) __attribute__((always_inline)) {
    pl = min(pc + lane, p1 - 1);
    if (NEED_UV) gu = cuv[pl];
    g0 = cdesc[2 * (int64_t)pl]; g1 = cdesc[2 * (int64_t)pl + 1];
  };
  walk_columns<TESTED>(s, cbs, c, UB0, UB1, VB0, VB1, ULO_MAX, UHI_MIN, VA0, VA1, load,
    [&](int32_t pc, int32_t p1, int32_t pa0, int32_t pa1, bool more, int32_t npc, int32_t np1) __attribute__((always_inline)) {
      const int32_t c_pl = pl;
      const uint32_t c_gu = gu;
      const uint4 c_g0 = g0, c_g1 = g1;
      if (more) load(npc, np1);  // next chunk's records: in flight while this one is consumed
      consume(pc, p1, pa0, pa1, c_pl, c_gu, c_g0, c_g1);
    });
}

// LDS-DMA (gfx950 global_load_lds_*): a wave-instruction copies 64 x 16 (or 4) bytes from per-lane global
// addresses straight to LDS at M0 + lane * size -- no VGPR destination, no ds_write.  hipcc does not count an asm
// memory operation, so completion is waited for by hand (vmcnt) before the chunk is read; the builtin form makes
// hipcc drain every DMA (vmcnt(0)) before ANY ds_read, which would serialise the prefetch of the next chunk.
// The source is a wave-uniform base (scalar registers) plus a per-lane 32-bit byte offset.
__device__ __forceinline__ void glds16(const void *gbase, uint32_t byte_off, uint32_t lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(byte_off), "s"(gbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds4(const void *gbase, uint32_t byte_off, uint32_t lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(byte_off), "s"(gbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ uint32_t lds_addr(const void *p) {
  return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p);
}

// The stream for the flow tiles, consumed from LDS: the records of a chunk travel global -> LDS by LDS-DMA into one
// of two wave-private buffers (wD: 2 x {64 first halves | 64 second halves}, wU: 2 x 64 u|v<<16 words, TESTED only),
// chunk k+1 in flight while `consume` reads chunk k.  No staging
// registers, no register copies of a software pipeline, no ds_write: ~10 instead of ~35 VALU instructions per chunk.
//   consume(pc, p1, pa0, pa1, cD, cU): chunk [pc, min(pc+64, p1)) staged at cD / cU (slot j: candidate min(pc+j, p1-1))
template <bool TESTED, class Consume>
__device__ __forceinline__ void walk_region_lds(const VhSets &s, const int32_t *__restrict__ cbs, const uint32_t *__restrict__ cuv,
                                                const uint4 *__restrict__ cdesc, int32_t c, int32_t UB0, int32_t UB1, int32_t VB0,
                                                int32_t VB1, int32_t ULO_MAX, int32_t UHI_MIN, int32_t VA0, int32_t VA1,
                                                uint4 *wD, uint32_t *wU, Consume consume) {
  const uint32_t ldsD = lds_addr(wD), ldsU = lds_addr(wU);
  const uint32_t lane32 = (uint32_t)(threadIdx.x & 63) * 32u;
  const auto issue = [&](int32_t b, int32_t pc, int32_t p1) __attribute__((always_inline)) {  // chunk [pc, p1) -> buffer b
    // 32 * min(pc + lane, p1 - 1) with the scalar terms shifted on the scalar unit: one add and one min per chunk
    const uint32_t off = min((uint32_t)pc * 32u + lane32, (uint32_t)(p1 - 1) * 32u);
    glds16(cdesc, off, ldsD + (uint32_t)b * 2048u); glds16(cdesc, off + 16u, ldsD + (uint32_t)b * 2048u + 1024u);
    if (TESTED) glds4(cuv, off >> 3, ldsU + (uint32_t)b * 256u);
  };
  int32_t buf = 0;
  walk_columns<TESTED>(s, cbs, c, UB0, UB1, VB0, VB1, ULO_MAX, UHI_MIN, VA0, VA1,
    [&](int32_t pc, int32_t p1) __attribute__((always_inline)) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every read of the buffers by an earlier walk has returned
      buf = 0;
      issue(0, pc, p1);
    },
    [&](int32_t pc, int32_t p1, int32_t pa0, int32_t pa1, bool more, int32_t npc, int32_t np1) __attribute__((always_inline)) {
      const int32_t c_buf = buf;
      if (more) {
        buf ^= 1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // chunk k-1, the last reader of this buffer, is consumed
        issue(buf, npc, np1);
        if (TESTED) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");  // chunk k has landed (k+1 may be in flight)
        else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      consume(pc, p1, pa0, pa1, (const uint4 *)(wD + c_buf * 128), (const uint32_t *)(wU + c_buf * 64));
    });
}

// One candidate (this lane's) against ONE wave-uniform query with the literal accept
// test of matcher.cpp:249: the key (SAD << 32 | position - pbase), or ~0.
// The slow, exact path behind the speculative searches below (lanes over candidates).
__device__ __forceinline__ uint64_t tested_key_uniform_query(const uint32_t (&qd)[8], us2 lo2, us2 span2, uint32_t uv2,
                                                             const uint4 &b0, const uint4 &b1, uint32_t relpos) {
  const bool out = outside_window(uv2, lo2, span2);
  const uint32_t sad = sad32(make_uint4(qd[0], qd[1], qd[2], qd[3]), make_uint4(qd[4], qd[5], qd[6], qd[7]), b0, b1, 0);
  return out ? ~0ull : (((uint64_t)sad << 32) | relpos);
}

// Match keys.  The minimum of (SAD, bin-order position relative to the first position of
// the class) in lexicographic order is findMatch's first strict minimum (matcher.cpp:264),
// because positions in bin order are the reference's visiting order.  Three encodings:
//   KEY_HI16  SAD << 16 | position: straight out of a v_sad_hi_u8 chain (it accumulates at
//             bit 16) seeded with the position; classes of < 2^16 - 64 features
//   KEY_W19   SAD << 19 | position from a v_sad_u8 chain and one v_lshl_or_b32
//             (SAD <= 8160 < 2^13); classes of <= VH_CLASS_POS_MAX features
//   KEY_64    SAD << 32 | position in 64 bits (compare + two selects per candidate):
//             any class size -- only images of more than 524 224 NMS blocks can need it
// rows_tile builds these per candidate; flow_tile builds a chunk-local KEY_HI16 key per candidate in every mode and
// one key of the class's encoding per query and chunk (see there).
enum { KEY_HI16 = 0, KEY_W19 = 1, KEY_64 = 2 };
template <int KM> struct KeyT { typedef uint32_t type; };
template <> struct KeyT<KEY_64> { typedef uint64_t type; };
template <int KM>
__device__ __forceinline__ typename KeyT<KM>::type sad_key(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1, uint32_t seed) {
  if (KM == KEY_HI16) return (typename KeyT<KM>::type)sad32<true>(a0, a1, b0, b1, seed);
  const uint32_t sad = sad32(a0, a1, b0, b1, 0);
  if (KM == KEY_W19) return (typename KeyT<KM>::type)((sad << 19) | seed);
  return (typename KeyT<KM>::type)(((uint64_t)sad << 32) | seed);
}
// The smallest key that stands for "no candidate": a SAD field of 0xFFFF (0x1FFF in 19-bit keys; no SAD exceeds 8160)
// over a zero position field.  ~0 is one such key; flow_tile's rejected candidates end as this one plus a position.
template <int KM>
__device__ __forceinline__ typename KeyT<KM>::type key_none_floor() {
  typedef typename KeyT<KM>::type key_t;
  return KM == KEY_HI16 ? (key_t)0xFFFF0000u : KM == KEY_W19 ? (key_t)0xFFF80000u : (key_t)0x0000FFFF00000000ull;
}
__device__ __forceinline__ int32_t key_mode_of(int32_t class_count, int32_t wide_keys) {
  // (+64: the copies past the end of a run carry positions up to 63 past it)
  if (class_count + 64 <= 0x10000 && !wide_keys) return KEY_HI16;
  return class_count <= VH_CLASS_POS_MAX && wide_keys < 2 ? KEY_W19 : KEY_64;
}

// Joins the partial minima of the four phases (lanes l, l + 16, l + 32, l + 48 hold those of the same two queries)
// and returns ONE winner per lane: the class-relative position of the winner of query slot 0 in lanes 0-31, of slot 1
// in lanes 32-63 (-1: none), each on both 16-lane rows of its half.
//   32-bit keys: their order is the order of (SAD, position), so the join stays in key space.  v_permlane32_swap with
//   slot 0's keys as the first and slot 1's as the second operand leaves {k0[l], k0[l + 32]} in lanes l < 32 and
//   {k1[l - 32], k1[l]} in lanes l >= 32: one swap and one v_min_u32 join the halves of BOTH slots.  v_permlane16_swap
//   of the result with itself pairs every row with its neighbour: a second swap and min complete the join.  Two swaps
//   and two minima per tile, no LDS; the round-5 form widened each key to 64 bits first and paid two ds_bpermute, a
//   64-bit compare and two selects per step and slot (31 VALU instructions per tile against 7).
//   64-bit keys: shuffles and 64-bit minima as before; each half then keeps its slot.
template <int Q, int P, int KM>
__device__ __forceinline__ int32_t join_phases(const typename KeyT<KM>::type (&best_key)[Q]) {
  static_assert(Q == 2 && P == 4, "the join splits the wave into two slots of two 16-lane rows");
  if (KM == KEY_64) {
    uint64_t k[Q];
#pragma unroll
    for (int32_t qi = 0; qi < Q; qi++) {
      k[qi] = (uint64_t)best_key[qi];
#pragma unroll
      for (int32_t d = 16; d < 64; d <<= 1) k[qi] = min(k[qi], vh_shfl_xor_u64(k[qi], d));
    }
    const uint64_t kk = (threadIdx.x & 32) ? k[1] : k[0];
    return kk >= key_none_floor<KEY_64>() ? -1 : (int32_t)(uint32_t)kk;
  }
  const auto h = __builtin_amdgcn_permlane32_swap((uint32_t)best_key[0], (uint32_t)best_key[1], false, false);
  const uint32_t kh = min(h[0], h[1]);
  const auto r = __builtin_amdgcn_permlane16_swap(kh, kh, false, false);
  const uint32_t k = min(r[0], r[1]);
  return k >= key_none_floor<KM>() ? -1 : (int32_t)(k & (KM == KEY_HI16 ? 0xFFFFu : 0x7FFFFu));
}

// Second half of the speculative searches.  A query whose winner over the walked region lies
// outside its own window is searched again with the literal accept test of matcher.cpp:249, lanes
// over candidates.  Up to VH_REDO_G such queries of a tile share ONE walk over the union of their
// own regions: the candidate records are loaded once per group (round 2 walked once per query, and
// that stream of 40 KB per query, not the arithmetic, is what made the speculative form lose on
// images full of features without a partner), every lane tests its candidate against each query of
// the group (descriptors and windows wave-uniform, in scalar registers).  Measured on MI355X (KITTI, S = 256,
// speculative loops forced, k pairs/s at noise 0 / +-1 / +-2 grey levels; the tested loops: 101.9 / 67.2 / 48.5):
// G = 1: 101.3 / 55.3 / 38.0, G = 2: 101.1 / 60.3 / 42.1, G = 4: 100.9 / 62.7 / 43.9, G = 8: 93.1* / 58.2 / 42.0
// (* with the position tables of branch exp/position-tables).  Round 2's one-walk-per-query form: 51.9 / 34.0.
#ifndef VH_REDO_G
#define VH_REDO_G 2
#endif
struct RedoGroup {
  uint32_t qd[VH_REDO_G][8];  // descriptors (wave-uniform)
  us2 lo2[VH_REDO_G];         // window origins
  int32_t lane[VH_REDO_G], n;  // lane: the lane of finish_tile that owns the query
  int32_t umin, umax, vmin, vmax;
};
// Takes up to VH_REDO_G lanes off the ballot `todo`; false when none is left.  A lane of the ballot stands for its own
// query slot (finish_tile: lane >> 5), lowest lane first: slot 0's queries before slot 1's, each in tile order.
template <int Q>
__device__ __forceinline__ bool redo_take(uint64_t &todo, const uint4 (&a0)[Q], const uint4 (&a1)[Q], const uint32_t (&uv1)[Q],
                                          int32_t radius, int32_t rv, RedoGroup &g) {
  g.n = 0; g.umin = g.vmin = 0x7FFFFFFF; g.umax = g.vmax = -1;
#pragma unroll
  for (int32_t k = 0; k < VH_REDO_G; k++) {
    if (!todo) break;  // wave-uniform
    const int32_t fl = (int32_t)__builtin_ctzll(todo), fq = fl >> 5;
    todo &= todo - 1;
    uint4 x0 = a0[0], x1 = a1[0];
    uint32_t xu = uv1[0];
#pragma unroll
    for (int32_t qi = 1; qi < Q; qi++) if (fq == qi) { x0 = a0[qi]; x1 = a1[qi]; xu = uv1[qi]; }
    g.qd[k][0] = __builtin_amdgcn_readlane(x0.x, fl); g.qd[k][1] = __builtin_amdgcn_readlane(x0.y, fl);
    g.qd[k][2] = __builtin_amdgcn_readlane(x0.z, fl); g.qd[k][3] = __builtin_amdgcn_readlane(x0.w, fl);
    g.qd[k][4] = __builtin_amdgcn_readlane(x1.x, fl); g.qd[k][5] = __builtin_amdgcn_readlane(x1.y, fl);
    g.qd[k][6] = __builtin_amdgcn_readlane(x1.z, fl); g.qd[k][7] = __builtin_amdgcn_readlane(x1.w, fl);
    const uint32_t quv1 = __builtin_amdgcn_readlane(xu, fl);
    const int32_t u1 = (int32_t)(quv1 & 0xFFFF), v1 = (int32_t)(quv1 >> 16);
    g.lo2[k] = window_lo2(quv1, radius, rv);
    g.lane[k] = fl; g.n = k + 1;
    g.umin = min(g.umin, u1); g.umax = max(g.umax, u1); g.vmin = min(g.vmin, v1); g.vmax = max(g.vmax, v1);
  }
  return g.n > 0;
}

// What a tile hands to finish_tile: the winner over the walked region of ONE query per lane, joined over the phases
// (join_phases: lanes 0-31 hold query slot 0, lanes 32-63 slot 1), and the lane's queries themselves.
template <int Q> struct TileOut {
  int32_t wp;  // class-relative position of the winner of query slot (lane >> 5), -1: none
  uint4 a0[Q], a1[Q];
  uint32_t uv1[Q];
  int32_t qpos[Q];  // the query's bin-order position
  bool valid[Q];
};

// The end of a tile, shared by every key encoding and by both kinds of pass (one copy of this code per
// kernel: inside the KM-templated tile functions it would be there six times).  Speculative form: the
// winner over the walked region is tested against the query's own window, and the queries that fail are
// searched again in groups (RedoGroup above).  The results go to the table as the reference's findMatch
// returns them: best[query's feature index] = winner's feature index.  (Round 3 also built the tables in
// position space -- entries = bin-order positions, stored at the queries' own positions, whole rows per
// store, the chain followed in position space: branch exp/position-tables.  The table writes fell from
// 14x to 1x their payload, but the chain then needs eleven gathers and a scattered record per circle
// instead of six gathers: 126 vs 65 us, and the step 99.1 k vs 102.0 k pairs/s on the same box.  The
// 4-byte scatter below costs no time; it stays.)
template <int Q, int P, bool SPEC, bool FLOW>
__device__ __forceinline__ void finish_tile(const VhSets &s, const VhMatchArgs &a, int32_t pass, int32_t stream, int32_t qset, int32_t cset,
                                            int32_t c, int32_t pbase, int32_t pcnt, const TileOut<Q> &o,
                                            int32_t *__restrict__ best, int32_t *__restrict__ redo_count) {
  static_assert(Q == 2 && P == 4, "one query per lane: slot lane >> 5, on the first 16-lane row of each half (join_phases)");
  const int32_t lane = threadIdx.x & 63;
  const uint32_t *__restrict__ cuv = s.s_uv + (int64_t)cset * s.cap;
  const uint4 *__restrict__ cdesc = (const uint4 *)(s.s_desc + (int64_t)cset * s.cap * 8);
  const int32_t *__restrict__ cbs = s.bin_start + (int64_t)cset * (s.nbins + 1);
  const int32_t rv = FLOW ? a.radius : a.disp_tol;
  const us2 span2 = window_span2(a.radius, rv);
  const int32_t *__restrict__ cidx = s.s_idx + (int64_t)cset * s.cap;
  const int32_t *__restrict__ qidx = s.s_idx + (int64_t)qset * s.cap;
  int32_t *__restrict__ tbl = best + ((int64_t)stream * 4 + a.pass[pass].slot) * s.cap;
  // After the join every lane holds a winner, so the test, the gathers and the store run ONCE for the tile's 32
  // queries, on 32 lanes (rows 0 and 2), instead of once per slot on the 16 lanes of phase 0.
  const bool hi = lane & 32;
  const bool mine = !(lane & 16) && (hi ? o.valid[1] : o.valid[0]);
  const uint32_t uv1 = hi ? o.uv1[1] : o.uv1[0];
  const int32_t qpos = hi ? o.qpos[1] : o.qpos[0];
  int32_t res = -1;  // no candidate accepted
  bool fail = false;
  if (mine && o.wp >= 0) {
    // (a winner is never one of the copies past the end of a run -- the original has the same SAD at a lower
    //  position -- so its position lies inside the class)
    int32_t wp = o.wp;
    VH_CHECK_RANGE(s, 7, wp, 0, pcnt);
    res = pbase + wp;
    // the winner over the walked region: inside this query's own window?
    if (SPEC) fail = outside_window(ld_off(cuv, (uint32_t)res * 4u), window_lo2(uv1, a.radius, rv), span2);
  }
  if (SPEC) {
    uint64_t todo = __ballot(fail);
    if (todo) {  // wave-uniform
      const int32_t nfail = (int32_t)__popcll(todo);
      VH_STAT(FLOW ? 7 : 10, nfail);
      if (lane == 0) atomicAdd(redo_count, nfail);
      RedoGroup g;
      while (redo_take<Q>(todo, o.a0, o.a1, o.uv1, a.radius, rv, g)) {
        uint64_t kk[VH_REDO_G];
#pragma unroll
        for (int32_t k = 0; k < VH_REDO_G; k++) kk[k] = ~0ull;
        if (FLOW) {
          // the union of the group's own bin ranges
          const VhBins b = bins_of_interest(s, VhWindow{g.umin - a.radius, g.umax + a.radius, g.vmin - rv, g.vmax + rv});
          walk_region<false, true>(s, cbs, cuv, cdesc, c, b.ub0, b.ub1, b.vb0, b.vb1, 0, 0, 0, 0,
            [&](int32_t, int32_t, int32_t, int32_t, int32_t pl, uint32_t gu, const uint4 &g0, const uint4 &g1) {
#pragma unroll
              for (int32_t k = 0; k < VH_REDO_G; k++)
                if (k < g.n) kk[k] = min(kk[k], tested_key_uniform_query(g.qd[k], g.lo2[k], span2, gu, g0, g1, (uint32_t)(pl - pbase)));
            });
        } else {
          // the union of the group's own rows [v - tol, v + tol]
          const int32_t *__restrict__ crs = s.row_start + (int64_t)cset * (4 * s.H + 1);
          const int32_t *__restrict__ cpos = s.r_pos + (int64_t)cset * s.cap;
          const int32_t x0 = ld_uniform_i32(crs + c * s.H + max(g.vmin - rv, 0));
          const int32_t x1 = ld_uniform_i32(crs + c * s.H + min(g.vmax + rv, s.H - 1) + 1);
          for (int32_t x = x0 + lane; x < x1; x += 64) {
            int32_t cp = cpos[x];
            VH_CHECK_RANGE(s, 3, cp, pbase, pbase + pcnt);
            const uint32_t gu = cuv[cp];
            const uint4 g0 = cdesc[2 * (int64_t)cp], g1 = cdesc[2 * (int64_t)cp + 1];
#pragma unroll
            for (int32_t k = 0; k < VH_REDO_G; k++)
              if (k < g.n) kk[k] = min(kk[k], tested_key_uniform_query(g.qd[k], g.lo2[k], span2, gu, g0, g1, (uint32_t)(cp - pbase)));
          }
        }
#pragma unroll
        for (int32_t k = 0; k < VH_REDO_G; k++)
          if (k < g.n) {
            const uint64_t kf = vh_wave_min_u64(kk[k]);
            int32_t wp = (int32_t)(uint32_t)kf;
            if (kf != ~0ull) VH_CHECK_RANGE(s, 7, wp, 0, pcnt);
            if (lane == g.lane[k]) res = kf == ~0ull ? -1 : pbase + wp;
          }
      }
    }
  }
  // min_ind defaults to 0 when no candidate was accepted (matcher.cpp:221)
  if (mine) st_off(tbl, (uint32_t)ld_off(qidx, (uint32_t)qpos * 4u) * 4u, res < 0 ? 0 : ld_off(cidx, (uint32_t)res * 4u));
}

// One tile of the flow search.
//
// A tile is T = 64*Q/P consecutive queries of one class in snake order.  The wave's
// 64 lanes are P *phases* of L = 64/P lanes; lane (phase, l) holds the Q queries
// l, l+L, .. of the tile, so every phase holds the whole tile, and the P phases
// take the candidates j, j+1, .., j+P-1 of the staged chunk in the same step:
// one candidate stream shared by all phases, each candidate evaluated by exactly
// one phase.  Compared with one query per lane and a wave-uniform candidate
// (round 1: T = 64, P = 1, Q = 1):
//  * a 16- or 32-query tile is compact (about one 50x50 bin), so the union of its
//    lanes' windows exceeds each lane's own window by less: fewer evaluated pairs
//    outside the window (tools/tile_model3.py, tools/flow_stats.py);
//  * with Q = 2 every candidate record read from LDS serves two queries per
//    lane.  The record reads (4 LDS cycles per ds_read_b128 and wave, four SIMDs
//    sharing one LDS array) otherwise saturate the LDS beside 8 v_sad_u8 per
//    step: profiles/r02_ubench_valu.txt, last block.
// The minimum over a query's candidates is split over the P phases and joined
// once per tile (join_phases).
//
// SPEC (the default): *speculative* search.  The per-pair accept test of
// matcher.cpp:249 is not applied in the loop at all: every lane takes the minimum
// key over the whole union region the wave walks -- a superset of its own window
// -- which costs 8 v_sad_hi_u8 + 1.25 other VALU instructions per pair instead of
// 8 + 3.5..5.25 (the tests were 29 % of the loop's instructions, more than the
// pairs evaluated outside the window).  At the end each lane tests ONE candidate,
// its winner: if it lies inside the lane's window it is also the minimum over the
// window (keys are unique), i.e. exactly findMatch's result.  Otherwise (some
// out-of-window candidate resembled the query more than every in-window one:
// 0.5 % of the queries on the benchmark frames, ~10 % with two grey levels of
// sensor noise added, where most features have no true partner) the query is
// searched again with the literal test, in groups sharing one walk (finish_tile: RedoGroup / redo_take).
// Results are identical either way; only the time depends on the data.
// !SPEC keeps the tested loop: three accept-test classes per bin as in round 1.
//
// Staged chunk: 64 candidates, lane j loads candidate min(pc+j, p1-1).  Slots
// past the end of the column therefore hold copies of its last candidate; they
// are evaluated like real ones with positions p1, p1+1, ..: same SAD as the
// original at a larger position, so their keys are larger than the original's
// key and never change a minimum.  That lets every range of the chunk be rounded
// outward to whole trips of 2*P candidates without any tail code.
// The part of a flow tile that does not depend on the key encoding: the queries and the region the wave walks.
struct FlowRegion {
  int32_t UB0, UB1, VB0, VB1;                 // bins of interest of the union window
  int32_t ULO_MAX, UHI_MIN, VA0, VA1;         // (tested loop) what lies inside EVERY query's window
};
template <int Q, int P, bool SPEC>
__device__ __forceinline__ FlowRegion flow_queries(const VhSets &s, const VhMatchArgs &a, int32_t rv, int32_t qset, int32_t q0, int32_t q1,
                                                   int32_t c, TileOut<Q> &out) {
  constexpr int L = 64 / P;
  static_assert(L == 8 || L == 16, "every 16-lane row must hold the whole tile (row-wise window reduction)");
  const int32_t l = (threadIdx.x & 63) % L;
  const uint32_t *__restrict__ quv = s.s_uv + (int64_t)qset * s.cap;
  const uint4 *__restrict__ qdesc = (const uint4 *)(s.s_desc + (int64_t)qset * s.cap * 8);
  bool (&valid)[Q] = out.valid;  // the lane's queries live in the tile's result
  uint4 (&a0)[Q] = out.a0, (&a1)[Q] = out.a1;
  uint32_t (&uv1)[Q] = out.uv1;
  int32_t umin = 0x7FFFFFFF, umax = -1, vmin = 0x7FFFFFFF, vmax = -1;
  // [q0, q1) are SNAKE indices; bin_sort resolved them to positions of the query set's bin order once for the set
  // (snake_pos): one gather per query slot.  Without the snake (VH_SNAKE=0) an index is its position.
  int32_t (&qp)[Q] = out.qpos;
  const int32_t *__restrict__ qsnake = s.snake_pos + (int64_t)qset * s.cap;
#pragma unroll
  for (int32_t qi = 0; qi < Q; qi++) {
    const int32_t q = q0 + L * qi + l;
    valid[qi] = q < q1;
    qp[qi] = valid[qi] ? q : q0;
    if (VH_SNAKE) qp[qi] = ld_off(qsnake, (uint32_t)qp[qi] * 4u);
#ifdef VH_CHECK
    {  // the gathered position lies among the positions of the tile's class in the query set's bin order
      const int32_t *qbs = s.bin_start + (int64_t)qset * (s.nbins + 1);
      VH_CHECK_RANGE(s, 14, qp[qi], qbs[c * s.ubn * s.vbn], qbs[(c + 1) * s.ubn * s.vbn]);
    }
#endif
  }
#pragma unroll
  for (int32_t qi = 0; qi < Q; qi++) {
    const int32_t ql = qp[qi];
    uv1[qi] = ld_off(quv, (uint32_t)ql * 4u);
    a0[qi] = ld_off(qdesc, (uint32_t)ql * 32u); a1[qi] = ld_off(qdesc, (uint32_t)ql * 32u + 16u);
    const int32_t u1 = uv1[qi] & 0xFFFF, v1 = uv1[qi] >> 16;
    // (lanes past q1 repeat query q0: it is valid, so the extrema are unchanged)
    umin = min(umin, u1); umax = max(umax, u1); vmin = min(vmin, v1); vmax = max(vmax, v1);
  }
  // every 16-lane row holds all queries of the tile: row-wise extrema are the tile's
  umin = __builtin_amdgcn_readfirstlane(row16_allreduce<false>(umin));
  umax = __builtin_amdgcn_readfirstlane(row16_allreduce<true>(umax));
  vmin = __builtin_amdgcn_readfirstlane(row16_allreduce<false>(vmin));
  vmax = __builtin_amdgcn_readfirstlane(row16_allreduce<true>(vmax));
  // bins of interest of the union window: the bin of a coordinate is monotone, so the union's bins follow from the
  // extreme queries
  const VhBins ub = bins_of_interest(s, VhWindow{umin - a.radius, umax + a.radius, vmin - rv, vmax + rv});
  FlowRegion r;
  r.UB0 = ub.ub0; r.UB1 = ub.ub1; r.VB0 = ub.vb0; r.VB1 = ub.vb1;
  // (tested loop) columns whose pixel range [ub*bs, ub*bs+bs-1] is inside EVERY query's u
  // window, and v-bins [VA0, VA1] whose pixel rows lie inside EVERY query's v window: in
  // an interior column their candidates need no accept test at all
  r.ULO_MAX = umax - a.radius; r.UHI_MIN = umin + a.radius;
  const int32_t VLO_MAX = vmax - rv, VHI_MIN = vmin + rv;
  r.VA0 = SPEC ? 0 : max(r.VB0, (max(VLO_MAX, 0) + s.binsize - 1) / s.binsize);
  r.VA1 = SPEC ? 0 : min(r.VB1, (VHI_MIN + 1) / s.binsize - 1);
  VH_STAT(0, 1); VH_STAT(5, q1 - q0); VH_STAT(6, r.UB1 - r.UB0 + 1);
  return r;
}

template <int Q, int P, int KM, bool SPEC>
__device__ __forceinline__ void flow_tile(const VhSets &s, const VhMatchArgs &a, int32_t rv, int32_t cset, int32_t c, const FlowRegion &r,
                                          int32_t pbase, uint4 *wD, uint32_t *wU, TileOut<Q> &out) {
  constexpr int L = 64 / P;
  constexpr int TRIP = 2 * P;  // candidates per trip: two steps, joined by one v_min3_u32 per query
  constexpr int CH = 64 / TRIP;  // trips of a full chunk
  static_assert(P * (2 * CH - 1) <= 64, "the chunk-local seeds P * k must be inline constants (integers up to 64)");
  const int32_t ph = (threadIdx.x & 63) / L;
  const uint32_t *__restrict__ cuv = s.s_uv + (int64_t)cset * s.cap;
  const uint4 *__restrict__ cdesc = (const uint4 *)(s.s_desc + (int64_t)cset * s.cap * 8);
  const int32_t *__restrict__ cbs = s.bin_start + (int64_t)cset * (s.nbins + 1);
  const uint4 (&a0)[Q] = out.a0, (&a1)[Q] = out.a1;
  typedef typename KeyT<KM>::type key_t;
  const key_t KNONE = (key_t)~(key_t)0;
  key_t best_key[Q];
  int32_t v_lo[Q];
  us2 lo2[Q];
#pragma unroll
  for (int32_t qi = 0; qi < Q; qi++) {
    // search window (matcher.cpp:231-234; stereo: v narrowed to +-disp_tolerance), packed as vh_findmatch.h says
    v_lo[qi] = (int32_t)(out.uv1[qi] >> 16) - rv;
    lo2[qi] = window_lo2(out.uv1[qi], a.radius, rv);
    best_key[qi] = KNONE;
  }
  const us2 span2 = window_span2(a.radius, rv);

  // best = min over candidates of the key (SAD, then bin-order position), the encoding KM of sad_key.
  //
  // Chunk-local keys.  Inside a chunk [pc, pc + 64) the lanes of phase ph see the slots ph + P * k, k = 0 .. 2 * CH - 1.
  // The loop does not build the key of a slot with its class-relative position (pc - pbase) + ph + P * k, which cost a
  // register and an add per step: it builds the LOCAL key SAD << 16 | P * k -- one v_sad_hi_u8 chain seeded with P * k,
  // a compile-time constant of the unrolled trip and at most 60, so an inline operand -- whatever the encoding KM (a SAD
  // is below 2^13, so the local key always fits 32 bits).  The lane keeps the minimum of the local keys over the chunk
  // and turns it into the key of encoding KM ONCE per query and chunk (global_key): SAD field moved to its place, position
  // field P * k + vbase, vbase = (pc - pbase) + ph.  This is still findMatch's first strict minimum:
  //  * global_key of a slot's local key IS the key the loop built for that slot before: same SAD, same position (below
  //    2^16 / 2^19 by key_mode_of, so nothing carries into the SAD field);
  //  * vbase is the same for every slot a lane sees in a chunk and P * k ascends with the position, so global_key is
  //    strictly monotone over them: global_key of the minimum local key is the minimum of those slots' global keys;
  //  * the minimum is associative: the minimum over chunks, phases and lanes of these per-chunk minima is the minimum
  //    over the very set of keys the loop folded one by one before -- bit for bit, copies included.
  // The trailing slots of a short chunk hold copies of the column's last candidate, and a copy in slot j gets the
  // position (pc - pbase) + j, beyond the true one, exactly as before.  Its key never wins: the original sits in slot
  // mcnt - 1 < j with the same SAD; in the same lane that is a smaller P * k, in another phase it is that lane's global
  // key at the true, smaller position, and both reach the same final minimum.
  // A candidate the accept test rejects gets LNONE, an all-ones SAD field over a zero position field: it is above every
  // real local key, and global_key takes it to key_none_floor or above without wrapping, which join_phases reads as
  // "none" like the ~0 the minima start from.
  // TEST: 2 = full (u,v) window test, 1 = v only, 0 = none
  constexpr uint32_t LNONE = 0xFFFF0000u;
  auto make_key = [&](auto test, int32_t qi, uint32_t uv2, const uint4 &b0, const uint4 &b1, uint32_t seed) -> uint32_t {
    constexpr int TEST = decltype(test)::value;
    bool out = false;
    if (TEST == 2) {
      out = outside_window(uv2, lo2[qi], span2);
    } else if (TEST == 1) {
      out = (uint32_t)((int32_t)(uv2 >> 16) - v_lo[qi]) > (uint32_t)(2 * rv);
    }
    const uint32_t key = sad_key<KEY_HI16>(a0[qi], a1[qi], b0, b1, seed);
    return (TEST != 0 && out) ? LNONE : key;
  };
  // the key of encoding KM of a local key `k` of a chunk whose slot 0 this lane sees at class-relative position vbase
  auto global_key = [](uint32_t k, uint32_t vbase) -> key_t {
    if (KM == KEY_HI16) return (key_t)(k + vbase);
    const uint32_t pos = (k & 0xFFFFu) + vbase;
    if (KM == KEY_W19) return (key_t)(((k & 0xFFFF0000u) << 3) | pos);
    return (key_t)(((uint64_t)(k >> 16) << 32) | pos);
  };
  walk_region_lds<!SPEC>(s, cbs, cuv, cdesc, c, r.UB0, r.UB1, r.VB0, r.VB1, r.ULO_MAX, r.UHI_MIN, r.VA0, r.VA1, wD, wU,
    [&](int32_t pc, int32_t p1, int32_t pa0, int32_t pa1, const uint4 *cD, const uint32_t *cU) {
      VH_STAT(1, 1);
      const int32_t mcnt = min(64, p1 - pc);
      const int32_t nt = (mcnt + TRIP - 1) / TRIP;  // 1..CH trips: trailing slots hold copies of the last candidate
      const uint4 *rd = cD + ph;                     // this phase's slot of step 0 (second half: +64)
      const uint32_t *ru = cU + ph;
      uint32_t cm[Q];  // the chunk's minima of the local keys
      // trip t of the chunk: candidates (TRIP * t + ph) and (TRIP * t + P + ph), steps k = 2t and 2t + 1 of this lane.
      // Called with t constant (unrolled), so the slots are immediate offsets of the LDS reads and the seeds P * k are
      // inline constants: no pointer and no seed lives in a register or is advanced inside a chunk.
      auto trip = [&](auto test, int32_t t) __attribute__((always_inline)) {
        VH_STAT(2 + decltype(test)::value, 1);
        const int32_t o = TRIP * t;
        const uint4 dA0 = rd[o], dA1 = rd[o + 64], dB0 = rd[o + P], dB1 = rd[o + 64 + P];
        uint32_t uA = 0, uB = 0;
        if (decltype(test)::value != 0) { uA = ru[o]; uB = ru[o + P]; }
#pragma unroll
        for (int32_t qi = 0; qi < Q; qi++) {
          // (slot o + ph is step k = o / P of this lane: the seed P * k is o)
          const uint32_t kA = make_key(test, qi, uA, dA0, dA1, (uint32_t)o), kB = make_key(test, qi, uB, dB0, dB1, (uint32_t)(o + P));
          cm[qi] = t == 0 ? min(kA, kB) : min(min(kA, kB), cm[qi]);  // (trip 0 runs in every chunk)
        }
      };
      if (SPEC && nt == CH) {
        // full chunk: one straight run of CH trips
#pragma unroll
        for (int32_t t = 0; t < CH; t++) {
          trip(std::integral_constant<int, 0>{}, t);
          // reads are scheduled at most two trips ahead, as in a loop of two trips: further ahead they cost registers
          if (t & 1) __builtin_amdgcn_sched_barrier(0);
        }
      } else if (SPEC || pa0 > pa1) {
        // partial chunk (tested loop: any chunk of a column that is not interior): the same trips, left after nt of them
        constexpr int TEST = SPEC ? 0 : 2;
#pragma unroll
        for (int32_t t = 0; t < CH; t++) {
          if (t >= nt) break;
          trip(std::integral_constant<int, TEST>{}, t);
        }
      } else {
        // interior column.  Trips [0, ta): v test, [ta, tb): no test, [tb, nt): v test -- the
        // untested range shrunk inward to whole trips (testing a candidate that would
        // not need it is always valid)
        const int32_t ta = min((min(max(pa0 - pc, 0), mcnt) + TRIP - 1) / TRIP, nt);
        const int32_t tb = max(min(max(pa1 - pc, 0), mcnt) / TRIP, ta);
#pragma unroll
        for (int32_t t = 0; t < CH; t++) {
          if (t >= nt) break;
          if (t >= ta && t < tb) trip(std::integral_constant<int, 0>{}, t);
          else trip(std::integral_constant<int, 1>{}, t);
        }
      }
      // the chunk's winners as global keys, once per query
      const uint32_t vbase = (uint32_t)(pc - pbase + ph);
#pragma unroll
      for (int32_t qi = 0; qi < Q; qi++) best_key[qi] = min(best_key[qi], global_key(cm[qi], vbase));
    });
  // join the phases: lanes l, l+L, l+2L, .. hold partial minima of the same query
  out.wp = join_phases<Q, P, KM>(best_key);
}

// What surrounds a tile of either kind of pass: the class's span of candidate positions, the key encoding it needs
// (resolved once: tile(key mode constant, pbase, pcnt) is flow_tile or rows_tile, filling `out`), and the end of the tile.
template <bool SPEC, bool FLOW, class Tile>
__device__ __forceinline__ void search_tile(const VhSets &s, const VhMatchArgs &a, int32_t pass, int32_t stream, int32_t qset, int32_t cset,
                                            int32_t c, int32_t *__restrict__ best, int32_t *__restrict__ redo_count,
                                            TileOut<VH_FLOW_Q> &out, Tile tile) {
  // candidates of class c occupy the contiguous positions [pbase, pend) of the bin order
  const int32_t *cbs = s.bin_start + (int64_t)cset * (s.nbins + 1);
  const int32_t pbase = ld_uniform_i32(cbs + c * s.ubn * s.vbn);
  const int32_t pend = ld_uniform_i32(cbs + (c + 1) * s.ubn * s.vbn);
  const int32_t km = key_mode_of(pend - pbase, a.wide_keys);
  if (km == KEY_HI16) tile(std::integral_constant<int, KEY_HI16>{}, pbase, pend - pbase);
  else if (km == KEY_W19) tile(std::integral_constant<int, KEY_W19>{}, pbase, pend - pbase);
  else tile(std::integral_constant<int, KEY_64>{}, pbase, pend - pbase);
  finish_tile<VH_FLOW_Q, VH_FLOW_P, SPEC, FLOW>(s, a, pass, stream, qset, cset, c, pbase, pend - pbase, out, best, redo_count);
}

template <bool SPEC>
__device__ __forceinline__ void flow_pass(const VhSets &s, const VhMatchArgs &a, int32_t pass, int32_t stream, int32_t qset,
                                          int32_t cset, uint4 *wD, uint32_t *wU, int32_t *__restrict__ best, int32_t *__restrict__ redo_count) {
  const int32_t ntile = ld_uniform_i32(s.tile_cnt + qset);
  for (int32_t tile = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); tile < ntile;
       tile += gridDim.x * 4) {
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    const i32x4 t = ld_uniform((const i32x4 *)(s.tiles + (int64_t)qset * s.max_tiles + tile));
    const int32_t q0 = __builtin_amdgcn_readfirstlane(t.x), q1 = __builtin_amdgcn_readfirstlane(t.y);
    const int32_t c = __builtin_amdgcn_readfirstlane(t.z);
    // the queries and the region are loaded once, ahead of the key encoding's three copies of the walk
    TileOut<VH_FLOW_Q> out;
    const int32_t rv = a.pass[pass].flow ? a.radius : a.disp_tol;
    const FlowRegion r = flow_queries<VH_FLOW_Q, VH_FLOW_P, SPEC>(s, a, rv, qset, q0, q1, c, out);
    search_tile<SPEC, true>(s, a, pass, stream, qset, cset, c, best, redo_count, out,
      [&](auto km, int32_t pbase, int32_t) __attribute__((always_inline)) {
        flow_tile<VH_FLOW_Q, VH_FLOW_P, decltype(km)::value, SPEC>(s, a, rv, cset, c, r, pbase, wD, wU, out);
      });
  }
}

// -------------------------------------------------------------- match (stereo)
// The 1-d stereo search (v window of +-match_disp_tolerance, stock libviso2;
// SURVEY App. A.7) accepts only a few dozen candidates per query, all within a
// handful of image rows, so walking whole 50x50 bins would waste >95 % of the
// work.  It runs over the (class, v) ROW index on both sides instead: a tile is
// T = 64*Q/P consecutive row-ordered queries of one class (32 queries span three
// or four image rows), the candidate stream is the single contiguous row range
// [vmin-tol, vmax+tol] of the candidate set, shared by P phases of lanes exactly
// as in the flow search (flow_tile), Q queries per lane.  The search is
// speculative in the same way: no accept test in the loop (the stream holds every
// u of those rows, the window only +-match_radius of them), the winner is tested
// once, and a query whose winner lies outside its window is searched again over
// its group's own rows (finish_tile: RedoGroup / redo_take).  The key carries the
// candidate's BIN-order position (staged next to its descriptor), so the minimum
// is findMatch's first minimum in (u_bin, v_bin, list) order no matter in which
// order the rows are walked.  Round 1 used 64-query tiles with the test in the
// loop: 100 evaluated candidates and 13 instructions per query and candidate
// where ~15 candidates are inside the window; this form evaluates ~70 at 9.4.
template <int Q, int P, int KM, bool SPEC>
__device__ __forceinline__ void rows_tile(const VhSets &s, const VhMatchArgs &a, int32_t pass, int32_t stream, int32_t qset,
                                          int32_t cset, int32_t q0, int32_t q1, int32_t c, int32_t pbase, int32_t pcnt, uint4 *wD,
                                          uint32_t *wU, uint32_t *wV, TileOut<Q> &out) {
  constexpr int L = 64 / P;
  static_assert(L == 8 || L == 16, "every 16-lane row must hold the whole tile");
  constexpr int TRIP = 2 * P;
  const int32_t lane = threadIdx.x & 63, ph = lane / L, l = lane % L;
  const int32_t nrow = 4 * s.H;
  const int32_t *__restrict__ crs = s.row_start + (int64_t)cset * (nrow + 1);
  const int32_t *__restrict__ qpos = s.r_pos + (int64_t)qset * s.cap;
  const uint32_t *__restrict__ quv = s.s_uv + (int64_t)qset * s.cap;
  const uint4 *__restrict__ qdesc = (const uint4 *)(s.s_desc + (int64_t)qset * s.cap * 8);
  const int32_t *__restrict__ cpos = s.r_pos + (int64_t)cset * s.cap;
  const uint32_t *__restrict__ cuv = s.s_uv + (int64_t)cset * s.cap;
  const uint4 *__restrict__ cdesc = (const uint4 *)(s.s_desc + (int64_t)cset * s.cap * 8);

  bool (&valid)[Q] = out.valid;  // the lane's queries live in the tile's result
  uint4 (&a0)[Q] = out.a0, (&a1)[Q] = out.a1;
  uint32_t (&uv1)[Q] = out.uv1;
  int32_t (&qp)[Q] = out.qpos;
  typedef typename KeyT<KM>::type key_t;
  key_t best_key[Q];
  us2 lo2[Q];
  const us2 span2 = window_span2(a.radius, a.disp_tol);
  int32_t vmin = 0x7FFFFFFF, vmax = -1;
#pragma unroll
  for (int32_t qi = 0; qi < Q; qi++) {
    const int32_t q = q0 + L * qi + l;
    valid[qi] = q < q1;
    qp[qi] = ld_off(qpos, (uint32_t)(valid[qi] ? q : q0) * 4u);  // row order holds bin positions; the records are gathered from the bin-ordered arrays
    VH_CHECK_RANGE(s, 1, qp[qi], 0, s.cap);
    uv1[qi] = ld_off(quv, (uint32_t)qp[qi] * 4u);
    a0[qi] = ld_off(qdesc, (uint32_t)qp[qi] * 32u); a1[qi] = ld_off(qdesc, (uint32_t)qp[qi] * 32u + 16u);
    const int32_t v1 = uv1[qi] >> 16;
    lo2[qi] = window_lo2(uv1[qi], a.radius, a.disp_tol);
    best_key[qi] = (key_t)~(key_t)0;
    vmin = min(vmin, v1); vmax = max(vmax, v1);
  }
  vmin = __builtin_amdgcn_readfirstlane(row16_allreduce<false>(vmin));
  vmax = __builtin_amdgcn_readfirstlane(row16_allreduce<true>(vmax));
  VH_STAT(8, 1); VH_STAT(11, q1 - q0);
  const int32_t VLO = max(vmin - a.disp_tol, 0), VHI = min(vmax + a.disp_tol, s.H - 1);
  const int32_t r0 = ld_uniform_i32(crs + c * s.H + VLO);
  const int32_t r1 = ld_uniform_i32(crs + c * s.H + VHI + 1);
  for (int32_t rc = r0; rc < r1; rc += 64) {
    const int32_t mcnt = min(64, r1 - rc);
    // slots past the end repeat the last candidate: same key, harmless.  Every slot of the row index in
    // [row_start[0], row_start[4H]) holds a position of the row's own class (bin_sort writes each exactly once).
    int32_t cp = ld_off(cpos, (uint32_t)min(rc + lane, r1 - 1) * 4u);
    VH_CHECK_RANGE(s, 2, cp, pbase, pbase + pcnt);
    const uint4 g0 = ld_off(cdesc, (uint32_t)cp * 32u), g1 = ld_off(cdesc, (uint32_t)cp * 32u + 16u);
    uint32_t gu = 0;
    if (!SPEC) gu = ld_off(cuv, (uint32_t)cp * 4u);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // previous chunk fully consumed
    wD[lane] = g0; wD[64 + lane] = g1; wU[lane] = (uint32_t)(cp - pbase);
    if (!SPEC) wV[lane] = gu;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // chunk visible to every lane of the wave
    const int32_t jend = (mcnt + TRIP - 1) & ~(TRIP - 1);
    VH_STAT(9, jend / TRIP);
    const uint4 *rd = wD + ph;
    const uint32_t *ru = wU + ph, *rv = wV + ph;
    for (int32_t j = 0; j < jend; j += TRIP) {
      const uint4 dA0 = rd[0], dA1 = rd[64], dB0 = rd[P], dB1 = rd[64 + P];
      const uint32_t sA = ru[0], sB = ru[P];
      uint32_t uA = 0, uB = 0;
      if (!SPEC) { uA = rv[0]; uB = rv[P]; }
#pragma unroll
      for (int32_t qi = 0; qi < Q; qi++) {
        key_t kA = sad_key<KM>(a0[qi], a1[qi], dA0, dA1, sA), kB = sad_key<KM>(a0[qi], a1[qi], dB0, dB1, sB);
        if (!SPEC) {  // the accept test (matcher.cpp:249) per pair
          kA = outside_window(uA, lo2[qi], span2) ? (key_t)~(key_t)0 : kA;
          kB = outside_window(uB, lo2[qi], span2) ? (key_t)~(key_t)0 : kB;
        }
        best_key[qi] = min(min(kA, kB), best_key[qi]);
      }
      rd += TRIP; ru += TRIP; rv += TRIP;
    }
  }
  // join the phases
  out.wp = join_phases<Q, P, KM>(best_key);
}

template <bool SPEC>
__device__ __forceinline__ void rows_pass(const VhSets &s, const VhMatchArgs &a, int32_t pass, int32_t stream, int32_t qset,
                                          int32_t cset, uint4 *wD, uint32_t *wU, uint32_t *wV, int32_t *__restrict__ best, int32_t *__restrict__ redo_count) {
  const int32_t nrow = 4 * s.H;
  const int32_t *__restrict__ qrs = s.row_start + (int64_t)qset * (nrow + 1);
  // tile -> (class, query range): classes are contiguous in row order
  int32_t cls_q0[5];
#pragma unroll
  for (int32_t c = 0; c <= 4; c++) cls_q0[c] = ld_uniform_i32(qrs + c * s.H);
  constexpr int T = VH_TILE_Q;
  for (int32_t tile = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));; tile += gridDim.x * 4) {
    int32_t c = -1, q0 = 0, q1 = 0, t = tile;
#pragma unroll
    for (int32_t k = 0; k < 4; k++) {
      const int32_t nt = (cls_q0[k + 1] - cls_q0[k] + T - 1) / T;
      if (c < 0 && t < nt) { c = k; q0 = cls_q0[k] + T * t; q1 = min(cls_q0[k + 1], q0 + T); }
      if (c < 0) t -= nt;
    }
    if (c < 0) break;  // past the last tile (uniform)
    TileOut<VH_FLOW_Q> out;
    search_tile<SPEC, false>(s, a, pass, stream, qset, cset, c, best, redo_count, out,
      [&](auto km, int32_t pbase, int32_t pcnt) __attribute__((always_inline)) {
        rows_tile<VH_FLOW_Q, VH_FLOW_P, decltype(km)::value, SPEC>(s, a, pass, stream, qset, cset, q0, q1, c, pbase, pcnt, wD, wU, wV, out);
      });
  }
}

// Every pass of a matching method in ONE launch (blockIdx.y = pass): the 1-d stereo
// searches are chains of dependent L2 round trips around very little arithmetic
// (~75 candidates per tile), the 2-d flow searches are bound by VALU issue; as
// separate, serialised kernels the former cost as much time as ~half of the latter
// for 3 % of its instructions.  Mixed on the same CUs the flow waves fill the issue
// slots the stereo waves leave idle.  All passes of a method are independent of each
// other (each is a pure function of its two feature sets).
template <bool SPEC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VH_MATCH_WAVES, 8)))
match_kernel(VhSets s, VhMatchArgs a, int32_t *__restrict__ best, int32_t *__restrict__ redo) {
  __shared__ uint4 sDesc[4 * 256];   // per wave: 2 buffers of 64 staged candidates, first | second descriptor half
  __shared__ uint32_t sAux[4 * 128]; // per wave: 2 x their u | v << 16 (tested flow loop) or key seeds (stereo)
  __shared__ uint32_t sAux2[SPEC ? 1 : 4 * 64];  // per wave: u | v << 16 (tested stereo loop)
  const int32_t pass = blockIdx.y, stream = blockIdx.z;
  if (a.prior && pass == 1) return;  // (searched per driving feature, with its prediction: kernels_prior.hip)
#ifdef VH_EXP_SKIP  // timing-only builds (tools/ab_bench.sh): 1 = no stereo passes, 2 = no flow passes; results are wrong
  if (VH_EXP_SKIP & (a.pass[pass].flow ? 2 : 1)) return;
#endif
  const int32_t qset = vh_row_set(a, stream, a.pass[pass].qset);
  const int32_t cset = vh_row_set(a, stream, a.pass[pass].cset);
  uint4 *wD = sDesc + (threadIdx.x >> 6) * 256;
  uint32_t *wU = sAux + (threadIdx.x >> 6) * 128;
  uint32_t *wV = sAux2 + (SPEC ? 0 : (threadIdx.x >> 6) * 64);
  // queries searched again by this stream's speculative passes: read by the host (with a lag) to
  // choose between the speculative and the tested loops (engine.hip: match policy)
  int32_t *redo_count = redo + stream;
  if (a.pass[pass].flow) flow_pass<SPEC>(s, a, pass, stream, qset, cset, wD, wU, best, redo_count);
  else rows_pass<SPEC>(s, a, pass, stream, qset, cset, wD, wU, wV, best, redo_count);
}

}  // namespace

void vh_launch_match(const VhSets &s, const VhMatchArgs &a, int32_t *best, int32_t *redo, int32_t speculative, int32_t grid_x,
                     int32_t lds_bytes, hipStream_t st) {
  if (!a.npass) return;
  VhMatchArgs m = a;
  static const int wide = [] { const char *e = getenv("VH_FLOW_WIDE_KEYS"); return e ? atoi(e) : 0; }();
  m.wide_keys = wide;
  // Grid and occupancy.  The kernel loops over the tile list, so any grid is correct; what the choice decides is how the
  // searches share the chip with the detection chain of the next frame (round 5, MI355X, KITTI, S = 256, k pairs/s):
  //  * DEFAULT (no hint): one workgroup per 4 tiles of the capacity-sized tile list, width made odd (a multiple of 8 pins
  //    tile k of every row to one XCD: 128 -> 85.2, 129 -> 95.6 in round 2).  At typical densities 3 of 4 of these
  //    workgroups find no tile and leave at once; their churn is what lets the detection chain's workgroups in: 107.1-107.7.
  //  * TIGHT (grid_x = the tiles the sets really hold / 4, from the statistics of an earlier launch) alone is worse: the
  //    searches then hold all 7 wave slots per SIMD for their whole life, finish in 1 685 instead of 2 305 us, and the
  //    detection chain runs on after them on an empty chip: 100.3-100.5.
  //  * TIGHT + lds_bytes = 26 880 (21 of a CU's 128 LDS allocation units of 1 280 bytes: at most SIX search workgroups
  //    per CU, one wave slot per SIMD and 2 units left for everybody else): **110.5-111.8**; 20 units (153 600 in six
  //    workgroups) 104.2-105.2, 22 units (five workgroups) 104.8-105.1 -- the window is one allocation unit wide, because
  //    it is the arithmetic of what fits beside what (detect_nms 14 units, emit_features 21), and it moves with those.
  //    Same rule: 1080p 18.5 -> 19.2, KITTI + noise (tested loops) 73.2 -> 74.9, mono flow 140.7 -> 144.7, S = 32 / 64 /
  //    128 streams 93.0 -> 97.8 / 102.7 -> 104.9 / 105.7 -> 105.8.  4K (detect_nms<3>: 22 units, 69 registers; 79 now) wants FIVE
  //    workgroups instead: 21 / 22 / 23 / 24 / 25 / 26 units = 3.67 / 3.94 / 4.08 / 4.08 / 4.08 / 3.96 against 3.68 -- the
  //    caller picks the units per detector (engine.hip: match_queued).
  // VH_FLOW_WGS / VH_FLOW_LDS_PAD override both (experiments).
  static const int wgs = [] { const char *e = getenv("VH_FLOW_WGS"); return e ? atoi(e) : 0; }();
  static const int pad_env = [] { const char *e = getenv("VH_FLOW_LDS_PAD"); return e ? atoi(e) : -1; }();
  const int32_t gx = wgs > 0 ? wgs : (grid_x > 0 ? (grid_x | 1) : (((s.max_tiles + 3) / 4) | 1));
  dim3 grid(gx, m.npass, a.rows);
  static const size_t static_lds[2] = {
      [] { hipFuncAttributes at{}; return hipFuncGetAttributes(&at, (const void *)match_kernel<false>) == hipSuccess ? at.sharedSizeBytes : (size_t)0; }(),
      [] { hipFuncAttributes at{}; return hipFuncGetAttributes(&at, (const void *)match_kernel<true>) == hipSuccess ? at.sharedSizeBytes : (size_t)0; }()};
  const size_t have = static_lds[speculative ? 1 : 0];
  const int32_t pad = pad_env >= 0 ? pad_env : (wgs > 0 || grid_x <= 0 || lds_bytes <= 0 || have == 0 || (size_t)lds_bytes <= have ? 0 : (int32_t)((size_t)lds_bytes - have));
  if (speculative) hipLaunchKernelGGL(match_kernel<true>, grid, dim3(256), pad, st, s, m, best, redo);
  else hipLaunchKernelGGL(match_kernel<false>, grid, dim3(256), pad, st, s, m, best, redo);
}
