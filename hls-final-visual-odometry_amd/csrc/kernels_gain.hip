// kernels_gain.hip -- the camera gain between the previous and the current left image over index lists into match
// lists, on gfx950.
//
// Replaces, for every list of a call in one launch sequence:
//   Matcher::getGain                                  (reference src/matcher.h:145-148, src/viso.h:104; the body is
//                                                      commented out there -- stock libviso2's loop)
//   Matcher::mean                                     (reference src/matcher.cpp:347-354)
// Single precision, built with -ffp-contract=off; both divisions are plain `/` (correctly rounded).
//
//   gain_copy    a push's full-resolution left images into the handle's planes (pitch: W rounded up to 16).
//   gain_ratio   8 lanes per index entry: lane j < 7 sums row j of the previous and of the current window (three aligned
//                dwords per image, shifted by v_alignbyte, masked to the window's columns, v_sad_u8 against 0); the
//                lanes' integers are joined by shuffles; one float per entry: mean_curr / mean_prev, or GAIN_SKIP
//                (-0.0f) where the entry does not count.  No counted ratio is -0.0f (both means are >= +0), and
//                x + -0.0f == x for every x: the marker is the additive identity of gain_sum's chain.
//   gain_sum     one wave per list: 64 ratios per trip by one coalesced load, added lane after lane (v_readlane) in
//                ascending entry order -- the order of the index list is part of the result; the count by ballot.
// Plain vector stores only, no atomics, nothing waits for another workgroup.
#include "vh_dev.h"
#include "vh_wave.h"

namespace {

#define GAIN_T 256
#define GAIN_LANES 8                        // lanes per index entry
#define GAIN_TRIPS (VH_GAIN_TILE / (GAIN_T / GAIN_LANES))
#define GAIN_SKIP 0x80000000u               // -0.0f
static_assert(VH_GAIN_TILE % (GAIN_T / GAIN_LANES) == 0, "tile");

struct GainList {
  const vh_p_match *pm;
  int32_t n;            // records of the list
  const int32_t *idx;
  int32_t k;            // index entries
  float *ratio;
  const uint8_t *Ip, *Ic;
};
__device__ __forceinline__ GainList gain_list(const VhGainArgs &a, int32_t l) {
  const VhList L = vh_list(a.lists, l);
  GainList r;
  r.pm = L.pm; r.n = L.n;
  const int64_t i0 = a.idx_offsets ? (int64_t)a.idx_offsets[l] : (int64_t)l * a.idx_stride;
  r.idx = a.idx + i0; r.ratio = a.ratio + i0;
  r.k = a.idx_offsets ? a.idx_offsets[l + 1] - a.idx_offsets[l] : min(a.idx_counts[l], a.idx_cap);
  if (a.ok && !a.ok[l]) r.k = 0;
  if (a.by_set) {  // a handle: the planes of the list's previous and current left set (vh_row_set); two sets share a plane index
    if (a.m.seq_prev_last >= 0 && (l < a.m.seq_lo || l >= a.m.rows)) r.k = 0;  // (a sequence row without a pair: its sets are the empty ones)
    r.Ip = a.planes_prev + (int64_t)(vh_row_set(a.m, l, 0) >> 1) * a.plane;
    r.Ic = a.planes_cur + (int64_t)(vh_row_set(a.m, l, 2) >> 1) * a.plane;
  } else {
    r.Ip = a.planes_prev + (int64_t)l * a.plane;
    r.Ic = a.planes_cur + (int64_t)l * a.plane;
  }
  return r;
}

// This lane's row (sub) of the 7 x 7 window around (up, vp), clamped into the image: the sum of its bytes; *pixels: the
// pixel count of the whole window.  A clamped window has fewer rows (the lanes past the last one add 0) or fewer columns
// (a shorter mask): the same instructions either way.  Every dword read lies inside the row [0, pitch) of a row < H.
__device__ __forceinline__ uint32_t gain_row_sum(const VhGainArgs &a, const uint8_t *I, int32_t up, int32_t vp, int32_t sub, int32_t *pixels) {
  const int32_t u_min = min(max(up - 3, 0), a.W - 1), u_max = min(max(up + 3, 0), a.W - 1);
  const int32_t v_min = min(max(vp - 3, 0), a.H - 1), v_max = min(max(vp + 3, 0), a.H - 1);
  const int32_t len = u_max - u_min + 1;
  *pixels = len * (v_max - v_min + 1);
  const bool row_live = v_min + sub <= v_max;
  const int32_t v = min(v_min + sub, v_max);
  // the aligned dwords that hold columns u_min .. u_max: at most three; one past the last is read again as the last
  const int32_t c0 = u_min & ~3, c_last = u_max & ~3;
  const int32_t c1 = min(c0 + 4, c_last), c2 = min(c0 + 8, c_last);
  int64_t o0 = (int64_t)v * a.pitch + c0, o1 = (int64_t)v * a.pitch + c1, o2 = (int64_t)v * a.pitch + c2;
  VH_CHECK_RANGE(a, 12, o0, (int64_t)0, a.plane - 3);
  VH_CHECK_RANGE(a, 12, o1, (int64_t)0, a.plane - 3);
  VH_CHECK_RANGE(a, 12, o2, (int64_t)0, a.plane - 3);
  const uint32_t d0 = *(const uint32_t *)(I + o0), d1 = *(const uint32_t *)(I + o1), d2 = *(const uint32_t *)(I + o2);
  const uint32_t sh = (uint32_t)(u_min & 3);
  const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, sh), w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);  // columns u_min .. u_min + 7
  const uint64_t mask = (1ull << (8 * len)) - 1ull;  // len <= 7
  uint32_t s = __builtin_amdgcn_sad_u8(w0 & (uint32_t)mask, 0u, 0u);
  s = __builtin_amdgcn_sad_u8(w1 & (uint32_t)(mask >> 32), 0u, s);
  return row_live ? s : 0u;
}

__global__ __launch_bounds__(GAIN_T) void gain_ratio_kernel(const VhGainArgs a) {
  const int32_t l = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x, sub = tid & (GAIN_LANES - 1);
  const GainList L = gain_list(a, l);
  const int32_t e0 = tile * VH_GAIN_TILE + (tid >> 3);
  for (int32_t t = 0; t < GAIN_TRIPS; t++) {
    const int32_t e = e0 + t * (GAIN_T / GAIN_LANES);
    if (e >= L.k) break;  // (the 8 lanes of an entry leave together)
    int32_t i = L.idx[e];
    bool use = i >= 0 && i < L.n;
    float4 q0 = make_float4(0, 0, 0, 0), q1 = q0;
    if (use) {
      VH_CHECK_RANGE(a, 13, i, 0, L.n);
      const float4 *p = (const float4 *)(L.pm + i);  // {u1p, v1p, i1p, u2p} {v2p, i2p, u1c, v1c}
      q0 = p[0]; q1 = p[1];
    }
    // (a NaN or an infinity compares false)
    use = use && fabsf(q0.x) < 16777216.0f && fabsf(q0.y) < 16777216.0f && fabsf(q1.z) < 16777216.0f && fabsf(q1.w) < 16777216.0f;
    const int32_t up = use ? (int32_t)q0.x : 0, vp = use ? (int32_t)q0.y : 0;
    const int32_t uc = use ? (int32_t)q1.z : 0, vc = use ? (int32_t)q1.w : 0;
    int32_t np, nc;
    const uint32_t sp = gain_row_sum(a, L.Ip, up, vp, sub, &np), sc = gain_row_sum(a, L.Ic, uc, vc, sub, &nc);
    uint32_t both = sp | (sc << 16);  // a window's sum is at most 49 * 255 < 2^16: one reduction for both
#pragma unroll
    for (int32_t d = 1; d < GAIN_LANES; d <<= 1) both += (uint32_t)__shfl_xor((int32_t)both, d, GAIN_LANES);
    const float mean_prev = (float)(both & 0xFFFFu) / (float)np, mean_curr = (float)(both >> 16) / (float)nc;
    uint32_t r = GAIN_SKIP;
    if (use && mean_prev > 10.0f) r = __float_as_uint(mean_curr / mean_prev);
    if (sub == 0) L.ratio[e] = __uint_as_float(r);
  }
}

__global__ __launch_bounds__(64) void gain_sum_kernel(const VhGainArgs a) {
  const int32_t l = blockIdx.x, lane = threadIdx.x;
  const GainList L = gain_list(a, l);
  float gain = 0.0f;
  int32_t num = 0;
  uint32_t next = lane < L.k ? __float_as_uint(L.ratio[lane]) : GAIN_SKIP;
  for (int32_t c = 0; c < L.k; c += 64) {
    const uint32_t cur = next;
    const int32_t e = c + 64 + lane;
    next = e < L.k ? __float_as_uint(L.ratio[e]) : GAIN_SKIP;  // (in flight while the chain below runs)
    num += __popcll(__ballot(cur != GAIN_SKIP));
#pragma unroll
    for (int32_t j = 0; j < 64; j++) gain += __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int32_t)cur, j));  // + -0.0f: unchanged
  }
  if (lane == 0) {
    a.gain[l] = num > 0 ? gain / (float)num : 1.0f;
    a.num[l] = num;
  }
}

// 16 bytes of a plane per thread.  vec: every source row begins on a 16-byte boundary.
__global__ __launch_bounds__(256) void gain_copy_kernel(const uint8_t *src, int64_t stride, int32_t bpl, int32_t W, int32_t H, int32_t vec,
                                                        uint8_t *dst, int64_t plane, int32_t pitch) {
  const int32_t per_row = pitch >> 4;
  const int32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= per_row * H) return;
  const int32_t v = t / per_row, x = (t - v * per_row) << 4;
  const uint8_t *s = src + (int64_t)blockIdx.y * stride + (int64_t)v * bpl + x;
  uint4 q = make_uint4(0, 0, 0, 0);
  if (vec && x + 16 <= bpl) q = *(const uint4 *)s;  // (columns W .. bpl of the row: never summed)
  else {
    uint32_t w[4] = {0, 0, 0, 0};
    const int32_t nb = min(16, W - x);
#pragma unroll
    for (int32_t b = 0; b < 16; b++) if (b < nb) w[b >> 2] |= (uint32_t)s[b] << (8 * (b & 3));
    q = make_uint4(w[0], w[1], w[2], w[3]);
  }
  *(uint4 *)(dst + (int64_t)blockIdx.y * plane + (int64_t)v * pitch + x) = q;
}

}  // namespace

void vh_launch_gain_copy(const uint8_t *src, int64_t stride, int32_t bpl, int32_t W, int32_t H, int32_t n_images, uint8_t *dst, int64_t plane,
                         int32_t pitch, hipStream_t st) {
  if (n_images <= 0) return;
  const int32_t vec = (((uintptr_t)src | (uint64_t)stride | (uint64_t)bpl) & 15) == 0;
  const dim3 grid(((pitch >> 4) * H + 255) / 256, n_images);
  hipLaunchKernelGGL(gain_copy_kernel, grid, dim3(256), 0, st, src, stride, bpl, W, H, vec, dst, plane, pitch);
}

void vh_launch_gain_ratio(const VhGainArgs &a, hipStream_t st) {
  if (a.lists.n_lists <= 0 || a.tiles_per_list <= 0) return;
  hipLaunchKernelGGL(gain_ratio_kernel, dim3(a.lists.n_lists, a.tiles_per_list), dim3(GAIN_T), 0, st, a);
}

void vh_launch_gain_sum(const VhGainArgs &a, hipStream_t st) {
  if (a.lists.n_lists <= 0) return;
  hipLaunchKernelGGL(gain_sum_kernel, dim3(a.lists.n_lists), dim3(64), 0, st, a);
}
