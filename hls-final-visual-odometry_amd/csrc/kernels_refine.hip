// kernels_refine.hip -- Matcher::refinement: pixel (1) and sub-pixel (2) relocation of the match positions.
//
// Stock libviso2 refines in matchFeatures, between matching and removeOutliers (relocateMinimum /
// parabolicFitting) [upstream-recollection, parity unpinned: the reference tree has no refinement function].
// The primitives it rests on are pinned: the full-resolution Sobel planes (filter.cpp), the 16-byte
// small descriptor (computeSmallDescriptor, src/matcher.cpp:516-543) and the Gauss-Jordan solve (Matrix::solve,
// src/matrix.cpp:417-504).  DESIGN.md section 6 (f-3) is the specification this file follows byte for byte.
//
//   refine_planes   du/dv of every pushed image at full resolution, 8 pixels per lane in packed 16-bit arithmetic
//   refine_chain    per closed circle of a match step: the hops anchored at (u1c, v1c); refined coordinates go to a
//                   per-table-buffer array, dropped sub-pixel matches clear their keep flag and leave their chunk count
//   refine_records  the same hops on caller-owned records (vh_refine_matches)
//
// Built with -ffp-contract=off: every double and float rounding step of the sub-pixel fit is part of the result.
#include "vh_findmatch.h"
#include "../../include/viso_hip.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace {

typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ s16x2 as_s16x2(uint32_t x) { return __builtin_bit_cast(s16x2, x); }
__device__ __forceinline__ uint32_t as_u32(s16x2 x) { return __builtin_bit_cast(uint32_t, x); }

// ------------------------------------------------------------------ refine_planes
// du = (1,4,6,4,1)^T x (1,2,0,-2,-1), dv = (1,2,0,-2,-1)^T x (1,4,6,4,1), (sum >> 7) + 128 (filter.cpp:79-171, the
// planes of vh_filters).  A lane computes pixels x0 .. x0+7 of one row y in [2, H-3]: it reads columns
// x0-2 .. x0+9 of rows y-2 .. y+2 as aligned dwords, loading only dwords that hold at least one byte of the row's
// [0, W) (so it never leaves the image), and sums columns and rows on 16-bit pairs.  |sums| <= 12 240 fit in 16 bits
// and (sum >> 7) + 128 lies in [32, 223]: no saturation step.  Pixels with x < 2 or x > W-3 come from bytes that were
// not loaded; nothing reads them (the refinement's bounds keep every descriptor inside [2, W-3] x [2, H-3]).
__global__ void __launch_bounds__(256) refine_planes_kernel(VhImages im, VhRefine rf, int32_t lanes_per_row) {
  const int32_t id = blockIdx.y;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)(rf.H - 4) * lanes_per_row) return;
  const int32_t y = 2 + (int32_t)(t / lanes_per_row), x0 = 8 * (int32_t)(t % lanes_per_row);
  const uint8_t *img = vh_image_ptr(im, id);
  const int32_t set = vh_image_set(im, id);
  s16x2 cs[6], cd[6];
#pragma unroll
  for (int32_t r = 0; r < 5; r++) {
    const uintptr_t row = (uintptr_t)(img + (int64_t)(y - 2 + r) * rf.bpl);
    const uintptr_t first = row + x0 - 2;  // (may lie before the row for x0 = 0: only compared, never dereferenced)
    const uintptr_t a4 = first & ~(uintptr_t)3;
    const uint32_t sh = (uint32_t)(first & 3);
    uint32_t w[4];
#pragma unroll
    for (int32_t k = 0; k < 4; k++) {
      const uintptr_t q = a4 + 4 * k;
      w[k] = (q + 3 >= row && q < row + (uintptr_t)rf.W) ? *(const uint32_t *)q : 0u;
    }
    const uint32_t b[3] = {__builtin_amdgcn_alignbyte(w[1], w[0], sh), __builtin_amdgcn_alignbyte(w[2], w[1], sh),
                           __builtin_amdgcn_alignbyte(w[3], w[2], sh)};
#pragma unroll
    for (int32_t m = 0; m < 6; m++) {
      const s16x2 p = as_s16x2(__builtin_amdgcn_perm(0u, b[m >> 1], (m & 1) ? 0x0c030c02u : 0x0c010c00u));
      const short ks = r == 2 ? 6 : (r == 1 || r == 3 ? 4 : 1);
      const short kd = r == 0 ? 1 : (r == 1 ? 2 : (r == 3 ? -2 : (r == 4 ? -1 : 0)));
      if (r == 0) { cs[m] = p; cd[m] = p; }
      else {
        cs[m] += p * (s16x2)ks;
        if (kd) cd[m] += p * (s16x2)kd;
      }
    }
  }
  // pairs at odd columns: (c[2m+1], c[2m+2])
  s16x2 os[5], od[5];
#pragma unroll
  for (int32_t m = 0; m < 5; m++) {
    os[m] = as_s16x2(__builtin_amdgcn_alignbyte(as_u32(cs[m + 1]), as_u32(cs[m]), 2));
    od[m] = as_s16x2(__builtin_amdgcn_alignbyte(as_u32(cd[m + 1]), as_u32(cd[m]), 2));
  }
  uint32_t pu[4], pv[4];
#pragma unroll
  for (int32_t m = 0; m < 4; m++) {  // output pixels x0+2m, x0+2m+1 (loaded columns 2m+2, 2m+3)
    const s16x2 su = cs[m] + os[m] * (s16x2)2 - os[m + 1] * (s16x2)2 - cs[m + 2];
    const s16x2 sv = cd[m] + od[m] * (s16x2)4 + cd[m + 1] * (s16x2)6 + od[m + 1] * (s16x2)4 + cd[m + 2];
    pu[m] = as_u32((su >> (s16x2)7) + (s16x2)128);
    pv[m] = as_u32((sv >> (s16x2)7) + (s16x2)128);
  }
  const int64_t o = (int64_t)set * rf.plane + (int64_t)y * rf.pitch + x0;
  *(uint2 *)(rf.du + o) = make_uint2(__builtin_amdgcn_perm(pu[1], pu[0], 0x06040200u), __builtin_amdgcn_perm(pu[3], pu[2], 0x06040200u));
  *(uint2 *)(rf.dv + o) = make_uint2(__builtin_amdgcn_perm(pv[1], pv[0], 0x06040200u), __builtin_amdgcn_perm(pv[3], pv[2], 0x06040200u));
}

// ------------------------------------------------------------------ the hops
struct Planes {
  const uint8_t *du, *dv;
};

// computeSmallDescriptor (src/matcher.cpp:516-543) as four little-endian dwords, bytes in the reference's order
__device__ __forceinline__ uint4 small_desc(Planes P, int32_t pitch, int32_t u, int32_t v) {
  const uint8_t *du = P.du + (int64_t)v * pitch + u, *dv = P.dv + (int64_t)v * pitch + u;
  const uint32_t c = du[0];
  const uint32_t d0 = du[-2 * pitch] | (uint32_t)du[-pitch - 2] << 8 | (uint32_t)du[-pitch] << 16 | (uint32_t)du[-pitch + 2] << 24;
  const uint32_t d1 = du[-1] | c << 8 | c << 16 | (uint32_t)du[1] << 24;
  const uint32_t d2 = du[pitch - 2] | (uint32_t)du[pitch] << 8 | (uint32_t)du[pitch + 2] << 16 | (uint32_t)du[2 * pitch] << 24;
  const uint32_t d3 = dv[-pitch] | (uint32_t)dv[-1] << 8 | (uint32_t)dv[1] << 16 | (uint32_t)dv[pitch] << 24;
  return make_uint4(d0, d1, d2, d3);
}

__device__ __forceinline__ uint32_t sad16(uint4 a, uint4 b) {
  uint32_t s = __builtin_amdgcn_sad_u8(a.x, b.x, 0u);
  s = __builtin_amdgcn_sad_u8(a.y, b.y, s);
  s = __builtin_amdgcn_sad_u8(a.z, b.z, s);
  return __builtin_amdgcn_sad_u8(a.w, b.w, s);
}

// b[k] read / written at a launch-uniform index without a dynamically indexed (scratch) array
__device__ __forceinline__ double pick(const double (&b)[6], int32_t k) {
  double r = b[0];
#pragma unroll
  for (int32_t j = 1; j < 6; j++) r = k == j ? b[j] : r;
  return r;
}
__device__ __forceinline__ void put(double (&b)[6], int32_t k, double x) {
#pragma unroll
  for (int32_t j = 0; j < 6; j++) b[j] = k == j ? x : b[j];
}

// One hop anchored at (u1, v1) on image 1c towards (u2, v2) on image T.  Returns false when the match is dropped
// (sub-pixel mode only); pixel mode leaves a hop outside the bounds as it is.
template <int MODE>
__device__ __forceinline__ bool refine_hop(const VhRefine &rf, Planes A, Planes T, float u1, float v1, float &u2, float &v2) {
  constexpr int32_t R = MODE == 2 ? 3 : 2, N = 2 * R + 1;
  const bool inside = u1 >= 4.0f && u1 <= (float)(rf.W - 5) && v1 >= 4.0f && v1 <= (float)(rf.H - 5) &&
                      u2 >= (float)(4 + R) && u2 <= (float)(rf.W - 5 - R) && v2 >= (float)(4 + R) && v2 <= (float)(rf.H - 5 - R);
  if (!inside) return MODE != 2;
  const uint4 a = small_desc(A, rf.pitch, (int32_t)u1, (int32_t)v1);
  const int32_t x0 = (int32_t)u2 - R, y0 = (int32_t)v2 - R;
  // the running argmin only: the first strict minimum in row-major order
  uint32_t best = 0xFFFFFFFFu;
  int32_t m = 0;
  for (int32_t dy = 0; dy < N; dy++)
#pragma unroll
    for (int32_t dx = 0; dx < N; dx++) {
      const uint32_t c = sad16(a, small_desc(T, rf.pitch, x0 + dx, y0 + dy));
      if (c < best) { best = c; m = dy * N + dx; }
    }
  const int32_t du0 = m % N, dv0 = m / N;
  if (MODE != 2) {  // relocateMinimum
    u2 += (float)du0 - 2;
    v2 += (float)dv0 - 2;
    return true;
  }
  // parabolicFitting: a border minimum has no neighbourhood to fit
  if (du0 == 0 || du0 == N - 1 || dv0 == 0 || dv0 == N - 1) return false;
  double c[9];
#pragma unroll
  for (int32_t i = 0; i < 3; i++)
#pragma unroll
    for (int32_t j = 0; j < 3; j++)
      c[i * 3 + j] = i == 1 && j == 1 ? (double)best : (double)sad16(a, small_desc(T, rf.pitch, x0 + du0 + j - 1, y0 + dv0 + i - 1));
  // b = A^T c, rows of A = (x^2, y^2, xy, x, y, 1), y outer, x inner (Matrix::operator*, src/matrix.cpp:263-277)
  double b[6];
#pragma unroll
  for (int32_t k = 0; k < 6; k++) {
    double s = 0;
#pragma unroll
    for (int32_t r = 0; r < 9; r++) {
      const int32_t x = r % 3 - 1, y = r / 3 - 1;
      const int32_t e = k == 0 ? x * x : k == 1 ? y * y : k == 2 ? x * y : k == 3 ? x : k == 4 ? y : 1;
      s += (double)e * c[r];
    }
    b[k] = s;
  }
  // Matrix::solve (src/matrix.cpp:417-504) on the constant A^T A: its pivot order and factors were recorded on the
  // host by the same code (vh_refine_setup); the right-hand side takes the same double operations in the same order
#pragma unroll
  for (int32_t i = 0; i < 6; i++) {
    const int32_t ir = rf.gj_row[i], ic = rf.gj_col[i];
    if (ir != ic) { const double t = pick(b, ir); put(b, ir, pick(b, ic)); put(b, ic, t); }
    const double bc = pick(b, ic) * rf.gj_pivinv[i];
    put(b, ic, bc);
#pragma unroll
    for (int32_t ll = 0; ll < 6; ll++)
      if (ll != ic) b[ll] -= bc * rf.gj_dum[i][ll];
  }
  const float divisor = (float)(b[2] * b[2] - 4.0 * b[0] * b[1]);
  // (the second test is stock libviso2's: it also rejects fits whose cross term is exactly 0)
  if (fabs((double)divisor) < 1e-8 || fabs(b[2]) < 1e-8) return false;
  const float ddu = (float)((2.0 * b[1] * b[3] - b[2] * b[4]) / (double)divisor);
  const float ddv = (float)((2.0 * b[0] * b[4] - b[2] * b[3]) / (double)divisor);
  if (fabsf(ddu) >= 1.0f || fabsf(ddv) >= 1.0f) return false;
  u2 += ((float)du0 - 3) + ddu;
  v2 += ((float)dv0 - 3) + ddv;
  return true;
}

// the hops of one match: q = {u1p, v1p, u2p, v2p, u1c, v1c, u2c, v2c}, P = planes of {1p, 2p, 1c, 2c}
template <int MODE>
__device__ __forceinline__ bool refine_match(const VhRefine &rf, int32_t method, const Planes (&P)[4], float (&q)[8]) {
  const float u1 = q[4], v1 = q[5];
  if (method != 1 && !refine_hop<MODE>(rf, P[2], P[0], u1, v1, q[0], q[1])) return false;  // 1c -> 1p
  if (method == 0) return true;
  if (!refine_hop<MODE>(rf, P[2], P[3], u1, v1, q[6], q[7])) return false;                // 1c -> 2c
  if (method == 1) return true;
  return refine_hop<MODE>(rf, P[2], P[1], u1, v1, q[2], q[3]);                             // 1c -> 2p
}

// ------------------------------------------------------------------ refine_chain
// One lane per driving feature of a row (the chain kernel's layout): kept circles are refined into
// ref[row][i] = {u1p, v1p, u2p, v2p}, {u1c, v1c, u2c, v2c}; a sub-pixel drop clears the keep flag (chain z = -2)
// and takes the entry out of its emission chunk's survivor count, so emit_matches' ordered compaction stays the
// only place that assigns list positions.
template <int MODE>
__global__ void __launch_bounds__(256) refine_chain_kernel(VhSets s, VhMatchArgs a, int32_t method, VhRefine rf,
                                                           int4 *__restrict__ chain, float4 *__restrict__ ref,
                                                           int32_t *__restrict__ mchunk, int32_t nchm) {
  const int32_t row = blockIdx.y;
  int32_t set[4];
  Planes P[4];
#pragma unroll
  for (int32_t r = 0; r < 4; r++) {
    set[r] = vh_row_set(a, row, r);
    P[r] = Planes{rf.du + (int64_t)set[r] * rf.plane, rf.dv + (int64_t)set[r] * rf.plane};
  }
  const int32_t drive = method == 2 ? set[0] : set[2];
  const int32_t n = indexed_count(s, drive);
  int4 *__restrict__ ch = chain + 2 * (int64_t)row * s.cap;
  float4 *__restrict__ out = ref + 2 * (int64_t)row * s.cap;
  // the grid covers whole waves of consecutive features, so the 64 lanes of a wave share one 256-feature chunk
  for (int32_t i0 = blockIdx.x * blockDim.x; i0 < n; i0 += gridDim.x * blockDim.x) {
    const int32_t i = i0 + threadIdx.x;
    bool drop = false;
    if (i < n) {
      const int4 r = ch[2 * (int64_t)i];
      if (r.z >= 0) {
        const int4 c = ch[2 * (int64_t)i + 1];
        float q[8] = {(float)((uint32_t)c.x & 0xFFFFu), (float)((uint32_t)c.x >> 16), (float)((uint32_t)c.y & 0xFFFFu),
                      (float)((uint32_t)c.y >> 16), (float)((uint32_t)c.z & 0xFFFFu), (float)((uint32_t)c.z >> 16),
                      (float)((uint32_t)c.w & 0xFFFFu), (float)((uint32_t)c.w >> 16)};
        if (refine_match<MODE>(rf, method, P, q)) {
          out[2 * (int64_t)i] = make_float4(q[0], q[1], q[2], q[3]);
          out[2 * (int64_t)i + 1] = make_float4(q[4], q[5], q[6], q[7]);
        } else {
          ch[2 * (int64_t)i].z = -2;
          drop = true;
        }
      }
    }
    if (MODE == 2) {
      const uint64_t bal = __ballot(drop);
      if (bal && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(bal))
        atomicSub(mchunk + row * nchm + (i >> 8), (int32_t)__popcll(bal));
    }
  }
}

// ------------------------------------------------------------------ refine_records
template <int MODE>
__global__ void __launch_bounds__(256) refine_records_kernel(VhRefine rf, int32_t method, vh_p_match *__restrict__ pm, int32_t n,
                                                             int32_t *__restrict__ keep) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Planes P[4];
#pragma unroll
  for (int32_t r = 0; r < 4; r++) P[r] = Planes{rf.du + (int64_t)r * rf.plane, rf.dv + (int64_t)r * rf.plane};
  vh_p_match m = pm[i];
  float q[8] = {m.u1p, m.v1p, m.u2p, m.v2p, m.u1c, m.v1c, m.u2c, m.v2c};
  const bool k = refine_match<MODE>(rf, method, P, q);
  m.u1p = q[0]; m.v1p = q[1]; m.u2p = q[2]; m.v2p = q[3]; m.u1c = q[4]; m.v1c = q[5]; m.u2c = q[6]; m.v2c = q[7];
  pm[i] = m;
  keep[i] = k ? 1 : 0;
}

// Matrix::solve (src/matrix.cpp:417-504) on A^T A with a dummy
// right-hand side, recording what the right-hand side's updates need: the pivot (row, column) of each step, pivinv
// and the factor dum of every eliminated row.
void record_solve(VhRefine &rf) {
  double A[9][6], M[6][6];
  for (int32_t r = 0; r < 9; r++) {
    const double x = r % 3 - 1, y = r / 3 - 1;
    const double row[6] = {x * x, y * y, x * y, x, y, 1};
    for (int32_t k = 0; k < 6; k++) A[r][k] = row[k];
  }
  for (int32_t i = 0; i < 6; i++)  // Matrix::operator* (src/matrix.cpp:263-277): C = 0, C[i][j] += A^T[i][k] * A[k][j]
    for (int32_t j = 0; j < 6; j++) {
      M[i][j] = 0;
      for (int32_t k = 0; k < 9; k++) M[i][j] += A[k][i] * A[k][j];
    }
  int32_t ipiv[6] = {0, 0, 0, 0, 0, 0};
  for (int32_t i = 0; i < 6; i++) {
    double big = 0.0;
    int32_t irow = 0, icol = 0;
    for (int32_t j = 0; j < 6; j++)
      if (ipiv[j] != 1)
        for (int32_t k = 0; k < 6; k++)
          if (ipiv[k] == 0 && fabs(M[j][k]) >= big) { big = fabs(M[j][k]); irow = j; icol = k; }
    ++ipiv[icol];
    if (irow != icol)
      for (int32_t l = 0; l < 6; l++) std::swap(M[irow][l], M[icol][l]);
    rf.gj_row[i] = irow; rf.gj_col[i] = icol;
    const double pivinv = 1.0 / M[icol][icol];  // (A^T A is regular: the singular branch cannot be taken)
    rf.gj_pivinv[i] = pivinv;
    M[icol][icol] = 1.0;
    for (int32_t l = 0; l < 6; l++) M[icol][l] *= pivinv;
    for (int32_t ll = 0; ll < 6; ll++) {
      rf.gj_dum[i][ll] = 0.0;
      if (ll != icol) {
        const double dum = M[ll][icol];
        rf.gj_dum[i][ll] = dum;
        M[ll][icol] = 0.0;
        for (int32_t l = 0; l < 6; l++) M[ll][l] -= M[icol][l] * dum;
      }
    }
  }
}

}  // namespace

void vh_refine_setup(VhRefine &rf) { record_solve(rf); }

void vh_launch_refine_planes(const VhImages &im, const VhRefine &rf, hipStream_t st) {
  if (rf.W < 5 || rf.H < 5) return;
  const int32_t lanes = (rf.W + 7) / 8;
  const int64_t n = (int64_t)(rf.H - 4) * lanes;
  hipLaunchKernelGGL(refine_planes_kernel, dim3((uint32_t)((n + 255) / 256), im.S * im.ncam), dim3(256), 0, st, im, rf, lanes);
}

void vh_launch_refine(const VhSets &s, const VhMatchArgs &a, int32_t method, const VhRefine &rf, int4 *chain, float4 *ref,
                      int32_t *mchunk, hipStream_t st) {
  const int32_t nchm = (s.cap + 255) / 256;
  dim3 grid(std::min(std::max(s.cap / 1024, 8), 256), a.rows);
  if (rf.mode == 2)
    hipLaunchKernelGGL(refine_chain_kernel<2>, grid, dim3(256), 0, st, s, a, method, rf, chain, ref, mchunk, nchm);
  else
    hipLaunchKernelGGL(refine_chain_kernel<1>, grid, dim3(256), 0, st, s, a, method, rf, chain, ref, mchunk, nchm);
}

void vh_launch_refine_records(const VhRefine &rf, int32_t method, vh_p_match *pm, int32_t n, int32_t *keep, hipStream_t st) {
  if (n <= 0) return;
  const dim3 grid((n + 255) / 256);
  if (rf.mode == 2) hipLaunchKernelGGL(refine_records_kernel<2>, grid, dim3(256), 0, st, rf, method, pm, n, keep);
  else hipLaunchKernelGGL(refine_records_kernel<1>, grid, dim3(256), 0, st, rf, method, pm, n, keep);
}
