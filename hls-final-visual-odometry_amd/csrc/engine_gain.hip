// engine_gain.hip -- the camera gain between the previous and the current left image over the lists of a handle or
// caller-owned lists (kernels_gain.hip): the ring's image planes, the handle entries over the
// inlier positions of the current classification or over the caller's index lists, the stateless entry, and their
// part of the ABI.
#include "engine.h"

namespace vh_engine {

// a sub-batch's full-resolution left images into the planes of the slot being written, on the detect stream
int32_t Group::gain_copy(const VhImages &im) {
  Scope sc(this, "gain_copy", stream);
  uint8_t *dst = gn.d_planes + (int64_t)(vh_set_id(S, im.pair_cur, im.s0, 0) >> 1) * gn.plane;
  vh_launch_gain_copy(im.base[0], im.stride, g.bpl, g.W, g.H, im.S, dst, gn.plane, gn.pitch, stream);
  VH_HIP(hipGetLastError());
  return VH_OK;
}

// idx_offsets null: over the inlier positions of the current classification, which are on the device already; otherwise
// over idx[idx_offsets[s] .. idx_offsets[s + 1]) for list s, positions into the lists the getters return.
int32_t Group::gain_lists(const int32_t *idx, const int32_t *idx_offsets, float *gain, int32_t *num) {
  if (!gain || !num) return VH_ERR_INVALID_ARG;
  const bool by_inliers = !idx_offsets;
  // (a push ends the pair the lists belong to: last_method; stereo lists hold no previous frame)
  if (!gain_on || !allocated || failed || (last_method != VH_METHOD_FLOW && last_method != VH_METHOD_QUAD)) return VH_ERR_STATE;
  if (by_inliers && !inliers_current()) return VH_ERR_STATE;
  int64_t total = 0, kmax = mcap;
  ListSpan sp;
  if (!by_inliers) {
    if (check_offsets(idx_offsets, S, sp)) return VH_ERR_INVALID_ARG;
    kmax = sp.longest; total = sp.total;
    if (total > 0 && !idx) return VH_ERR_INVALID_ARG;
  }
  const int64_t tiles = (kmax + VH_GAIN_TILE - 1) / VH_GAIN_TILE;
  if (!inlier_grid_ok(S, tiles)) return VH_ERR_UNSUPPORTED;
  for (int32_t s = 0; s < S; s++) { gain[s] = 1.0f; num[s] = 0; }
  if (!by_inliers && total == 0) return VH_OK;
  int32_t rc = VH_OK;
  if (!gn.d_gain && (rc = dmalloc(&gn.d_gain, 2 * (size_t)S, false))) return rc;
  if (by_inliers && !gn.d_ratio && (rc = dmalloc(&gn.d_ratio, (size_t)S * mcap, false))) return rc;
  if (!by_inliers && gn.idx_cap < total) {  // idx | ratio | offsets; grows (the work on the old block has completed: every call waits)
    const int64_t want = total + total / 4;
    int32_t *const old = gn.d_idx;
    const size_t old_bytes = gn.idx_bytes;
    if ((rc = dmalloc_carved(static_cast<GainIndexArrays &>(gn), &gn.idx_bytes, true, (size_t)want, (size_t)S))) return rc;
    if (old) { dfree(old); device_bytes -= (int64_t)old_bytes; }
    gn.idx_cap = want;
  }
  hipStream_t ps = post_stream;
  VhGainArgs a{};
  a.lists = VhLists::slots((const vh_p_match *)mt.d_matches, mcap, mt.d_match_count, mcap, S);
  std::vector<int32_t> off;
  if (by_inliers) {
    if (inl.from_host) { a.lists.pm = inl.host.d_pm; a.lists.counts = inl.host.d_cnt; }  // the lists the classification read
    a.idx = inl.d_src; a.idx_stride = mcap; a.idx_counts = inl.d_ninl; a.idx_cap = mcap;
    a.ok = inl.d_ok;
    a.ratio = gn.d_ratio;
  } else {
    bool replaced = false;  // the getters serve a host-side list for some stream: the positions are positions in that list
    if ((rc = stage_host_lists(gn.host, ps, replaced, a.lists.pm, a.lists.counts))) return rc;
    off.resize((size_t)S + 1);
    for (int32_t s = 0; s <= S; s++) off[s] = idx_offsets[s] - idx_offsets[0];
    VH_HIP(hipMemcpyAsync(gn.d_idx, idx + sp.first, sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, ps));
    VH_HIP(hipMemcpyAsync(gn.d_idx_off, off.data(), sizeof(int32_t) * ((size_t)S + 1), hipMemcpyHostToDevice, ps));
    a.idx = gn.d_idx; a.idx_offsets = gn.d_idx_off;
    a.ratio = gn.d_idx_ratio;
  }
  a.tiles_per_list = (int32_t)tiles;
  a.planes_prev = a.planes_cur = gn.d_planes; a.plane = gn.plane; a.pitch = gn.pitch; a.W = dims[0]; a.H = dims[1];
  a.by_set = 1; a.m = role_args();
  a.gain = gn.d_gain; a.num = (int32_t *)(gn.d_gain + S);
  a.check = sets.check;
  // on the post stream, behind the emission of the lists and the classification
  { Scope sc(this, "gain_ratio", ps); vh_launch_gain_ratio(a, ps); }
  { Scope sc(this, "gain_sum", ps); vh_launch_gain_sum(a, ps); }
  VH_HIP(hipGetLastError());
  VH_HIP(hipMemcpyAsync(gain, a.gain, sizeof(float) * (size_t)S, hipMemcpyDeviceToHost, ps));
  VH_HIP(hipMemcpyAsync(num, a.num, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, ps));
  VH_HIP(hipStreamSynchronize(ps));
  return check_violation();
}

}  // namespace vh_engine

using namespace vh_engine;

// The stateless gain: validation, one device block (records | offsets | index entries | their offsets | ratios | gain,
// num | check words | the image planes, repacked to the pitch of a handle's), two launches, one download.
extern "C" int32_t vh_gain(int32_t device, int32_t n_sets, const int32_t *dims, const uint8_t *I_prev, const uint8_t *I_cur, int64_t image_stride,
                              const vh_p_match *pm, const int32_t *offsets, const int32_t *idx, const int32_t *idx_offsets, float *gain,
                              int32_t *num) {
  if (n_sets < 0) return VH_ERR_INVALID_ARG;
  if (n_sets == 0) return VH_OK;
  ListSpan rec, pos;
  // (the first offsets are judged before dims, the order of the others after them: the entry's precedence of refusals)
  if (!gain || !num || image_stride < 0 || check_offsets(offsets, 0, rec) || check_offsets(idx_offsets, 0, pos)) return VH_ERR_INVALID_ARG;
  const int32_t rd = check_dims(dims, true);
  if (rd) return rd;
  if (check_offsets(offsets, n_sets, rec) || check_offsets(idx_offsets, n_sets, pos)) return VH_ERR_INVALID_ARG;
  const int64_t nmax = rec.longest, kmax = pos.longest, total = rec.total, k_end = pos.end, k_total = pos.total;
  if ((total > 0 && !pm) || (k_total > 0 && (!idx || !I_prev || !I_cur))) return VH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < n_sets; s++) { gain[s] = 1.0f; num[s] = 0; }
  if (k_total == 0) return VH_OK;  // nothing to do: nothing is launched
  const int64_t tiles = (kmax + VH_GAIN_TILE - 1) / VH_GAIN_TILE;
  if (nmax > (1 << VH_TRACK_POS_BITS) - 1 || !inlier_grid_ok(n_sets, tiles)) return VH_ERR_UNSUPPORTED;  // (a list longer than any handle holds)
  const int32_t rc = select_device(device);
  if (rc) return rc;
  const size_t lists = (size_t)n_sets;
  const int32_t pitch = round_up(dims[0], 16);
  const size_t plane = (size_t)pitch * dims[1];
  PackedArrays in;
  int32_t *d_idx = nullptr, *d_ioff = nullptr, *d_num = nullptr;
  float *d_ratio = nullptr, *d_gain = nullptr;
  uint32_t *d_check = nullptr;
  uint8_t *d_prev = nullptr, *d_cur = nullptr;
  StagedBlock blk;
  VH_HIP(blk.alloc([&](Carver &c) {
    in.carve(c, rec, lists);
    d_idx = c.ptr<int32_t>((size_t)k_end); d_ioff = c.ptr<int32_t>(lists + 1); d_ratio = c.ptr<float>((size_t)k_end);
    d_gain = c.ptr<float>(lists); d_num = c.ptr<int32_t>(lists); d_check = c.ptr<uint32_t>(64);
    d_prev = c.ptr<uint8_t>(plane * lists); d_cur = c.ptr<uint8_t>(plane * lists);
  }));
  VH_HIP(blk.up_lists(in, pm, offsets, rec, lists));  // (the records only where there are some: pm may be null)
  VH_HIP(blk.up(d_idx + pos.first, idx + pos.first, (size_t)k_total));
  VH_HIP(blk.up(d_ioff, idx_offsets, lists + 1));
  VH_HIP(hipMemset(d_check, 0, 256));
  VH_HIP(hipMemset(d_prev, 0, 2 * up256(plane * lists)));  // (both to the end of the block; the planes' padding columns: read, never summed)
  for (size_t s = 0; s < lists; s++) {
    VH_HIP(hipMemcpy2D(d_prev + s * plane, (size_t)pitch, I_prev + s * (size_t)image_stride, (size_t)dims[2], (size_t)dims[0], (size_t)dims[1], hipMemcpyHostToDevice));
    VH_HIP(hipMemcpy2D(d_cur + s * plane, (size_t)pitch, I_cur + s * (size_t)image_stride, (size_t)dims[2], (size_t)dims[0], (size_t)dims[1], hipMemcpyHostToDevice));
  }
  VhGainArgs a{};
  a.lists = VhLists::packed(in.d_pm, in.d_off, n_sets);
  a.idx = d_idx; a.idx_offsets = d_ioff;
  a.tiles_per_list = (int32_t)tiles;
  a.planes_prev = d_prev; a.planes_cur = d_cur; a.plane = (int64_t)plane; a.pitch = pitch; a.W = dims[0]; a.H = dims[1];
  a.ratio = d_ratio; a.gain = d_gain; a.num = d_num;
  a.check = d_check;
  vh_launch_gain_ratio(a, nullptr);
  vh_launch_gain_sum(a, nullptr);
  VH_HIP(hipGetLastError());
  VH_HIP(hipDeviceSynchronize());
  { const int32_t rv = report_violation(a.check); if (rv) return rv; }
  VH_HIP(blk.down(gain, d_gain, lists));
  VH_HIP(blk.down(num, d_num, lists));
  return VH_OK;
}

extern "C" {

int32_t vh_group_set_gain(vh_group *g, int32_t on) {
  Group *gq = (Group *)g;
  if (!gq) return VH_ERR_INVALID_ARG;
  if (gq->allocated) return VH_ERR_STATE;  // before the first push only: the planes belong to every frame of the ring
  gq->gain_on = on != 0;
  return VH_OK;
}
int32_t vh_set_gain(vh_matcher *m, int32_t on) { return vh_group_set_gain((vh_group *)m, on); }
int32_t vh_group_gain(vh_group *g, float *gain, int32_t *num) {
  Group *gq = (Group *)g; ENTER(gq);
  return gq->gain_lists(nullptr, nullptr, gain, num);
}
int32_t vh_match_gain(vh_matcher *m, float *gain, int32_t *num) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1) return VH_ERR_INVALID_ARG;
  return gq->gain_lists(nullptr, nullptr, gain, num);
}
int32_t vh_group_gain_indices(vh_group *g, const int32_t *idx, const int32_t *idx_offsets, float *gain, int32_t *num) {
  Group *gq = (Group *)g; ENTER(gq);
  if (!idx_offsets) return VH_ERR_INVALID_ARG;
  return gq->gain_lists(idx, idx_offsets, gain, num);
}
int32_t vh_match_gain_indices(vh_matcher *m, const int32_t *idx, int32_t k, float *gain, int32_t *num) {
  Group *gq = (Group *)m; ENTER(gq);
  if (gq->S != 1 || k < 0) return VH_ERR_INVALID_ARG;
  const int32_t off[2] = {0, k};
  return gq->gain_lists(idx, off, gain, num);
}

}  // extern "C"
