#!/usr/bin/env python3
"""What the camera gain costs: S KITTI-size (1241 x 376) stereo streams resident in HBM, stepped
together and quad-matched with the image ring on (vh_group_set_gain); every step estimates the motion, classifies the dense
lists under it and takes the gain over the classification's inliers (vh_group_gain).  Prints one JSON line per step -- the
device times of gain_ratio, gain_sum and of the push's gain_copy, the bytes they move -- and a summary line with the medians
and, as the yardstick, a device-to-device hipMemcpyAsync of the same byte count timed in the same session (copy_ms).
  bytes: gain_ratio reads 4 (position) + 32 (the two 16-byte vectors of a record) per entry and 2 x 7 rows of 7 bytes, and
  writes 4; counted here as the bytes it needs, 36 + 98 + 4 -- the 64-byte sectors those rows touch are 14 x 64 = 896 per
  entry, which is what bounds it.  gain_sum reads 4 per entry.  gain_copy reads W x H and writes pitch x H per left image.
  --pairs: pairs/s of push + match with the switch off and on, alternating (the cost of the image copy per push).
  python tools/gain_rate.py [--streams 256] [--steps 8] [--warmup 3] [--pairs 0]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (loads its HIP runtime before the product library, as bench.py does)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--pairs", type=int, default=0, help="alternating rounds of the on / off pairs/s comparison (0: none)")
args = ap.parse_args()
S = args.streams

pkg = entry.load_package()
ob = entry.load_oracle()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
params = pkg.Params.default(**wl["params"])
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)
HIP = C.CDLL("libamdhip64.so")  # the runtime already in the process

P = 20  # stereo_sequence's pan repeats every 20 frames: stream s sees frame (t + s) % P at step t
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)
frames = uniq[torch.arange(S + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()

e = pkg.EgoParams.default(f=721.5, cu=609.6, cv=172.9, base=0.54)
r = ob.glibc_rand_after_srand0(3 * e.ransac_iters).reshape(e.ransac_iters, 3)
rand3 = np.stack([r] * S)


def copy_ms(nbytes, reps=5):
    """A device-to-device copy of nbytes on the current stream: the median of `reps` event-timed copies after one untimed."""
    a = torch.zeros(nbytes, dtype=torch.uint8, device=dev); b = torch.empty_like(a)
    st = torch.cuda.current_stream().cuda_stream

    def copy():
        assert HIP.hipMemcpyAsync(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), C.c_size_t(nbytes), 3, C.c_void_p(st)) == 0
    copy()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); copy(); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms))


g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
g.setGain(True)
g.setStream(torch.cuda.current_stream().cuda_stream)
g.profileEnable(True)
pitch = (W + 15) // 16 * 16
rows = []
for t in range(args.warmup + args.steps):
    g.profileReset()
    g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
    if t == 0:
        continue
    g.matchFeatures(pkg.METHOD_QUAD)
    tr, ok, _ = g.estimateMotion(e, rand3)
    counts = g.motionInliers(e, tr, ok.astype(np.int32))
    gain, num = g.gain()
    if t < args.warmup:
        continue
    k = int(counts.sum())
    ms = {name: g.profileRead(name)[0] for name in ("gain_ratio", "gain_sum", "gain_copy")}
    by = {"gain_ratio": (36 + 98 + 4) * k, "gain_sum": 4 * k, "gain_copy": S * H * (W + pitch)}
    row = {"step": t, "entries": k, "counted": int(num.sum()), "gain_median": round(float(np.median(gain[num > 0])), 4) if (num > 0).any() else None,
           "ms": {q: round(v, 4) for q, v in ms.items()}, "bytes": by,
           "GBps": {q: round(by[q] / (ms[q] * 1e6), 1) if ms[q] > 0 else None for q in ms},
           "sector_GBps_gain_ratio": round((36 + 896 + 4) * k / (ms["gain_ratio"] * 1e6), 1) if ms["gain_ratio"] > 0 else None,
           "copy_ms": {q: round(copy_ms(by[q]), 4) for q in by}}
    row["ratio_to_copy"] = {q: round(ms[q] / row["copy_ms"][q], 2) if row["copy_ms"][q] > 0 else None for q in by}
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 4)  # noqa: E731
print(json.dumps({"metric": "gain_device_time", "streams": S, "W": W, "H": H, "steps": len(rows), "entries_per_step": med(lambda x: x["entries"]),
                  **{q + "_ms": med(lambda x, q=q: x["ms"][q]) for q in ("gain_ratio", "gain_sum", "gain_copy")},
                  **{q + "_copy_ms": med(lambda x, q=q: x["copy_ms"][q]) for q in ("gain_ratio", "gain_sum", "gain_copy")},
                  **{q + "_ratio_to_copy": med(lambda x, q=q: x["ratio_to_copy"][q]) for q in ("gain_ratio", "gain_sum", "gain_copy")},
                  "gain_ratio_sector_GBps": med(lambda x: x["sector_GBps_gain_ratio"])}), flush=True)


def pairs_per_s(on, steps=24, warm=4):
    import time
    h = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
    h.setGain(on)
    h.setStream(torch.cuda.current_stream().cuda_stream)
    for t in range(warm + steps):
        if t == warm:
            h.synchronize(); t0 = time.perf_counter()
        h.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
        if t:
            h.matchFeatures(pkg.METHOD_QUAD)
    h.synchronize()
    dt = time.perf_counter() - t0
    h.close()
    return S * steps / dt


for r in range(args.pairs):
    off, on = pairs_per_s(False), pairs_per_s(True)
    print(json.dumps({"metric": "gain_copy_pairs_per_s", "round": r, "off": round(off, 1), "on": round(on, 1), "on_over_off": round(on / off, 4)}), flush=True)
