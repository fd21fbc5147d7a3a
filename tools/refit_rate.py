#!/usr/bin/env python3
"""What the motion refit costs: S KITTI-size (1241 x 376) stereo streams resident in HBM, stepped
together and quad-matched; every step estimates the motion (vh_group_estimate_motion), classifies the dense lists under
it (vh_group_motion_inliers) and refines the motion on all inliers, classifying again under the result
(vh_group_refit_motion, reclassify = 1).  Prints one JSON line per step -- the device time of the motion_refit scope, the
median and maximum n_updates, the bytes ONE update reads (48 per inlier record: three 16-byte loads), a device-to-device
hipMemcpyAsync of that byte count timed in the same session as the yardstick, the device time of ego_kernel on the same
dense lists (the ego_kernel scope) beside the wall time of the whole estimateMotion call and, since the synthetic
frames pan by a known number of pixels over a plane of known depth, the median |tr - truth| before and after the refit
-- and a summary line with the medians.
  python tools/refit_rate.py [--streams 256] [--steps 8] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


DISP = 12
Zp = e.f * e.base / DISP                      # depth of the plane the frames show
pan = np.array([[(5 * t) % 20, t % 20] for t in range(P)], np.float64)   # synth.stereo_sequence


def truth(t):
    """The motion between the frames the streams saw at steps t - 1 and t: stream s sees frame ((t % P) + s) % P."""
    cur = (np.arange(S) + t % P) % P
    prev = (np.arange(S) + (t - 1) % P) % P
    d = pan[cur] - pan[prev]                  # the crop moves by d: the content by -d pixels
    out = np.zeros((S, 6))
    out[:, 3] = -d[:, 0] * Zp / e.f; out[:, 4] = -d[:, 1] * Zp / e.f
    return out


g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
g.setStream(torch.cuda.current_stream().cuda_stream)
g.profileEnable(True)
rows = []
for t in range(args.warmup + args.steps):
    g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
    if t == 0:
        continue
    g.matchFeatures(pkg.METHOD_QUAD)
    g.synchronize()
    g.profileReset()
    w0 = time.perf_counter()
    tr, ok, _ = g.estimateMotion(e, rand3)
    ego_ms = (time.perf_counter() - w0) * 1e3
    ego_dev_ms = g.profileRead("ego_kernel")[0]
    counts = g.motionInliers(e, tr, ok.astype(np.int32))
    g.profileReset()
    tr2, ok2, nupd, counts2 = g.refitMotion(e, reclassify=True)
    if t < args.warmup:
        continue
    k = int(counts.sum())
    ms = g.profileRead("motion_refit")[0]
    started = nupd[nupd > 0]
    both = ok & ok2
    want = truth(t)
    err = lambda x: float(np.median(np.abs(x[both] - want[both]).max(axis=1))) if both.any() else None  # noqa: E731
    row = {"step": t, "inliers": k, "inliers_after": int(counts2.sum()), "ok_in": int(ok.sum()), "ok_out": int(ok2.sum()),
           "motion_refit_ms": round(ms, 4), "n_updates_median": float(np.median(started)) if len(started) else 0.0,
           "n_updates_max": int(nupd.max()), "bytes_per_update": 48 * k, "copy_ms": round(copy_ms(max(48 * k, 1)), 4),
           "ego_kernel_ms": round(ego_dev_ms, 4), "estimate_motion_call_ms": round(ego_ms, 4), "err_before": err(tr), "err_after": err(tr2)}
    upd = int(nupd.sum()) / max(len(started), 1)
    row["ms_per_update"] = round(ms / max(float(nupd.max()), 1.0), 4)   # the launch lasts as long as its slowest list
    row["mean_updates"] = round(upd, 2)
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731
print(json.dumps({"metric": "motion_refit_device_time", "streams": S, "W": W, "H": H, "steps": len(rows),
                  "inliers_per_step": med(lambda x: x["inliers"]), "motion_refit_ms": med(lambda x: x["motion_refit_ms"]),
                  "n_updates_median": med(lambda x: x["n_updates_median"]), "n_updates_max": int(max(x["n_updates_max"] for x in rows)),
                  "bytes_per_update": med(lambda x: x["bytes_per_update"]), "copy_ms": med(lambda x: x["copy_ms"]),
                  "ms_per_update": med(lambda x: x["ms_per_update"]),
                  "ego_kernel_ms": med(lambda x: x["ego_kernel_ms"]),
                  "estimate_motion_call_ms": med(lambda x: x["estimate_motion_call_ms"]),
                  "err_before": med(lambda x: x["err_before"] or 0.0), "err_after": med(lambda x: x["err_after"] or 0.0)}), flush=True)
