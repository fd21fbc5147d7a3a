#!/usr/bin/env python3
"""What the mono model refit costs: S KITTI-size (1241 x 376) streams resident in HBM, stepped
together and flow-matched; every step estimates the motion with the mono estimator, takes its models
(vh_group_estimate_motion_mono_model), classifies the dense lists under them (vh_group_motion_inliers_mono), then refits
the models on all inliers and classifies again (vh_group_refit_model_mono, reclassify = 1: nothing is uploaded).  Prints one
JSON line per step -- the device time of the mono_refit scope and of the reclassification's scopes, the bytes the refit
reads (32 per inlier record: two 16-byte loads), a device-to-device hipMemcpyAsync of that byte count timed in the same
session as the yardstick, the wall time of the whole call, the inliers before and after, how many lists got a refined
model -- and a summary line with the medians.
  python tools/mono_refit_rate.py [--streams 256] [--steps 8] [--warmup 3] [--iters 200]"""
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
ap.add_argument("--iters", type=int, default=200, help="RANSAC hypotheses of the mono estimator (it only supplies the models)")
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
left = frames[:, 0].contiguous()
torch.cuda.synchronize()

mono = pkg.MonoParams.default(ransac_iters=args.iters, f=721.5, cu=609.6, cv=172.9, height=1.65)
rand8 = np.stack([ob.glibc_rand_after_srand0(8 * mono.ransac_iters).reshape(mono.ransac_iters, 8)] * S)
SCOPES = ("mono_refit", "inlier_flag_mono", "inlier_compact")


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
g.setStream(torch.cuda.current_stream().cuda_stream)
g.profileEnable(True)
rows = []
for t in range(args.warmup + args.steps):
    g.pushBackDevice(left[t % P].data_ptr(), None, isz, dims)
    if t == 0:
        continue
    g.matchFeatures(pkg.METHOD_FLOW)
    _, _, _, models = g.estimateMotionMono(mono, rand8, model=True)
    before = g.motionInliersMono(mono, models, models["valid"].astype(np.int32))
    g.synchronize()
    g.profileReset()
    w0 = time.perf_counter()
    refined, ok, w, after = g.refitModelMono(mono, reclassify=True)
    call_ms = (time.perf_counter() - w0) * 1e3
    if t < args.warmup:
        continue
    k = int(before.sum())
    ms = {name: g.profileRead(name)[0] for name in SCOPES}
    row = {"step": t, "records": int(g.getCounts()[1].sum()), "inliers_before": k, "inliers_after": int(after.sum()),
           "valid": int(models["valid"].sum()), "ok_refit": int(ok.sum()), "ms": {q: round(v, 4) for q, v in ms.items()},
           "bytes_read": 32 * k, "copy_ms": round(copy_ms(max(32 * k, 1)), 4), "call_ms": round(call_ms, 4),
           "w8_over_w7_median": float(np.median(w[ok, 0] / w[ok, 1])) if ok.any() else None}
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731
print(json.dumps({"metric": "mono_refit_device_time", "streams": S, "W": W, "H": H, "steps": len(rows),
                  "inliers_before": med(lambda x: x["inliers_before"]), "inliers_after": med(lambda x: x["inliers_after"]),
                  "mono_refit_ms": med(lambda x: x["ms"]["mono_refit"]), "inlier_flag_mono_ms": med(lambda x: x["ms"]["inlier_flag_mono"]),
                  "inlier_compact_ms": med(lambda x: x["ms"]["inlier_compact"]), "bytes_read": med(lambda x: x["bytes_read"]),
                  "copy_ms": med(lambda x: x["copy_ms"]), "call_ms": med(lambda x: x["call_ms"]), "ok_refit": med(lambda x: x["ok_refit"])}), flush=True)
