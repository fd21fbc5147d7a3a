#!/usr/bin/env python3
"""What the scene points cost: S KITTI-size (1241 x 376) stereo streams resident in HBM, stepped
together and quad-matched.  Every step classifies the dense lists under the estimated motion, refines it and classifies
again, then asks for the points of the inliers in the current frame (vh_group_scene_points_stereo); then the same lists
are classified under the mono model, the mono pose is computed and the points are asked for again
(vh_group_scene_points_mono).  Prints one JSON line per step -- the device time of the "scene_points" scope of each
kind (flag + scan + store), the records read and the points kept per list, and a device-to-device hipMemcpyAsync of the
bytes the stereo pass reads once (48 per record) timed in the same session as the yardstick -- and a summary line with
the medians and the ratio stereo time / copy time.
  python tools/scene_points_rate.py [--streams 256] [--steps 8] [--warmup 3] [--iters 200]"""
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
ap.add_argument("--iters", type=int, default=200, help="RANSAC iterations of the mono estimator")
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
mono = pkg.MonoParams.default(ransac_iters=args.iters, f=721.5, cu=609.6, cv=172.9, height=1.65, motion_threshold=1e300)
rand8 = np.stack([ob.glibc_rand_after_srand0(8 * mono.ransac_iters).reshape(mono.ransac_iters, 8)] * S)


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
    g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
    if t == 0:
        continue
    g.matchFeatures(pkg.METHOD_QUAD)
    tr, ok, _ = g.estimateMotion(e, rand3)
    g.motionInliers(e, tr, ok.astype(np.int32))
    _, _, _, n_in = g.refitMotion(e, reclassify=True)
    g.synchronize()
    g.profileReset()
    w0 = time.perf_counter()
    kept = g.scenePoints(e)
    call_ms = (time.perf_counter() - w0) * 1e3
    stereo_ms = g.profileRead("scene_points")[0]
    _, _, _, models = g.estimateMotionMono(mono, rand8, model=True)
    n_mono = g.motionInliersMono(mono, models, models["valid"].astype(np.int32))
    _, okp, _ = g.poseMono(mono)
    g.synchronize()
    g.profileReset()
    kept_mono = g.scenePoints(mono)
    mono_ms = g.profileRead("scene_points")[0]
    if t < args.warmup:
        continue
    k = int(n_in.sum())
    row = {"step": t, "records_stereo": k, "kept_stereo_per_list": round(float(kept.mean()), 1), "scene_stereo_ms": round(stereo_ms, 4),
           "bytes_read": 48 * k, "copy_ms": round(copy_ms(max(48 * k, 1)), 4), "call_ms": round(call_ms, 4),
           "records_mono": int(n_mono.sum()), "poses_ok": int(okp.sum()), "kept_mono_per_list": round(float(kept_mono.mean()), 1),
           "scene_mono_ms": round(mono_ms, 4)}
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731
out = {"metric": "scene_points_device_time", "streams": S, "W": W, "H": H, "steps": len(rows)}
out.update({k: med(lambda x, k=k: x[k]) for k in rows[0] if k != "step"})
out["stereo_over_copy"] = round(out["scene_stereo_ms"] / out["copy_ms"], 3) if out["copy_ms"] else None
print(json.dumps(out), flush=True)
