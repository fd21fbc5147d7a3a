#!/usr/bin/env python3
"""What the mono pose on the dense inliers costs: S KITTI-size (1241 x 376) streams resident in
HBM, stepped together and flow-matched; every step estimates the motion with the mono estimator, takes its models,
classifies the dense lists under them, refits the models on all inliers and classifies again, then computes the pose over
those inliers (vh_group_pose_mono: nothing is uploaded).  Prints one JSON line per step -- the device time of each of the
pose's six scopes, of mono_refit and the wall time of the bucketed estimator's call in the same session for scale,
the bytes the pass reads (48 per inlier record and candidate pass: tri and front each read the records once; 16 per point
in front and workgroup of rank / vote), a device-to-device hipMemcpyAsync of the records' byte count as the yardstick, the
wall time of the call, the inliers, the refusal reasons -- and a summary line with the medians.
  python tools/mono_pose_rate.py [--streams 256] [--steps 8] [--warmup 3] [--iters 200]"""
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

# (a pan has no depth: motion_threshold is raised so that the lists reach the median's test and run the vote)
mono = pkg.MonoParams.default(ransac_iters=args.iters, f=721.5, cu=609.6, cv=172.9, height=1.65, motion_threshold=1e300)
rand8 = np.stack([ob.glibc_rand_after_srand0(8 * mono.ransac_iters).reshape(mono.ransac_iters, 8)] * S)
POSE = ("mono_pose_head", "mono_pose_tri", "mono_pose_front", "mono_pose_rank", "mono_pose_vote", "mono_pose_finish")


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
    g.synchronize()
    g.profileReset()
    w0 = time.perf_counter()
    _, _, _, models = g.estimateMotionMono(mono, rand8, model=True)   # (synchronous and without a scope of its own: wall time)
    est_ms = (time.perf_counter() - w0) * 1e3
    g.motionInliersMono(mono, models, models["valid"].astype(np.int32))
    refined, ok, w, after = g.refitModelMono(mono, reclassify=True)
    g.synchronize()
    w0 = time.perf_counter()
    tr, okp, counts, pose = g.poseMono(mono, pose=True)
    call_ms = (time.perf_counter() - w0) * 1e3
    if t < args.warmup:
        continue
    k = int(counts.sum())
    names = POSE + ("mono_refit",)
    ms = {name: g.profileRead(name)[0] for name in names}
    nf = pose["n_front"].astype(np.int64)
    row = {"step": t, "inliers": k, "inliers_per_list": round(k / S, 1), "n_front": int(nf.sum()), "ok": int(okp.sum()),
           "reasons": {str(r): int((pose["reason"] == r).sum()) for r in np.unique(pose["reason"])},
           "ms": {q: round(v, 4) for q, v in ms.items()}, "pose_ms": round(sum(ms[q] for q in POSE), 4),
           "record_bytes": 48 * k, "copy_ms": round(copy_ms(max(48 * k, 1)), 4), "call_ms": round(call_ms, 4), "estimator_call_ms": round(est_ms, 4),
           "vote_exp": int((nf * nf).sum())}
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731
out = {"metric": "mono_pose_device_time", "streams": S, "W": W, "H": H, "steps": len(rows), "inliers": med(lambda x: x["inliers"]),
       "inliers_per_list": med(lambda x: x["inliers_per_list"]), "n_front": med(lambda x: x["n_front"]), "ok": med(lambda x: x["ok"]),
       "pose_ms": med(lambda x: x["pose_ms"]), "record_bytes": med(lambda x: x["record_bytes"]), "copy_ms": med(lambda x: x["copy_ms"]),
       "call_ms": med(lambda x: x["call_ms"]), "estimator_call_ms": med(lambda x: x["estimator_call_ms"]), "vote_exp": med(lambda x: x["vote_exp"])}
for q in POSE + ("mono_refit",):
    out[q + "_ms"] = med(lambda x, q=q: x["ms"][q])
print(json.dumps(out), flush=True)
