#!/usr/bin/env python3
"""What the mono pose refinement on the dense inliers costs: S KITTI-size (1241 x 376) streams
resident in HBM, stepped together and flow-matched; every step estimates the motion with the mono estimator, takes its
models, classifies the dense lists under them, refits the models on all inliers and classifies again, then computes the
refined pose over those inliers (vh_group_pose_mono_refined: nothing is uploaded).  Prints one JSON line per step -- the
device time of mono_pose_refine, of the six pose scopes and of mono_refit, the updates per list (median and maximum over
the lists that converged) and the statuses, the bytes ONE update reads (32 per inlier record: two 16-byte loads of the 48)
with a device-to-device hipMemcpyAsync of that size as the yardstick, the wall time of the call -- and a summary line with
the medians.  Then, in the same session, a second handle on quad lists runs the stereo chain for --motion-steps steps and
reports motion_refit (vh_group_refit_motion) for scale.
  python tools/mono_pose_refine_rate.py [--streams 256] [--steps 6] [--warmup 2] [--iters 200] [--motion-steps 3]"""
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
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=200, help="RANSAC hypotheses of the mono estimator (it only supplies the models)")
ap.add_argument("--motion-steps", type=int, default=3, help="steps of the stereo chain for motion_refit (0: leave it out)")
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


med = lambda rows, f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731

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
    g.motionInliersMono(mono, models, models["valid"].astype(np.int32))
    g.refitModelMono(mono, reclassify=True)
    g.synchronize()
    g.profileReset()
    g.refitModelMono(mono)                                    # (mono_refit of the same lists, for scale; the classification is untouched)
    w0 = time.perf_counter()
    tr, okp, counts, pose, rec = g.poseMono(mono, pose=True, refine=True)
    call_ms = (time.perf_counter() - w0) * 1e3
    if t < args.warmup:
        continue
    k = int(counts.sum())
    ms = {name: g.profileRead(name)[0] for name in POSE + ("mono_pose_refine", "mono_refit")}
    conv = rec["n_updates"][rec["status"] == 0]
    passes = int(rec["n_updates"].max()) + 1                  # the launch lasts as long as its slowest list: its updates and the covariance pass
    row = {"step": t, "inliers": k, "inliers_per_list": round(k / S, 1), "ok": int(okp.sum()),
           "status": {str(v): int((rec["status"] == v).sum()) for v in np.unique(rec["status"])},
           "updates_median": float(np.median(conv)) if len(conv) else None, "updates_max": int(conv.max()) if len(conv) else None,
           "updates_max_any": int(rec["n_updates"].max()), "passes_of_the_slowest_list": passes,
           "ms": {q: round(v, 4) for q, v in ms.items()}, "tail_ms": round(sum(ms[q] for q in POSE), 4),
           "ms_per_pass_of_the_slowest": round(ms["mono_pose_refine"] / passes, 5),
           "bytes_per_update": 32 * k, "copy_ms": round(copy_ms(max(32 * k, 1)), 4), "call_ms": round(call_ms, 4),
           "ssr_ratio_median": float(np.median(rec["ssr"][rec["status"] == 0] / rec["ssr_start"][rec["status"] == 0])) if len(conv) else None,
           "moved_R_median": float(np.median(rec["moved_R"][rec["status"] == 0])) if len(conv) else None}
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
out = {"metric": "mono_pose_refine_device_time", "streams": S, "W": W, "H": H, "steps": len(rows),
       "inliers": med(rows, lambda x: x["inliers"]), "inliers_per_list": med(rows, lambda x: x["inliers_per_list"]),
       "converged_lists": med(rows, lambda x: x["status"].get("0", 0)),
       "updates_median": med(rows, lambda x: x["updates_median"] or 0), "updates_max": int(max(x["updates_max_any"] for x in rows)),
       "mono_pose_refine_ms": med(rows, lambda x: x["ms"]["mono_pose_refine"]), "ms_per_pass_of_the_slowest": med(rows, lambda x: x["ms_per_pass_of_the_slowest"]),
       "tail_ms": med(rows, lambda x: x["tail_ms"]), "mono_refit_ms": med(rows, lambda x: x["ms"]["mono_refit"]),
       "bytes_per_update": med(rows, lambda x: x["bytes_per_update"]), "copy_ms": med(rows, lambda x: x["copy_ms"]), "call_ms": med(rows, lambda x: x["call_ms"])}
for q in POSE:
    out[q + "_ms"] = med(rows, lambda x, q=q: x["ms"][q])

if args.motion_steps > 0:   # the stereo refit of the same session, on quad lists
    e = pkg.EgoParams.default(f=721.5, cu=609.6, cv=172.9, base=0.54)
    r3 = ob.glibc_rand_after_srand0(3 * e.ransac_iters).reshape(e.ransac_iters, 3)
    rand3 = np.stack([r3] * S)
    g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
    g.setStream(torch.cuda.current_stream().cuda_stream)
    g.profileEnable(True)
    mrows = []
    for t in range(1 + args.motion_steps + 1):
        g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
        if t == 0:
            continue
        g.matchFeatures(pkg.METHOD_QUAD)
        tr, ok, _ = g.estimateMotion(e, rand3)
        g.motionInliers(e, tr, ok.astype(np.int32))
        g.synchronize()
        g.profileReset()
        tr2, ok2, nupd, n = g.refitMotion(e)
        if t == 1:
            continue                                          # (warm-up)
        mrows.append({"motion_refit_ms": g.profileRead("motion_refit")[0], "inliers": int(n.sum()), "updates_max": int(nupd.max())})
    g.close()
    out.update(motion_refit_ms=med(mrows, lambda x: x["motion_refit_ms"]), motion_refit_inliers=med(mrows, lambda x: x["inliers"]),
               motion_refit_updates_max=int(max(x["updates_max"] for x in mrows)))
print(json.dumps(out), flush=True)
