"""Device time of the "trajectory" scope beside what it replaces, on small synthetic frames (the
kernel's time depends on the number of chains and rows, not on the images):
  (a) a plain group of S = 256 streams: 256 chains of one row;
  (b) a sequence handle with chunks of 256 frames: one chain of 256 rows.
Beside each: the call's wall time, the numpy chain pose @ inv(T) over the same rows on the host, and scenePoints with an
uploaded Tw against scenePointsWorld (wall time and the "scene_points" scope).  The step is idempotent for a pushed pair,
so the call is repeated REPS times per pair.  Prints one JSON line.

    python tools/trajectory_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

W, H, S = 320, 160, 256
QUAD = 2


def transform(tr):
    rx, ry, rz, tx, ty, tz = tr
    sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    return np.array([[+cy * cz, -cy * sz, +sy, tx],
                     [+sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy, ty],
                     [-cx * sy * cz + sx * sz, +cx * sy * sz + sx * cz, +cx * cy, tz],
                     [0, 0, 0, 1.0]])


def host_chain(tr, chained):
    """the demo loop over the rows: one pose through all of them (chained) or one step per row from the unit matrix"""
    t0 = time.perf_counter()
    pose = np.eye(4)
    out = np.zeros((len(tr), 16))
    for r in range(len(tr)):
        Tinv = np.linalg.inv(transform(tr[r]))
        pose = pose @ Tinv if chained else Tinv
        out[r] = pose.reshape(16)
    return out, (time.perf_counter() - t0) * 1e3


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def measure(pkg, g, e, tr, reps, chained):
    g.motionInliers(e, tr, np.ones(S, np.int32))
    g.synchronize(); g.profileReset()
    t_call = wall(lambda: g.trajectory(), reps)
    g.synchronize()
    ms, n = g.profileRead("trajectory")
    Tw, t_host = host_chain(tr, chained)
    sp = pkg.SceneParams.default(frame=1)
    g.profileReset()
    t_world = wall(lambda: g.scenePointsWorld(e, sp), reps)
    g.synchronize()
    ms_w, n_w = g.profileRead("scene_points")
    g.profileReset()
    t_up = wall(lambda: g.scenePoints(e, sp, Tw.reshape(S, 4, 4)), reps)
    g.synchronize()
    ms_u, n_u = g.profileRead("scene_points")
    return dict(trajectory_scope_ms=ms / max(n, 1), launches=n, trajectory_call_wall_ms=t_call, host_numpy_chain_ms=t_host,
                scene_points_world_wall_ms=t_world, scene_points_world_scope_ms=ms_w / max(n_w, 1),
                scene_points_uploaded_Tw_wall_ms=t_up, scene_points_uploaded_Tw_scope_ms=ms_u / max(n_u, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    pkg = entry.load_package()
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    seq = pkg.synth.stereo_sequence(W, H, 8, disparity=6, blur=4)
    e = pkg.EgoParams.default(f=300.0, cu=W / 2.0, cv=H / 2.0, base=0.5, inlier_threshold=3.0)
    rng = np.random.default_rng(1)
    tr = np.concatenate([rng.uniform(-0.05, 0.05, (S, 3)), rng.uniform(-2, 2, (S, 3))], 1)
    res = {}
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setTrajectory(); g.profileEnable(True)
    for t in range(2):
        g.pushBack(np.stack([seq[t][0]] * S), np.stack([seq[t][1]] * S), dims)
    g.matchFeatures(QUAD)
    res["group_S256"] = measure(pkg, g, e, tr, a.reps, False)
    g.close()
    g = pkg.SequenceGroup(S, pkg.Params.default())
    g.setTrajectory(); g.profileEnable(True)
    for c in range(2):                       # the second chunk: every row holds a pair
        g.pushBack(np.stack([seq[(c * S + r) % 8][0] for r in range(S)]), np.stack([seq[(c * S + r) % 8][1] for r in range(S)]), dims)
    g.matchFeatures(QUAD)
    res["sequence_chunk256"] = measure(pkg, g, e, tr, a.reps, True)
    g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
