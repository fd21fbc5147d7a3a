#!/usr/bin/env python3
"""Records tests/golden/reconstruction_reference.npz: a synthetic drive (match lists and the Tr of every update) and what
the REFERENCE's Reconstruction::getPoints() returns after every update.  Test infrastructure: compiles
tools/recon_ref_harness.cpp against the reference tree (oracle.binding.REFERENCE_ROOT) into the ignored oracle/_ref/ and
runs it; only the data is kept.

The drive: a KITTI-like camera (tests/egomotion_scene.py: KITTI) moving forward about 0.85 m per frame with a slight turn,
13 frames = 12 updates, about 300 static points of which each is tracked from its own first to its own last frame (2 to 12
frames), positions rounded to pixels.  Per update the match list is shuffled; a few matches repeat another's i1p or i1c
(the association's table then has two claimants), a few carry i1p of a feature that no track ends in, and update 7 is a
gap: its list holds a handful of matches only, so that nearly every track is lost at once and starts anew after it."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import binding as ob  # noqa: E402
from egomotion_scene import KITTI, rot  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reconstruction_reference.npz")
W, H = 1241, 376
N_UPDATES, GAP = 12, 7


def drive(seed=2024, n_points=300):
    """-> (lists [N_UPDATES] of p_match arrays, Trs [N_UPDATES, 4, 4])."""
    rng = np.random.default_rng(seed)
    f, cu, cv = KITTI["f"], KITTI["cu"], KITTI["cv"]
    Trs, poses = [], [np.eye(4)]   # pose k: world (= frame 0) -> frame k
    for k in range(N_UPDATES):
        Tr = np.eye(4)
        Tr[:3, :3] = rot(rng.normal(0, 0.002), -0.01 + rng.normal(0, 0.003), rng.normal(0, 0.001))
        Tr[:3, 3] = (rng.normal(0.02, 0.01), rng.normal(-0.005, 0.005), -0.85 + rng.normal(0, 0.05))
        Trs.append(Tr)
        poses.append(Tr @ poses[-1])
    # points: drawn in front of the frame they enter in; a share on the road plane 1.65 m below the camera
    feats = []
    while len(feats) < n_points:
        enter = int(rng.integers(0, N_UPDATES))
        leave = min(N_UPDATES, enter + int(rng.choice([1, 1, 2, 2, 3, 4, 5, 7, 12])))
        Z = rng.uniform(4, 45)
        if rng.random() < 0.4:
            X, Y = rng.uniform(-0.8, 0.8) * Z * 0.5, 1.65
        else:
            X, Y = rng.uniform(-1, 1) * Z * 0.8, rng.uniform(-0.28, 0.05) * Z
        Pw = np.linalg.inv(poses[enter]) @ np.array([X, Y, Z, 1.0])
        px = {}
        for k in range(enter, leave + 1):
            q = poses[k] @ Pw
            if q[2] < 1.5:
                break
            u, v = np.round(f * q[0] / q[2] + cu), np.round(f * q[1] / q[2] + cv)
            if not (0 <= u < W and 0 <= v < H):
                break
            px[k] = (u, v)
        if len(px) >= 2:
            feats.append(px)
    # feature indices per frame: a permutation of the features visible in it
    index = []
    for k in range(N_UPDATES + 1):
        vis = [i for i, px in enumerate(feats) if k in px]
        perm = rng.permutation(len(vis))
        index.append({i: int(perm[j]) for j, i in enumerate(vis)})
    lists = []
    for k in range(1, N_UPDATES + 1):
        both = [i for i, px in enumerate(feats) if k - 1 in px and k in px]
        if k == GAP:
            both = both[:5]
        pm = np.zeros(len(both), ob.P_MATCH_DTYPE)
        for name in pm.dtype.names:
            pm[name] = -1
        for j, i in enumerate(both):
            pm[j]["u1p"], pm[j]["v1p"] = feats[i][k - 1]
            pm[j]["u1c"], pm[j]["v1c"] = feats[i][k]
            pm[j]["i1p"], pm[j]["i1c"] = index[k - 1][i], index[k][i]
        extra = []
        if len(pm) > 20 and k != GAP:
            n_next = len(index[k])
            for j in rng.choice(len(pm), 4, replace=False):      # a second match from the same previous feature
                m = pm[j].copy(); m["u1c"] += 3; m["v1c"] -= 2; m["i1c"] = n_next; n_next += 1
                extra.append(m)
            for j in rng.choice(len(pm), 3, replace=False):      # a second match INTO the same current feature
                m = pm[j].copy(); m["u1p"] -= 4; m["v1p"] += 1; m["i1p"] = len(index[k - 1]) + 5
                extra.append(m)
        if extra:
            pm = np.concatenate([pm, np.array(extra, ob.P_MATCH_DTYPE)])
        lists.append(pm[rng.permutation(len(pm))])
    return lists, np.array(Trs)


def main():
    lists, Trs = drive()
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(ref_dir, exist_ok=True)
    exe = os.path.join(ref_dir, "recon_ref_harness")
    src = os.path.join(ob.REFERENCE_ROOT, "src")
    subprocess.check_call(["g++", "-std=gnu++11", "-O2", "-msse3", "-w", "-I" + src, os.path.join(ROOT, "tools", "recon_ref_harness.cpp"),
                           os.path.join(src, "reconstruction.cpp"), os.path.join(src, "matrix.cpp"), "-o", exe])
    din, dout = os.path.join(ref_dir, "recon_drive.bin"), os.path.join(ref_dir, "recon_points.bin")
    with open(din, "wb") as fh:
        fh.write(np.int32(len(lists)).tobytes())
        fh.write(np.array([KITTI["f"], KITTI["cu"], KITTI["cv"]], np.float64).tobytes())
        for pm, Tr in zip(lists, Trs):
            fh.write(np.ascontiguousarray(Tr, np.float64).tobytes())
            fh.write(np.int32(len(pm)).tobytes())
            fh.write(pm.tobytes())
    subprocess.check_call([exe, din, dout])
    raw = open(dout, "rb").read()
    pos, counts, pts = 0, [], np.zeros((0, 3), np.float32)
    for _ in lists:
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0]); pos += 4
        cur = np.frombuffer(raw, np.float32, 3 * n, pos).reshape(n, 3); pos += 12 * n
        assert cur[:len(pts)].tobytes() == pts.tobytes(), "getPoints() only ever appends"
        pts = cur.copy(); counts.append(n)
    assert pos == len(raw)
    np.savez_compressed(OUT, calibration=np.array([KITTI["f"], KITTI["cu"], KITTI["cv"]]), Trs=Trs,
                        matches=np.concatenate(lists), list_counts=np.array([len(m) for m in lists], np.int32),
                        points=pts, point_counts=np.array(counts, np.int32))
    print(f"{OUT}: {len(lists)} updates, {sum(len(m) for m in lists)} matches, points after each update {counts}, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
