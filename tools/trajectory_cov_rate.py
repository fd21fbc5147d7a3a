"""Device time of the "trajectory_cov" scope beside the "trajectory" scope of the same calls, on
small synthetic frames (the kernels' time depends on the number of chains and rows, not on the images):
  (a) a plain group of S = 256 streams: 256 chains of one row;
  (b) a sequence handle with chunks of 256 frames: one chain of 256 rows.
Every figure is the median over REPS calls, each call read on its own (the step is idempotent for a pushed pair, so the
call is repeated).  Beside each: the call's wall time and the numpy restatement of the same rows on the host --
Sigma' = Ad (Sigma + Q) Ad^T with numpy's own products, one row after the other.  (b) - (a) over 255 rows is phase B's
cost per row.  Prints one JSON line.

    python tools/trajectory_cov_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

W, H, S = 320, 160, 256
QUAD = 2


def host_chain(tr, cov, chained):
    """the rule in numpy's own linear algebra: one Sigma through all rows (chained) or one step per row from zero"""
    import trajectory_cov_oracle as tc
    t0 = time.perf_counter()
    Sg = np.zeros((6, 6))
    out = np.zeros((len(tr), 6, 6))
    for r in range(len(tr)):
        rr, drx, dry, drz = [np.array(m).reshape(3, 3) for m in tc.rot(tr[r])]
        G = np.zeros((6, 6))
        for k, dR in enumerate((drx, dry, drz)):
            Wm = rr.T @ dR
            G[:3, k] = (Wm[2, 1], Wm[0, 2], Wm[1, 0])
        G[3:, 3:] = rr.T
        t = tr[r, 3:]
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        Ad = np.zeros((6, 6)); Ad[:3, :3] = rr; Ad[3:, 3:] = rr; Ad[3:, :3] = tx @ rr
        Sg = Ad @ ((Sg if chained else 0) + G @ cov[r] @ G.T) @ Ad.T
        out[r] = Sg
    return out, (time.perf_counter() - t0) * 1e3


def measure(g, e, tr, reps, chained):
    g.motionInliers(e, tr, np.ones(S, np.int32))
    cov, _, okc, _ = g.motionCovariance(e)
    g.synchronize()
    scope = {"trajectory": [], "trajectory_cov": []}
    walls = []
    for _ in range(reps):
        g.profileReset()
        t0 = time.perf_counter(); g.trajectory(); walls.append((time.perf_counter() - t0) * 1e3)
        g.synchronize()
        for name in scope:
            ms, n = g.profileRead(name)
            assert n == 1, (name, n)
            scope[name].append(ms)
    got = g.getPoseCovariances()
    want, t_host = host_chain(tr, cov, chained)
    own = okc.astype(bool) & (got["status"] == 0)
    sel = own if not chained else np.ones(S, bool) & bool(own.all())
    err = float(np.abs(got["cov"][sel] - want[sel]).max() / np.abs(want[sel]).max()) if sel.any() else None
    return dict(trajectory_cov_scope_ms=float(np.median(scope["trajectory_cov"])), trajectory_scope_ms=float(np.median(scope["trajectory"])),
                call_wall_ms=float(np.median(walls)), host_numpy_chain_ms=t_host, rows_with_own_covariance=int(own.sum()),
                device_against_numpy=err)


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
    g.setTrajectory(); g.setTrajectoryCovariance(); g.profileEnable(True)
    for t in range(2):
        g.pushBack(np.stack([seq[t][0]] * S), np.stack([seq[t][1]] * S), dims)
    g.matchFeatures(QUAD)
    res["group_S256"] = measure(g, e, tr, a.reps, False)
    g.close()
    g = pkg.SequenceGroup(S, pkg.Params.default())
    g.setTrajectory(); g.setTrajectoryCovariance(); g.profileEnable(True)
    for c in range(2):                       # the second chunk: every row holds a pair
        g.pushBack(np.stack([seq[(c * S + r) % 8][0] for r in range(S)]), np.stack([seq[(c * S + r) % 8][1] for r in range(S)]), dims)
    g.matchFeatures(QUAD)
    res["sequence_chunk256"] = measure(g, e, tr, a.reps, True)
    g.close()
    a_, b_ = res["group_S256"], res["sequence_chunk256"]
    res["phase_b_us_per_row"] = (b_["trajectory_cov_scope_ms"] - a_["trajectory_cov_scope_ms"]) * 1e3 / (S - 1)
    res["pose_us_per_row"] = (b_["trajectory_scope_ms"] - a_["trajectory_scope_ms"]) * 1e3 / (S - 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
