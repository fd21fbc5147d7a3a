"""Helper of test_multistage_scale.py::test_child_kitti_group_in_sub_batches (run as a script under VH_SUBBATCH=3).

Six streams of 1241 x 376 frames with multi-stage matching on: every row equals the lone matcher's list and the
restatement's; vh_group_remove_outliers, the host chain (vh_group_post_begin / _finish, _finish_mono for flow) see the
pass-2 list: against oracle.remove_outliers -> bucketFeatures -> the oracle's estimator on the restatement's pass-2 list,
lists bit for bit, inlier counts exact, tr to 1e-9 relative."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as entry  # noqa: E402
import multistage_oracle as mo  # noqa: E402
from test_multistage import check_not_vacuous, images_of, lone_lists  # noqa: E402
from test_multistage_scale import KH, KW, kitti_frames  # noqa: E402


def bucketed(oracle, pm):
    q = oracle.remove_outliers(pm)[0].copy()
    n = oracle.lib.vo_bucket_features(q.ctypes.data_as(C.c_void_p), len(q), 2, C.c_float(50), C.c_float(50))
    return q[:n].copy()


def main():
    assert os.environ.get("VH_SUBBATCH") == "3"
    pkg, ob = entry.load_package(), entry.load_oracle()
    oracle = ob.Oracle()
    S = 6
    dims = [KW, KH, pkg.synth.bytes_per_line(KW)]
    fr = kitti_frames(pkg, S + 1)
    p, po = pkg.Params.default(multi_stage=1), ob.Params.default(multi_stage=1)
    lone = lone_lists(pkg, p, fr, dims, (0, 2), True)
    want = {}
    for s in range(S):
        for method in (0, 2):
            r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[s], fr[s + 1]), fast=True)
            check_not_vacuous(po, method, r)
            assert r["dense"].tobytes() != oracle.matching(po, dims, method, *r["dense_sets"]).tobytes()
            want[(s, method)] = r
    g = pkg.StreamGroup(S, p)
    g.setMultiStageMatching(True)
    for step in range(2):
        g.pushBack(np.stack([fr[s + step][0] for s in range(S)]), np.stack([fr[s + step][1] for s in range(S)]), dims)

    def rows(method):
        for s in range(S):
            got = g.getMatches(s)
            assert got.tobytes() == lone[(s + 1, method)].tobytes(), (method, s)
            assert got.tobytes() == want[(s, method)]["dense"].tobytes(), (method, s)
            assert g.getSparseMatches(s).tobytes() == want[(s, method)]["sparse"].tobytes(), (method, s)

    g.matchFeatures(2)
    rows(2)
    g.removeOutliers(host_threads=3)
    for s in range(S):
        voted = oracle.remove_outliers(want[(s, 2)]["dense"])[0]
        assert 0 < len(voted) < len(want[(s, 2)]["dense"]) and g.getMatches(s).tobytes() == voted.tobytes(), s
    # the host chain, stereo estimator
    g.matchFeatures(2)
    rows(2)
    ge = pkg.EgoParams.default(f=700.0, cu=KW / 2, cv=KH / 2, base=0.5)
    e = ob.EgoParams.default(f=700.0, cu=KW / 2, cv=KH / 2, base=0.5)
    raw = np.random.default_rng(6).integers(0, 2 ** 31 - 1, (S, 200, 3)).astype(np.int32)
    g.postBegin(32768)
    got = g.postFinish(0, 2, 50.0, 50.0, host_threads=2, ego=ge, rand3=raw)
    for s in range(S):
        q = bucketed(oracle, want[(s, 2)]["dense"])
        ok_o, tr_o, inl_o = oracle.estimate_motion_stereo(e, q, oracle.draw_samples(len(q), 200, raw[s].reshape(-1)))
        assert len(q) > 20 and got["lists"][s].tobytes() == q.tobytes(), s
        assert got["ok"][s] == ok_o and got["n_inliers"][s] == len(inl_o), s
        assert np.allclose(got["tr"][s], tr_o, rtol=1e-9, atol=1e-12), (s, got["tr"][s], tr_o)
    # flow, monocular estimator
    g.matchFeatures(0)
    rows(0)
    em = ob.MonoParams.default(ransac_iters=300, height=1.65, f=700.0, cu=KW / 2, cv=KH / 2)
    gm = pkg.MonoParams.default(ransac_iters=em.ransac_iters, inlier_threshold=em.inlier_threshold, motion_threshold=em.motion_threshold,
                                height=em.height, pitch=em.pitch, f=em.f, cu=em.cu, cv=em.cv)
    raw8 = np.random.default_rng(7).integers(0, 2 ** 31 - 1, (S, 300, 8)).astype(np.int32)
    g.postBegin(32768)
    got = g.postFinish(0, 2, 50.0, 50.0, host_threads=2, mono=gm, rand8=raw8)
    for s in range(S):
        q = bucketed(oracle, want[(s, 0)]["dense"])
        ok_o, tr_o, inl_o = oracle.estimate_motion_mono(em, q, oracle.draw_samples_n(len(q), 8, 300, raw8[s].reshape(-1)))
        assert len(q) > 20 and got["lists"][s].tobytes() == q.tobytes(), s
        assert got["ok"][s] == ok_o and got["n_inliers"][s] == len(inl_o), s
        assert np.allclose(got["tr"][s], tr_o, rtol=1e-9, atol=1e-12), (s, got["tr"][s], tr_o)
    g.close()
    print("multistage group ok")


if __name__ == "__main__":
    main()
