"""The motion prior together with multi-stage matching (vh_set_multi_stage_prior, vh_group_set_multi_stage_prior; DESIGN.md
section 6, "Prior contract").

tests/multistage_prior_oracle.py restates pass 2 with the distance term; with every range at +-R it equals the pinned
oracle.matching_quad_prior, and lone matchers, groups and sequence handles must equal it byte for byte.

Equal double costs: no scene gives two candidates that tie at the minimum WITH the term added, and the library has no
stateless entry that takes constructed features together with a motion estimate; the ties asserted below are those of
the estimate whose predictions are negative (the term is skipped, the costs are the same doubles in the kernel and go
through the same (cost, position) reduction)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import multistage_oracle as mo
import multistage_prior_oracle as mpo
from conftest import ROOT
from test_multistage import scene

W, H = 320, 160
CAM = dict(f=300.0, cu=W / 2, cv=H / 2, base=0.5)
NEW_SYMBOLS = ("vh_sequence_set_multi_stage", "vh_set_multi_stage_prior", "vh_group_set_multi_stage_prior")
SEED = 7


def motion(tx=0.0, ty=0.0, tz=0.0, ry=0.0):
    t = np.eye(4)
    t[0, 3], t[1, 3], t[2, 3] = tx, ty, tz
    c, s = np.cos(ry), np.sin(ry)
    t[0, 0], t[0, 2], t[2, 0], t[2, 2] = c, s, -s, c
    return t.reshape(16)


#: identity, a forward motion, a prediction right of the image, negative predictions (the term is skipped)
MOTIONS = {"eye": motion(), "forward": motion(tz=-1.0), "outside": motion(tx=30.0), "negative": motion(tx=-200.0)}

_cache = {}


def case(pkg, ob, oracle):
    """The pair of the tests, its oracle answers per motion estimate (computed once) and the list without the prior."""
    if not _cache:
        dims = [W, H, pkg.synth.bytes_per_line(W)]
        fr = scene(pkg, 3, seed=SEED)
        po = ob.Params.default(multi_stage=1, **CAM)
        imgs = (fr[0][0], fr[0][1], fr[1][0], fr[1][1])
        plain = mo.multistage(ob, oracle, po, dims, 2, imgs)
        trs = dict(MOTIONS)
        # z2c = 0 for a known driver: the third row of the estimate maps its 3-d point to depth 0
        sets = [mo.Index(po, dims, m) for m in plain["dense_sets"]]
        i = len(sets[0].m) // 2
        u1p, v1p = int(sets[0].m[i, 0]), int(sets[0].m[i, 1])
        ubn, vbn = mo.bin_grid(po, dims)
        sb = min(v1p // po.match_binsize, vbn - 1) * ubn + min(u1p // po.match_binsize, ubn - 1)
        i2p = mo.find_match(po, sets[0], i, sets[1], plain["ranges"][sb, 0], False)
        d = max(float(u1p - int(sets[1].m[i2p, 0])), 1.0)
        t = motion()
        t[11] = -(CAM["f"] * CAM["base"] / d)
        trs["zero_depth"] = t
        ans = {}
        for name, tr in trs.items():
            trace = {}
            ans[name] = mpo.multistage_prior(ob, oracle, po, dims, imgs, tr, trace)
            ans[name]["trace"] = trace
        _cache.update(dims=dims, fr=fr, po=po, plain=plain, trs=trs, ans=ans, driver=i)
    return _cache


# ------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = C.CDLL(pkg.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert callable(pkg.SequenceGroup.setMultiStage)
    assert pkg.SequenceGroup.setMultiStageMatching is not pkg.StreamGroup.setMultiStageMatching
    assert pkg.SequenceGroup.setMultiStageDevice is not pkg.StreamGroup.setMultiStageDevice
    assert callable(pkg.Matcher.setMultiStagePrior) and callable(pkg.StreamGroup.setMultiStagePrior)
    shim = open(os.path.join(ROOT, "include", "viso_hip_matcher.hpp")).read()
    assert "setMultiStagePrior" in shim and "vh_set_multi_stage_prior" in shim


def test_null_handles_need_no_gpu(pkg):
    lib = pkg._lib()
    for mode in (0, 1, 2, 3, -1):
        assert lib.vh_sequence_set_multi_stage(None, mode) == pkg.VH_ERR_INVALID_ARG
    for on in (0, 1):
        assert lib.vh_set_multi_stage_prior(None, on) == pkg.VH_ERR_INVALID_ARG
        assert lib.vh_group_set_multi_stage_prior(None, on) == pkg.VH_ERR_INVALID_ARG


def test_oracle_with_full_ranges_equals_the_pinned_prior_matching(pkg, ob, oracle):
    """The chain to reference-pinned code: with every range at +-R the restatement is oracle.matching_quad_prior."""
    c = case(pkg, ob, oracle)
    sets = c["plain"]["dense_sets"]
    for name in ("eye", "forward", "outside", "negative", "zero_depth"):
        want = oracle.matching_quad_prior(c["po"], c["dims"], c["trs"][name], *sets)
        got = mpo.ranged_matching_prior(c["po"], c["dims"], *sets, mo.full_ranges(c["po"], c["dims"]), c["trs"][name])
        assert len(want) > 50 and got.tobytes() == want.tobytes(), name
    # the sparse sets too (pass 1 runs the pinned code on them)
    sp = c["plain"]["sparse_sets"]
    want = oracle.matching_quad_prior(c["po"], c["dims"], c["trs"]["forward"], *sp)
    assert mpo.ranged_matching_prior(c["po"], c["dims"], *sp, mo.full_ranges(c["po"], c["dims"]), c["trs"]["forward"]).tobytes() == want.tobytes()


def test_the_cases_show_something(pkg, ob, oracle):
    """Properties of the oracle's answers alone: the estimates change the list, and every edge of the issue occurs."""
    c = case(pkg, ob, oracle)
    plain = c["plain"]["dense"].tobytes()
    ans = c["ans"]
    assert any(ans[n]["dense"].tobytes() != plain for n in ("eye", "forward", "outside"))
    assert ans["outside"]["dense"].tobytes() != plain
    rg = ans["forward"]["ranges"]
    assert ((rg[:, :, 0::2] != -200) | (rg[:, :, 1::2] != 200)).any()

    def preds(name):
        tr = ans[name]["trace"]
        return np.array([v[0] for v in tr.values()]), np.array([v[1] for v in tr.values()])

    u, v = preds("outside")
    assert (u >= W).sum() > 100
    u, v = preds("negative")
    assert ((u < 0) | (v < 0)).all() and ans["negative"]["dense"].tobytes() == plain  # the term is skipped everywhere
    ties = sum(len(x[3]) > 1 and (x[3] == x[3].min()).sum() > 1 for x in ans["negative"]["trace"].values())
    assert ties > 0, "no two candidates tie at the minimum"
    u, v = preds("zero_depth")
    du, dv = ans["zero_depth"]["trace"][c["driver"]][:2]
    assert not np.isfinite(du) or not np.isfinite(dv), (du, dv)
    assert (~np.isfinite(u) | ~np.isfinite(v)).sum() >= 1
    for name in ans:
        assert len(ans[name]["dense"]) > 50 and len(ans[name]["sparse"]) > 20, name


# ------------------------------------------------------------------ GPU
def prior_matcher(pkg, p, cam=True):
    m = pkg.Matcher(p, outlier_removal=False)
    if cam:
        m.setIntrinsics(CAM["f"], CAM["cu"], CAM["cv"], CAM["base"])
    m.setMultiStageMatching(True)
    m.setMultiStagePrior(True)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("device_mode", (False, True))
def test_lone_matcher_equals_the_oracle(pkg, ob, oracle, gpu, device_mode):
    c = case(pkg, ob, oracle)
    p = pkg.Params.default(multi_stage=1)
    m = prior_matcher(pkg, p)
    if device_mode:
        m.setMultiStageDevice(True)
    for t in range(2):
        m.pushBack(c["fr"][t][0], c["fr"][t][1], c["dims"])
    for name, tr in c["trs"].items():
        m.matchFeatures(2, tr)
        got = m.getMatches()
        want = c["ans"][name]
        assert got.tobytes() == want["dense"].tobytes(), (name, len(got), len(want["dense"]))
        assert m.getSparseMatches().tobytes() == want["sparse"].tobytes(), name
    # without an estimate the call is today's multi-stage matching; flow and stereo ignore the estimate
    m.matchFeatures(2)
    assert m.getMatches().tobytes() == c["plain"]["dense"].tobytes()
    for meth in (0, 1):
        m.matchFeatures(meth)
        want = m.getMatches().tobytes()
        m.matchFeatures(meth, c["trs"]["forward"])
        assert len(want) > 0 and m.getMatches().tobytes() == want, meth
    m.close()


@pytest.mark.gpu
def test_group_and_sequence_equal_the_oracle(pkg, ob, oracle, gpu):
    """Every stream / row under its own estimate: one Tr per row."""
    c = case(pkg, ob, oracle)
    p = pkg.Params.default(multi_stage=1, **CAM)
    names = list(c["trs"])
    S = len(names)
    trs = np.stack([c["trs"][n] for n in names])
    for device_mode in (False, True):
        g = pkg.StreamGroup(S, p)
        g.setMultiStageMatching(True)
        if device_mode:
            g.setMultiStageDevice(True)
        g.setMultiStagePrior(True)
        for t in range(2):
            g.pushBack(np.stack([c["fr"][t][0]] * S), np.stack([c["fr"][t][1]] * S), c["dims"])
        g.matchFeaturesPrior(2, trs)
        for s, n in enumerate(names):
            assert g.getMatches(s).tobytes() == c["ans"][n]["dense"].tobytes(), (device_mode, n)
            assert g.getSparseMatches(s).tobytes() == c["ans"][n]["sparse"].tobytes(), (device_mode, n)
        g.close()
    # a sequence whose frames alternate between the pair's two frames: every row is the pair or its reverse
    for mode in (1, 2):
        q = pkg.SequenceGroup(3, p)
        q.setMultiStage(mode)
        q.setMultiStagePrior(True)
        for chunk in ((0, 1, 0), (1,)):
            q.pushBack(np.stack([c["fr"][t][0] for t in chunk]), np.stack([c["fr"][t][1] for t in chunk]), c["dims"])
            if len(chunk) == 3:
                q.matchFeaturesPrior(2, np.stack([c["trs"]["eye"], c["trs"]["forward"], c["trs"]["eye"]]))
                assert len(q.getMatches(0)) == 0
                assert q.getMatches(1).tobytes() == c["ans"]["forward"]["dense"].tobytes(), mode
                assert q.getSparseMatches(1).tobytes() == c["ans"]["forward"]["sparse"].tobytes(), mode
            else:  # row 0 links to the last row of the previous chunk
                q.matchFeaturesPrior(2, c["trs"]["outside"].reshape(1, 16))
                assert q.getMatches(0).tobytes() == c["ans"]["outside"]["dense"].tobytes(), mode
                assert q.getSparseMatches(0).tobytes() == c["ans"]["outside"]["sparse"].tobytes(), mode
        q.close()


@pytest.mark.gpu
def test_switch_states(pkg, ob, oracle, gpu):
    lib = pkg._lib()
    c = case(pkg, ob, oracle)
    tr = c["trs"]["forward"]
    T = tr.ctypes.data_as(C.c_void_p)
    p = pkg.Params.default(multi_stage=1)
    # set after multi-stage matching, before the first push
    m = pkg.Matcher(p, outlier_removal=False)
    assert lib.vh_set_multi_stage_prior(m._h, 1) == pkg.VH_ERR_STATE
    assert lib.vh_set_multi_stage_prior(m._h, 0) == pkg.VH_OK
    m.setMultiStageMatching(True)
    m.setIntrinsics(CAM["f"], CAM["cu"], CAM["cv"], CAM["base"])
    for t in range(2):
        m.pushBack(c["fr"][t][0], c["fr"][t][1], c["dims"])
    assert lib.vh_set_multi_stage_prior(m._h, 1) == pkg.VH_ERR_STATE
    # off (the default): the refusal the earlier tests pin
    assert lib.vh_match_features(m._h, 2, T) == pkg.VH_ERR_UNSUPPORTED
    assert lib.vh_match_features(m._h, 0, T) == pkg.VH_ERR_UNSUPPORTED
    m.close()
    # switching multi-stage matching off clears it
    m = pkg.Matcher(p, outlier_removal=False)
    m.setMultiStageMatching(True)
    m.setMultiStagePrior(True)
    m.setMultiStageMatching(False)
    assert lib.vh_set_multi_stage_prior(m._h, 1) == pkg.VH_ERR_STATE
    m.close()
    # on without intrinsics
    m = prior_matcher(pkg, p, cam=False)
    for t in range(2):
        m.pushBack(c["fr"][t][0], c["fr"][t][1], c["dims"])
    assert lib.vh_match_features(m._h, 2, T) == pkg.VH_ERR_STATE
    m.matchFeatures(2)
    assert m.getMatches().tobytes() == c["plain"]["dense"].tobytes()
    m.close()
    # the sequence entry: kinds, modes, order
    g = pkg.StreamGroup(2, p)
    assert lib.vh_sequence_set_multi_stage(g._h, 1) == pkg.VH_ERR_UNSUPPORTED
    assert lib.vh_sequence_set_multi_stage(g._h, 0) == pkg.VH_ERR_UNSUPPORTED
    g.close()
    m = pkg.Matcher(p)
    assert lib.vh_sequence_set_multi_stage(m._h, 1) == pkg.VH_ERR_UNSUPPORTED
    m.close()
    q = pkg.SequenceGroup(2, pkg.Params.default(multi_stage=0))
    assert lib.vh_sequence_set_multi_stage(q._h, 1) == pkg.VH_ERR_INVALID_ARG  # needs p.multi_stage = 1
    assert lib.vh_sequence_set_multi_stage(q._h, 0) == pkg.VH_OK
    q.close()
    q = pkg.SequenceGroup(2, p)
    assert lib.vh_sequence_set_multi_stage(q._h, 3) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_sequence_set_multi_stage(q._h, -1) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_set_multi_stage_prior(q._h, 1) == pkg.VH_ERR_STATE
    with pytest.raises(pkg.VisoHipError):
        q.setMultiStageDevice(True)  # multi-stage matching first, as on a group
    for mode in (2, 1, 0, 1):
        assert lib.vh_sequence_set_multi_stage(q._h, mode) == pkg.VH_OK
    assert lib.vh_group_set_multi_stage_prior(q._h, 1) == pkg.VH_OK
    assert lib.vh_group_set_multi_stage_matching(q._h, 1) == pkg.VH_ERR_UNSUPPORTED  # the old entries keep refusing
    assert lib.vh_group_set_multi_stage_device(q._h, 1) == pkg.VH_ERR_UNSUPPORTED
    q.pushBack(np.stack([c["fr"][0][0]]), np.stack([c["fr"][0][1]]), c["dims"])
    for mode in (0, 1, 2):
        assert lib.vh_sequence_set_multi_stage(q._h, mode) == pkg.VH_ERR_STATE
    assert lib.vh_group_set_multi_stage_prior(q._h, 0) == pkg.VH_ERR_STATE
    q.close()


@pytest.mark.gpu
def test_child_prior_checking_build(pkg, gpu):
    """The lone, group and sequence cases on libviso_hip_check.so (-DVH_CHECK), detection in sub-batches."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH, VH_SUBBATCH="3")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "lone_matcher_equals or group_and_sequence"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "3 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr
