"""Reconstruction on a plain group: vh_group_set_reconstruction, vh_group_reconstruct,
vh_group_get_recon_tracks, vh_group_get_recon_counts.  Stream s's records over a drive are what
tests/sequence_recon_oracle.py gives for stream s's own lists and motions -- byte for byte, the angle to 1e-9 degrees --
whatever the other streams hold."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import recon_cases as rc
import reconstruction_oracle as ro
import sequence_recon_oracle as so
import test_sequence_recon as sr   # its helpers: same(), the constructed lists, the synthetic frames
from conftest import ROOT

SYMBOLS = ("vh_group_set_reconstruction", "vh_group_reconstruct", "vh_group_get_recon_tracks", "vh_group_get_recon_counts")
SCOPES = ("recon_store", "recon_tails", "recon_gather", "recon_solve")
FLOW, QUAD = sr.FLOW, sr.QUAD
CAL, LOOSE = sr.CAL, sr.LOOSE
ptr, same, expect = sr.ptr, sr.same, sr.expect
S3, STEPS = 3, 12
SEEDS = (61, 62, 63)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = C.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS + ("vh_group_debug_reconstruct_lists",):
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    for meth in ("setReconstruction", "reconstruct", "getReconCounts"):
        assert meth in vars(pkg.StreamGroup), meth
    for meth in ("setReconstruction", "reconstruct"):   # the sequence handle keeps its own
        assert meth in vars(pkg.SequenceGroup), meth


def test_null_and_argument_errors_need_no_gpu(pkg):
    lib = pkg._lib()
    r = pkg.ReconParams.default()
    n, na = C.c_int32(7), C.c_int32(7)
    out = np.zeros(4, pkg.RECON_TRACK)
    tr = np.zeros((2, 16))
    cnt = np.zeros(2, np.int32)
    inv = pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_set_reconstruction(None, C.byref(r), 4) == inv
    assert lib.vh_group_reconstruct(None, ptr(tr), C.byref(n), C.byref(na)) == inv
    assert lib.vh_group_get_recon_tracks(None, 0, ptr(out), 4, C.byref(n)) == inv
    assert lib.vh_group_get_recon_counts(None, ptr(cnt), ptr(cnt)) == inv
    pm = np.zeros(4, pkg.P_MATCH_DTYPE)
    c1 = np.array([4], np.int32)
    call = lambda *a: lib.vh_group_debug_reconstruct_lists(*a)  # noqa: E731
    assert call(None, 0, 1, 1, ptr(pm), 4, ptr(c1), 8, ptr(tr), ptr(out), 4, ptr(cnt)) == inv
    assert call(C.byref(r), 0, 0, 1, ptr(pm), 4, ptr(c1), 8, ptr(tr), ptr(out), 4, ptr(cnt)) == inv
    assert call(C.byref(r), 0, 1, 1, ptr(pm), 2, ptr(c1), 8, ptr(tr), ptr(out), 4, ptr(cnt)) == inv   # count > stride
    assert call(C.byref(r), 0, 1, 1, None, 4, ptr(c1), 8, ptr(tr), ptr(out), 4, ptr(cnt)) == inv
    assert call(C.byref(r), 0, 1, 1, ptr(pm), 4, ptr(c1), 8, ptr(tr), ptr(out), 4, None) == inv


# ------------------------------------------------------------------------------------------------------------ GPU
def poses_of(n, s):
    """Another motion per stream."""
    return [rc.pose(0.0, -0.004 * k * (1 + s), 0.001 * s * k, (0.03 * k, 0.01 * s * k, (0.5 + 0.1 * s) * k)) for k in range(n)]


def stream_frames(pkg, seeds, T, flat=()):
    """frames[s][t] = (left, right); the streams in `flat` see constant images (no feature, empty lists)."""
    out = [sr.frames_of(pkg, T, seed) for seed in seeds]
    for s in flat:
        out[s] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in out[s]]
    return out


def push(g, frames, t, dims, replace=False):
    g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims, replace=replace)


def lists_of(g):
    return [g.getMatches(s) for s in range(g.S)]


def step_trs(Trs, k):
    """One Tr per stream for the step of serial k: the motion k-1 -> k (the first step holds no pair)."""
    return np.array([T[k - 1] if k >= 1 else np.eye(4) for T in Trs])


_DRIVES = {}


def drive(pkg, oracle, meth):
    """S3 streams of STEPS + 1 frames: the lists (from a group without reconstruction), each stream's Trs and the oracle's
    whole-drive records per stream, computed once per method and left unchanged."""
    if meth not in _DRIVES:
        frames, dims = stream_frames(pkg, SEEDS, STEPS + 1), sr.dims_of(pkg)
        g = pkg.StreamGroup(S3, pkg.Params.default())
        lists = [[] for _ in range(S3)]
        for t in range(STEPS + 1):
            push(g, frames, t, dims)
            g.matchFeatures(meth)
            if t:
                for s, pm in enumerate(lists_of(g)):
                    lists[s].append(pm)
        g.close()
        Trs = [rc.trs_of(poses_of(STEPS + 1, s)) for s in range(S3)]
        wholes = [so.whole(oracle.svd, CAL, lists[s], Trs[s], **LOOSE) for s in range(S3)]
        _DRIVES[meth] = (frames, dims, lists, Trs, wholes)
    return _DRIVES[meth]


def run_group(pkg, frames, dims, meth, Hh, Trs, wholes, after_next_push=False):
    """The drive through a group with reconstruction on; every step's records per stream against the oracle's records
    lost at that step.  -> per stream all records, per stream the lists seen."""
    S, T = len(frames), len(frames[0])
    want = [sr.history_of(w, Hh) for w in wholes]
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setReconstruction(sr.recon_params(pkg), Hh)
    got_all, seen = [[] for _ in range(S)], [[] for _ in range(S)]
    for t in range(T):
        if not (after_next_push and t):
            push(g, frames, t, dims)
        g.matchFeatures(meth)
        if t:
            for s, pm in enumerate(lists_of(g)):
                seen[s].append(pm)
        if after_next_push and t + 1 < T:
            push(g, frames, t + 1, dims)      # detection of step t + 1 runs beside reconstruct t
        got = g.reconstruct(step_trs(Trs, t))
        nt, na = g.getReconCounts()
        assert len(got) == S
        for s in range(S):
            same(got[s], want[s][want[s]["lost_frame"] == t], (t, s))
            assert nt[s] == len(got[s]) and na[s] == int((got[s]["status"] == pkg.RECON_ACCEPTED).sum())
            got_all[s].append(got[s])
    g.close()
    return [np.concatenate(x) for x in got_all], seen


@pytest.mark.gpu
@pytest.mark.parametrize("meth", (FLOW, QUAD))
def test_group_equals_oracle_per_stream(pkg, oracle, gpu, meth):
    frames, dims, lists, Trs, wholes = drive(pkg, oracle, meth)
    for s in range(S3):
        for pm in lists[s]:
            assert len(np.unique(pm["i1c"])) == len(pm)
        # properties of the inputs, on the oracle's answer alone
        assert (wholes[s]["status"] == ro.ACCEPTED).any() and len(np.unique(wholes[s]["frames"])) >= 3, s
    assert len({w.tobytes() for w in wholes}) == S3                       # three different drives
    Hh = max(int(w["frames"].max()) - 1 for w in wholes)                  # from the oracle: no record is HISTORY
    got, seen = run_group(pkg, frames, dims, meth, Hh, Trs, wholes)
    for s in range(S3):
        assert len(seen[s]) == len(lists[s]) and all(a.tobytes() == b.tobytes() for a, b in zip(seen[s], lists[s]))
        assert not (got[s]["status"] == pkg.RECON_HISTORY).any()
        same(got[s], wholes[s], s)


@pytest.mark.gpu
def test_group_short_history_ring_wraps(pkg, oracle, gpu):
    frames, dims, lists, Trs, wholes = drive(pkg, oracle, FLOW)
    got, _ = run_group(pkg, frames, dims, FLOW, 2, Trs, wholes)          # 3 ring slots, 13 steps
    for s in range(S3):
        n_old = int((wholes[s]["frames"] - 1 > 2).sum())
        assert 0 < n_old < len(wholes[s]) and int((got[s]["status"] == pkg.RECON_HISTORY).sum()) == n_old


@pytest.mark.gpu
def test_group_reconstruct_after_the_next_push(pkg, oracle, gpu):
    frames, dims, lists, Trs, wholes = drive(pkg, oracle, FLOW)
    got, _ = run_group(pkg, frames, dims, FLOW, 16, Trs, wholes, after_next_push=True)
    assert all(len(x) > 20 for x in got)


@pytest.mark.gpu
def test_group_of_one_equals_sequence_handle(pkg, oracle, gpu):
    frames, dims, lists, Trs, wholes = drive(pkg, oracle, QUAD)
    one = [frames[1]]
    g = pkg.StreamGroup(1, pkg.Params.default())
    q = pkg.SequenceGroup(1, pkg.Params.default())
    g.setReconstruction(sr.recon_params(pkg), 3)
    q.setReconstruction(sr.recon_params(pkg), 3)
    total = 0
    for t in range(STEPS + 1):
        push(g, one, t, dims)
        sr.push(q, one[0], t, 1, dims)
        g.matchFeatures(QUAD)
        q.matchFeatures(QUAD)
        a, b = g.reconstruct(step_trs([Trs[1]], t))[0], q.reconstruct(sr.row_trs(Trs[1], t, 1))
        assert a.tobytes() == b.tobytes(), t
        total += len(a)
    assert total == len(wholes[1]) > 20
    g.close()
    q.close()


@pytest.mark.gpu
def test_group_empty_stream_beside_live_ones(pkg, oracle, gpu):
    frames, dims, lists, Trs, wholes = drive(pkg, oracle, FLOW)
    flat = stream_frames(pkg, SEEDS, STEPS + 1, flat=(1,))
    Hh = max(int(w["frames"].max()) - 1 for w in wholes)
    empty = np.zeros(0, so.RECON_TRACK)
    got, seen = run_group(pkg, flat, dims, FLOW, Hh, Trs, [wholes[0], empty, wholes[2]])
    assert all(len(pm) == 0 for pm in seen[1]) and len(got[1]) == 0
    assert len(got[0]) == len(wholes[0]) and len(got[2]) == len(wholes[2])


@pytest.mark.gpu
def test_group_lists_wave_boundaries_across_streams(pkg, oracle, gpu):
    """Constructed lists through the group form of the kernels (vh_group_debug_reconstruct_lists): per stream 0, 1, 63, 64,
    65 and 257 tracks lost in ONE step (part of a wave, one wave, more than a workgroup; nothing at all) -- where the
    per-wave hand-out of track indices and pixel offsets meets the stream boundaries.  Before it a step in which some
    tracks go on and some end, with duplicate i1p and i1c, i1p = -1 and indices beyond the table."""
    rng = np.random.default_rng(17)
    lost = (0, 1, 63, 64, 65, 257)
    streams, Trs, want = [], [], []
    for s, n in enumerate(lost):
        lists, T = sr.random_chain_lists(pkg, rng, 4, 0, 400, lengths=[n, (n * 3) // 4 + (n > 0), n, 0], empty=(3,))
        streams.append(lists)
        Trs.append(T)
        want.append(so.whole(oracle.svd, CAL, lists, T, n_index=400, **LOOSE))
        assert int((want[s]["lost_frame"] == 4).sum()) == n
    assert any(len(np.unique(w["frames"])) >= 3 for w in want)
    r = sr.recon_params(pkg)
    got = pkg.debug_group_reconstruct_lists(r, streams, np.array(Trs), 400)
    assert len(got) == len(lost) and len(got[0]) == 0
    for s in range(len(lost)):
        same(got[s], want[s], s)
    # the same streams in another order: the neighbours change, the records do not
    order = (4, 0, 5, 2, 1, 3)
    again = pkg.debug_group_reconstruct_lists(r, [streams[s] for s in order], np.array([Trs[s] for s in order]), 400)
    for k, s in enumerate(order):
        assert again[k].tobytes() == got[s].tobytes(), (k, s)


@pytest.mark.gpu
def test_group_call_order_rematch_and_resets(pkg, oracle, gpu):
    """Twice for one step and before any match: VH_ERR_STATE.  A rematch before the call replaces the lists.  A rematch
    after the call, a skipped call, a step never matched, a replace push and a dims change restart every stream, as the
    oracle's reset()."""
    dims = sr.dims_of(pkg)
    S = 2
    frames = stream_frames(pkg, (71, 72), 16)
    Trs = [rc.trs_of(poses_of(16, s)) for s in range(S)]
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setReconstruction(sr.recon_params(pkg), 8)
    d = [so.Drive(oracle.svd, CAL, 8, **LOOSE) for _ in range(S)]

    def check(t, what):
        got = g.reconstruct(step_trs(Trs, t))
        for s, pm in enumerate(lists_of(g)):
            same(got[s], d[s].chunk(t, [pm], [Trs[s][t - 1]]), (t, what, s))
        return got

    def reset():
        for x in d:
            x.reset()

    expect(pkg, pkg.VH_ERR_STATE, lambda: g.reconstruct(step_trs(Trs, 0)))
    push(g, frames, 0, dims)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.reconstruct(step_trs(Trs, 0)))   # pushed, not matched
    g.matchFeatures(FLOW)
    assert all(len(x) == 0 for x in g.reconstruct(step_trs(Trs, 0)))          # the first step holds no pair
    push(g, frames, 1, dims)
    g.matchFeatures(FLOW)
    g.matchFeatures(QUAD)                                                    # the call sees the last lists
    check(1, "rematch before")
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.reconstruct(step_trs(Trs, 1)))   # twice
    total = 0
    plan = {2: "go", 3: "go", 4: "rematch after", 5: "go", 6: "skip", 7: "go", 8: "go", 9: "unmatched", 10: "go", 11: "go",
            12: "replace", 13: "go"}
    for t, what in plan.items():
        push(g, frames, t, dims)
        if what == "unmatched":
            reset()
            continue
        if what == "replace":
            push(g, frames, t, dims, replace=True)
            reset()
        g.matchFeatures(QUAD)
        if what == "skip":
            reset()
            continue
        got = check(t, what)
        if what == "rematch after":
            g.matchFeatures(QUAD)
            reset()
            got = check(t, "rematched")
        if what in ("rematch after", "replace") or plan.get(t - 1) in ("skip", "unmatched"):   # after a break
            for s in range(S):
                assert len(got[s]) == 0 and (g.getTracks(s)["age"] == 1).all(), (t, s)
        elif plan.get(t - 1) in ("rematch after", "replace") or plan.get(t - 2) in ("skip", "unmatched"):
            for s in range(S):   # nothing older than the break: every track was born in the step of the break
                assert len(got[s]) and int(got[s]["birth_frame"].min()) == t - 1 == int(got[s]["birth_frame"].max()), (t, s)
        total += sum(len(x) for x in got)
    assert total > 50
    w2, h2 = 288, 144
    fb = [sr.frames_of(pkg, 4, seed, w=w2, h=h2) for seed in (81, 82)]
    reset()
    for t in range(4):
        push(g, fb, t, sr.dims_of(pkg, w2, h2))
        g.matchFeatures(QUAD)
        if t:
            check(t, "dims")
        else:
            assert all(len(x) == 0 for x in g.reconstruct(step_trs(Trs, 0)))
    g.close()


@pytest.mark.gpu
def test_group_switch_rules_and_capacity(pkg, oracle, gpu):
    r = sr.recon_params(pkg)
    dims = sr.dims_of(pkg)
    frames = stream_frames(pkg, (91, 92), 4)
    Trs = [rc.trs_of(poses_of(4, s)) for s in range(2)]
    q = pkg.SequenceGroup(2, pkg.Params.default())
    assert pkg._lib().vh_group_set_reconstruction(q._h, C.byref(r), 4) == pkg.VH_ERR_UNSUPPORTED
    q.close()
    g = pkg.StreamGroup(2, pkg.Params.default())
    assert pkg._lib().vh_group_set_reconstruction(g._h, C.byref(r), 0) == pkg.VH_ERR_INVALID_ARG
    g.setReconstruction(r, 8)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.setTrackLinking(False))   # linking is on underneath, and stays
    push(g, frames, 0, dims)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.setReconstruction(r, 8))   # after the first push
    g.matchFeatures(FLOW)
    n = C.c_int32(0)
    assert pkg._lib().vh_group_get_recon_tracks(g._h, 0, None, 0, C.byref(n)) == pkg.VH_ERR_STATE   # nothing reconstructed yet
    assert pkg._lib().vh_group_get_recon_counts(g._h, None, None) == pkg.VH_ERR_STATE
    full = g.reconstruct(step_trs(Trs, 0))
    for t in range(1, 4):
        push(g, frames, t, dims)
        g.matchFeatures(FLOW)
        assert len(g.getTracks(1)) == len(g.getMatches(1)) > 20
        full = g.reconstruct(step_trs(Trs, t))
    assert len(full[1]) > 10
    assert pkg._lib().vh_group_get_recon_tracks(g._h, 2, None, 0, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    part = np.zeros(10, pkg.RECON_TRACK)
    rcode = pkg._lib().vh_group_get_recon_tracks(g._h, 1, ptr(part), 10, C.byref(n))
    assert rcode == pkg.VH_ERR_CAPACITY and n.value == len(full[1]) and part.tobytes() == full[1][:10].tobytes()
    na = np.zeros(2, np.int32)
    assert pkg._lib().vh_group_get_recon_counts(g._h, None, ptr(na)) == pkg.VH_OK
    assert na.tolist() == [int((x["status"] == pkg.RECON_ACCEPTED).sum()) for x in full]
    g.close()


@pytest.mark.gpu
def test_group_switch_off_changes_nothing_and_memory(pkg, gpu):
    """Linking on, against reconstruction set and cleared again: same lists, tracks and device bytes, no launch in the
    recon scopes.  Reconstruction on: same lists and tracks, the ring counted in the device bytes."""
    dims = sr.dims_of(pkg)
    S, Hh, mm = 3, 5, 4096
    frames = stream_frames(pkg, SEEDS, 4)
    Trs = [rc.trs_of(poses_of(4, s)) for s in range(S)]
    seen = {}
    for name in ("link", "cleared", "on"):
        g = pkg.StreamGroup(S, pkg.Params.default(), max_features=4096, max_matches=mm)
        if name == "link":
            g.setTrackLinking(True)
        else:
            g.setReconstruction(sr.recon_params(pkg), Hh)
            if name == "cleared":
                g.setReconstruction(None)
        g.profileEnable(True)
        out = []
        for t in range(4):
            push(g, frames, t, dims)
            g.matchFeatures(QUAD)
            out += [g.getMatches(s).tobytes() for s in range(S)] + [g.getTracks(s).tobytes() for s in range(S)]
            if name == "on":
                g.reconstruct(step_trs(Trs, t))
            else:
                expect(pkg, pkg.VH_ERR_STATE, lambda: g.reconstruct(step_trs(Trs, t)))
        seen[name] = (out, g.deviceBytes(), tuple(g.profileRead(k)[1] for k in SCOPES))
        g.close()
    assert seen["link"] == seen["cleared"] and seen["link"][2] == (0, 0, 0, 0)
    assert seen["on"][0] == seen["link"][0]
    assert seen["on"][2] == (3, 5, 2, 2)   # per step with a pair: one store; tails counting, and appending once a list is pending
    assert seen["on"][1] - seen["link"][1] >= 32 * mm * S * (Hh + 1)


@pytest.mark.gpu
def test_group_failed_allocation_inside_the_first_reconstruct(pkg, oracle, gpu):
    """The first reconstruct call allocates the ring, its counters and the first gather buffers; the first call that has
    tracks to gather grows those.  Either fails once: VH_ERR_HIP, and the same call made again gives the oracle's records."""
    dims = sr.dims_of(pkg)
    S = 2
    frames = stream_frames(pkg, (57, 58), 3)
    Trs = [rc.trs_of(poses_of(3, s)) for s in range(S)]
    for skip in (0, 2, 3, 7, 11):   # the ring, its counters, the first and later gather buffers
        g = pkg.StreamGroup(S, pkg.Params.default())
        g.setReconstruction(sr.recon_params(pkg), 4)
        d = [so.Drive(oracle.svd, CAL, 4, **LOOSE) for _ in range(S)]
        push(g, frames, 0, dims)
        push(g, frames, 1, dims)            # (the first step was never matched: the drive starts at step 1)
        for t, sk in ((1, skip), (2, 0)):
            if t == 2:
                push(g, frames, 2, dims)
            g.matchFeatures(FLOW)
            g.debugFailAllocAfter(sk)
            expect(pkg, pkg.VH_ERR_HIP, lambda: g.reconstruct(step_trs(Trs, t)))
            got = g.reconstruct(step_trs(Trs, t))
            for s, pm in enumerate(lists_of(g)):
                want = d[s].chunk(t, [pm], [Trs[s][t - 1]])
                assert len(want) > 10 or t == 1
                same(got[s], want, (skip, t, s))
        g.close()


@pytest.mark.gpu
def test_group_child_checking_build(pkg, gpu):
    """The parity test once more on libviso_hip_check.so (-DVH_CHECK): every position the gather kernels follow is checked
    against the count of the slot of its own stream."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "equals_oracle_per_stream or wave_boundaries"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "3 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr
