"""Reads of memory nobody wrote.  The parity files hold every kernel to its restatement, but they run in one process: a
fresh allocation is zero or holds what the call before it left, which is usually the right answer.  With VH_POISON=1
(csrc/vh_poison.h) every device and page-locked buffer the library allocates starts as 0xA5 bytes, and the stateless
estimators' kept work buffer is filled again at every call, so a status word that was not stored, a count that was not
cleared or an output that a refusal skipped changes the bytes the parity tests compare.

CPU part: no allocation of csrc/ escapes the rule -- every call of an allocating HIP function lies in one of the
functions that poison what they allocate, or in the one exemption.  GPU part: one child process per row of ROWS, the
row's selection of a parity file on poisoned buffers; and the estimators' kept work buffer, a short batch behind a long
one, here and (through its own row) poisoned."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import egomotion_scene as es
from conftest import ROOT

CSRC = os.path.join(ROOT, "hls-final-visual-odometry_amd", "csrc")

# ---------------------------------------------------------------------------------------- CPU: every allocation site

ALLOCATORS = ("hipMalloc", "hipMallocAsync", "hipMallocManaged", "hipHostMalloc", "hipExtMallocWithFlags")
#: (file, enclosing function) -> the helper of vh_poison.h that function calls on what it allocated
POISONED_SITES = {
    ("engine.h", "HostBlock::alloc"): "vh_poison_host",        # page-locked buffers the host reads after kernels or copies wrote them
    ("engine.h", "DeviceBlock::alloc"): "vh_poison_device",    # the block of every stateless entry (StagedBlock), reconstruction, link_lists_device
    ("engine.h", "Group::dmalloc"): "vh_poison_device",        # a handle's arena
    ("engine_api.hip", "EgoWorkLease::take"): "vh_poison_device",  # the stateless estimators' work buffer, on every take
    ("vh_vote.h", "VhVoteBuffers::alloc"): "vh_poison_device",  # the device vote's carved block
}
#: the caller's own buffer: the library reads nothing from it that the caller did not put there
EXEMPT_SITES = {("engine_api.hip", "vh_host_alloc")}

_CONTROL = {"if", "for", "while", "switch", "catch", "return", "sizeof", "decltype", "alignas", "static_assert"}


def _blank(text):
    """text without comments, string and character literals, every other character (and every newline) in its place"""
    def spaces(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    return re.sub(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'", spaces, text, flags=re.S)


def _scopes(text):
    """-> [(kind, name, open, close)] for every brace pair: kind 'type' (struct / class / namespace ...), 'function' (a
    definition: a name, its parameters, a body) or 'other' (control statements, lambdas, initialisers)"""
    out, stack = [], []
    for m in re.finditer(r"[{}]", text):
        at = m.start()
        if text[at] == "}":
            if stack:
                kind, name, start = stack.pop()
                out.append((kind, name, start, at))
            continue
        head = text[max(text.rfind(";", 0, at), text.rfind("{", 0, at), text.rfind("}", 0, at)) + 1:at]
        head = re.sub(r"^\s*template\s*<[^{;]*?>\s*(?=(struct|class|union)\b)", "", head.strip())
        kind, name = "other", ""
        t = re.match(r"(?:struct|class|union|namespace|enum(?:\s+class)?)\b\s*(\w*)", head)
        f = re.search(r"([~\w:]+)\s*\(", head)
        if t:
            kind, name = "type", t.group(1)
        elif f and f.group(1) not in _CONTROL and not re.search(r"\[[^\]]*\]\s*(\([^)]*\))?\s*(mutable\s*)?(->[^{]*)?$", head) \
                and not re.search(r"=\s*$", head):
            kind, name = "function", f.group(1)
        stack.append((kind, name, at))
    return out


def allocation_sites(csrc):
    """-> [(file, qualified enclosing function, line, body of that function)] for every call of an ALLOCATORS function"""
    sites = []
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".h")):
            continue
        with open(os.path.join(csrc, fn)) as f:
            text = _blank(f.read())
        scopes = _scopes(text)
        for m in re.finditer(r"\b(%s)\s*\(" % "|".join(ALLOCATORS), text):
            around = sorted((s for s in scopes if s[2] < m.start() < s[3]), key=lambda s: s[2])   # outermost first
            funcs = [s for s in around if s[0] == "function"]
            if not funcs:
                sites.append((fn, "(file scope)", text.count("\n", 0, m.start()) + 1, ""))
                continue
            func = funcs[0]   # (the definition itself, not a local struct's member or a lambda inside it)
            owners = [s[1] for s in around if s[0] == "type" and s[1] and s[2] < func[2] and not s[1].startswith("vh_engine")]
            name = func[1] if "::" in func[1] else "::".join(owners + [func[1]])
            sites.append((fn, name, text.count("\n", 0, m.start()) + 1, text[func[2]:func[3]]))
    return sites


def unpoisoned_sites(csrc):
    """the allocation sites of csrc that escape the rule, as messages.

    The limit of the check: a site passes when its enclosing function is listed and that function's body calls the helper
    somewhere -- not when every allocating path reaches the call.  EgoWorkLease::take has two hipMalloc calls (the kept
    buffer, the one-off above 1 GiB) and two of vh_poison_device, and they are judged together; a path added to a listed
    function that skips the helper passes here and is for the review to see.  _scopes is no C++ parser either: it knows the
    brace heads csrc/ uses (definitions, types, control statements, lambdas, initialisers), test_the_scan_sees_a_bare_allocation
    holds it to them, and a site it cannot name shows up as "(file scope)" or under an unlisted name, which fails."""
    bad = []
    for fn, func, line, body in allocation_sites(csrc):
        helper = POISONED_SITES.get((fn, func))
        if (fn, func) in EXEMPT_SITES or (helper and re.search(r"\b%s\s*\(" % helper, body)):
            continue
        bad.append(f"{fn}:{line}: {func} allocates without the poison rule: allocate through DeviceBlock::alloc, Group::dmalloc or "
                   "HostBlock::alloc, or call vh_poison_device / vh_poison_host (csrc/vh_poison.h) on the fresh buffer and list the "
                   "function in POISONED_SITES")
    return bad


def test_no_allocation_site_escapes_the_poison_rule():
    found = {(fn, func) for fn, func, _, _ in allocation_sites(CSRC)}
    assert found >= set(POISONED_SITES) | EXEMPT_SITES, ("the scan lost a known site", sorted(found))
    bad = unpoisoned_sites(CSRC)
    assert not bad, "\n".join(bad)


def test_the_scan_sees_a_bare_allocation(tmp_path):
    """A unit with a bare hipMalloc in a free function, one inside a lambda of a member function and one in a comment: the
    first two are reported under their functions' names, the third is not a call."""
    (tmp_path / "engine_new.hip").write_text(
        "namespace vh_engine {\n"
        "// hipMalloc(&q, 1) in a comment\n"
        "static int32_t stage(void **q, size_t n) {\n  if (n) { VH_HIP(hipMalloc(q, n)); }\n  return 0;\n}\n"
        "struct Owner {\n  template <class T> hipError_t grow(size_t n) {\n"
        "    const auto a = [&](void **p) { return hipHostMalloc(p, n, 0); };\n    return a(&p_);\n  }\n  void *p_;\n};\n"
        "}\n")
    sites = [(fn, func, line) for fn, func, line, _ in allocation_sites(str(tmp_path))]
    assert sites == [("engine_new.hip", "stage", 4), ("engine_new.hip", "Owner::grow", 9)], sites
    bad = unpoisoned_sites(str(tmp_path))
    assert len(bad) == 2 and all("vh_poison_device" in b for b in bad)


# ------------------------------------------------------------------------- GPU: the estimators' kept work buffer

def _draws(seed, n_sets, iters, k):
    return np.random.default_rng(seed).integers(0, 2 ** 31 - 1, (n_sets, iters, k)).astype(np.int32)


def _estimates_equal_the_oracle(estimate, oracle_one, lists, raw, label):
    tr, ok, inl = estimate(lists, raw)
    for s, pm in enumerate(lists):
        ok_o, tr_o, inl_o = oracle_one(pm, raw[s])
        assert ok[s] == ok_o, (label, s, len(pm), ok[s], ok_o, len(inl[s]), len(inl_o))
        assert np.array_equal(inl[s], inl_o), (label, s, len(pm), len(inl[s]), len(inl_o))
        assert np.allclose(tr[s], tr_o, rtol=1e-9, atol=1e-12), (label, s, tr[s], tr_o)
        if not ok_o:
            assert tr[s].tobytes() == bytes(48), (label, s, tr[s])
    return ok


@pytest.mark.gpu
def test_gpu_kept_work_buffer_short_batch_behind_a_long_one(pkg, ob, oracle, gpu):
    """vh_estimate_motion_stereo and _mono keep one grow-only work buffer per device.  A long healthy batch, then a batch
    that is shorter, has fewer lists and holds an empty list and a too-short one (2 records stereo, 7 mono): every array of
    the second call lies inside what the first one filled with records, so a result the kernels do not store comes back as
    the first call's bytes -- or, on poisoned buffers (ROWS), as 0xA5.  ok, the inlier lists (n_inliers is their length)
    and tr of both calls equal the oracle, as in test_egomotion_edges.py and test_mono_edges.py."""
    D = ob.P_MATCH_DTYPE
    iters = 64
    e, ge = ob.EgoParams.default(**dict(es.KITTI, ransac_iters=iters)), pkg.EgoParams.default(**dict(es.KITTI, ransac_iters=iters))

    def stereo_oracle(pm, raw):
        samples = oracle.draw_samples(len(pm), iters, np.ascontiguousarray(raw).reshape(-1)) if len(pm) >= 6 else np.zeros((iters, 3), np.int32)
        return oracle.estimate_motion_stereo(e, pm, samples)

    def stereo(lists, raw):
        return pkg.estimate_motion_stereo(ge, lists, raw)

    long_lists = [es.scene(D, 400, 700 + s, outliers=0.2, noise=0.2)[0] for s in range(6)]
    healthy = es.scene(D, 150, 710, outliers=0.2, noise=0.2)[0]
    ok = _estimates_equal_the_oracle(stereo, stereo_oracle, long_lists, _draws(31, 6, iters, 3), "stereo, long")
    assert ok.all()
    short_lists = [healthy[:0], healthy[:2], healthy]
    ok = _estimates_equal_the_oracle(stereo, stereo_oracle, short_lists, _draws(32, 3, iters, 3), "stereo, short")
    assert list(ok) == [False, False, True]

    m, gm = ob.MonoParams.default(**dict(es.MONO_KITTI, ransac_iters=iters)), pkg.MonoParams.default(**dict(es.MONO_KITTI, ransac_iters=iters))

    def mono_oracle(pm, raw):
        samples = oracle.draw_samples_n(len(pm), 8, iters, np.ascontiguousarray(raw).reshape(-1)) if len(pm) >= 10 else np.zeros((iters, 8), np.int32)
        return oracle.estimate_motion_mono(m, pm, samples)

    def mono(lists, raw):
        return pkg.estimate_motion_mono(gm, lists, raw)

    long_lists = [es.mono_scene(D, 300, 720 + s, outliers=0.2, noise=0.2)[0] for s in range(5)]
    healthy = es.mono_scene(D, 120, 730, outliers=0.2, noise=0.2)[0]
    ok = _estimates_equal_the_oracle(mono, mono_oracle, long_lists, _draws(33, 5, iters, 8), "mono, long")
    assert ok.all()
    short_lists = [healthy[:0], healthy[:7], healthy]
    ok = _estimates_equal_the_oracle(mono, mono_oracle, short_lists, _draws(34, 3, iters, 8), "mono, short")
    assert list(ok) == [False, False, True]


# -------------------------------------------------------------------------- GPU: each feature's edges, poisoned

#: (test file, -k expression, tests the expression selects at least, marker expression).  An expression reaches every form
#: the feature has (stateless entry, group handle, sequence handle, inside the device post batch) and the file's cases where
#: an output is easiest to leave unwritten (empty, refused, ok = 0, degenerate and shortest lists, capacity overflow, the first
#: chunk of a carry, a shorter call behind a longer one); it leaves out the tests that start children of their own and the
#: KITTI-size, 1080p, 4K and long-list cases -- the smallest shapes already allocate every buffer.
#: A new output array gets a row here, or a case in a file that has one.
ROWS = [
    ("test_gpu_parity.py", "tiny_and_empty_inputs or capacity_errors or feature_capacity_overflow or bucket_features or failed_mask_allocation "
                           "or group_get_matches_all or group_async_download or dims_change or page_locked_host_images or small_default", 11, "gpu"),
    ("test_detect_tiles.py", "partial_edge_tiles or full_queues", 20, "gpu"),
    ("test_emit_paths.py", "lone_feature or fifteen_seventeen or empty_chunk_between or saturation or capacity or half_resolution", 8, "gpu"),
    ("test_match_tile_paths.py", "empty_class or partial_last_tile or second_searches", 4, "gpu"),
    ("test_match_snake_record.py", "tile_ends or two_streams_with_different or multi_stage_pair or sequence_rows", 4, "gpu"),
    ("test_multistage.py", "match_ranged or group_equals_lone_matchers or state_and_envelope", 3, "gpu"),
    ("test_multistage_device.py", "statistics_kernel or non_finite or plain or lone_matcher_in_device_mode or vote_refuses "
                                  "or failed_allocations or empty_frames", 10, "gpu"),
    ("test_multistage_prior.py", "group_and_sequence or switch_states", 2, "gpu"),
    ("test_sequence.py", "single_frame_chunks or dims_change_restarts or mode_mismatch or sequence_prior or post_chain", 5, "gpu"),
    ("test_sequence_multistage.py", "crosses_a_chunk_boundary or device_post_chain or unmatched_chunk or vote_refuses or allocation_failure", 6, "gpu"),
    ("test_device_bucketing.py", "bucketing_statuses or bucketing_capacity_boundary or grid_shrinks or single_bucket_occupancy", 7, "gpu"),
    ("test_outliers.py", "stereo_matches_are_not_voted or group_remove_outliers or flip_stack or refuses_what_it_cannot "
                         "or gpu_device_post_stage_matches or ring_discipline or leaves_stereo_lists_unvoted", 9, "gpu"),
    ("test_vote_rule.py", "sizes_lanes_and_bucketing or edges_and_refusals or group_votes_under or gpu_sequence_handle "
                          "or lone_matcher or multi_stage_votes", 11, "gpu"),
    ("test_egomotion_edges.py", "list_lengths or failure_paths or degenerate_geometry or residuals_of_exactly_zero or second_intrinsics "
                                "or batch_width or empty_and_tiny_streams", 7, "gpu"),
    ("test_mono_edges.py", "shortest_lists or lds_global_switch or degenerate_and_rejection or sampson", 4, "gpu"),
    ("test_motion_inliers.py", "not child", 10, "gpu"),
    ("test_mono_inliers.py", "not child", 13, "gpu"),
    ("test_motion_refit.py", "not child", 9, "gpu"),
    ("test_motion_cov.py", "not child", 10, "gpu"),
    ("test_gain.py", "not child", 14, "gpu"),
    ("test_mono_refit.py", "not child", 6, "gpu"),
    ("test_mono_pose.py", "not child", 7, "gpu"),
    ("test_mono_pose_refined.py", "not child", 6, "gpu"),
    ("test_scene_points.py", "not child", 9, "gpu"),
    ("test_landmarks.py", "not child", 5, "gpu"),
    ("test_sequence_landmarks.py", "not child", 4, "gpu"),
    ("test_trajectory.py", "not child", 8, "gpu"),
    ("test_post_dense.py", "not child", 8, "gpu"),
    ("test_post_tail.py", "not child", 12, "gpu"),
    ("test_group_recon.py", "not child", 11, "gpu"),
    ("test_reconstruction.py", "not child", 15, "gpu"),
    ("test_tracks.py", "not child", 14, "gpu"),
    ("test_packed_first_offset.py", "lists_behind_first_offset", 9, "gpu"),
    # (no test of this file carries the gpu marker -- its answers are the same with and without a device -- so its row selects
    # by name alone; the last test builds and runs a program of its own.  Its calls return before a device is selected, so the
    # row reaches no allocation at all: what it pins is that the refusals, and the answers the host settles alone -- counts
    # of empty lists written straight to the caller's arrays -- are the same with the variable set, no poisoned staging
    # buffer in between)
    ("test_stateless_validation.py", "not engine_lists_header_alone", 22, "not gpu"),
    ("test_poisoned_buffers.py", "kept_work_buffer", 1, "gpu"),
]
CHILD_TIMEOUT = 120  # s: the slowest row (test_device_bucketing) takes 6.9 s poisoned on an MI355X (profiles/EXPERIMENTS.md)

_crashed = []  # the rows whose child ended by a signal, an abort or its time limit: nothing more runs on the GPU behind one


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r[0][5:-3] for r in ROWS])
def test_child_on_poisoned_buffers(row, gpu):
    fn, expr, at_least, marker = row
    assert not _crashed, f"not run: an earlier poisoned child crashed ({_crashed[0]})"
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", fn), "-q", "-x", "-m", marker, "-k", expr]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, VH_POISON="1"), capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _crashed.append(fn)
        pytest.fail(f"{fn}: the poisoned child did not end in {CHILD_TIMEOUT} s\n{(e.stdout or b'')[-2000:]!r}")
    if r.returncode < 0 or r.returncode in (134, 139):
        _crashed.append(fn)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr, r.stderr[-2000:]
    ran = int(re.search(r"(\d+) passed", r.stdout).group(1))
    assert ran >= at_least, f"{fn} -k {expr!r} ran {ran} tests, the row states {at_least}: a renamed test left the selection"

