"""Segmented MSM (plk_msm_g1_segments*) without a GPU: the Python model of tests/msm_segments_model.py against every
reference output in tests/golden/msm_segments.json, the host-only plan and workspace functions, and the argument
checks that come before any device query.  No CPU fallback: a well-formed call without a device is PLK_ERR_NODEV."""
import ctypes as C
import os

import numpy as np
import pytest

import g1_encoding_cases as E
import gen
import make_msm_segments_golden as mk
import msm_segments_model as S
from conftest import ROOT, load_golden

REF_SRC = "/root/reference/src"
NEW = ("plk_msm_g1_segments_plan", "plk_msm_g1_segments_workspace", "plk_msm_g1_segments_dev", "plk_msm_g1_segments")
LANE, PREFIX = 0, 1


@pytest.fixture(scope="module")
def gold():
    return load_golden("msm_segments.json")


def rows(entry):
    return np.frombuffer(bytes.fromhex(entry["out3"]), np.uint8).reshape(-1, 3)


# ------------------------------------------------------------------ the golden file and the model
def test_golden_file_is_small_and_what_the_issue_asks(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "msm_segments.json")) < 300 * 1024
    assert sorted(gold["lists"]) == ["irregular", "random"]
    pts, sc, off = mk.list_inputs("random")
    lens = np.diff(off.astype(np.int64))
    assert 200 <= lens.size == gold["lists"]["random"]["segments"] and lens.min() == 0 and lens.max() == 300
    assert int(off[-1]) == gold["lists"]["random"]["total"] == sc.size
    assert {tuple(p) for p in pts.tolist()} == {tuple(p) for p in gen.all_points().tolist()}
    assert len(set(sc.tolist())) == 256
    pts, sc, off = mk.list_inputs("irregular")
    cands = mk.irregular_candidates()
    assert len(cands) >= 50 and off.size - 1 == 3 * len(cands) == gold["lists"]["irregular"]["segments"]
    assert cands[:, 2].max() == 1 and cands[:, :2].max() >= 101 and not E.canonical_mask(cands).any()
    for i, c in enumerate(cands):       # first, middle and last position of three segments of its own
        a = off[3 * i:3 * i + 4].astype(np.int64)
        for pos in (a[0], a[1] + (a[2] - a[1]) // 2, a[3] - 1):
            assert tuple(pts[pos]) == tuple(c) and sc[pos] != 0
    bad = ~E.canonical_mask(pts)
    assert int(bad.sum()) == 3 * len(cands)


@pytest.mark.parametrize("kind", ["random", "irregular"])
def test_model_reproduces_every_golden_entry(gold, kind):
    pts, sc, off = mk.list_inputs(kind)
    exp = rows(gold["lists"][kind])
    got = S.segments_host(pts, sc, off)
    assert np.array_equal(got, exp), np.flatnonzero((got != exp).any(1))[:8]
    dev = S.segments_dev(pts, sc, off)
    if kind == "random":                # canonical inputs: the log-domain form is the fold, status 0
        assert np.array_equal(dev[:, :3], exp) and not dev[:, 3].any()
        assert len({tuple(r) for r in exp.tolist()}) > 90
    else:                               # every segment holds its planted encoding
        assert (dev == (0xFF, 0xFF, 0xFF, S.IRREGULAR)).all()
        assert len({tuple(r) for r in exp.tolist()}) > 50


def test_byte_level_fold_agrees_with_pairing_model_on_valid_encodings():
    """the two restatements of g1_add / g1_mul the model folds with are the same function where both apply"""
    r = gen.splitmix64(0x5E99, 4 * 3000)
    for i in range(3000):
        a = (int(r[4 * i] % 101), int(r[4 * i + 1] % 101), int(r[4 * i + 2] % 4 == 0))
        b = (int(r[4 * i + 1] % 101), int(r[4 * i + 3] % 101), int(r[4 * i + 2] % 8 == 1))
        k = int(r[4 * i + 3] >> 8) % 256
        assert E.py_add(a, b) == S.M.g1_add(a, b) and S._byte_mul(a, k) == S.M.g1_mul(a, k), (a, b, k)


def test_model_statuses_and_clamping():
    pts, sc = E.fillers(E.rng_for("msm_segments/statuses"), 40)
    pts[10] = (5, 5, 0)                                  # off the curve
    off = [0, 10, 11, 11, 40, 30, 45, 40]                # ends at the bad point, holds it, empty, falls, above total
    d = S.segments_dev(pts, sc, off)
    assert d[:, 3].tolist() == [0, 1, 0, 0, 2, 2, 2]
    assert tuple(d[2]) == (0, 0, 1, 0)                   # an empty segment is the identity
    assert np.array_equal(d[0, :3], S.segments_host(pts, sc, [0, 10])[0])
    assert np.array_equal(d[3, :3], S.segments_host(pts, sc, [11, 40])[0])
    u = S.segments_dev(pts, sc, m=8)
    assert u[:, 3].tolist() == [0, 1, 0, 0, 0]
    assert np.array_equal(u[[0, 2, 3, 4], :3], S.segments_host(pts, sc, m=8)[[0, 2, 3, 4]])


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="reference sources not present")
def test_generator_reproduces_the_committed_file(gold):
    assert mk.generate(REF_SRC) == gold


# ------------------------------------------------------------------ plan and workspace: host only
def plan(h, total, m, nseg, ragged):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    rc = h.lib().plk_msm_g1_segments_plan(total, m, nseg, ragged, out)
    return rc, list(out)


def test_exports_and_wrappers():
    import plonkhip as h
    for name in NEW:
        assert name in h.SIGNATURES and hasattr(h.lib(), name), name
    for name in ("msm_g1_segments_plan", "msm_g1_segments_workspace", "msm_g1_segments_dev", "msm_g1_segments"):
        assert hasattr(h, name), name
    assert (h.PLK_MSM_SEG_IRREGULAR, h.PLK_MSM_SEG_BAD) == (1, 2) == (S.IRREGULAR, S.BAD)


def test_plan_and_workspace_are_pure_and_agree():
    import plonkhip as h
    shapes = [(m * n, m, n, 0) for m in (1, 2, 9, 16, 17, 31, 32, 33, 64, 4095, 4096, 4097, 1 << 18) for n in (1, 3, 65, 1000)]
    shapes += [(t, 0, n, 1) for t in (1, 15, 16, 17, 4095, 4096, 4097, 12325, 1 << 24, (1 << 32) - 1) for n in (1, 7, 1 << 20)]
    shapes += [(t, 77, n, 1) for t in (5, 4096) for n in (1, 9)]          # m is ignored with offsets
    paths = set()
    for total, m, nseg, ragged in shapes:
        p, ws = h.msm_g1_segments_plan(total, m, nseg, ragged), h.msm_g1_segments_workspace(total, m, nseg, ragged)
        assert p == h.msm_g1_segments_plan(total, m, nseg, ragged) and ws == h.msm_g1_segments_workspace(total, m, nseg, ragged)
        lane = not ragged and m <= 32
        assert p["path"] == (LANE if lane else PREFIX), (total, m, nseg, ragged, p)
        assert (ws == 0) == (p["launches"] == 1) == lane
        assert p["launches"] in (1, 3) and p["blocks"] >= 1 and p["tile"] >= 1
        if not lane:
            t = p["tile"]
            assert t % 16 == 0 and p["blocks"] == -(-(total // 16 + 1) // (t // 16))
            assert ws == 8 * p["blocks"] + 4 * (total // 16 + 1) and ws % 4 == 0
        if ragged:
            assert p == h.msm_g1_segments_plan(total, 123, nseg, ragged)
        paths.add(p["path"])
    assert paths == {LANE, PREFIX}


def test_plan_and_workspace_bad_arguments():
    import plonkhip as h
    arg = [(0, 1, 1, 0), (4, 2, 0, 0), (4, 0, 4, 0), (5, 2, 2, 0), (4, 2, 3, 0), (0, 0, 1, 1), (4, 0, 0, 1), (1 << 40, 3, 5, 0)]
    for a in arg:
        assert plan(h, *a) == (h.PLK_ERR_ARG, [-1] * 4) and h.msm_g1_segments_workspace(*a) == 0, a
    rng = [(1 << 32, 1, 1 << 32, 0), (1 << 32, 1 << 32, 1, 0), (1 << 32, 0, 5, 1), (1 << 40, 0, 1, 1), (8, 0, (1 << 30) + 1, 1),
           ((1 << 30) + 1, 1, (1 << 30) + 1, 0)]
    for a in rng:
        assert plan(h, *a) == (h.PLK_ERR_RANGE, [-1] * 4) and h.msm_g1_segments_workspace(*a) == 0, a
    assert "2^32" in h.last_error()
    assert h.lib().plk_msm_g1_segments_plan(4, 2, 2, 0, None) == h.PLK_ERR_ARG
    assert plan(h, (1 << 32) - 1, 0, 1 << 30, 1)[0] == h.PLK_OK and plan(h, 1 << 30, 1, 1 << 30, 0)[0] == h.PLK_OK


# ------------------------------------------------------------------ the entry points' checks
def _bufs(total=8, nseg=2):
    """host blocks (their addresses also stand in for device pointers in calls that fail before any device query)"""
    b = {"p": (C.c_uint8 * (3 * total))(), "s": (C.c_uint8 * total)(), "o": (C.c_uint32 * (nseg + 1))(),
         "out": (C.c_uint8 * (4 * nseg))(), "work": (C.c_uint32 * 64)()}
    for i in range(total):
        b["p"][3 * i], b["p"][3 * i + 1] = 1, 2
    for g in range(nseg + 1):
        b["o"][g] = min(total, g * (total // nseg))
    return b


def _addr(x):
    return None if x is None else C.addressof(x)


def _dev(h, b, total, m, nseg, ragged, drop=None, work_shift=0):
    a = {k: (None if k == drop else v) for k, v in b.items()}
    w = None if a["work"] is None else _addr(a["work"]) + work_shift
    return h.lib().plk_msm_g1_segments_dev(_addr(a["p"]), _addr(a["s"]), total, _addr(a["o"]) if ragged else None, m, nseg,
                                           _addr(a["out"]), w, None)


def _host(h, b, total, m, nseg, ragged, drop=None):
    a = {k: (None if k == drop else v) for k, v in b.items()}
    return h.lib().plk_msm_g1_segments(a["p"], a["s"], total, a["o"] if ragged else None, m, nseg, a["out"])


@pytest.mark.parametrize("form", ["host", "dev"])
def test_arg_and_range_errors_come_before_any_device_query(form):
    import plonkhip as h
    call = _dev if form == "dev" else _host
    b = _bufs()
    for ragged in (0, 1):
        for drop in ("p", "s", "out"):
            assert call(h, b, 8, 4, 2, ragged, drop) == h.PLK_ERR_ARG, (ragged, drop)
        assert "plk_msm_g1_segments" in h.last_error()
        assert call(h, b, 8, 4, 0, ragged) == h.PLK_ERR_ARG        # nseg == 0
        assert call(h, b, 0, 4, 2, ragged) == h.PLK_ERR_ARG        # total == 0
        assert call(h, b, 1 << 32, 1 << 31, 2, ragged) == h.PLK_ERR_RANGE
        assert call(h, b, 1 << 33, 2, 1 << 32, ragged) == h.PLK_ERR_RANGE
    assert call(h, b, 8, 0, 2, 0) == h.PLK_ERR_ARG                 # uniform: m == 0
    assert call(h, b, 8, 3, 2, 0) == h.PLK_ERR_ARG                 # uniform: m nseg != total
    assert call(h, b, 8, 4, 3, 0) == h.PLK_ERR_ARG
    assert call(h, b, 8, 0, (1 << 30) + 1, 1) == h.PLK_ERR_RANGE   # ragged: nseg > 2^30 (the offsets are not read)
    if form == "dev":   # the workspace is an argument only where the plan has more than one launch
        assert h.msm_g1_segments_workspace(8, 0, 2, 1) > 0 and h.msm_g1_segments_workspace(66, 33, 2, 0) > 0
        assert _dev(h, b, 8, 0, 2, 1, "work") == h.PLK_ERR_ARG and "d_work" in h.last_error()
        assert _dev(h, b, 8, 0, 2, 1, work_shift=2) == h.PLK_ERR_ARG
        assert _dev(h, _bufs(66), 66, 33, 2, 0, "work") == h.PLK_ERR_ARG


def test_host_form_validates_the_offsets_before_any_device_query():
    import plonkhip as h
    for bad in ([0, 5, 4], [3, 2, 8], [0, 4, 9], [9, 9, 9], [0, 1 << 31, 8]):
        b = _bufs()
        for g, v in enumerate(bad):
            b["o"][g] = v
        assert _host(h, b, 8, 0, 2, 1) == h.PLK_ERR_ARG, bad
        assert "offsets" in h.last_error()
    with pytest.raises(h.PlonkHipError) as e:
        h.msm_g1_segments(np.zeros((8, 3), np.uint8), np.zeros(8, np.uint8), offsets=[0, 6, 5])
    assert e.value.code == h.PLK_ERR_ARG


def test_well_formed_call_without_gpu_is_nodev():
    """(where this process sees no device; on a GPU machine the GPU tests make the well-formed calls)"""
    import plonkhip as h
    if h.device_count() == 0:
        for ragged in (0, 1):
            assert _host(h, _bufs(), 8, 4, 2, ragged) == h.PLK_ERR_NODEV
            assert _dev(h, _bufs(), 8, 4, 2, ragged) == h.PLK_ERR_NODEV
