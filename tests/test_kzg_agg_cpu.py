"""KZG aggregate verification (plk_kzg_verify_agg_*) without a GPU: the two Python models of
tests/kzg_agg_model.py against every reference verdict in tests/golden/kzg_agg.json and against each other,
m = 1 with r = 1 against pairing.json's exhaustive bitmap, the host-only plan and workspace functions, and
the argument checks that come before any device query.  No CPU fallback: a well-formed call without a
device is PLK_ERR_NODEV."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gen
import kzg_agg_model as A
import make_kzg_agg_golden as mk
from conftest import ROOT, load_golden

REF_SRC = "/root/reference/src"
NEW = ("plk_kzg_verify_agg_plan", "plk_kzg_verify_agg_workspace", "plk_kzg_verify_agg_batch",
       "plk_kzg_verify_agg_batch_dev")
MAX_JOBS = 1 << 30


@pytest.fixture(scope="module")
def gold():
    return load_golden("kzg_agg.json")


def bits_of(case):
    return np.array([int(b) for b in case["bits"]], np.uint8)


def flat(case):
    d = mk.case_inputs(case["kind"], case["m"], case["seed"], case["groups"])
    assert d["vk"].tobytes().hex() == case["vk"]
    return mk.key_of(d["vk"]), d


def test_golden_file_is_small_and_complete(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kzg_agg.json")) < 100 * 1024
    shapes = sorted((c["kind"], c["m"]) for c in gold["cases"])
    assert shapes == sorted([("regular", m) for m in (1, 2, 3, 16, 17, 65)] + [("raw", m) for m in (1, 2, 5, 33)])
    for c in gold["cases"]:
        bits = bits_of(c)
        assert bits.size == c["groups"] and 0 < bits.sum() < bits.size, (c["kind"], c["m"])   # accepts and rejects mix


def test_golden_inputs_are_what_the_issue_asks(gold):
    """regular: every one of the 102 elements occurs; raw: mostly off the curve, about a quarter flagged"""
    seen = set()
    for c in gold["cases"]:
        _, d = flat(c)
        pts = np.concatenate([d["c"], d["w"]])
        on = (pts[:, 1].astype(int) ** 2 - pts[:, 0].astype(int) ** 3 - 3) % 101 == 0
        if c["kind"] == "regular":
            seen |= {tuple(p) for p in pts.tolist()}
            assert (A.logs_of(pts)[0] >= 0).all()
        else:
            assert on.mean() < 0.1 and 0.15 < pts[:, 2].mean() < 0.35
        assert max(d["z"].max(), d["y"].max(), d["r"].max()) == 16 or c["m"] == 1
    assert seen == {tuple(p) for p in gen.all_points().tolist()}


def test_raw_model_reproduces_every_bit(gold):
    for c in gold["cases"]:
        key, d = flat(c)
        got = A.agg_raw_flat(key, c["m"], d["c"], d["z"], d["y"], d["w"], d["r"])
        assert np.array_equal(got, bits_of(c)), (c["kind"], c["m"], np.flatnonzero(got != bits_of(c))[:8])


def test_log_model_reproduces_every_bit(gold):
    """the regular groups bit for bit; a raw group is undecided unless all its points happen to be canonical"""
    undecided = 0
    for c in gold["cases"]:
        key, d = flat(c)
        got = A.agg_log(key, c["m"], d["c"], d["z"], d["y"], d["w"], d["r"])
        exp = bits_of(c)
        if c["kind"] == "regular":
            assert np.array_equal(got, exp), (c["m"], np.flatnonzero(got != exp)[:8])
        else:
            dec = got != A.UNDECIDED
            assert np.array_equal(got[dec], exp[dec]) and got.max() <= A.UNDECIDED
            undecided += int((~dec).sum())
    assert undecided > 400


def test_log_model_equals_raw_model_on_the_regular_groups(gold):
    for c in gold["cases"]:
        if c["kind"] != "regular":
            continue
        key, d = flat(c)
        args = (key, c["m"], d["c"], d["z"], d["y"], d["w"], d["r"])
        assert np.array_equal(A.agg_log(*args), A.agg_raw_flat(*args)), c["m"]


def test_log_tables_are_the_group():
    exp, log = A.group_tables()
    assert sorted(exp) == sorted(tuple(p) for p in gen.all_points().tolist())
    assert exp[0] == (0, 0, 1) and exp[51] == (48, 0, 0)            # the identity and the 2-torsion point
    assert int((log >= 0).sum()) == 102
    for a in (1, 17, 50, 101):
        for b in (0, 1, 51, 85):
            assert A.M.g1_add(exp[a], exp[b]) == exp[(a + b) % 102]


def exhaustive():
    g = load_golden("pairing.json")
    bits = np.unpackbits(np.frombuffer(bytes.fromhex(g["verify_exhaustive"]["bits"]), np.uint8), bitorder="little")[:17 ** 4]
    kg = np.array(gen.KG, np.uint8)
    c, w, z, y = (v.reshape(-1) for v in np.meshgrid(*[np.arange(17)] * 4, indexing="ij"))
    vk = bytes.fromhex(g["verify_exhaustive"]["vk"])
    return mk.key_of(vk), kg[c], kg[w], z.astype(np.uint8), y.astype(np.uint8), bits


def test_m1_r1_is_the_per_opening_check():
    """all 17^4 exhaustive openings as groups of one under weight 1, through both models"""
    key, c, w, z, y, bits = exhaustive()
    ones = np.ones(z.size, np.uint8)
    assert np.array_equal(A.agg_log(key, 1, c, z, y, w, ones), bits)
    assert np.array_equal(A.agg_raw_flat(key, 1, c, z, y, w, ones), bits)


def test_models_mark_invalid_bytes_and_undecided_groups():
    vk = ((1, 2, 0), (36, 31), (90, 82))
    good = (gen.KG[5], gen.KG[3], 1, 2, 1)
    assert A.agg_raw(vk, [good]) == 1
    for col, val in ((0, (101, 2, 0)), (0, (1, 2, 2)), (1, (1, 255, 0)), (2, 17), (3, 17), (4, 17)):
        bad = list(good)
        bad[col] = val
        assert A.agg_raw(vk, [good, tuple(bad)]) == 2
        arr = lambda k: [j[k] for j in (good, tuple(bad))]   # noqa: E731
        assert A.agg_log(vk, 2, arr(0), arr(2), arr(3), arr(1), arr(4)).tolist() == [2]
    off = ((5, 5, 0), gen.KG[3], 1, 2, 1)       # valid, off the curve
    flagged = (gen.KG[5], (1, 2, 1), 1, 2, 1)   # valid, the flag with coordinates
    for j in (off, flagged):
        assert A.agg_log(vk, 1, [j[0]], [j[2]], [j[3]], [j[1]], [j[4]]).tolist() == [A.UNDECIDED]
        assert A.agg_raw(vk, [j]) in (0, 1)
    assert A.agg_log(((5, 5, 0), (36, 31), (90, 82)), 1, [good[0]], [1], [2], [good[1]], [1]).tolist() == [A.UNDECIDED]
    # a wrong y under weight 0 is not seen: the accept is a statement about the weighted sum
    wrong = (gen.KG[5], gen.KG[3], 1, 3, 0)
    assert A.agg_raw(vk, [good, wrong]) == 1 and A.agg_raw(vk, [good, wrong[:4] + (1,)]) == 0


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="reference sources not present")
def test_generator_reproduces_the_committed_file(gold):
    assert mk.generate(REF_SRC) == gold


# ------------------------------------------------------------------ plan and workspace: host only
def plan(h, m, n):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    rc = h.lib().plk_kzg_verify_agg_plan(m, n, out)
    return rc, list(out)


def test_exports_and_signatures():
    import plonkhip as h
    for name in NEW:
        assert name in h.SIGNATURES and hasattr(h.lib(), name), name
    for name in ("kzg_verify_agg", "kzg_verify_agg_dev", "kzg_verify_agg_workspace", "kzg_verify_agg_plan"):
        assert hasattr(h, name), name
    assert h.PLK_KZG_AGG_UNDECIDED == 3 == A.UNDECIDED


def test_plan_and_workspace_need_no_device_and_agree():
    import plonkhip as h
    ms = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 16384, 16385, 32768, 32769,
          1 << 20, (1 << 20) + 1, 1 << 24, 1 << 30]
    paths = set()
    for m in ms:
        for n in (1, 2, 257, 1 << 20):
            if m * n > MAX_JOBS:
                continue
            p, ws = h.kzg_verify_agg_plan(m, n), h.kzg_verify_agg_workspace(m, n)
            paths.add(p["path"])
            assert p["path"] in (0, 1, 2) and p["launches"] in (1, 2) and 1 <= p["blocks"] <= 1 << 13, (m, n, p)
            assert (ws == 0) == (p["launches"] == 1) == (p["path"] == 0), (m, n, p, ws)
            assert ws == 16 * p["slices"] * n
            if p["path"] == 1:
                assert p["slices"] == 1
            if p["path"] == 2:
                assert 1 <= p["slices"] <= 1024 and p["slices"] * 16 <= m   # every slice can be a multiple of 16 jobs
    assert paths == {0, 1, 2}


def test_plan_and_workspace_are_monotone():
    """for fixed n the path, the slices and the workspace never fall as m grows; for fixed m the workspace and
    the blocks never fall as n grows and the path and slices do not depend on n at all"""
    import plonkhip as h
    ms = sorted(set([1, 16, 32, 33, 64, 2048, 2049, 5000, 16384, 16385, 40000, 1 << 17, 1 << 20, 1 << 24] +
                    list(range(1, 80))))
    ns = [1, 2, 3, 64, 257, 1 << 10, 1 << 12, 1 << 16]
    for n in ns:
        prev = None
        for m in ms:
            if m * n > MAX_JOBS:
                continue
            p = h.kzg_verify_agg_plan(m, n)
            cur = (p["path"], p["slices"], h.kzg_verify_agg_workspace(m, n))
            assert prev is None or all(a <= b for a, b in zip(prev, cur)), (m, n, prev, cur)
            prev = cur
    for m in ms:
        prev = None
        for n in ns:
            if m * n > MAX_JOBS:
                continue
            p = h.kzg_verify_agg_plan(m, n)
            assert prev is None or (prev[0], prev[1]) == (p["path"], p["slices"])
            assert prev is None or (prev[2] <= p["blocks"] and prev[3] <= h.kzg_verify_agg_workspace(m, n))
            prev = (p["path"], p["slices"], p["blocks"], h.kzg_verify_agg_workspace(m, n))


def test_plan_and_workspace_bad_arguments():
    import plonkhip as h
    for m, n in ((0, 1), (1, 0), (0, 0)):
        assert plan(h, m, n)[0] == h.PLK_ERR_ARG and h.kzg_verify_agg_workspace(m, n) == 0
    for m, n in (((1 << 30) + 1, 1), (1, (1 << 30) + 1), (1 << 15, (1 << 15) + 1), (1 << 40, 1 << 40), (3, 1 << 63)):
        assert plan(h, m, n) == (h.PLK_ERR_RANGE, [-1] * 4) and h.kzg_verify_agg_workspace(m, n) == 0
    assert "2^30" in h.last_error()
    assert h.lib().plk_kzg_verify_agg_plan(1, 1, None) == h.PLK_ERR_ARG
    assert plan(h, 1 << 30, 1)[0] == h.PLK_OK and plan(h, 1 << 15, 1 << 15)[0] == h.PLK_OK
    assert h.kzg_verify_agg_workspace(1 << 15, 1 << 15) == 16 * 2 * (1 << 15)


# ------------------------------------------------------------------ the entry points' checks
def _bufs(e=4):
    """host blocks a failing call never reads (their addresses also stand in for device pointers)"""
    b = {k: (C.c_uint8 * (s * e))() for k, s in (("c", 3), ("w", 3), ("z", 1), ("y", 1), ("r", 1), ("ok", 1), ("work", 64))}
    for i in range(e):
        b["c"][3 * i], b["c"][3 * i + 1] = 1, 2
        b["w"][3 * i], b["w"][3 * i + 1] = 1, 2
        b["r"][i] = 1
    return b


def _addr(x):
    return None if x is None else C.addressof(x)


def _call(h, vk, b, m, n, dev, drop=None):
    a = {k: (None if drop == k else b[k]) for k in b}
    v = None if vk is None else C.byref(vk)
    if dev:
        return h.lib().plk_kzg_verify_agg_batch_dev(v, m, _addr(a["c"]), _addr(a["z"]), _addr(a["y"]), _addr(a["w"]),
                                                    _addr(a["r"]), n, _addr(a["ok"]), _addr(a["work"]), None)
    return h.lib().plk_kzg_verify_agg_batch(v, m, a["c"], a["z"], a["y"], a["w"], a["r"], n, a["ok"])


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_arg_errors_come_before_any_device_query(dev):
    import plonkhip as h
    b = _bufs()
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    for drop in ("c", "z", "y", "w", "r", "ok"):
        assert _call(h, vk, b, 2, 2, dev, drop) == h.PLK_ERR_ARG, drop
    assert "plk_kzg_verify_agg_batch" in h.last_error()
    assert _call(h, None, b, 2, 2, dev) == h.PLK_ERR_ARG
    assert _call(h, vk, b, 0, 2, dev) == h.PLK_ERR_ARG
    assert _call(h, vk, b, 2, 0, dev) == h.PLK_ERR_ARG
    if dev:   # the workspace is an argument only where the plan has a second launch
        assert h.kzg_verify_agg_workspace(64, 1) > 0
        assert _call(h, vk, b, 64, 1, True, "work") == h.PLK_ERR_ARG
        assert "d_work" in h.last_error()
        assert h.lib().plk_kzg_verify_agg_batch_dev(C.byref(vk), 64, _addr(b["c"]), _addr(b["z"]), _addr(b["y"]),
                                                    _addr(b["w"]), _addr(b["r"]), 1, _addr(b["ok"]),
                                                    _addr(b["work"]) + 2, None) == h.PLK_ERR_ARG


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("field,index,value", [("g1", 0, 101), ("g1", 1, 255), ("g1", 2, 2), ("g2_1", 0, 101),
                                               ("g2_1", 1, 200), ("g2_s", 0, 255), ("g2_s", 1, 101)])
def test_invalid_vk_byte_is_arg_error(dev, field, index, value):
    import plonkhip as h
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    getattr(vk, field)[index] = value
    assert _call(h, vk, _bufs(), 2, 2, dev) == h.PLK_ERR_ARG
    assert "verification key" in h.last_error()
    assert _call(h, vk, _bufs(), (1 << 30) + 1, 1, dev) == h.PLK_ERR_ARG   # a bad key before the range


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_more_than_2_30_jobs_is_range_error(dev):
    import plonkhip as h
    b = _bufs()
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    for m, n in (((1 << 30) + 1, 1), (1, (1 << 30) + 1), (1 << 15, (1 << 15) + 1), (1 << 40, 1 << 40), (3, 1 << 63)):
        assert _call(h, vk, b, m, n, dev) == h.PLK_ERR_RANGE, (m, n)
    assert "2^30" in h.last_error()


_NODEV_CHILD = r"""
import sys
sys.path[:0] = %r
import test_kzg_agg_cpu as t
import plonkhip as h
assert h.device_count() == 0, "the device is still visible"
print("codes", *t.valid_call_codes(h))
"""


def valid_call_codes(h):
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    return [_call(h, vk, _bufs(), 2, 2, dev) for dev in (False, True)] + [_call(h, vk, _bufs(64), 64, 1, dev) for dev in (False, True)]


def test_well_formed_call_without_gpu_is_nodev():
    """in this process when it has no device; otherwise in one child process that hides it"""
    import plonkhip as h
    if h.device_count() == 0:
        codes = valid_call_codes(h)
    else:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        paths = [os.path.dirname(os.path.abspath(__file__))] + [p for p in sys.path if p.startswith(ROOT)]
        out = subprocess.run([sys.executable, "-c", _NODEV_CHILD % (paths,)], env=env, capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        codes = [int(v) for v in out.stdout.split("codes", 1)[1].split()]
    assert codes == [h.PLK_ERR_NODEV] * 4
    if h.device_count() == 0:
        with pytest.raises(h.PlonkHipError) as e:
            h.kzg_verify_agg(vk=h.KzgVk((1, 2, 0), (36, 31), (90, 82)), m=1, commits=[1, 2, 0], zs=[1], ys=[1],
                             proofs=[1, 2, 0], rs=[1])
        assert e.value.code == h.PLK_ERR_NODEV
