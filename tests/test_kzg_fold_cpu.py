"""KZG folded openings (plk_kzg_open_fold_batch*, plk_kzg_verify_fold_batch*, plk_kzg_fold_workspace)
without a GPU: the Python model of tests/kzg_fold_model.py against every reference output in
tests/golden/kzg_fold.json, the generator's determinism, the exports, the host-only workspace size and
the argument checks that come before any device query.  No CPU fallback: a valid call without a
device is PLK_ERR_NODEV."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kzg_fold_model as F
import pairing_model as M
from conftest import ROOT, load_golden

REF_SRC = "/root/reference/src"
NEW = ("plk_kzg_fold_workspace", "plk_kzg_open_fold_batch", "plk_kzg_open_fold_batch_dev",
       "plk_kzg_verify_fold_batch", "plk_kzg_verify_fold_batch_dev")


@pytest.fixture(scope="module")
def gold():
    """the committed record, and it joined with its inputs (rebuilt from the recorded seeds)"""
    import make_kzg_fold_golden as mk
    raw = load_golden("kzg_fold.json")
    return (raw,) + mk.expand(raw)


def unhex(s):
    return list(bytes.fromhex(s))


def key_of(b):
    b = tuple(b)
    return (b[0:3], b[3:5], b[5:7])


def split_job(row, k):
    """(vk, commits, weights, ys, z, proof) of one recorded verification job"""
    row = [int(v) for v in row]
    ent = [row[7 + 5 * i:12 + 5 * i] for i in range(k)]
    return (key_of(row[:7]), [tuple(e[:3]) for e in ent], [e[3] for e in ent], [e[4] for e in ent], row[-1],
            tuple(row[7 + 5 * k:10 + 5 * k]))


# ------------------------------------------------------------------ the golden file and the model
def test_golden_file_is_small_and_complete(gold):
    import gen
    raw, groups, verify, cases = gold
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kzg_fold.json")) < 64 * 1024
    assert len(groups) >= 200 and {len(g["polys"]) for g in groups} == set(range(1, 17))
    assert any(set(g["weights"]) == {0} for g in groups)
    assert any(0 in g["weights"] and any(g["weights"]) for g in groups)
    assert max(len(p) for g in groups for p in g["polys"]) >= 38
    assert any(len(g["polys"]) > 1 and len(g["polys"][0]) < max(len(p) for p in g["polys"]) for g in groups)
    assert sorted(verify) == [1, 2, 3, 9, 16] and sum(len(b) for _, b in verify.values()) >= 2048
    srs = np.array(unhex(raw["srs"]), np.uint8).reshape(-1, 3)
    assert [tuple(p) for p in srs.tolist()] == [gen.KG[pow(2, i, 17)] for i in range(len(srs))]
    assert unhex(raw["key"]) == [1, 2, 0, 36, 31, 90, 82] and len(cases) >= 32


def test_model_reproduces_every_opening(gold):
    raw, groups, _, _ = gold
    srs = np.array(unhex(raw["srs"]), np.uint8).reshape(-1, 3)
    cancelled = 0
    for i, g in enumerate(groups):
        ys, Fb, proof = F.open_fold(srs, g["polys"], g["weights"], g["z"])
        assert ys == g["ys"], i
        assert F.trim(Fb).tolist() == g["F"], i                    # the reference's poly_add trims
        assert proof == g["proof"], i
        cancelled += len(g["F"]) < max(len(p) for p in g["polys"])
    assert cancelled >= 20                                         # zero weights and cancelling pairs


@pytest.mark.parametrize("k", [1, 2, 3, 9, 16])
def test_model_reproduces_every_verification(gold, k):
    raw, _, verify, _ = gold
    rows, bits = verify[k]
    assert 0 < bits.sum() < len(bits)
    flagged = sum(int(r[7 + 5 * i + 2]) for r in rows for i in range(k))
    assert flagged > 0.08 * len(rows) * k                          # a quarter of the random encodings
    own = sum(tuple(r[:7]) != tuple(unhex(raw["key"])) for r in rows.tolist())
    assert own >= len(rows) // 5                                   # jobs carrying their own key
    for i, r in enumerate(rows):
        vk, cs, ws, ys, z, w = split_job(r, k)
        assert F.verify_fold(vk, cs, ws, ys, z, w) == bits[i], (k, i, r.tolist())


def test_model_reproduces_end_to_end_cases(gold):
    raw, _, _, cases = gold
    srs = np.array(unhex(raw["srs"]), np.uint8).reshape(-1, 3)
    vk = key_of(unhex(raw["key"]))
    seen = set()
    for n, c in enumerate(cases):
        assert c["commits"] == [F.msm(srs[:len(F.trim(p))], F.trim(p)) for p in c["polys"]], n
        ys, _, proof = F.open_fold(srs, c["polys"], c["weights"], c["z"])
        assert ys == c["ys"] and proof == c["proof"], n
        got = [F.verify_fold(vk, c["commits"], w, y, c["z"], p) for w, y, p in c["variants"]]
        assert "".join(str(b) for b in got) == c["bits"], n
        assert c["bits"][0] == "1", n                              # every honest group is accepted
        seen.add(c["bits"])
    assert len(seen) > 1 and any(b[1:] == "000" for b in seen)


def test_model_marks_invalid_bytes():
    vk = ((1, 2, 0), (36, 31), (90, 82))
    g = (1, 2, 0)
    assert F.verify_fold(vk, [g, g], [1, 1], [0, 0], 0, g) in (0, 1)
    for cs, ws, ys, z, w in (([g, (101, 2, 0)], [1, 1], [0, 0], 0, g), ([g, (1, 2, 2)], [1, 1], [0, 0], 0, g),
                             ([g, g], [1, 17], [0, 0], 0, g), ([g, g], [1, 1], [17, 0], 0, g),
                             ([g, g], [1, 1], [0, 0], 17, g), ([g, g], [1, 1], [0, 0], 0, (1, 255, 0))):
        assert F.verify_fold(vk, cs, ws, ys, z, w) == 2
    # the fold applies the raw formulas blindly: a flagged C with coordinates survives w = 1 byte for
    # byte (g1_add hands back its other operand) and becomes the canonical identity under w = 3
    assert F.fold_commitments([(5, 7, 1)], [1]) == (5, 7, 1)
    assert F.fold_commitments([(5, 7, 1)], [3]) == M.IDENTITY


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="reference sources not present")
def test_generator_reproduces_the_committed_file(gold):
    import make_kzg_fold_golden as mk
    assert mk.generate(REF_SRC) == gold[0]


# ------------------------------------------------------------------ exports and the workspace size
def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("kzg_fold_workspace", "kzg_open_fold", "kzg_open_fold_dev", "kzg_verify_fold", "kzg_verify_fold_dev"):
        assert hasattr(h, name), name
    with open(os.path.join(ROOT, "include", "plonkhip.h")) as f:
        assert "#define PLK_KZG_FOLD_MAX 16" in f.read()


def test_workspace_is_host_only_and_monotone():
    import plonkhip as h
    lib = h.lib()
    ws = h.kzg_fold_workspace
    assert ws([], [0]) == 0
    assert lib.plk_kzg_fold_workspace(None, (C.c_int * 2)(0, 1), 1) == 0
    assert lib.plk_kzg_fold_workspace((C.c_size_t * 1)(5), None, 1) == 0
    assert ws([5, 5], [0, 2, 2]) == 0 and ws([5, 5], [1, 2]) == 0 and ws([5, 5], [0, 2, 1]) == 0
    assert ws([5] * 17, [0, 17]) == 0                              # a group of more than 16
    assert ws([5] * 16, [0, 16]) > 0
    one = ws([4096], [0, 1])
    assert one > 0 and one % 256 == 0
    sizes = [ws([n] * 9, [0, 9]) for n in (1, 4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 22)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1]
    # one word per (polynomial, chunk) and one folded word per (group, chunk)
    assert sizes[3] >= 4 * 10 * ((1 << 20) // 4096) and sizes[5] >= 4 * 10 * ((1 << 22) // 4096)
    assert ws([1 << 20] * 9, [0, 9]) <= ws([1 << 20] * 9, [0, 4, 9])   # a second group adds its folded words
    assert ws([1 << 20, 1 << 21], [0, 2]) < ws([1 << 21, 1 << 21], [0, 2])
    grow = [ws([1 << 16] * k, [0, k]) for k in range(1, 17)]
    assert grow == sorted(grow) and grow[-1] > grow[0]


# ------------------------------------------------------------------ argument checks, no device
def _opaque_handle():
    """a non-NULL handle the calls under test must never look into: their argument checks return first"""
    return (C.c_uint8 * 256)()


class OpenArgs:
    """ctypes blocks of two groups (2 + 3 polynomials) that a failing call never reads"""

    def __init__(self, counts=(2, 3), length=4):
        n = sum(counts)
        self.bufs = [(C.c_uint8 * length)() for _ in range(n)]
        self.ptrs = (C.POINTER(C.c_uint8) * n)(*[C.cast(b, C.POINTER(C.c_uint8)) for b in self.bufs])
        self.vptrs = (C.c_void_p * n)(*[C.addressof(b) for b in self.bufs])
        self.lens = (C.c_size_t * n)(*[length] * n)
        self.weights = (C.c_uint8 * n)(*[1] * n)
        start = [0]
        for k in counts:
            start.append(start[-1] + k)
        self.start = (C.c_int * len(start))(*start)
        self.zs = (C.c_uint8 * len(counts))(*[3] * len(counts))
        self.ng = len(counts)
        self.ys = (C.c_uint8 * n)()
        self.out = (C.c_uint8 * (3 * len(counts)))()
        self.res = (C.c_uint8 * (2176 * len(counts)))()

    def call(self, h, s, dev, drop=None, ng=None):
        a = {k: (None if drop == k else getattr(self, k)) for k in ("lens", "weights", "start", "zs", "ys", "out", "res")}
        ng = self.ng if ng is None else ng
        if dev:
            polys = None if drop == "polys" else self.vptrs
            res = None if a["res"] is None else C.addressof(a["res"])
            ys = None if a["ys"] is None else C.addressof(a["ys"])
            return h.lib().plk_kzg_open_fold_batch_dev(s, polys, a["lens"], a["weights"], a["start"], a["zs"], ng, ys, res,
                                                       None, None, None)
        polys = None if drop == "polys" else self.ptrs
        return h.lib().plk_kzg_open_fold_batch(s, polys, a["lens"], a["weights"], a["start"], a["zs"], ng, a["ys"], a["out"])


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_open_null_handle_is_arg_error(dev):
    import plonkhip as h
    assert OpenArgs().call(h, None, dev) == h.PLK_ERR_ARG
    assert "plk_kzg_open_fold_batch" in h.last_error()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("case", ["ngroups0", "ngroups_negative", "null_polys", "null_lens", "null_weights", "null_start",
                                  "null_zs", "null_ys", "null_out", "start_not_from_0", "start_flat", "start_falls",
                                  "group_of_17", "len0", "weight17", "weight255", "z17"])
def test_open_arg_errors_come_before_any_device_query(case, dev):
    import plonkhip as h
    fake = _opaque_handle()
    s = C.addressof(fake)
    a = OpenArgs((17,)) if case == "group_of_17" else OpenArgs()
    drop, ng = None, None
    if case == "ngroups0":
        ng = 0
    elif case == "ngroups_negative":
        ng = -2
    elif case.startswith("null_"):
        drop = case[5:]
        if drop == "out":
            drop = "res" if dev else "out"
    elif case == "start_not_from_0":
        a.start[0] = 1
    elif case == "start_flat":
        a.start[1] = 0
    elif case == "start_falls":
        a.start[2] = 1
    elif case == "len0":
        a.lens[3] = 0
    elif case == "weight17":
        a.weights[4] = 17
    elif case == "weight255":
        a.weights[0] = 255
    elif case == "z17":
        a.zs[a.ng - 1] = 17
    assert a.call(h, s, dev, drop, ng) == h.PLK_ERR_ARG, case
    assert "plk_kzg_open_fold_batch" in h.last_error()


def test_open_length_beyond_one_records_finish_is_range_error():
    """a length no record's finish can count is refused before the handle is read"""
    import plonkhip as h
    fake = _opaque_handle()
    for dev in (False, True):
        a = OpenArgs()
        a.lens[1] = 1 << 40
        assert a.call(h, C.addressof(fake), dev) == h.PLK_ERR_RANGE


def _verify_bufs(k, n=4):
    b = {"c": (C.c_uint8 * (3 * n * k))(), "wt": (C.c_uint8 * (n * k))(), "y": (C.c_uint8 * (n * k))(),
         "z": (C.c_uint8 * n)(), "w": (C.c_uint8 * (3 * n))(), "ok": (C.c_uint8 * n)()}
    for i in range(n * k):
        b["c"][3 * i], b["c"][3 * i + 1], b["wt"][i] = 1, 2, 1
    for i in range(n):
        b["w"][3 * i], b["w"][3 * i + 1] = 1, 2
    return b


def _addr(x):
    return None if x is None else C.addressof(x)


def _call_verify(h, vk, k, b, n, dev, drop=None):
    a = [None if drop == key else b[key] for key in ("c", "wt", "y", "z", "w", "ok")]
    v = None if vk is None else C.byref(vk)
    if dev:
        return h.lib().plk_kzg_verify_fold_batch_dev(v, k, *[_addr(x) for x in a[:5]], n, _addr(a[5]), None)
    return h.lib().plk_kzg_verify_fold_batch(v, k, a[0], a[1], a[2], a[3], a[4], n, a[5])


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_verify_arg_errors_come_before_any_device_query(dev):
    import plonkhip as h
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    b = _verify_bufs(16)
    for k in (0, -1, 17, 1 << 20):
        assert _call_verify(h, vk, k, b, 4, dev) == h.PLK_ERR_ARG, k
    assert "plk_kzg_verify_fold_batch" in h.last_error()
    for drop in ("c", "wt", "y", "z", "w", "ok"):
        assert _call_verify(h, vk, 3, b, 4, dev, drop) == h.PLK_ERR_ARG, drop
    assert _call_verify(h, None, 3, b, 4, dev) == h.PLK_ERR_ARG
    assert _call_verify(h, vk, 3, b, 0, dev) == h.PLK_ERR_ARG
    for field, index, value in (("g1", 0, 101), ("g1", 2, 2), ("g2_1", 1, 200), ("g2_s", 0, 255)):
        bad = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
        getattr(bad, field)[index] = value
        assert _call_verify(h, bad, 3, b, 4, dev) == h.PLK_ERR_ARG, field
        assert "verification key" in h.last_error()
        assert _call_verify(h, bad, 3, b, (1 << 30) + 1, dev) == h.PLK_ERR_ARG      # the key comes first


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_verify_n_k_beyond_2_30_is_range_error(dev):
    import plonkhip as h
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    b = _verify_bufs(16)
    for k, n in ((1, (1 << 30) + 1), (2, (1 << 29) + 1), (16, (1 << 26) + 1), (9, (1 << 30) // 9 + 1), (3, 1 << 62)):
        assert _call_verify(h, vk, k, b, n, dev) == h.PLK_ERR_RANGE, (k, n)
    assert "2^30" in h.last_error()


_NODEV_CHILD = r"""
import sys
sys.path[:0] = %r
import test_kzg_fold_cpu as t
import plonkhip as h
assert h.device_count() == 0, "the device is still visible"
print("codes", *t.valid_call_codes(h))
"""


def valid_call_codes(h):
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    codes = []
    for k, n in ((1, 4), (16, 4), (16, 1 << 26)):
        b = _verify_bufs(k)
        codes += [_call_verify(h, vk, k, b, n, False), _call_verify(h, vk, k, b, n, True)]
    return codes


def test_valid_call_without_gpu_is_nodev():
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
    assert codes == [h.PLK_ERR_NODEV] * 6
    if h.device_count() == 0:
        with pytest.raises(h.PlonkHipError) as e:
            h.kzg_verify_fold(vk=h.KzgVk((1, 2, 0), (36, 31), (90, 82)), k=2, commits=[1, 2, 0] * 2, weights=[1, 1],
                              ys=[0, 0], zs=[1], proofs=[1, 2, 0])
        assert e.value.code == h.PLK_ERR_NODEV
        with pytest.raises(h.PlonkHipError) as e:      # the opening needs a resident SRS, which needs a device
            h.Srs([1, 2, 0])
        assert e.value.code == h.PLK_ERR_NODEV
