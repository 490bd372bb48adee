"""Pairings and KZG verification (plk_pairing_batch*, plk_kzg_verify_batch*) without a GPU: the Python
model of the kernel's schedule against every reference output in tests/golden/pairing.json, the
algebra those outputs must satisfy, the generator's determinism, the exports, and the argument checks
that come before any device query.  No CPU fallback: a valid call without a device is PLK_ERR_NODEV."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gen
import pairing_model as M
from conftest import ROOT, load_golden

REF_SRC = "/root/reference/src"
NEW = ("plk_pairing_batch", "plk_pairing_batch_dev", "plk_kzg_verify_batch", "plk_kzg_verify_batch_dev")


@pytest.fixture(scope="module")
def gold():
    return load_golden("pairing.json")


def g2_multiples(gold):
    return {int(k): tuple(bytes.fromhex(v)) for k, v in gold["g2_multiples"].items()}


def ints(row):
    return tuple(int(v) for v in row)


def test_golden_file_is_small_and_complete(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pairing.json")) < 128 * 1024
    assert sorted(g2_multiples(gold)) == list(range(1, 17))
    assert g2_multiples(gold)[1] == (36, 31)                       # g2_generator()
    assert len(gold["table"]) == 2 * 2 * 102 * 16
    assert len(gold["raw"]["out"]) == 2 * 2 * 1024 and len(gold["raw"]["inputs"]) == 2 * 5 * 1024
    assert len(gold["verify_exhaustive"]["bits"]) == 2 * ((17 ** 4 + 7) // 8)
    assert len(gold["verify_raw"]["bits"]) == 2048 and len(gold["verify_raw"]["jobs"]) == 2 * 15 * 2048
    ns = gold["reference_ns"]
    assert ns["pairing"] > 0 and ns["verify"] > 0 and ns["cpu"]


def test_model_reproduces_table(gold):
    g2m = g2_multiples(gold)
    tab = bytes.fromhex(gold["table"])
    for i, p in enumerate(gen.all_points()):
        for k in range(1, 17):
            o = 2 * (16 * i + k - 1)
            assert M.pairing(ints(p), g2m[k]) == (tab[o], tab[o + 1]), (ints(p), k)


def test_model_reproduces_raw(gold):
    raw = np.frombuffer(bytes.fromhex(gold["raw"]["inputs"]), np.uint8).reshape(-1, 5)
    out = bytes.fromhex(gold["raw"]["out"])
    assert 200 < int(raw[:, 2].sum()) < 320                        # about a quarter carry the flag
    off = sum((int(y) ** 2 - int(x) ** 3 - 3) % 101 != 0 for x, y, _ in raw[:, :3])
    assert off > 900                                                # most are off the curve
    for i, r in enumerate(raw):
        assert M.pairing_bytes(ints(r[:3]), ints(r[3:])) == (out[2 * i], out[2 * i + 1]), (i, ints(r))


def test_table_is_bilinear_on_the_subgroup(gold):
    """e(aG, bH) = e(G, H)^(ab) for a, b in 1 .. 16, and e(G, H) has order 17; e(O, Q) = (0, 0)"""
    g2m = g2_multiples(gold)
    tab = bytes.fromhex(gold["table"])
    pts = [ints(p) for p in gen.all_points()]
    at = {(p, k): (tab[2 * (16 * i + k - 1)], tab[2 * (16 * i + k - 1) + 1]) for i, p in enumerate(pts) for k in g2m}
    e = at[(gen.KG[1], 1)]
    pw = [(1, 0)]
    for _ in range(17):
        pw.append(M.gt_mul(pw[-1], e))
    assert pw[17] == (1, 0) and all(v != (1, 0) for v in pw[1:17])
    for a in range(1, 17):
        for b in range(1, 17):
            assert at[(gen.KG[a], b)] == pw[a * b % 17], (a, b)
    assert all(at[(gen.KG[0], k)] == (0, 0) for k in g2m)


def exhaustive_bits(gold):
    packed = np.frombuffer(bytes.fromhex(gold["verify_exhaustive"]["bits"]), np.uint8)
    return np.unpackbits(packed, bitorder="little")[:17 ** 4]


def test_exhaustive_bitmap_is_the_opening_equation(gold):
    """accept exactly when c - y + z w = 2 w (mod 17): s = 2, C = cG, W = wG"""
    g2m = g2_multiples(gold)
    vk = bytes.fromhex(gold["verify_exhaustive"]["vk"])
    assert ints(vk) == (1, 2, 0) + g2m[1] + g2m[2]
    bits = exhaustive_bits(gold)
    c, w, z, y = (v.reshape(-1) for v in np.meshgrid(*[np.arange(17)] * 4, indexing="ij"))
    assert np.array_equal(bits, ((c - y + z * w - 2 * w) % 17 == 0).astype(np.uint8))


def test_model_reproduces_every_exhaustive_entry(gold):
    """all 83,521 openings through the model (its pairings repeat, so they are remembered)"""
    g2m = g2_multiples(gold)
    key = ((1, 2, 0), g2m[1], g2m[2])
    bits = exhaustive_bits(gold).tolist()
    i = 0
    for c in range(17):
        for w in range(17):
            for z in range(17):
                for y in range(17):
                    assert M.kzg_verify(key, gen.KG[c], gen.KG[w], z, y) == bits[i], (c, w, z, y)
                    i += 1
    assert i == len(bits) == 17 ** 4


def test_model_reproduces_verify_raw(gold):
    jobs = np.frombuffer(bytes.fromhex(gold["verify_raw"]["jobs"]), np.uint8).reshape(-1, 15)
    bits = gold["verify_raw"]["bits"]
    assert 0 < bits.count("1") < len(bits)
    for i, j in enumerate(jobs):
        j = ints(j)
        assert M.kzg_verify((j[0:3], j[3:5], j[5:7]), j[7:10], j[10:13], j[13], j[14]) == int(bits[i]), (i, j)


def test_model_marks_invalid_encodings():
    assert M.pairing_bytes((101, 0, 0), (1, 1)) == (0xFF, 0xFF)
    assert M.pairing_bytes((0, 0, 2), (1, 1)) == (0xFF, 0xFF)
    assert M.pairing_bytes((0, 0, 1), (1, 255)) == (0xFF, 0xFF)
    vk = ((1, 2, 0), (36, 31), (90, 82))
    assert M.kzg_verify(vk, (1, 2, 0), (1, 2, 0), 17, 0) == 2
    assert M.kzg_verify(vk, (1, 2, 0), (1, 2, 0), 0, 17) == 2
    assert M.kzg_verify(vk, (1, 2, 0), (1, 101, 0), 0, 0) == 2
    # a constant polynomial: the proof is the identity and C = yG is what is accepted
    assert [M.kzg_verify(vk, gen.KG[5], gen.KG[0], 3, y) for y in range(17)] == [int(y == 5) for y in range(17)]


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="reference sources not present")
def test_generator_reproduces_the_committed_file(gold):
    import make_pairing_golden as mk
    again = mk.generate(REF_SRC, timing=False)
    for k in gold:
        if k != "reference_ns":
            assert again[k] == gold[k], k
    assert set(again) == set(gold)


def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("KzgVk", "pairing", "pairing_dev", "kzg_verify", "kzg_verify_dev"):
        assert hasattr(h, name), name
    assert C.sizeof(h.KzgVk) == 8
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    assert bytes(vk) == bytes([1, 2, 0, 36, 31, 90, 82, 0])


def _bufs(n=4):
    """host blocks a failing call never reads (their addresses also stand in for device pointers)"""
    b = {k: (C.c_uint8 * (m * n))() for k, m in (("g1", 3), ("g2", 2), ("gt", 2), ("c", 3), ("w", 3), ("z", 1),
                                                 ("y", 1), ("ok", 1))}
    for i in range(n):
        b["g1"][3 * i], b["g1"][3 * i + 1] = 1, 2
        b["c"][3 * i], b["c"][3 * i + 1] = 1, 2
        b["w"][3 * i], b["w"][3 * i + 1] = 1, 2
        b["g2"][2 * i], b["g2"][2 * i + 1] = 36, 31
    return b


def _addr(x):
    return None if x is None else C.addressof(x)


def _call_pairing(h, b, n, dev, drop=None):
    a = [None if drop == k else b[k] for k in ("g1", "g2", "gt")]
    if dev:
        return h.lib().plk_pairing_batch_dev(_addr(a[0]), _addr(a[1]), n, _addr(a[2]), None)
    return h.lib().plk_pairing_batch(a[0], a[1], n, a[2])


def _call_verify(h, vk, b, n, dev, drop=None):
    a = [None if drop == k else b[k] for k in ("c", "z", "y", "w", "ok")]
    v = None if vk is None else C.byref(vk)
    if dev:
        return h.lib().plk_kzg_verify_batch_dev(v, _addr(a[0]), _addr(a[1]), _addr(a[2]), _addr(a[3]), n, _addr(a[4]), None)
    return h.lib().plk_kzg_verify_batch(v, a[0], a[1], a[2], a[3], n, a[4])


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_arg_errors_come_before_any_device_query(dev):
    import plonkhip as h
    b = _bufs()
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    for drop in ("g1", "g2", "gt"):
        assert _call_pairing(h, b, 4, dev, drop) == h.PLK_ERR_ARG, drop
    assert "plk_pairing_batch" in h.last_error()
    assert _call_pairing(h, b, 0, dev) == h.PLK_ERR_ARG
    for drop in ("c", "z", "y", "w", "ok"):
        assert _call_verify(h, vk, b, 4, dev, drop) == h.PLK_ERR_ARG, drop
    assert _call_verify(h, None, b, 4, dev) == h.PLK_ERR_ARG
    assert _call_verify(h, vk, b, 0, dev) == h.PLK_ERR_ARG
    assert "plk_kzg_verify_batch" in h.last_error()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("field,index,value", [("g1", 0, 101), ("g1", 1, 255), ("g1", 2, 2), ("g2_1", 0, 101),
                                               ("g2_1", 1, 200), ("g2_s", 0, 255), ("g2_s", 1, 101)])
def test_invalid_vk_byte_is_arg_error(dev, field, index, value):
    import plonkhip as h
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    getattr(vk, field)[index] = value
    assert _call_verify(h, vk, _bufs(), 4, dev) == h.PLK_ERR_ARG
    assert "verification key" in h.last_error()
    # n beyond the range is still an argument error when the key is bad
    assert _call_verify(h, vk, _bufs(), (1 << 30) + 1, dev) == h.PLK_ERR_ARG


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_n_beyond_2_30_is_range_error(dev):
    import plonkhip as h
    b = _bufs()
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    for n in ((1 << 30) + 1, 1 << 40):
        assert _call_pairing(h, b, n, dev) == h.PLK_ERR_RANGE
        assert _call_verify(h, vk, b, n, dev) == h.PLK_ERR_RANGE
    assert "2^30" in h.last_error()


_NODEV_CHILD = r"""
import sys
sys.path[:0] = %r
import test_pairing_cpu as t
import plonkhip as h
assert h.device_count() == 0, "the device is still visible"
print("codes", *t.valid_call_codes(h))
"""


def valid_call_codes(h):
    b = _bufs()
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    return [_call_pairing(h, b, 4, False), _call_verify(h, vk, b, 4, False),
            _call_pairing(h, b, 4, True), _call_verify(h, vk, b, 4, True)]


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
    assert codes == [h.PLK_ERR_NODEV] * 4
    if h.device_count() == 0:
        with pytest.raises(h.PlonkHipError) as e:
            h.pairing([1, 2, 0], [36, 31])
        assert e.value.code == h.PLK_ERR_NODEV
