"""KZG multi-point openings (plk_kzg_multi_coeffs, plk_kzg_multi_workspace, plk_kzg_open_multi_batch*,
plk_kzg_verify_multi_batch*) without a GPU: the Python model of tests/kzg_multi_model.py against every
reference output in tests/golden/kzg_multi.json, the generator's determinism, the host-only calls and the
argument checks that come before any device query.  No CPU fallback: a valid call without a device is
PLK_ERR_NODEV."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kzg_multi_model as MM
from conftest import ROOT, load_golden

REF_SRC = os.path.join(os.path.dirname(ROOT), "reference", "src")
NEW = ("plk_kzg_multi_coeffs", "plk_kzg_multi_workspace", "plk_kzg_open_multi_batch", "plk_kzg_open_multi_batch_dev",
       "plk_kzg_verify_multi_batch", "plk_kzg_verify_multi_batch_dev")
FULL = MM.FULL


@pytest.fixture(scope="module")
def gold():
    """the committed record, and it joined with its inputs (rebuilt from the recorded seeds)"""
    import make_kzg_multi_golden as mk
    raw = load_golden("kzg_multi.json")
    return (raw,) + mk.expand(raw)


def unhex(s):
    return list(bytes.fromhex(s))


def key_of(b):
    b = tuple(b)
    return (b[0:3], b[3:5], b[5:7])


def split_job(row, k):
    """(vk, commits, sets, weights, ys 17 k, u, proofs6) of one recorded verification job"""
    row = [int(v) for v in row]
    ent = [row[7 + 25 * i:32 + 25 * i] for i in range(k)]
    return (key_of(row[:7]), [tuple(e[:3]) for e in ent], [int.from_bytes(bytes(e[3:7]), "little") for e in ent],
            [e[7] for e in ent], [v for e in ent for v in e[8:25]], row[-1], row[7 + 25 * k:13 + 25 * k])


# ------------------------------------------------------------------ the golden file and the model
def test_golden_file_is_small_and_complete(gold):
    import gen
    raw, groups, verify, cases = gold
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kzg_multi.json")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "kzg_fold.json"))
    assert len(groups) >= 200 and {len(g["polys"]) for g in groups} == {1, 2, 3, 9, 15}
    sizes = {len(MM.points(m)) for g in groups for m in g["sets"]}
    assert sizes == set(range(1, 17))
    assert any(m & 1 for g in groups for m in g["sets"]) and any(not m & 1 for g in groups for m in g["sets"])
    inside = [bool((1 << g["u"]) & MM.mask_of(a for m in g["sets"] for a in MM.points(m))) for g in groups]
    assert 40 < sum(inside) < len(groups) - 40
    assert any(set(g["weights"]) == {0} for g in groups)
    assert max(len(p) for g in groups for p in g["polys"]) >= 38
    shapes = [(len(p), len(MM.points(m))) for g in groups for p, m in zip(g["polys"], g["sets"])]
    assert any(n <= t for n, t in shapes) and any(n == t + 1 for n, t in shapes) and any(n == 1 for n, _ in shapes)
    assert sorted(verify) == [1, 2, 3, 9, 15] and sum(len(b) for _, b in verify.values()) >= 2000
    srs = np.array(unhex(raw["srs"]), np.uint8).reshape(-1, 3)
    assert [tuple(p) for p in srs.tolist()] == [gen.KG[pow(2, i, 17)] for i in range(len(srs))]
    assert unhex(raw["key"]) == [1, 2, 0, 36, 31, 90, 82] and len(cases) >= 30


def test_model_reproduces_every_opening(gold):
    import make_kzg_multi_golden as mk
    raw, groups, _, _ = gold
    srs = np.array(unhex(raw["srs"]), np.uint8).reshape(-1, 3)
    zero_h = 0
    for i, g in enumerate(groups):
        ys, h, W, Wp = MM.open_multi(srs, g["polys"], g["sets"], g["weights"], g["u"])
        assert mk.digest(ys, MM.F.trim(h).tolist()) == g["digest"], i      # the reference's poly_add trims
        assert (W, Wp) == (g["W"], g["Wp"]), i
        zero_h += not h.any()
    assert zero_h >= 20                                                    # zero weights, cancelling pairs, len <= t


@pytest.mark.parametrize("k", [1, 2, 3, 9, 15])
def test_model_reproduces_every_verification(gold, k):
    raw, _, verify, _ = gold
    rows, bits = verify[k]
    assert 0.1 * len(bits) < bits.sum() < 0.6 * len(bits)
    own = sum(tuple(r[:7]) != tuple(unhex(raw["key"])) for r in rows.tolist())
    assert own >= len(rows) // 5                                           # jobs carrying their own key
    for i, r in enumerate(rows):
        vk, cs, ss, ws, ys, u, pr = split_job(r, k)
        assert MM.verify_multi(vk, cs, ss, ws, ys, u, pr) == bits[i], (k, i)


def test_model_reproduces_end_to_end_cases(gold):
    import make_kzg_multi_golden as mk
    raw, _, _, cases = gold
    srs = np.array(unhex(raw["srs"]), np.uint8).reshape(-1, 3)
    vk = key_of(unhex(raw["key"]))
    for n, c in enumerate(cases):
        assert c["commits"] == [MM.F.msm(srs[:len(MM.F.trim(p))], MM.F.trim(p)) for p in c["polys"]], n
        ys, h, W, Wp = MM.open_multi(srs, c["polys"], c["sets"], c["weights"], c["u"])
        assert mk.digest(ys, MM.F.trim(h).tolist()) == c["digest"] and (W, Wp) == (c["W"], c["Wp"]), n
        got = [MM.verify_multi(vk, cm, s, c["weights"], y, c["u"], list(w) + list(p))
               for s, y, cm, w, p in mk.e2e_variants(n, c["sets"], ys, c["commits"], W, Wp)]
        assert "".join(str(b) for b in got) == c["bits"], n
        # honest accepted; an altered value, W or commitment rejected (u outside T and non-zero weights: its
        # coefficient in the left-hand side is non-zero); an altered W' rejected unless u = s = 2, where the
        # check reads (C - y G) = (s - u) W' = 0 for every W'
        assert c["bits"][0] == "1" and c["bits"][1] == "0" and c["bits"][3] == c["bits"][5] == "0", n
        assert c["bits"][4] == ("1" if c["u"] == 2 else "0"), n


def test_model_marks_invalid_bytes():
    vk = ((1, 2, 0), (36, 31), (90, 82))
    g = (1, 2, 0)
    row = [3] * 17
    ok = dict(commits=[g, g], sets=[0b11, 0b100], weights=[1, 1], ys=row + row, u=5, proofs6=list(g + g))
    assert MM.verify_multi(vk, **ok) in (0, 1)
    for field, value in (("commits", [g, (101, 2, 0)]), ("commits", [g, (1, 2, 2)]), ("sets", [0, 0b100]),
                         ("sets", [0b11, 1 << 17]), ("sets", [FULL, 0b100]), ("weights", [1, 17]), ("u", 17),
                         ("ys", row + [3, 3, 17] + [3] * 14), ("proofs6", [1, 2, 0, 1, 255, 0]),
                         ("proofs6", [1, 2, 7, 1, 2, 0])):
        assert MM.verify_multi(vk, **dict(ok, **{field: value})) == 2, field
    # a byte >= 17 away from the set is not read
    assert MM.verify_multi(vk, **dict(ok, ys=row + [200, 200, 3] + [200] * 14)) == MM.verify_multi(vk, **ok)


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="reference sources not present")
def test_generator_reproduces_the_committed_file(gold):
    import make_kzg_multi_golden as mk
    assert mk.generate(REF_SRC) == gold[0]


# ------------------------------------------------------------------ exports and the host-only calls
def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("kzg_multi_coeffs", "kzg_multi_workspace", "kzg_open_multi", "kzg_open_multi_dev", "kzg_verify_multi",
                 "kzg_verify_multi_dev"):
        assert hasattr(h, name), name
    with open(os.path.join(ROOT, "include", "plonkhip.h")) as f:
        txt = f.read()
    assert "#define PLK_KZG_MULTI_MAX 15" in txt and "#define PLK_KZG_MULTI_POINTS 16" in txt


def seeded_masks(seed, n):
    import gen
    import make_kzg_multi_golden as mk
    r = [int(v >> np.uint64(8)) for v in gen.splitmix64(seed, 3 * n)]
    return [mk.random_mask(r[3 * i], r[3 * i + 1], r[3 * i + 2] % 6) for i in range(n)], r


def test_multi_coeffs_equals_the_model_for_every_u():
    import plonkhip as h
    for k in range(1, 16):
        sets, r = seeded_masks(0xC0EF + k, k)
        ws = [v % 17 for v in r[:k]]
        for u in range(17):
            assert h.kzg_multi_coeffs(sets, ws, u) == MM.multi_coeffs(sets, ws, u), (k, u)
    # T = every point: c_T = 0 at every u; one set: c_0 = w_0
    assert h.kzg_multi_coeffs([FULL & ~1, 1], [3, 4], 6)[2] == 0
    assert h.kzg_multi_coeffs([0b1010], [7], 3) == [7, 0] and h.kzg_multi_coeffs([0b1010], [7], 2) == [7, (17 - 16 * 1) % 17]


def test_multi_coeffs_argument_checks():
    import plonkhip as h
    lib = h.lib()
    s, w, c = (C.c_uint32 * 16)(*[3] * 16), (C.c_uint8 * 16)(*[1] * 16), (C.c_uint8 * 17)()
    assert lib.plk_kzg_multi_coeffs(s, w, 15, 16, c) == h.PLK_OK
    for args in ((None, w, 2, 0, c), (s, None, 2, 0, c), (s, w, 2, 0, None), (s, w, 0, 0, c), (s, w, -1, 0, c),
                 (s, w, 16, 0, c), (s, w, 2, 17, c)):
        assert lib.plk_kzg_multi_coeffs(*args) == h.PLK_ERR_ARG, args[2:4]
    for bad in (0, 1 << 17, FULL, 0xFFFFFFFF):
        s2 = (C.c_uint32 * 2)(3, bad)
        assert lib.plk_kzg_multi_coeffs(s2, w, 2, 0, c) == h.PLK_ERR_ARG, bad
    w2 = (C.c_uint8 * 2)(1, 17)
    assert lib.plk_kzg_multi_coeffs(s, w2, 2, 0, c) == h.PLK_ERR_ARG
    assert "plk_kzg_multi_coeffs" in h.last_error()


def test_workspace_is_host_only_and_zero_on_bad_arguments():
    import plonkhip as h
    lib = h.lib()
    ws = h.kzg_multi_workspace
    assert ws([], [], [0]) == 0
    assert lib.plk_kzg_multi_workspace(None, (C.c_uint32 * 1)(1), (C.c_int * 2)(0, 1), 1) == 0
    assert lib.plk_kzg_multi_workspace((C.c_size_t * 1)(5), None, (C.c_int * 2)(0, 1), 1) == 0
    assert lib.plk_kzg_multi_workspace((C.c_size_t * 1)(5), (C.c_uint32 * 1)(1), None, 1) == 0
    assert ws([5, 5], [1, 1], [0, 2, 2]) == 0 and ws([5, 5], [1, 1], [1, 2]) == 0 and ws([5, 5], [1, 1], [0, 2, 1]) == 0
    assert ws([5] * 16, [1] * 16, [0, 16]) == 0                      # a group of more than 15
    assert ws([5] * 15, [1] * 15, [0, 15]) > 0
    assert ws([5, 0], [1, 1], [0, 2]) == 0
    for bad in (0, 1 << 17, FULL):
        assert ws([5, 5], [1, bad], [0, 2]) == 0, bad
    one = ws([4096], [2], [0, 1])
    assert one > 0 and one % 256 == 0
    sizes = [ws([n] * 9, [0b11] * 9, [0, 9]) for n in (1, 4096, 4097, 1 << 20, 1 << 22)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[4]
    assert sizes[4] >= (1 << 22) - 2                                 # h lives in the workspace
    assert ws([1 << 16] * 4, [2] * 4, [0, 4]) < ws([1 << 16] * 4, [2] * 4, [0, 2, 4])   # a second group has its own h


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
        self.sets = (C.c_uint32 * n)(*[0b101] * n)
        self.weights = (C.c_uint8 * n)(*[1] * n)
        start = [0]
        for k in counts:
            start.append(start[-1] + k)
        self.start = (C.c_int * len(start))(*start)
        self.us = (C.c_uint8 * len(counts))(*[3] * len(counts))
        self.ng = len(counts)
        self.ys = (C.c_uint8 * (17 * n))()
        self.out = (C.c_uint8 * (6 * len(counts)))()
        self.res = (C.c_uint8 * (2 * 2176 * len(counts)))()

    def call(self, h, s, dev, drop=None, ng=None):
        a = {k: (None if drop == k else getattr(self, k))
             for k in ("lens", "sets", "weights", "start", "us", "ys", "out", "res")}
        ng = self.ng if ng is None else ng
        if dev:
            polys = None if drop == "polys" else self.vptrs
            res = None if a["res"] is None else C.addressof(a["res"])
            ys = None if a["ys"] is None else C.addressof(a["ys"])
            return h.lib().plk_kzg_open_multi_batch_dev(s, polys, a["lens"], a["sets"], a["weights"], a["start"], a["us"], ng,
                                                        ys, res, None, None, None)
        polys = None if drop == "polys" else self.ptrs
        return h.lib().plk_kzg_open_multi_batch(s, polys, a["lens"], a["sets"], a["weights"], a["start"], a["us"], ng,
                                                a["ys"], a["out"])


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_open_null_handle_is_arg_error(dev):
    import plonkhip as h
    assert OpenArgs().call(h, None, dev) == h.PLK_ERR_ARG
    assert "plk_kzg_open_multi_batch" in h.last_error()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("case", ["ngroups0", "ngroups_negative", "null_polys", "null_lens", "null_sets", "null_weights",
                                  "null_start", "null_us", "null_ys", "null_out", "start_not_from_0", "start_flat",
                                  "start_falls", "group_of_16", "len0", "mask0", "mask_bit17", "mask_all17", "weight17",
                                  "weight255", "u17"])
def test_open_arg_errors_come_before_any_device_query(case, dev):
    import plonkhip as h
    fake = _opaque_handle()
    s = C.addressof(fake)
    a = OpenArgs((16,)) if case == "group_of_16" else OpenArgs()
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
    elif case == "mask0":
        a.sets[2] = 0
    elif case == "mask_bit17":
        a.sets[4] = 1 << 17 | 1
    elif case == "mask_all17":
        a.sets[0] = FULL
    elif case == "weight17":
        a.weights[4] = 17
    elif case == "weight255":
        a.weights[0] = 255
    elif case == "u17":
        a.us[a.ng - 1] = 17
    assert a.call(h, s, dev, drop, ng) == h.PLK_ERR_ARG, case
    assert "plk_kzg_open_multi_batch" in h.last_error()


def test_open_length_beyond_one_records_finish_is_range_error():
    """a length no record's finish can count is refused before the handle is read"""
    import plonkhip as h
    fake = _opaque_handle()
    for dev in (False, True):
        a = OpenArgs()
        a.lens[1] = 1 << 40
        assert a.call(h, C.addressof(fake), dev) == h.PLK_ERR_RANGE


def _verify_bufs(k, n=4):
    b = {"c": (C.c_uint8 * (3 * n * k))(), "s": (C.c_uint32 * (n * k))(*[0b11] * (n * k)), "wt": (C.c_uint8 * (n * k))(),
         "y": (C.c_uint8 * (17 * n * k))(), "u": (C.c_uint8 * n)(), "w": (C.c_uint8 * (6 * n))(), "ok": (C.c_uint8 * n)()}
    for i in range(n * k):
        b["c"][3 * i], b["c"][3 * i + 1], b["wt"][i] = 1, 2, 1
    for i in range(2 * n):
        b["w"][3 * i], b["w"][3 * i + 1] = 1, 2
    return b


def _addr(x):
    return None if x is None else C.addressof(x)


def _call_verify(h, vk, k, b, n, dev, drop=None):
    a = [None if drop == key else b[key] for key in ("c", "s", "wt", "y", "u", "w", "ok")]
    v = None if vk is None else C.byref(vk)
    if dev:
        return h.lib().plk_kzg_verify_multi_batch_dev(v, k, *[_addr(x) for x in a[:6]], n, _addr(a[6]), None)
    return h.lib().plk_kzg_verify_multi_batch(v, k, a[0], a[1], a[2], a[3], a[4], a[5], n, a[6])


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_verify_arg_errors_come_before_any_device_query(dev):
    import plonkhip as h
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    b = _verify_bufs(15)
    for k in (0, -1, 16, 1 << 20):
        assert _call_verify(h, vk, k, b, 4, dev) == h.PLK_ERR_ARG, k
    assert "plk_kzg_verify_multi_batch" in h.last_error()
    for drop in ("c", "s", "wt", "y", "u", "w", "ok"):
        assert _call_verify(h, vk, 3, b, 4, dev, drop) == h.PLK_ERR_ARG, drop
    assert _call_verify(h, None, 3, b, 4, dev) == h.PLK_ERR_ARG
    assert _call_verify(h, vk, 3, b, 0, dev) == h.PLK_ERR_ARG
    for field, index, value in (("g1", 0, 101), ("g1", 2, 2), ("g2_1", 1, 200), ("g2_s", 0, 255)):
        bad = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
        getattr(bad, field)[index] = value
        assert _call_verify(h, bad, 3, b, 4, dev) == h.PLK_ERR_ARG, field
        assert "verification key" in h.last_error()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_verify_n_k_beyond_2_30_is_range_error(dev):
    import plonkhip as h
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    b = _verify_bufs(15)
    for k, n in ((1, (1 << 30) + 1), (2, (1 << 29) + 1), (15, (1 << 30) // 15 + 1), (3, 1 << 62)):
        assert _call_verify(h, vk, k, b, n, dev) == h.PLK_ERR_RANGE, (k, n)
    assert "2^30" in h.last_error()


def test_verify_dev_wants_aligned_masks():
    import plonkhip as h
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    b = _verify_bufs(2)
    a = [_addr(b[key]) for key in ("c", "s", "wt", "y", "u", "w", "ok")]
    assert h.lib().plk_kzg_verify_multi_batch_dev(C.byref(vk), 2, a[0], a[1] + 2, a[2], a[3], a[4], a[5], 4, a[6], None) == \
        h.PLK_ERR_ARG
    assert "aligned" in h.last_error()


_NODEV_CHILD = r"""
import sys
sys.path[:0] = %r
import test_kzg_multi_cpu as t
import plonkhip as h
assert h.device_count() == 0, "the device is still visible"
print("codes", *t.valid_call_codes(h))
"""


def valid_call_codes(h):
    vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))
    codes = []
    for k, n in ((1, 4), (15, 4), (15, 1 << 26)):
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
            h.kzg_verify_multi(h.KzgVk((1, 2, 0), (36, 31), (90, 82)), 2, [1, 2, 0] * 2, [1, 2], [1, 1], [0] * 34, [1],
                               [1, 2, 0] * 2)
        assert e.value.code == h.PLK_ERR_NODEV
