"""Division by short divisors without a GPU: every argument error (which must come back before any
device query), the host-only plan, workspace and from_roots calls, and the chunked model of the kernels
against the oracle's long division and the reference's recorded outputs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import divide_short_model as M  # noqa: E402
from conftest import load_golden  # noqa: E402

import plonkhip  # noqa: E402
from plonkhip import DivShortJob, PLK_ERR_ARG, PLK_ERR_NODEV, PLK_ERR_RANGE, PLK_OK  # noqa: E402

DEN3 = np.array([3, 0, 5], np.uint8)
KEEP = [DEN3]


def _den(vals):
    a = np.array(vals, np.uint8)
    KEEP.append(a)
    return a.ctypes.data


def _job(num=1, nl=8, den=None, dl=3, quot=1, rem=1):
    """fake non-NULL pointers where the call must fail before it looks at them"""
    return DivShortJob(num, nl, DEN3.ctypes.data if den is None else den, dl, quot, rem)


BAD = {
    "null num": (lambda: _job(num=None), PLK_ERR_ARG),
    "null den": (lambda: DivShortJob(1, 8, None, 3, 1, 1), PLK_ERR_ARG),
    "null quot": (lambda: _job(quot=None), PLK_ERR_ARG),
    "null rem": (lambda: _job(rem=None), PLK_ERR_ARG),
    "nl 0": (lambda: _job(nl=0), PLK_ERR_ARG),
    "dl 0": (lambda: _job(dl=0), PLK_ERR_ARG),
    "dl 1": (lambda: _job(dl=1), PLK_ERR_ARG),
    "den byte 17": (lambda: _job(den=_den([1, 17, 1])), PLK_ERR_ARG),
    "den byte 255": (lambda: _job(den=_den([255, 1])), PLK_ERR_ARG),
    "lead 17": (lambda: _job(den=_den([1, 2, 17])), PLK_ERR_ARG),
    "zero lead": (lambda: _job(den=_den([1, 2, 0])), PLK_ERR_ARG),
    "dl 18": (lambda: _job(den=_den([1] * 18), dl=18), PLK_ERR_RANGE),
    "dl huge": (lambda: _job(den=_den([1] * 18), dl=1 << 40), PLK_ERR_RANGE),
    "nl 2^32": (lambda: _job(nl=1 << 32), PLK_ERR_RANGE),
    "nl 2^40": (lambda: _job(nl=1 << 40), PLK_ERR_RANGE),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_errors_need_no_device(name):
    lib = plonkhip.lib()
    make, code = BAD[name]
    ql, rl = (C.c_size_t * 2)(), (C.c_size_t * 2)()
    assert lib.plk_poly_divide_short_batch_dev(C.byref(make()), 1, 1, 1, None) == code, name
    assert lib.plk_poly_divide_short_batch(C.byref(make()), 1, ql, rl) == code, name
    # a bad job behind a good one is found as well
    arr = (DivShortJob * 2)(_job(), make())
    assert lib.plk_poly_divide_short_batch_dev(arr, 2, 1, 1, None) == code, name
    assert lib.plk_poly_divide_short_batch(arr, 2, ql, rl) == code, name


def test_null_and_count_errors():
    lib = plonkhip.lib()
    good = _job()
    ql, rl = (C.c_size_t * 1)(), (C.c_size_t * 1)()
    assert lib.plk_poly_divide_short_batch_dev(None, 1, 1, 1, None) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_batch_dev(C.byref(good), 0, 1, 1, None) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_batch_dev(C.byref(good), -2, 1, 1, None) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_batch_dev(C.byref(good), 1, None, 1, None) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_batch_dev(C.byref(good), 1, 1, None, None) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_batch(None, 1, ql, rl) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_batch(C.byref(good), 0, ql, rl) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_batch(C.byref(good), 1, None, rl) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_batch(C.byref(good), 1, ql, None) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_workspace(None, 1) == 0
    assert lib.plk_poly_divide_short_workspace(C.byref(good), 0) == 0


def test_valid_call_without_a_gpu_is_nodev():
    if plonkhip.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(plonkhip.PlonkHipError) as e:
        plonkhip.poly_divide_short_batch([[1, 2, 3, 4]], [[1, 1]])
    assert e.value.code == PLK_ERR_NODEV
    buf = np.zeros(64, np.uint8)
    job = _job(num=buf.ctypes.data, quot=buf.ctypes.data + 16, rem=buf.ctypes.data + 32)
    assert plonkhip.lib().plk_poly_divide_short_batch_dev(C.byref(job), 1, buf.ctypes.data + 48, buf.ctypes.data, None) == \
        PLK_ERR_NODEV


# ---- the plan and the workspace
@pytest.mark.parametrize("dl", range(2, 18))
def test_plan_is_consistent(dl):
    p = plonkhip.poly_divide_short_plan(1, dl)
    e, b, lim = p["per_thread"], p["per_block"], p["one_kernel_max"]
    assert p["kernels"] == 1 and e > 0 and b > 0 and b % e == 0 and b % (64 * e) == 0 and 0 < lim <= b
    for nl in (1, dl - 1, dl, e, 64 * e, lim - 1, lim):
        q = plonkhip.poly_divide_short_plan(nl, dl)
        assert q["kernels"] == 1 and (q["per_thread"], q["per_block"], q["one_kernel_max"]) == (e, b, lim), nl
    for nl in (lim + 1, lim + 2, 2 * b, 100 * b + 7, (1 << 32) - 1):
        q = plonkhip.poly_divide_short_plan(nl, dl)
        assert q["kernels"] == 3 and (q["per_thread"], q["per_block"], q["one_kernel_max"]) == (e, b, lim), nl
    assert plonkhip.PLK_DIV_SHORT_LAUNCH_JOBS < 70      # tests/test_divide_short_gpu.py's ragged batch exceeds it


def test_plan_errors():
    lib = plonkhip.lib()
    out = (C.c_int * 4)()
    assert lib.plk_poly_divide_short_plan(8, 3, out) == PLK_OK
    assert lib.plk_poly_divide_short_plan(8, 3, None) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_plan(0, 3, out) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_plan(8, 1, out) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_plan(8, 0, out) == PLK_ERR_ARG
    assert lib.plk_poly_divide_short_plan(8, 18, out) == PLK_ERR_RANGE
    assert lib.plk_poly_divide_short_plan(1 << 32, 3, out) == PLK_ERR_RANGE


def test_workspace():
    W = plonkhip.poly_divide_short_workspace
    for bad in ([], [(0, 3)], [(8, 1)], [(8, 0)], [(8, 18)], [(1 << 32, 3)], [(8, 3), (0, 3)]):
        assert W(bad) == 0, bad
    for dl in (2, 3, 5, 9, 17):
        b = plonkhip.poly_divide_short_plan(1, dl)["per_block"]
        sizes = [1, dl, b - 20, b, b + 1, 2 * b, 2 * b + 1, 65 * b, 257 * b + 3, 1 << 24, (1 << 32) - 1]
        ws = [W([(nl, dl)]) for nl in sizes]
        assert ws[0] > 0 and all(x <= y for x, y in zip(ws, ws[1:])), (dl, ws)
        assert ws[-1] > ws[0]
        assert W([(sizes[3], dl), (sizes[6], dl)]) >= max(ws[3], ws[6])


# ---- plk_poly_from_roots
def test_from_roots_matches_the_oracle_product(oracle):
    rng = np.random.default_rng(5)
    sets = [[z] for z in range(17)] + [list(range(1, 17)), list(range(16)), [3] * 16, [0] * 5, [2, 2, 5, 5, 5, 11]]
    sets += [rng.integers(0, 17, int(rng.integers(1, 17))).tolist() for _ in range(60)]
    for roots in sets:
        want = bytes([1])
        for r in roots:
            want = oracle.poly_mul(want, bytes([(17 - r) % 17, 1]))
        assert plonkhip.poly_from_roots(roots) == want, roots
    assert plonkhip.poly_from_roots(list(range(1, 17))) == bytes([16] + [0] * 15 + [1])   # x^16 - 1


def test_from_roots_errors():
    lib = plonkhip.lib()
    r = np.array([1] * 17, np.uint8)
    out = np.zeros(18, np.uint8)
    rp, op = r.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.plk_poly_from_roots(None, 2, op) == PLK_ERR_ARG
    assert lib.plk_poly_from_roots(rp, 2, None) == PLK_ERR_ARG
    assert lib.plk_poly_from_roots(rp, 0, op) == PLK_ERR_ARG
    assert lib.plk_poly_from_roots(rp, 17, op) == PLK_ERR_RANGE
    r[1] = 17
    assert lib.plk_poly_from_roots(rp, 2, op) == PLK_ERR_ARG


# ---- the model
CHUNKS = range(1, 21)


@pytest.fixture(scope="module")
def golden():
    return [(c["tag"],) + tuple(bytes.fromhex(c[k]) for k in ("num", "den", "quot", "rem"))
            for c in load_golden("divide_short.json")["cases"]]


def _trimmed(p):
    return bytes(p[:max(M.trim(p), 1)])


def test_golden_covers_the_cases(golden):
    tags = {t for t, *_ in golden}
    assert tags == {"t", "d0", "mono", "rep", "zs", "lead", "zero", "exact", "ztop", "one", "raw"}
    assert {len(d) - 1 for _, _, d, _, _ in golden} == set(range(1, 17))
    assert max(len(n) for _, n, _, _, _ in golden) == 64
    assert {d[-1] for t, _, d, _, _ in golden if t == "lead"} == set(range(1, 17))
    assert any(d == bytes([16] + [0] * 15 + [1]) for t, _, d, _, _ in golden if t == "zs")
    assert all(d[0] == 0 for t, _, d, _, _ in golden if t == "d0")
    assert all(not any(d[:-1]) for t, _, d, _, _ in golden if t == "mono")
    assert all(r == b"\0" for t, _, _, _, r in golden if t == "exact")
    assert all(q == b"\0" and r == b"\0" for t, _, _, q, r in golden if t == "zero")
    assert all(len(q) < len(n) - len(d) + 1 for t, n, d, q, _ in golden if t == "ztop")
    for dl in range(2, 18):
        assert {dl - 1, dl, dl + 1} <= {len(n) for t, n, d, _, _ in golden if len(d) == dl}, dl
    raw = [n for t, n, _, _, _ in golden if t == "raw"]
    assert all(max(n) >= 17 for n in raw) and any(0xFF in n for n in raw) and any(0xEE in n for n in raw)
    assert all(max(n) < 17 for t, n, _, _, _ in golden if t != "raw")


def test_model_matches_the_goldens(golden):
    for g, (tag, n, d, q, r) in enumerate(golden):
        if tag == "raw":
            continue
        lq, lr = M.long_divide(n, d)
        assert (_trimmed(lq), _trimmed(lr)) == (q, r), g
        assert len(lq) == max(len(n) - len(d) + 1, 1) and len(lr) == min(len(d) - 1, len(n))
        for chunk in CHUNKS:
            T = M.bucket_of(len(d)) if (g + chunk) % 2 else None
            assert M.divide_chunked(n, d, chunk, 1 + (g + chunk) % 4, T) == (lq, lr), (g, chunk)


def test_model_matches_the_oracle(oracle):
    rng = np.random.default_rng(0x5C41)
    for it in range(300):
        t = 1 + it % 16
        nl = int(rng.integers(1, 400))
        n = rng.integers(0, 17, nl).astype(np.uint8)
        d = rng.integers(0, 17, t + 1).astype(np.uint8)
        d[t] = int(rng.integers(1, 17))
        if it % 5 == 0:
            d[0] = 0
        if it % 11 == 0:
            d[:t] = 0
        if it % 13 == 0:
            n[:] = 0
        want = oracle.poly_divide(n, d)
        chunk = CHUNKS[it % len(CHUNKS)]
        lq, lr = M.divide_chunked(n, d, chunk, 1 + it % 5, M.bucket_of(t + 1) if it % 2 else None)
        assert (_trimmed(lq), _trimmed(lr)) == want, (it, t, nl, chunk)
        assert (lq, lr) == M.long_divide(n, d)
