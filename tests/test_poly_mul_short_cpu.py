"""Products by short operands without a GPU: every argument error (which must come back before any device
query), the host-only plan, the run structure's layout, and the model (numpy.convolve over the operands mod
17) against the reference's recorded products."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import poly_mul_short_model as M  # noqa: E402
from conftest import ROOT, load_golden  # noqa: E402

import plonkhip  # noqa: E402
from plonkhip import MulShortRun, PLK_ERR_ARG, PLK_ERR_NODEV, PLK_ERR_RANGE, PLK_OK  # noqa: E402

MAX = plonkhip.PLK_MUL_SHORT_MAX


def _run(a=1, la=8, sa=0, b=1, lb=3, sb=0, out=1, so=0, count=1):
    """fake non-NULL pointers where the call must fail before it looks at them"""
    return MulShortRun(a, la, sa, b, lb, sb, out, so, count)


BAD = {
    "null a": (lambda: _run(a=None), PLK_ERR_ARG),
    "null b": (lambda: _run(b=None), PLK_ERR_ARG),
    "null out": (lambda: _run(out=None), PLK_ERR_ARG),
    "count 0": (lambda: _run(count=0), PLK_ERR_ARG),
    "la 0": (lambda: _run(la=0), PLK_ERR_ARG),
    "lb 0": (lambda: _run(lb=0), PLK_ERR_ARG),
    "out_stride 0 count 2": (lambda: _run(count=2), PLK_ERR_ARG),
    "out_stride one short": (lambda: _run(so=9, count=2), PLK_ERR_ARG),
    "out_stride one short, b long": (lambda: _run(la=3, lb=1 << 20, so=(1 << 20) + 1, count=3), PLK_ERR_ARG),
    "both 1025": (lambda: _run(la=MAX + 1, lb=MAX + 1), PLK_ERR_RANGE),
    "1025 x 2^20": (lambda: _run(la=MAX + 1, lb=1 << 20), PLK_ERR_RANGE),
    "2^20 x 1025": (lambda: _run(la=1 << 20, lb=MAX + 1), PLK_ERR_RANGE),
    "product 2^32": (lambda: _run(la=2, lb=(1 << 32) - 1), PLK_ERR_RANGE),
    "product 2^32, a long": (lambda: _run(la=(1 << 32) - MAX + 1, lb=MAX), PLK_ERR_RANGE),
    "la 2^40": (lambda: _run(la=1 << 40, lb=1), PLK_ERR_RANGE),
    "la 2^64 - 1": (lambda: _run(la=(1 << 64) - 1, lb=2), PLK_ERR_RANGE),
    "2^24 + 1 products": (lambda: _run(so=16, count=(1 << 24) + 1), PLK_ERR_RANGE),
    "a run past the grid": (lambda: _run(la=1 << 20, lb=MAX, so=1 << 21, count=1 << 16), PLK_ERR_RANGE),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_errors_need_no_device(name):
    lib = plonkhip.lib()
    make, code = BAD[name]
    lens = (C.c_size_t * 4)()
    assert lib.plk_poly_mul_short_batch_dev(C.byref(make()), 1, 1, None) == code, name
    assert lib.plk_poly_mul_short_batch_dev(C.byref(make()), 1, None, None) == code, name
    assert lib.plk_poly_mul_short_batch(C.byref(make()), 1, lens) == code, name
    assert lib.plk_poly_mul_short_batch(C.byref(make()), 1, None) == code, name
    # a bad run behind a good one is found as well
    arr = (MulShortRun * 2)(_run(), make())
    assert lib.plk_poly_mul_short_batch_dev(arr, 2, 1, None) == code, name
    assert lib.plk_poly_mul_short_batch(arr, 2, lens) == code, name


def test_null_and_count_errors():
    lib = plonkhip.lib()
    good = _run()
    lens = (C.c_size_t * 1)()
    assert lib.plk_poly_mul_short_batch_dev(None, 1, 1, None) == PLK_ERR_ARG
    assert lib.plk_poly_mul_short_batch_dev(C.byref(good), 0, 1, None) == PLK_ERR_ARG
    assert lib.plk_poly_mul_short_batch_dev(C.byref(good), -2, 1, None) == PLK_ERR_ARG
    assert lib.plk_poly_mul_short_batch(None, 1, lens) == PLK_ERR_ARG
    assert lib.plk_poly_mul_short_batch(C.byref(good), 0, lens) == PLK_ERR_ARG


def test_products_of_a_call_are_counted_over_its_runs():
    """2^24 products are accepted as far as the argument checks go, one more over two runs is not"""
    lib = plonkhip.lib()
    arr = (MulShortRun * 2)(_run(so=16, count=1 << 23), _run(so=16, count=(1 << 23) + 1))
    assert lib.plk_poly_mul_short_batch_dev(arr, 2, None, None) == PLK_ERR_RANGE
    if plonkhip.device_count() == 0:
        arr = (MulShortRun * 2)(_run(so=16, count=1 << 23), _run(so=16, count=1 << 23))
        assert lib.plk_poly_mul_short_batch_dev(arr, 2, None, None) == PLK_ERR_NODEV


def test_valid_call_without_a_gpu_is_nodev():
    if plonkhip.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(plonkhip.PlonkHipError) as e:
        plonkhip.poly_mul_short_batch([([1, 2, 3, 4], [1, 1])])
    assert e.value.code == PLK_ERR_NODEV
    lib = plonkhip.lib()
    for run in (_run(), _run(so=10, count=5), _run(la=MAX, lb=MAX), _run(la=MAX, lb=(1 << 32) - MAX),
                _run(la=1, lb=1, so=1, count=1 << 24)):
        assert lib.plk_poly_mul_short_batch_dev(C.byref(run), 1, None, None) == PLK_ERR_NODEV
        assert lib.plk_poly_mul_short_batch_dev(C.byref(run), 1, 1, None) == PLK_ERR_NODEV


# ---- the plan
def _ceil(a, b):
    return -(-a // b)


def test_plan_is_consistent():
    p = plonkhip.poly_mul_short_plan(1, 1)
    U, per_block = p["per_unit"], p["units_per_block"]
    assert p == {"per_unit": U, "units_per_product": 1, "units_per_block": per_block, "blocks": 1}
    assert U >= 64 and U % 64 == 0 and (U // 64) % 4 == 0 and per_block >= 1
    assert plonkhip.PLK_MUL_SHORT_LAUNCH_RUNS >= 1
    outs = (1, 2, U - 1, U, U + 1, 2 * U - 1, 2 * U, 2 * U + 1, 100 * U + 7, (1 << 32) - 1)
    for lo in outs:
        for ls in (1, 2, 5, 48, MAX - 1, MAX):
            ll = lo + 1 - ls
            if ll < 1:
                continue
            for la, lb in ((ls, ll), (ll, ls)):
                for count in (1, 2, per_block - 1, per_block, per_block + 1, 257, 1 << 16):
                    if count < 1 or (count > 300 and lo > 2 * U + 1) or (count > per_block + 1 and lo > 1 << 30):
                        continue                      # (kept inside one grid)
                    q = plonkhip.poly_mul_short_plan(la, lb, count)
                    assert q["per_unit"] == U and q["units_per_block"] == per_block, (la, lb, count)
                    assert q["units_per_product"] == _ceil(la + lb - 1, U), (la, lb, count)
                    assert q["blocks"] == _ceil(count * q["units_per_product"], per_block), (la, lb, count)
    assert plonkhip.poly_mul_short_plan(48, 48, 1 << 24)["blocks"] == _ceil(1 << 24, per_block)


def test_plan_errors():
    lib = plonkhip.lib()
    out = (C.c_int64 * 4)()
    assert lib.plk_poly_mul_short_plan(8, 3, 1, out) == PLK_OK
    assert lib.plk_poly_mul_short_plan(8, 3, 1, None) == PLK_ERR_ARG
    assert lib.plk_poly_mul_short_plan(0, 3, 1, out) == PLK_ERR_ARG
    assert lib.plk_poly_mul_short_plan(8, 0, 1, out) == PLK_ERR_ARG
    assert lib.plk_poly_mul_short_plan(8, 3, 0, out) == PLK_ERR_ARG
    assert lib.plk_poly_mul_short_plan(MAX + 1, MAX + 1, 1, out) == PLK_ERR_RANGE
    assert lib.plk_poly_mul_short_plan(MAX, MAX, 1, out) == PLK_OK
    assert lib.plk_poly_mul_short_plan(MAX, (1 << 32) - MAX, 1, out) == PLK_OK
    assert lib.plk_poly_mul_short_plan(MAX, (1 << 32) - MAX + 1, 1, out) == PLK_ERR_RANGE
    assert lib.plk_poly_mul_short_plan(1, 1, 1 << 24, out) == PLK_OK
    assert lib.plk_poly_mul_short_plan(1, 1, (1 << 24) + 1, out) == PLK_ERR_RANGE
    assert lib.plk_poly_mul_short_plan(MAX, 1 << 20, 1 << 16, out) == PLK_ERR_RANGE     # more blocks than a grid holds
    with pytest.raises(plonkhip.PlonkHipError) as e:
        plonkhip.poly_mul_short_plan(MAX + 1, MAX + 1)
    assert e.value.code == PLK_ERR_RANGE


# ---- the structure
def test_run_structure_layout(tmp_path):
    assert C.sizeof(MulShortRun) == 72
    names = [f[0] for f in MulShortRun._fields_]
    assert names == ["a", "la", "a_stride", "b", "lb", "b_stride", "out", "out_stride", "count"]
    (tmp_path / "l.c").write_text(
        '#include "plonkhip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
        "int main(void){ printf(\"%zu\", sizeof(plk_mulshort_run_t));\n"
        + "".join('  printf(" %%zu", offsetof(plk_mulshort_run_t, %s));\n' % n for n in names)
        + '  printf(" %d %d", PLK_MUL_SHORT_MAX, PLK_MUL_SHORT_LAUNCH_RUNS); return 0; }\n')
    r = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(tmp_path / "l")], capture_output=True, text=True).stdout.split()
    want = [C.sizeof(MulShortRun)] + [getattr(MulShortRun, n).offset for n in names] + \
        [plonkhip.PLK_MUL_SHORT_MAX, plonkhip.PLK_MUL_SHORT_LAUNCH_RUNS]
    assert [int(v) for v in out] == want


# ---- the model and the goldens
@pytest.fixture(scope="module")
def golden():
    return [(c["tag"],) + tuple(bytes.fromhex(c[k]) for k in ("a", "b", "out"))
            for c in load_golden("poly_mul_short.json")["cases"]]


def test_golden_covers_the_cases(golden):
    lens = {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 64}
    assert {t for t, *_ in golden} == {"t", "zero", "ztop", "raw"}
    assert {len(a) for t, a, _, _ in golden if t == "t"} == lens == {len(b) for t, _, b, _ in golden if t == "t"}
    assert max(max(len(a), len(b)) for _, a, b, _ in golden) == 64
    assert len(golden) > 2 * plonkhip.PLK_MUL_SHORT_LAUNCH_RUNS     # a ragged call of them crosses launches
    assert all(o == b"\0" for t, _, _, o in golden if t == "zero")
    assert all(len(o) < len(a) + len(b) - 1 for t, a, b, o in golden if t == "ztop")
    assert all(max(a + b) < 17 for t, a, b, _ in golden if t != "raw")
    raw = [a + b for t, a, b, _ in golden if t == "raw"]
    assert all(max(x) >= 17 for x in raw)
    for v in (0xFF, 0xEE, 0xA5, 17, 33, 34):
        assert any(v in x for x in raw), v
    assert os.path.getsize(os.path.join(HERE, "golden", "poly_mul_short.json")) <= \
        os.path.getsize(os.path.join(HERE, "golden", "divide_short.json"))


def test_model_matches_the_goldens(golden):
    for g, (tag, a, b, out) in enumerate(golden):
        p = M.product(a, b)
        assert len(p) == len(a) + len(b) - 1 and M.trimmed(p) == out, (g, tag)
        assert M.product(b, a) == p, (g, tag)


def test_model_matches_the_oracle(oracle):
    import numpy as np
    rng = np.random.default_rng(0x4D53)
    for it in range(60):
        la, lb = int(rng.integers(1, 200)), int(rng.integers(1, 1500))
        a = rng.integers(0, 17, la).astype(np.uint8)
        b = rng.integers(0, 17, lb).astype(np.uint8)
        if it % 7 == 0:
            a[la // 2:] = 0
        assert M.trimmed(M.product(a, b)) == oracle.poly_mul(a, b), (it, la, lb)
