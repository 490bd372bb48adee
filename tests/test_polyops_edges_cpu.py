"""The oracle restatement (oracle/oracle.c) equals the reference compiled from its unmodified headers
(oracle/_ref/libplonkref.so) at every input of tests/polyops_edge_cases.py: the chain
reference -> oracle -> kernel (tests/test_polyops_edges_gpu.py) holds at sizes the goldens never
reached.  poly_eval, poly_divide, matrix_mul and matrix_inv byte for byte; interpolate has no
reference function at general n, so it is pinned as matrix_mul(M, n, n, v, 1) (the trim is
polyops_edge_cases.trimmed)."""
import os

import pytest

import polyops_edge_cases as pe
from conftest import ROOT

REFLIB = os.path.join(ROOT, "oracle", "_ref", "libplonkref.so")


@pytest.fixture(scope="module")
def ref():
    assert os.path.exists(REFLIB), "%s missing: `make -C oracle` where /root/reference exists" % REFLIB
    from pyoracle import Reference
    return Reference(REFLIB)


def test_eval_cases(oracle, ref):
    n = 0
    for p, x in pe.eval_all_host_arrays():
        assert oracle.poly_eval(p, x) == ref.poly_eval(p, x), (p.size, x)
        n += 1
    assert n > 1000


def test_one_hot_expectation_is_the_references(ref):
    """the Python-integer expectation of the position-weight test is what the reference computes"""
    for idx in (pe.ONE_HOT_SMALL, pe.ONE_HOT_LARGE):
        polys, xs, want = pe.eval_one_hot(idx)
        assert [ref.poly_eval(p, x) for p, x in zip(polys, xs)] == want


def test_raw_eval_cases_depend_on_the_byte_arithmetic(oracle):
    """the cases meant for the serial loop give another value under arithmetic mod 17 (a block that
    failed to flag would show); bytes below 240 and a raw c_0 do not need the loop"""
    for name, p, x in pe.eval_raw_four_blocks():
        differs = oracle.poly_eval(p, x) != oracle.poly_eval(p % 17, x)
        if name.startswith(("d_", "e_")) or name in ("b_240_at_1/x3", "b_240_at_1/x16"):
            assert differs, name
        elif name.startswith("b_"):
            assert not differs, name
    polys, xs = pe.eval_raw_all_255()
    assert oracle.poly_eval(polys[0], xs[0]) != oracle.poly_eval(polys[0] % 17, xs[0])


def test_raw_numerator_cases_depend_on_the_byte_arithmetic(oracle):
    for m, kind in pe.DIVIDE_RAW_SHAPES:
        for name, num, den, _ in pe.divide_raw_numerator((m, kind), oracle):
            differs = oracle.poly_divide(num, den) != oracle.poly_divide(num % 17, den)
            assert differs == pe.raw_numerator_is_sensitive(name, m, num.size), name


@pytest.mark.parametrize("group", pe.DIVIDE_GROUPS)
def test_divide_cases(oracle, ref, group):
    n = 0
    for name, num, den, _ in pe.divide_groups(oracle)[group]():
        assert oracle.poly_divide(num, den) == ref.poly_divide(num, den), name
        n += 1
    assert n


def test_divide_groups_are_all_listed(oracle):
    assert set(pe.divide_groups(oracle)) == set(pe.DIVIDE_GROUPS)


def test_divide_device_shapes(oracle, ref):
    for name, num, den in pe.divide_device_shapes():
        assert oracle.poly_divide(num, den) == ref.poly_divide(num, den), name
        if name == "long_raw":
            assert oracle.poly_divide(num, den) != oracle.poly_divide(num % 17, den)


def test_exact_divisions_leave_no_remainder(oracle):
    got = [(name, oracle.poly_divide(num, den)[1]) for name, num, den, _ in pe.divide_trim(oracle) if "exact" in name]
    assert len(got) == 2 and all(r == b"\x00" for _, r in got), got


@pytest.mark.parametrize("shape", pe.MATRIX_MUL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matrix_mul_cases(oracle, ref, shape):
    m, k, n = shape
    a, b = pe.matrix_mul_case(m, k, n)
    assert oracle.matrix_mul(a, m, k, b, n) == ref.matrix_mul(a, m, k, b, n)


@pytest.mark.parametrize("n", pe.MATRIX_INV_SIZES)
def test_matrix_inv_cases(oracle, ref, n):
    for variant in pe.MATRIX_INV_VARIANTS:
        mat = pe.matrix_inv_case(n, variant)
        assert oracle.matrix_inv(mat, n) == ref.matrix_inv(mat, n), variant


@pytest.mark.parametrize("n,variant", pe.INTERPOLATE_CASES)
def test_interpolate_cases(oracle, ref, n, variant):
    mat, v = pe.interpolate_case(n, variant)
    out = oracle.matrix_mul(mat, n, n, v, 1)
    assert out == ref.matrix_mul(mat, n, n, v, 1)
    if variant == "tail_rows_zero":
        assert len(pe.trimmed(out)) <= n - 40
    if variant == "zero":
        assert pe.trimmed(out) == b"\x00"
