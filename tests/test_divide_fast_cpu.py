"""The routing of poly_divide without a GPU: PLK_OPT_DIVIDE_FAST_MIN and plk_poly_divide_path
(which path -- trivial, constant, binomial scan, the reference's loop on one thread, Newton inverse
over the exact products -- a divisor and numerator length take under the current options)."""
import numpy as np
import pytest

import plonkhip as h

# the measured crossover (profiles/divide_fast_crossover.txt): the smallest ladder size
# (nl - dl + 1) * dl at which the Newton path beat the one-thread loop, rounded up to a power of two
DEFAULT = 256

TRIVIAL, CONSTANT, BINOMIAL, SERIAL, NEWTON = range(5)


def _general(dl, seed=3):
    den = np.random.default_rng(seed).integers(0, 17, dl).astype(np.uint8)
    den[1] = den[-1] = 5   # a middle term: not binomial; a canonical non-zero lead
    return den


def test_option_default_and_range():
    assert h.OPTIONS["DIVIDE_FAST_MIN"] == 29
    assert h.get_option("DIVIDE_FAST_MIN") == DEFAULT
    for v in (0, 1):
        with h.options(DIVIDE_FAST_MIN=v):
            assert h.get_option("DIVIDE_FAST_MIN") == v
    assert h.get_option("DIVIDE_FAST_MIN") == DEFAULT
    with pytest.raises(h.PlonkHipError) as e:
        h.set_option("DIVIDE_FAST_MIN", -1)
    assert e.value.code == h.PLK_ERR_ARG
    assert h.get_option("DIVIDE_FAST_MIN") == DEFAULT


def test_path_classes():
    assert h.poly_divide_path([7], 100) == CONSTANT
    assert h.poly_divide_path([3, 1], 100) == BINOMIAL          # linear x - z
    assert h.poly_divide_path([16, 0, 0, 0, 1], 100) == BINOMIAL
    assert h.poly_divide_path([16, 0, 0, 0, 1], 5 * DEFAULT) == BINOMIAL   # never Newton: the scans are faster
    dl = 64
    den = _general(dl)
    above = DEFAULT // dl + dl                                  # ql = DEFAULT / dl + 1
    assert (above - dl + 1) * dl >= DEFAULT
    assert h.poly_divide_path(den, above) == NEWTON
    below = above - 2
    assert (below - dl + 1) * dl < DEFAULT
    assert h.poly_divide_path(den, below) == SERIAL
    assert h.poly_divide_path(den, above - 1) == NEWTON         # ql * dl == DEFAULT exactly
    raw = den.copy()
    raw[2] = 17                                                 # = 0 mod 17, but not a canonical byte
    assert h.poly_divide_path(raw, above) == SERIAL
    low = den.copy()
    low[-1] = 0                                                 # lead byte 0: the loop's own behaviour
    assert h.poly_divide_path(low, above) == SERIAL
    assert h.poly_divide_path(den, dl - 1) == TRIVIAL
    assert h.poly_divide_path([3, 1], 1) == TRIVIAL
    assert h.poly_divide_path([0, 0, 0], 100) == -h.PLK_ERR_ARG
    assert "Division by zero polynomial" in h.last_error()
    assert h.poly_divide_path([], 100) == -h.PLK_ERR_ARG
    assert h.poly_divide_path([1, 2, 20], 100) == -h.PLK_ERR_RANGE


def test_forced_and_off():
    den3 = np.array([1, 2, 3], np.uint8)
    shapes = [(den3, 3), (den3, 4), (_general(64), 1 << 20), (_general(1 << 12), 1 << 13), (_general(5), 5 << 20)]
    with h.options(DIVIDE_FAST_MIN=1):
        for den, nl in shapes:
            assert h.poly_divide_path(den, nl) == NEWTON, (den.size, nl)
        assert h.poly_divide_path(den3, 2) == TRIVIAL
        assert h.poly_divide_path([3, 1], 100) == BINOMIAL
        assert h.poly_divide_path([1, 2, 17, 3], 100) == SERIAL
    with h.options(DIVIDE_FAST_MIN=0):
        for den, nl in shapes:
            assert h.poly_divide_path(den, nl) == SERIAL, (den.size, nl)


def test_workspace_covers_the_newton_buffers_whatever_the_option():
    """a caller who sized d_work once stays safe when the option changes: the size depends on the
    shape alone, and for shapes that could take the Newton path it holds g (2k), both reversed
    operands (k + min(dl, k)) and a product output (2k - 1) on top of the serial part"""
    for nl, dl in ((3, 3), (5000, 1500), (1537, 1500), (1 << 16, 1 << 15)):
        k = nl - dl + 1
        sizes = []
        for v in (0, 1, DEFAULT):
            with h.options(DIVIDE_FAST_MIN=v):
                sizes.append(h.poly_divide_workspace(nl, dl))
        assert len(set(sizes)) == 1
        assert sizes[0] >= nl + dl + 2 * k + k + min(dl, k) + 2 * k - 1 + h.poly_mul_workspace(k, k)
    # constants and linear divisors never take it: their workspace is what it was
    assert h.poly_divide_workspace(1 << 16, 2) < (1 << 16) + 4096
