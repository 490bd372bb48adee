"""plk_poly_lincomb without a GPU: the numpy model against the reference's recorded outputs, the
host-only length query, and every argument error, which must come back before any device query."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_poly_lincomb_golden as mk  # noqa: E402
import poly_lincomb_model as M  # noqa: E402

import plonkhip  # noqa: E402
from plonkhip import LcJob, LcTerm, PLK_ERR_ARG, PLK_ERR_NODEV, PLK_ERR_RANGE, PLK_LC_RAW  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "poly_lincomb.json")) as f:
        return mk.expand(json.load(f))


def test_golden_covers_the_cases(golden):
    assert len(golden) == 512
    wild = sum(any(max(t["p"]) >= 17 for t in terms if t["scale"] == M.RAW and t["twist"] == 0) for terms, _, _ in golden)
    assert wild >= 165                                                  # about a third: arbitrary raw bytes
    assert sum(any(t["scale"] == 0 for t in terms) for terms, _, _ in golden) >= 32
    assert sum(len(terms) == 1 for terms, _, _ in golden) >= 16
    assert sum(len(terms) > 1 and o == b"\0" for terms, _, o in golden) >= 8   # cancelling terms
    assert {len(terms) for terms, _, _ in golden} == set(range(1, 17))
    assert max(len(t["p"]) for terms, _, _ in golden for t in terms) == 40
    assert max(t["shift"] for terms, _, _ in golden for t in terms) == 24


def test_model_matches_every_golden_entry(golden):
    for g, (terms, add_hf, ref) in enumerate(golden):
        out = M.lincomb(terms, add_hf)
        n = max(M.nz(out), 1)
        assert bytes(out[:n]) == ref and not out[n:].any(), g


# ---- the C ABI with no device
def _job(terms, add_hf=-1, out=1, keep=None):
    """terms: (p, len, shift, sub, scale, neg, twist) tuples with p a fake non-NULL pointer by default"""
    arr = (LcTerm * max(len(terms), 1))(*[LcTerm(*t) for t in terms])
    if keep is not None:
        keep.append(arr)
    return LcJob(arr, len(terms), add_hf, out)


def T(p=1, ln=4, shift=0, sub=0, scale=PLK_LC_RAW, neg=0, twist=0):
    return (p, ln, shift, sub, scale, neg, twist)


BAD = {
    "null terms": lambda: LcJob(None, 1, -1, 1),
    "null out": lambda: _job([T()], out=None),
    "null p": lambda: _job([T(p=None)]),
    "nterms 0": lambda: _job([], -1),
    "nterms 17": lambda: _job([T()] * 17),
    "len 0": lambda: _job([T(ln=0)]),
    "len 0 later": lambda: _job([T(), T(ln=0)]),
    "sub 2": lambda: _job([T(), T(sub=2)]),
    "neg 2": lambda: _job([T(neg=2)]),
    "scale 17": lambda: _job([T(scale=17)]),
    "scale 254": lambda: _job([T(scale=254)]),
    "twist 17": lambda: _job([T(twist=17)]),
    "add_hf -2": lambda: _job([T()], add_hf=-2),
    "add_hf 17": lambda: _job([T()], add_hf=17),
    "term 0 sub": lambda: _job([T(sub=1)]),
}


def test_len_values():
    L = plonkhip.lib().plk_poly_lincomb_len
    assert L(C.byref(_job([T(ln=1)]))) == 1
    assert L(C.byref(_job([T(ln=5, shift=3), T(ln=9)]))) == 9
    assert L(C.byref(_job([T(ln=5, shift=3), T(ln=7, sub=1, scale=0, neg=1, twist=16)], add_hf=16))) == 8
    assert L(C.byref(_job([T(ln=3)] * 15 + [T(ln=2, shift=1 << 20)]))) == (1 << 20) + 2
    assert L(C.byref(_job([T(ln=1, shift=(1 << 32) - 2)]))) == (1 << 32) - 1
    assert L(C.byref(_job([T(ln=40, shift=24)], out=None))) == 64          # out is not read
    assert L(None) == 0


@pytest.mark.parametrize("name", sorted(set(BAD) - {"null out"}))
def test_len_is_zero_for_bad_arguments(name):
    assert plonkhip.lib().plk_poly_lincomb_len(C.byref(BAD[name]())) == 0, name


@pytest.mark.parametrize("name", sorted(BAD))
def test_arg_errors_need_no_device(name):
    lib = plonkhip.lib()
    n = C.c_size_t(0)
    assert lib.plk_poly_lincomb(C.byref(BAD[name]()), C.byref(n)) == PLK_ERR_ARG, name
    assert lib.plk_poly_lincomb_batch_dev(C.byref(BAD[name]()), 1, None, None) == PLK_ERR_ARG, name
    # a bad job behind a good one is found as well
    arr = (LcJob * 2)(_job([T()]), BAD[name]())
    assert lib.plk_poly_lincomb_batch_dev(arr, 2, None, None) == PLK_ERR_ARG, name


def test_null_and_count_errors():
    lib = plonkhip.lib()
    n = C.c_size_t(0)
    good = _job([T()])
    assert lib.plk_poly_lincomb(None, C.byref(n)) == PLK_ERR_ARG
    assert lib.plk_poly_lincomb(C.byref(good), None) == PLK_ERR_ARG
    assert lib.plk_poly_lincomb_batch_dev(None, 1, None, None) == PLK_ERR_ARG
    assert lib.plk_poly_lincomb_batch_dev(C.byref(good), 0, None, None) == PLK_ERR_ARG
    assert lib.plk_poly_lincomb_batch_dev(C.byref(good), -3, None, None) == PLK_ERR_ARG


@pytest.mark.parametrize("ln,shift", [(1 << 32, 0), (1, (1 << 32) - 1), (1 << 31, 1 << 31), (5, (1 << 64) - 3)])
def test_range_errors_need_no_device(ln, shift):
    lib = plonkhip.lib()
    n = C.c_size_t(0)
    job = _job([T(), T(ln=ln, shift=shift)])
    assert lib.plk_poly_lincomb(C.byref(job), C.byref(n)) == PLK_ERR_RANGE
    assert lib.plk_poly_lincomb_batch_dev(C.byref(job), 1, None, None) == PLK_ERR_RANGE
    # an argument error anywhere in the batch comes first
    arr = (LcJob * 2)(job, BAD["len 0"]())
    assert lib.plk_poly_lincomb_batch_dev(arr, 2, None, None) == PLK_ERR_ARG


def test_valid_call_without_a_gpu_is_nodev():
    if plonkhip.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(plonkhip.PlonkHipError) as e:
        plonkhip.poly_lincomb(([plonkhip.lc_term([1, 2, 3]), plonkhip.lc_term([4, 5], shift=2, scale=3)], None))
    assert e.value.code == PLK_ERR_NODEV
    buf = np.zeros(8, np.uint8)
    keep = []
    job = _job([T(p=buf.ctypes.data, ln=8)], out=buf.ctypes.data, keep=keep)
    assert plonkhip.lib().plk_poly_lincomb_batch_dev(C.byref(job), 1, None, None) == PLK_ERR_NODEV
