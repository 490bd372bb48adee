"""Sum groups of plk_poly_mul_batch_dev at the edges of the two fields' exact ranges.

A sum group (a leader and the members after it, added before ONE inverse transform) is exact
over F29 (p29 = 7 2^26 + 1, coefficients as centred residues in [-8, 8]) while
64 sum(min(la, lb)) <= (p29 - 1) / 2, i.e. up to sum(min) = 3,670,016 where the two are EQUAL,
and over BabyBear (pBB = 15 2^27 + 1, bytes as they are) while 256 sum(min) < pBB, i.e. up to
sum(min) = 7,864,320 where 256 sum(min) = pBB - 1; past that the batch returns PLK_ERR_RANGE.
The bound is on a sum over the group's products, and the members are added lazily (in the centre
launch, PLK_OPT_NTT_CENTER_SUM = 1, or in the first inverse pass, 0), so a centring or reduction
slip shows only with every term at the extreme: all-9 x all-9 (each term +64), all-9 x all-8
(-64), all-16 x all-16 (+256) at lengths whose full-overlap stretches meet.

References are closed forms in int64 numpy: constant x constant is a b cnt(i) with
cnt(i) = min(i + 1, la, lb, la + lb - 1 - i); constant x anything is a sliding-window sum."""
import numpy as np
import pytest

import gen
import prove_large_cases as PL
from test_polymul_gpu import _run_batch

pytestmark = pytest.mark.gpu

_REF = {}


def _cnt(la, lb):
    i = np.arange(la + lb - 1, dtype=np.int64)
    return np.minimum(np.minimum(i + 1, la), np.minimum(lb, la + lb - 1 - i))


def _operand(val, n, seed):
    if val == "r":     # uniform in [0, 17)
        return gen.poly_inputs(seed, n, 1)[0]
    return np.full(n, val, np.uint8)


def _product(av, a, b):
    """(constant av, len(a) long) x b over the integers mod 17"""
    la, lb = len(a), len(b)
    cs = np.concatenate([[0], np.cumsum(b, dtype=np.int64)])
    i = np.arange(la + lb - 1, dtype=np.int64)
    return av * (cs[np.minimum(i + 1, lb)] - cs[np.maximum(i - la + 1, 0)]) % 17


def _case(shapes, av, bv):
    """operands, the group's expected bytes and the largest number of terms any coefficient sums
    (computed once per case, shared by the NTT_CENTER_SUM settings)"""
    key = (tuple(shapes), av, bv)
    if key not in _REF:
        polys = []
        for m, (la, lb) in enumerate(shapes):
            polys += [_operand(av, la, 0), _operand(bv, lb, 700 + m)]
        full = shapes[0][0] + shapes[0][1] - 1
        want = np.zeros(full, np.int64)
        terms = np.zeros(full, np.int64)
        for m, (la, lb) in enumerate(shapes):
            assert la + lb - 1 <= full
            want[:la + lb - 1] += _product(av, polys[2 * m], polys[2 * m + 1])
            terms[:la + lb - 1] += _cnt(la, lb)
        if bv != "r":     # the two closed forms agree
            chk = sum(np.pad(av * bv * _cnt(la, lb), (0, full - (la + lb - 1))) for la, lb in shapes) % 17
            assert np.array_equal(chk, want % 17)
        _REF[key] = (polys, (want % 17).astype(np.uint8).tobytes(), int(terms.max()))
    return _REF[key]


def _run_logged(hip, polys, spec, csum):
    hip.ntt_launch_log()
    with hip.options(NTT_CENTER_SUM=csum, NTT_LAUNCH_LOG=1):
        try:
            outs = _run_batch(hip, polys, spec)
        finally:
            log = hip.ntt_launch_log()
    return outs, [(r["k"], r["field"], r["n"]) for r in log if r["kind"] == 2]


def _check_group(hip, shapes, av, bv, csum, k, field, bystander=None):
    """the group alone (or after one bystander product of its transform size) in one batch: the
    leader's output is the sum, the members' outputs are untouched, one centre launch of 2^k
    points in `field`"""
    smin = sum(min(s) for s in shapes)
    assert all(PL.product_plan(la, lb)[0] == k for la, lb in shapes)      # one transform size
    assert field == (PL.F29 if smin * 128 < PL.P29 else PL.BABYBEAR) and smin * 256 < PL.PBB
    polys, want, peak = _case(shapes, av, bv)
    assert peak == smin                          # some coefficient sums every term of every member
    polys = list(polys)
    spec = [(2 * m, 2 * m + 1, 1 if m else 0) for m in range(len(shapes))]
    if bystander:
        assert PL.product_plan(*bystander)[0] == k
        polys += [np.full(bystander[0], 3, np.uint8), np.full(bystander[1], 5, np.uint8)]
        spec = [(len(polys) - 2, len(polys) - 1, 0)] + spec
    outs, centres = _run_logged(hip, polys, spec, csum)
    assert centres == [(k, field, len(spec))]
    if bystander:
        assert outs[0] == (15 * _cnt(*bystander) % 17).astype(np.uint8).tobytes()
        outs = outs[1:]
    assert outs[0] == want
    for m in range(1, len(shapes)):
        assert outs[m] == b"\xEE" * (shapes[m][0] + shapes[m][1] - 1)


# sum(min) = 1223339 + 1223339 + 1223338 = 3,670,016: 64 sum(min) = (p29 - 1) / 2 exactly
_F29_3 = [(1223339, 1223345), (1223339, 1223340), (1223338, 1223340)]
_F29_3_OVER = [(1223339, 1223345), (1223339, 1223340), (1223339, 1223340)]     # 3,670,017
_F29_2 = [(1835008, 1835020), (1835008, 1835010)]                               # 3,670,016
_F29_2_OVER = [(1835008, 1835020), (1835009, 1835010)]
# the leader wrapped by 16 (la + lb - 1 = 2^22 + 16, the most), a member wrapped by 3, one not wrapped
_F29_WRAP = [(1223339, 2970982), (1223339, 1223340), (1223338, 2970970)]
# sum(min) = 3 x 2,621,440 = 7,864,320: 256 sum(min) = pBB - 1; 2^23-point transforms
_BB_3 = [(2621440, 5767169), (2621440, 5767000), (2621440, 5000000)]
_BB_3_OVER = [(2621440, 5767169), (2621440, 5767000), (2621441, 5000000)]


def test_edge_figures():
    assert 64 * sum(min(s) for s in _F29_3) == (PL.P29 - 1) // 2 == 64 * sum(min(s) for s in _F29_2)
    assert sum(min(s) for s in _F29_WRAP) == 3670016
    assert sum(min(s) for s in _F29_3_OVER) == sum(min(s) for s in _F29_2_OVER) == 3670017
    assert 256 * sum(min(s) for s in _BB_3) == PL.PBB - 1
    assert sum(min(s) for s in _BB_3_OVER) == 7864321
    assert [PL.product_plan(*s) for s in _F29_WRAP] == [(22, 16), (22, 0), (22, 3)]
    assert PL.product_plan(*_BB_3[0]) == (23, 0) and sum(_BB_3[0]) - 1 == 1 << 23


@pytest.mark.parametrize("csum", [0, 1])
@pytest.mark.parametrize("av,bv", [(9, 9), (9, 8), (9, "r")])
def test_f29_edge_three_members(hip, av, bv, csum):
    """every term +64 (9 = -8 centred, squared), every term -64 (-8 x 8), and 9 x random bytes for
    position sensitivity: peak sums +-(p29 - 1) / 2, still F29; a bystander product in the same
    launch is unharmed"""
    _check_group(hip, _F29_3, av, bv, csum, 22, PL.F29, bystander=(1100000, 1100001))


@pytest.mark.parametrize("csum", [0, 1])
@pytest.mark.parametrize("av,bv", [(9, 9), (9, 8)])
def test_f29_edge_three_members_one_more(hip, av, bv, csum):
    """one more coefficient in a member: sum(min) = 3,670,017, so the launch runs in BabyBear"""
    _check_group(hip, _F29_3_OVER, av, bv, csum, 22, PL.BABYBEAR)


@pytest.mark.parametrize("csum", [0, 1])
@pytest.mark.parametrize("av,bv", [(9, 9), (9, 8)])
def test_f29_edge_two_members(hip, av, bv, csum):
    _check_group(hip, _F29_2, av, bv, csum, 22, PL.F29)
    _check_group(hip, _F29_2_OVER, av, bv, csum, 22, PL.BABYBEAR)


@pytest.mark.parametrize("csum", [0, 1])
@pytest.mark.parametrize("av,bv", [(9, 9), (9, 8)])
def test_f29_edge_wrapped_leader(hip, av, bv, csum):
    """the largest wrapped shape leads: its top 16 coefficients come from the operands' ends, the
    cyclic sums below them carry the group's extreme"""
    _check_group(hip, _F29_WRAP, av, bv, csum, 22, PL.F29)


@pytest.mark.parametrize("csum", [0, 1])
@pytest.mark.parametrize("av,bv", [(16, 16), (16, "r")])
def test_babybear_edge_three_members(hip, av, bv, csum):
    """NTT_F29 at its default: the group is past F29's range, and in BabyBear all-16 x all-16 peaks
    at 256 x 7,864,320 = pBB - 1"""
    assert hip.get_option("NTT_F29") == 1
    _check_group(hip, _BB_3, av, bv, csum, 23, PL.BABYBEAR)


@pytest.mark.parametrize("csum", [0, 1])
def test_babybear_edge_refusals(hip, csum):
    """sum(min) = 7,864,321 in a group: PLK_ERR_RANGE ("exceeds both fields"); a single product
    with min = 7,864,321 in a batch: PLK_ERR_RANGE ("outside the exact range": the batch has no
    blocked path, plk_poly_mul runs such a shape blocked).  Both are refused before any launch."""
    polys = []
    for la, lb in _BB_3_OVER:
        polys += [np.full(la, 16, np.uint8), np.full(lb, 16, np.uint8)]
    hip.ntt_launch_log()
    with hip.options(NTT_CENTER_SUM=csum, NTT_LAUNCH_LOG=1):
        with pytest.raises(hip.PlonkHipError, match="exceeds both fields") as e:
            _run_batch(hip, polys, [(0, 1, 0), (2, 3, 1), (4, 5, 1)])
        assert e.value.code == hip.PLK_ERR_RANGE
        one = [np.full(4096, 16, np.uint8), np.full(4097, 16, np.uint8), np.full(7864321, 16, np.uint8)]
        with pytest.raises(hip.PlonkHipError, match="outside the exact range") as e:
            _run_batch(hip, one, [(0, 1, 0), (2, 2, 0)])
        assert e.value.code == hip.PLK_ERR_RANGE
        assert hip.ntt_launch_log() == []


def test_babybear_edge_single_job(hip):
    """the other side of the single-product refusal: min = 7,864,320 as a batch job is exact, its
    middle coefficient 256 x 7,864,320 = pBB - 1"""
    m = 7864320
    assert m * 256 == PL.PBB - 1 and PL.product_plan(m, m) == (24, 0)
    outs, centres = _run_logged(hip, [np.full(m, 16, np.uint8)], [(0, 0, 0)], 1)
    assert centres == [(24, PL.BABYBEAR, 1)]
    assert outs[0] == (_cnt(m, m) % 17).astype(np.uint8).tobytes()      # 256 = 1 mod 17
