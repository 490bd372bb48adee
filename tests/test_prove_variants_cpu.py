"""The placement lists of tests/prove_variant_cases.py reach every kernel choice of the device
prover's rounds(), the derived launch model is consistent, and every size has an instance that the
oracle proves (no GPU)."""
import numpy as np
import pytest

import gen
import prove_variant_cases as V
from prove_ref import Prover as RefProver, ProveError
from prove_strict_case import strict_case


def _all_cases():
    for n in V.SIZES:
        for name, res in V.placements(n):
            yield n, name, res


def test_lists_are_what_the_issue_sets():
    assert len(V.SINGLE) == 39 and len(V.TOGETHER) == 5 and len(V.MIXES) == 16
    assert {r for _, res in V.SINGLE for r in res} == {0, 1, 4, 8}
    assert all(sum(1 for r in res if r) == 1 for _, res in V.SINGLE)
    assert [res[0] for _, res in V.TOGETHER] == [1, 2, 4, 8, 15]
    assert {r for _, res in V.MIXES for r in res} == {0, 1, 4, 8, 12, 15}
    assert len({res for _, res in V.MIXES}) == 16
    assert sorted(V.SIZES) == [1000, 1001, 1004, 1008, 1023, 4112, 8200, 20000]
    assert [n % 16 for n in sorted(V.SIZES)] == [8, 9, 12, 0, 15, 0, 8, 0]
    for n in V.SIZES:
        assert len(V.placements(n)) == (60 if n in V.SINGLE_SIZES else 21)
        la, lzx = n + 2, n + 3
        assert la <= lzx <= la + 1          # prep's length condition holds at every chosen size


def test_every_variant_both_ways():
    seen = {k: set() for k in ("prep", "numdiv", "fuse5", "agg")}
    vec = set()
    for n, _, res in _all_cases():
        for k, v in V.variants(n, res).items():
            seen[k].add(v)
        vec |= set(V.vec_modes(n, res).values())
    assert all(s == {True, False} for s in seen.values()), seen
    assert vec == {0, 1, 2}
    # an address 0 mod 4 but not 0 mod 16: the numerator stays fused, everything else falls back
    v = V.variants(1008, (4,) * 13)
    assert v == dict(prep=False, numdiv=True, fuse5=False, agg=False)
    # one polynomial moves exactly the switches that read it
    assert V.variants(1008, V.only(V.QC)) == dict(prep=True, numdiv=False, fuse5=True, agg=True)
    assert V.variants(1008, V.only(V.QC, r=4)) == dict(prep=True, numdiv=True, fuse5=True, agg=True)
    assert V.variants(1008, V.only(V.QM)) == dict(prep=True, numdiv=True, fuse5=False, agg=False)
    assert V.variants(1008, V.only(V.FA)) == dict(prep=False, numdiv=True, fuse5=True, agg=True)
    assert V.variants(1008, V.only(V.S1)) == dict(prep=False, numdiv=True, fuse5=False, agg=False)
    assert V.variants(1008, V.only(V.L1)) == dict(prep=True, numdiv=True, fuse5=True, agg=True)
    assert V.vec_modes(1008, V.only(V.L1))[V.L1] == 0 and V.vec_modes(1000, V.ALIGNED)[V.L1] == 1


def test_launch_model():
    for n in V.SIZES:
        for opt in [None] + V.OPTION_SETS:
            assert V.launch_delta(n, V.ALIGNED, opt) == 0
    # derived by hand from rounds(): all thirteen at an odd address
    #   prep 1 -> 1 + 4 + 3 + 1 + 8 = 17; numdiv 1 -> 3; round 5: 1 -> 2 + 2
    assert V.launch_delta(1008, (1,) * 13) == 16 + 2 + 3
    assert V.launch_delta(1008, (4,) * 13) == 16 + 0 + 3
    #   n % 16 != 0: round 5 is lincomb_batch (1) + 2 when aligned, one launch more when not
    assert V.launch_delta(1000, (1,) * 13) == 16 + 2 + 1
    #   n % 4 != 0: the numerator is never fused
    assert V.launch_delta(1001, (1,) * 13) == 16 + 0 + 1
    assert V.launch_delta(1008, V.only(V.QC)) == 2 and V.launch_delta(1008, V.only(V.QC, r=4)) == 0
    assert V.launch_delta(1001, V.only(V.QC)) == 0
    assert V.launch_delta(1008, V.only(V.L1)) == 0 and V.launch_delta(1008, V.only(V.S3)) == 16 - 2 + 0
    assert V.launch_delta(1008, V.only(V.FA)) == 1 + 4 + 3 + 1 + 1 - 1
    assert V.launch_delta(1008, V.only(V.ACC)) == 1 + 4 + 1 + 1 + 1 - 1
    assert V.launch_delta(1008, V.only(V.QM)) == 3 and V.launch_delta(1000, V.only(V.QM)) == 1
    deltas = {V.launch_delta(n, res) for n, _, res in _all_cases()}
    assert len(deltas) >= 8, deltas


@pytest.mark.parametrize("n", sorted(V.SIZES))
def test_oracle_proves_every_size(oracle, n):
    """the fixed seed gives a proof (a size whose seed exits is a failure, not a skip), with no
    degenerate challenge"""
    polys, chal, rnd, zh, pts = gen.prove_instance(n, V.SIZES[n], 2 * n + 8)
    assert all(chal) and chal[3] > 1, chal
    ref = RefProver(oracle, pts.tobytes(), n, z_h=zh.tobytes())
    want = ref.rounds(polys, chal, rnd, strict=False)
    assert len(want) == 34
    with pytest.raises(ProveError, match="remainder"):
        ref.rounds(polys, chal, rnd, strict=True)


@pytest.mark.parametrize("n", sorted(V.STRICT))
def test_strict_instances(oracle, n):
    c = strict_case(oracle, n, V.STRICT[n])
    assert len(c["want"]) == 34 and np.any(c["polys"][V.QC]) and len(c["polys"][V.QC]) == n
