"""Circuit-form prover, CPU side: tests/golden/prove_circuits.json (random circuits at n = 1..16 through
the compiled reference, tests/golden/make_prove_circuits.py) holds what it was built to hold, and the
restatement oracle/prove_ref.py gives every recorded proof and takes every recorded exit, so it can
answer for the device on circuits the file does not hold."""
import pytest

import prove_circuit_cases as pc
from conftest import load_golden
from pyoracle import Reference

_SETS = {}


def _sets():
    if not _SETS:
        _SETS.update(pc.expand(load_golden("prove_circuits.json")))
    return _SETS


def test_fixture_holds_what_it_was_built_to():
    """the counts of proofs and exits per n, the copy layouts at n = 4, the GATE / COPY exits and the
    order-of-exits cases: conditions, asserted as the maker asserts them"""
    g = load_golden("prove_circuits.json")
    sets = _sets()
    assert list(g["setups"]) == list(g["cases"]) == list(sets)
    per_n = pc.check_counts(sets)
    assert sum(sum(c.values()) for c in per_n.values()) >= 1000
    for key, (n, s, cases) in sets.items():
        srs_n = int(key.split("/")[1])
        assert len(s["h"]) == len(s["k1_h"]) == len(s["k2_h"]) == n and len(s["h_pows_inv"]) == n * n
        assert len(s["g1s"]) == 3 * (srs_n + 1) and len(s["z_h"]) <= n + 1
        assert list(s["h"]) == [pow(4, i, 17) for i in range(n)]
        assert len({(c["kind"], c["seed"]) for c in cases}) == len(cases)
    # every exit the circuit form can take on a long SRS is in the file, and both kinds of rejection mix with
    # proofs inside every long setup (the batches run a setup as one call)
    assert {k for c in per_n.values() for k in c} == {"proof", "GATE", "COPY", "ACC", "REM_T", "SLICE"}


def test_restatement_reproduces_every_recorded_case(oracle):
    bad = []
    for key, (n, s, cases) in _sets().items():
        for c in cases:
            got = pc.restated(oracle, n, s, c)
            if got != c["outcome"]:
                bad.append((key, c["kind"], c["seed"], got, c["outcome"]))
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("n", [4, 16])
def test_restatement_copy_index_out_of_range_is_the_copy_exit(oracle, n):
    """a copy index of 0 or n + 1 is undefined in the reference (read out of bounds); the device and the
    restatement define it as the COPY exit, after the gate check as for a bad copy type"""
    n_, s, cases = _sets()[pc.long_key(n)]
    base = next(c for c in cases if pc.is_proof(c["outcome"]))
    for slot, idx in ((0, 0), (3 * n - 1, n + 1), (n, 0), (n + 1, n + 1)):
        c = dict(base, copies=list(base["copies"]))
        c["copies"][2 * slot + 1] = idx
        assert pc.restated(oracle, n, s, c) == "COPY"
        c["gates"] = list(base["gates"])
        c["gates"][4 * n + n - 1] = (c["gates"][4 * n + n - 1] + 1) % 17       # q_c of the last gate
        assert pc.restated(oracle, n, s, c) == "GATE %d" % (n - 1)
    assert pc.restated(oracle, n, s, base) == base["outcome"]


@pytest.mark.skipif(not Reference.has_generic(), reason="needs the compiled reference (oracle/_ref) with ref_prove_n")
def test_generic_harness_entries_equal_the_four_gate_ones():
    R = Reference()
    for srs_n, mode in ((6, 0), (6, 1), (4, 0)):
        assert R.plonk_data(4, 2, srs_n, mode) == R.plonk4_data(2, srs_n, mode)
    toy = load_golden("prove.json")["proofs"]
    for case in toy[:4]:
        args = (case["gates"], case["copies"], case["wires"], case["chal"], case["rand"])
        kw = dict(secret=case["secret"], srs_n=case["srs_n"], srs_mode=case["srs_mode"])
        want = R.prove4(*args, **kw)
        assert want.hex() == case["proof"] and R.prove_n(4, *args, **kw) == (want, None, None)
    # one recorded case of each outcome through the compiled reference again
    seen = set()
    for key, (n, s, cases) in _sets().items():
        _, srs_n, mode = (int(x) for x in key.split("/"))
        for c in cases:
            what = "proof" if pc.is_proof(c["outcome"]) else c["outcome"].split()[0]
            if (n, what) in seen or n not in (2, 4, 16):
                continue
            seen.add((n, what))
            got = R.prove_n(n, c["gates"], c["copies"], c["wires"], c["chal"], c["rand"], 2, srs_n, mode)
            assert pc.outcome_text(*got) == c["outcome"], (key, c["kind"], c["seed"])
    assert len(seen) >= 12
