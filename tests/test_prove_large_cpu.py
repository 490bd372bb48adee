"""tests/golden/prove_large.json (the CPU oracle's proofs at the gate counts where the device
prover's round-3 plan switches, made by tests/golden/make_prove_large.py): the file has the
shape tests/test_prove_large_gpu.py relies on, its smallest entry is what the oracle computes
today (so the maker and the file cannot drift apart), and the expected-launch table of
tests/prove_large_cases.py follows from the plan rules restated there."""
import importlib.util
import os

import prove_large_cases as PL
from conftest import GOLDEN, load_golden


def _maker():
    spec = importlib.util.spec_from_file_location("make_prove_large", os.path.join(GOLDEN, "make_prove_large.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_prove_large_file_shape():
    g = load_golden("prove_large.json")
    cases = g["cases"]
    assert [(c["n"], c["seed"]) for c in cases] == _maker().CASES
    assert len({(c["n"], c["seed"]) for c in cases}) == len(cases) == 12
    for c in cases:
        assert c["srs_len"] == 2 * c["n"] + 8 and c["oracle_seconds"] > 0
        assert (c["proof"] is None) != (c["exit"] is None)
        if c["proof"] is not None:
            assert len(bytes.fromhex(c["proof"])) == 34
    exits = [(c["n"], c["seed"], c["exit"]) for c in cases if c["exit"]]
    assert exits == [(600000, 51, "Invalid slice indices in poly_slice")]
    # every gate count has its expected plan, and the largest is the documented limit
    assert {c["n"] for c in cases} == set(PL.LAUNCHES)
    assert max(PL.LAUNCHES) == PL.N_MAX


def test_prove_large_smallest_entry_reproduced():
    """n = 131072 again through the maker's own function (~2 s of oracle time)"""
    want = load_golden("prove_large.json")["cases"][0]
    got = _maker().run_case((want["n"], want["seed"]))
    assert want["n"] == 131072
    assert {k: got[k] for k in ("n", "seed", "srs_len", "proof", "exit")} == \
           {k: want[k] for k in ("n", "seed", "srs_len", "proof", "exit")}


def test_launch_table_follows_from_the_plan_rules():
    for n, want in PL.LAUNCHES.items():
        assert PL.prover_launches(n) == want, n
    for n, used in PL.QM_TRANSFORM_USED.items():
        assert PL.qm_transform_used(n) == used, n
    # the switches sit where the table's comments say
    assert PL.prover_launches(PL.N_MAX + 1) is None
    assert (2 * PL.N_MAX + 3) * 256 < PL.PBB <= (2 * (PL.N_MAX + 1) + 3) * 256
    assert 3 * (1223336 + 2) * 128 < PL.P29 <= 3 * (1223337 + 2) * 128
    assert (2 * 1835006 + 3) * 128 < PL.P29 <= (2 * 1835007 + 3) * 128
    assert (3 * 1223337 + 3) * 128 < PL.P29 <= (3 * 1223338 + 3) * 128   # the t_2 group's range
    assert PL.prover_batches(1398106)[1] == [(23, 13, PL.F29, 2, 2), (22, 13, PL.F29, 1, 1)]   # 3n + 2 = 2^22 + 16
    assert PL.prover_batches(1398107)[1] == [(23, 13, PL.F29, 3, 3)]   # plans agree, range refuses
    assert {tb for _, tb, _, _, _ in PL.prover_launches(1 << 19)} == {12, 13}
    assert {tb for _, tb, _, _, _ in PL.prover_launches(1 << 18)} == {12}
    # the wrap range: 2n + 4 / 4n + 6 at e = 14, 16 and just unwrapped next to each other
    assert PL.product_plan(4098 + 2, 4098 + 3) == (13, 8) and PL.product_plan(2 * 4098 + 3, 2 * 4098 + 4) == (14, 14)
    assert PL.product_plan(4102 + 2, 4102 + 3) == (13, 16) and PL.product_plan(4103 + 2, 4103 + 2) == (14, 0)
    assert PL.product_plan(2 * 4099 + 3, 2 * 4099 + 4) == (15, 0)
