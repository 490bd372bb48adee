"""Stage A of the circuit-form prover (gate check, copy constraints to roots, the interpolations, round 2's
grand product, the acc_x(omega^n) == 1 assert) on the device, in both of its implementations: the single call
plk_prover_prove (prove.hip) and the fused batch kernel (prove_batch.hip).  Random circuits at n = 1..16 with
the outcomes the compiled reference recorded in tests/golden/prove_circuits.json -- proofs byte for byte, exits
by message, code and gate index -- and fresh circuits against the restatement oracle/prove_ref.py."""
import numpy as np
import pytest
import torch

import gen
import prove_circuit_cases as pc
from conftest import load_golden

pytestmark = pytest.mark.gpu

_SETS = {}


def _sets():
    if not _SETS:
        _SETS.update(pc.expand(load_golden("prove_circuits.json")))
    return _SETS


def _keys(n):
    return [k for k, v in _sets().items() if v[0] == n]


def _prover(hip, n, s):
    return hip.Prover(n, s["z_h"], s["g1s"], s["h"], s["k1_h"], s["k2_h"], s["h_pows_inv"])


def _kw(n, c):
    g, cp, w = c["gates"], c["copies"], c["wires"]
    return dict(q_m=g[0:n], q_l=g[n:2 * n], q_r=g[2 * n:3 * n], q_o=g[3 * n:4 * n], q_c=g[4 * n:5 * n],
                copy_a=cp[0:2 * n], copy_b=cp[2 * n:4 * n], copy_c=cp[4 * n:6 * n], a=w[0:n], b=w[n:2 * n],
                c=w[2 * n:3 * n], chal=c["chal"], rand=c["rand"])


def _code(hip, outcome):
    return hip.PLK_ERR_RANGE if outcome.split()[0] in pc.RANGE_EXITS else hip.PLK_ERR_ARG


def _word(hip, outcome):
    """the batch status word of a recorded outcome: code, exit number, gate index in bits 16-31"""
    if pc.is_proof(outcome):
        return 0
    name, _, gate = outcome.partition(" ")
    return _code(hip, outcome) | (pc.EXIT_NUMBER[name] << 8) | (int(gate or 0) << 16)


def _single_diff(hip, pr, n, c, want):
    """'' if prove() gives the recorded proof or takes the recorded exit (text, code, gate index), else what differs"""
    try:
        got = pr.prove(**_kw(n, c)).hex()
    except hip.PlonkHipError as e:
        if e.code not in (hip.PLK_ERR_ARG, hip.PLK_ERR_RANGE):
            raise                     # not a reference exit: a runtime failure ends the test
        text = str(e).split("): ", 1)[1]
        if pc.is_proof(want):
            return "raised %r, want proof %s" % (text, want)
        if text != pc.message(want) or e.code != _code(hip, want):
            return "raised %r (code %d), want %r (code %d)" % (text, e.code, pc.message(want), _code(hip, want))
        return ""
    return "" if got == want else "proof %s, want %s" % (got, want)


def _entries(cases):
    return (b"".join(gen.circuit_bytes(c) for c in cases), np.array([c["chal"] for c in cases], np.uint8),
            np.array([c["rand"] for c in cases], np.uint8))


def _batch_diff(hip, proofs, status, want):
    """want: an outcome per entry; entry -> what differs (proof bytes, status word, its text, zeroed rejections)"""
    assert len(proofs) == 34 * len(want) and len(status) == len(want)
    bad = {}
    for i, w in enumerate(want):
        st, got = int(status[i]), proofs[34 * i:34 * i + 34]
        if pc.is_proof(w):
            if st != 0 or got.hex() != w:
                bad[i] = "status 0x%x proof %s, want proof %s" % (st, got.hex(), w)
        elif st != _word(hip, w) or hip.prove_exit_message(st) != pc.message(w) or got != bytes(34):
            bad[i] = "status 0x%x proof %s, want %s (status 0x%x)" % (st, got.hex(), w, _word(hip, w))
    return bad


def _outcomes(cases):
    return [c["outcome"] for c in cases]


# ------------------------------------------------------------------ recorded cases, single calls
def _single_sweep(hip, n):
    bad, ran = [], 0
    for key in _keys(n):
        _, s, cases = _sets()[key]
        pr = _prover(hip, n, s)
        for c in cases:
            d = _single_diff(hip, pr, n, c, c["outcome"])
            if d:
                bad.append((key, c["kind"], c["seed"], d))
        ran += len(cases)
        pr.close()
    return bad, ran


@pytest.mark.parametrize("n", range(1, 17))
def test_single_calls_match_the_reference(hip, n):
    """every recorded case of every setup at n through plk_prover_prove: circuit_check_kernel, interpolate_kernel,
    grand_product_kernel and the acc_x exit of prove.hip"""
    bad, ran = _single_sweep(hip, n)
    assert ran >= 30
    assert not bad, (len(bad), bad[:8])


def test_single_calls_n4_commitments_in_g1_form(hip):
    with hip.options(PROVE_SRS_LOGS=0):
        bad, ran = _single_sweep(hip, 4)
    assert ran >= 250
    assert not bad, (len(bad), bad[:8])


def test_acc_exit_is_taken_on_the_device(hip):
    """at n = 4 (and 1) acc_x(omega^n) is acc[0] = 1 whatever the circuit; here the assert fails at n = 2, 3 and
    16, in the single call and as status word PLK_ERR_ARG | X_ACC << 8"""
    for n in (2, 3, 16):
        _, s, cases = _sets()[pc.long_key(n)]
        acc = [c for c in cases if c["outcome"] == "ACC"]
        assert len(acc) >= 8
        pr = _prover(hip, n, s)
        with pytest.raises(hip.PlonkHipError) as e:
            pr.prove(**_kw(n, acc[0]))
        assert e.value.code == hip.PLK_ERR_ARG and str(e.value).endswith(pc.MESSAGES["ACC"])
        proofs, status = pr.prove_batch(*_entries(acc))
        assert all(int(x) == hip.PLK_ERR_ARG | (4 << 8) for x in status) and proofs == bytes(34 * len(acc))
        pr.close()


# ------------------------------------------------------------------ recorded cases, batches
@pytest.mark.parametrize("n", range(1, 17))
def test_batches_match_the_reference(hip, n):
    """every setup at n as ONE prove_batch call in file order (proofs and exits interleaved), compared with the
    recorded outcomes themselves, not with the single call"""
    for key in _keys(n):
        _, s, cases = _sets()[key]
        pr = _prover(hip, n, s)
        assert pr.batch_path() == 1
        proofs, status = pr.prove_batch(*_entries(cases))
        bad = _batch_diff(hip, proofs, status, _outcomes(cases))
        assert not bad, (key, len(bad), {i: (cases[i]["kind"], cases[i]["seed"], v) for i, v in list(bad.items())[:8]})
        if key == pc.long_key(n):
            assert np.any(status == 0) and np.any(status != 0)
        pr.close()


def _dev_batch(hip, pr, cases, stream):
    cir, ch, rd = _entries(cases)
    batch = len(cases)
    d = [torch.from_numpy(np.frombuffer(cir, np.uint8).copy()).to("cuda"), torch.from_numpy(ch.reshape(-1)).to("cuda"),
         torch.from_numpy(rd.reshape(-1)).to("cuda")]
    proofs = torch.full((34 * batch,), 0xEE, dtype=torch.uint8, device="cuda")
    status = torch.full((batch,), -1, dtype=torch.int32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())     # the copies and fills above
    pr.prove_batch_dev(d[0], d[1], d[2], batch, proofs, status, stream=stream)
    stream.synchronize()
    return proofs.cpu().numpy().tobytes(), status.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("n", [1, 5, 16])
def test_device_batches_on_a_side_stream(hip, n):
    """prove_batch_dev over prefilled outputs (0xEE / -1): the recorded outcomes, which are the host form's bytes"""
    _, s, cases = _sets()[pc.long_key(n)]
    pr = _prover(hip, n, s)
    proofs, status = _dev_batch(hip, pr, cases, torch.cuda.Stream())
    assert not _batch_diff(hip, proofs, status, _outcomes(cases))
    hp, hs = pr.prove_batch(*_entries(cases))
    assert proofs == hp and np.array_equal(status, hs)
    pr.close()


def test_batch_past_the_grid_stride(hip):
    """the n = 16 set repeated to 4099 entries: every block carries proofs and exits of the largest n"""
    _, s, cases = _sets()[pc.long_key(16)]
    many = [cases[i % len(cases)] for i in range(4099)]
    pr = _prover(hip, 16, s)
    assert pr.batch_path() == 1
    proofs, status = pr.prove_batch(*_entries(many))
    bad = _batch_diff(hip, proofs, status, _outcomes(many))
    assert not bad, (len(bad), list(bad.items())[:8])
    pr.close()


# ------------------------------------------------------------------ order of exits
@pytest.mark.parametrize("n", [2, 3])
def test_order_of_exits_on_short_srs(hip, n):
    """check_status's order SRS(a, b, c) < ACC < SRS(z), as the reference recorded it: a_x has n + 2 coefficients
    (b1 != 0) and z_x n + 3 (b7 != 0).  A failing acc check: n + 1 points give the SRS exit, n + 2 the ACC exit
    (z does not fit either, the assert comes first); a passing one: n + 2 points give the SRS exit."""
    sets = _sets()
    fails, passes = pc.order_cases(sets, n)
    for key, want in ((pc.key_of(n, n, 1), {"SRS"}), (pc.key_of(n, n + 1, 1), {"SRS", "ACC"})):
        _, s, cases = sets[key]
        by = {(c["kind"], c["seed"]): c["outcome"] for c in cases}
        assert {by[k] for k in fails + passes} == want and len(s["g1s"]) == 3 * int(key.split("/")[1]) + 3
        if key == pc.key_of(n, n + 1, 1):
            assert all(by[k] == "ACC" for k in fails) and all(by[k] == "SRS" for k in passes)
        pr = _prover(hip, n, s)
        assert pr.batch_path() == 1
        bad = [(c["kind"], c["seed"], d) for c in cases for d in [_single_diff(hip, pr, n, c, c["outcome"])] if d]
        assert not bad, (key, bad)
        proofs, status = pr.prove_batch(*_entries(cases))
        assert not _batch_diff(hip, proofs, status, _outcomes(cases)), key
        assert [int(x) for x in status] == [_word(hip, o) for o in _outcomes(cases)]
        pr.close()


# ------------------------------------------------------------------ copy indices the reference leaves undefined
@pytest.mark.parametrize("n", [4, 16])
def test_copy_index_out_of_range(hip, oracle, n):
    """a copy index of 0 or n + 1 (the reference reads out of bounds there): the COPY exit in both forms, GATE
    where a gate fails too, as include/plonkhip.h ("bad copy") and the restatement define it; the recorded
    proofs around them in the batch stay what they were"""
    _, s, cases = _sets()[pc.long_key(n)]
    good = [c for c in cases if pc.is_proof(c["outcome"])][:5]
    assert len(good) == 5
    changed = []
    for base, (slot, idx, gate) in zip(good, ((0, 0, None), (3 * n - 1, n + 1, None), (n + 1, 0, None),
                                              (2 * n, n + 1, n - 1), (n - 1, 0, 0))):
        c = dict(base, copies=list(base["copies"]), gates=list(base["gates"]))
        c["copies"][2 * slot + 1] = idx
        if gate is not None:
            c["gates"][4 * n + gate] = (c["gates"][4 * n + gate] + 1) % 17       # q_c of that gate
        c["outcome"] = "COPY" if gate is None else "GATE %d" % gate
        assert pc.restated(oracle, n, s, c) == c["outcome"]
        changed.append(c)
    entries = [x for pair in zip(good, changed) for x in pair] + [good[0]]
    pr = _prover(hip, n, s)
    bad = [d for c in entries for d in [_single_diff(hip, pr, n, c, c["outcome"])] if d]
    assert not bad, bad
    with pytest.raises(hip.PlonkHipError) as e:
        pr.prove(**_kw(n, changed[0]))
    assert e.value.code == hip.PLK_ERR_ARG and str(e.value).endswith("Invalid copy_of type")
    proofs, status = pr.prove_batch(*_entries(entries))
    assert not _batch_diff(hip, proofs, status, _outcomes(entries))
    assert int(status[1]) == hip.PLK_ERR_ARG | (2 << 8) and int(status[7]) == hip.PLK_ERR_ARG | (1 << 8) | ((n - 1) << 16)
    pr.close()


# ------------------------------------------------------------------ unrecorded circuits against the restatement
FRESH_SEED = 1 << 20          # the fixture's seeds are below 1500
FRESH_KINDS = ("respect17", "perm", "respect3", "map", "identity", "mixed", "degenerate", "respect17", "gate2", "copy3")


@pytest.mark.parametrize("n", [2, 4, 7, 16])
def test_fresh_circuits_against_the_restatement(hip, oracle, n):
    """40 circuits the fixture does not hold, answered by oracle/prove_ref.py in the test: the device cannot pass
    by having been fitted to the file"""
    sets = _sets()
    _, s, recorded = sets[pc.long_key(n)]
    kinds = ("respect17", "respect3") if n == 4 else FRESH_KINDS
    fresh = []
    for i in range(40):
        kind, seed = kinds[i % len(kinds)], FRESH_SEED + i
        c = gen.prove_circuit(n, kind, seed)
        c.update(kind=kind, seed=seed)
        c["outcome"] = pc.restated(oracle, n, s, c)
        fresh.append(c)
    assert all(c["seed"] < FRESH_SEED for _, _, cases in sets.values() for c in cases)
    entry = lambda c: gen.circuit_bytes(c) + bytes(c["chal"]) + bytes(c["rand"])   # noqa: E731
    assert not {entry(c) for c in fresh} & {entry(c) for c in recorded} and len({entry(c) for c in fresh}) == 40
    if n == 4:
        assert sum(pc.is_proof(c["outcome"]) for c in fresh) >= 15
    else:
        assert len({c["outcome"].split()[0] for c in fresh if not pc.is_proof(c["outcome"])}) >= 3
    pr = _prover(hip, n, s)
    assert pr.batch_path() == 1
    proofs, status = pr.prove_batch(*_entries(fresh))
    bad = _batch_diff(hip, proofs, status, _outcomes(fresh))
    assert not bad, {i: (fresh[i]["kind"], fresh[i]["seed"], v) for i, v in bad.items()}
    pr.close()
