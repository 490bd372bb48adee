"""tests/golden/prove_circuits.json for the CPU and GPU tests of the circuit-form prover: its cases
expanded through gen.prove_circuit, the exits' texts and codes, and the counts the file must hold
(asserted by the maker when it writes the file and by the tests on the loaded file)."""
import collections

import gen
from prove_ref import Prover, ProveError

# a recorded exit by name -> the text check_status (prove.hip) sets, which is the restatement's too
MESSAGES = {
    "GATE": "Constraint %d not satisfied.",
    "COPY": "Invalid copy_of type",
    "SRS": "SRS length is less than polynomial length",
    "ACC": "assertion acc_x(omega^n) == 1 failed",
    "REM_T": "Non-zero remainder in t(x) division",
    "SLICE": "Invalid slice indices in poly_slice",
    "REM_W1": "assertion poly_is_zero(&rem1) failed",
    "REM_W2": "assertion poly_is_zero(&rem2) failed",
}
EXIT_NUMBER = {k: i + 1 for i, k in enumerate(MESSAGES)}          # the status word's bits 8-15 (plonkhip.h)
RANGE_EXITS = ("SRS", "SLICE")                                     # PLK_ERR_RANGE; the others PLK_ERR_ARG
TOY_COPIES = [1, 1, 1, 2, 1, 3, 2, 1, 0, 1, 0, 2, 0, 3, 2, 2, 0, 4, 1, 4, 2, 4, 2, 3]   # src/plonk-test.c


def outcome_text(proof, exit_name, gate):
    """what the fixture stores: the proof's hex, or 'ACC', 'REM_T', ..., 'GATE 3'"""
    if proof is not None:
        return bytes(proof).hex()
    return exit_name if gate is None else "%s %d" % (exit_name, gate)


def message(outcome):
    """None for a proof, else the exit's text with the gate index filled in"""
    name, _, gate = outcome.partition(" ")
    if name not in MESSAGES:
        return None
    return MESSAGES[name] % int(gate) if name == "GATE" else MESSAGES[name]


def is_proof(outcome):
    return outcome.partition(" ")[0] not in MESSAGES


def key_of(n, srs_n, srs_mode):
    return "%d/%d/%d" % (n, srs_n, srs_mode)


def long_key(n, srs_mode=1):
    """the setup whose SRS holds every commitment of an n-gate proof (2n + 3 points)"""
    return key_of(n, 2 * n + 2, srs_mode)


def expand(g):
    """setup key -> (n, setup bytes, [case dict with kind, seed, outcome and the circuit]) in file order"""
    out = collections.OrderedDict()
    for key in g["cases"]:
        n = int(key.split("/")[0])
        cases = []
        for kind, seed, outcome in g["cases"][key]:
            c = gen.prove_circuit(n, kind, seed)
            c.update(kind=kind, seed=seed, outcome=outcome)
            cases.append(c)
        out[key] = (n, {k: bytes.fromhex(v) for k, v in g["setups"][key].items()}, cases)
    return out


def restated(orc, n, s, c):
    """the restatement's outcome for one circuit dict, in the fixture's form"""
    ref = Prover(orc, s["g1s"], n, s["h"], s["k1_h"], s["k2_h"], s["h_pows_inv"], s["z_h"])
    gt, cp, w = c["gates"], c["copies"], c["wires"]
    copies = [list(zip(cp[2 * n * k:2 * n * (k + 1):2], cp[2 * n * k + 1:2 * n * (k + 1):2])) for k in range(3)]
    try:
        return ref.prove(*(gt[n * k:n * (k + 1)] for k in range(5)), copies, w[0:n], w[n:2 * n], w[2 * n:3 * n],
                         c["chal"], c["rand"]).hex()
    except ProveError as e:
        names = [k for k in MESSAGES if k != "GATE" and MESSAGES[k] == str(e)]
        if names:
            return names[0]
        assert str(e).startswith("Constraint ") and str(e).endswith(" not satisfied."), str(e)
        return "GATE %d" % int(str(e).split()[1])


def order_cases(sets, n):
    """the order-of-exits cases at n: (kind, seed) of the circuit whose acc check fails and of the one whose
    acc check passes, by their outcomes on the SRS of n + 2 points"""
    mid = {(c["kind"], c["seed"]): c["outcome"] for c in sets[key_of(n, n + 1, 1)][2]}
    fails = [k for k, o in mid.items() if o == "ACC"]
    passes = [k for k, o in mid.items() if o == "SRS"]
    return fails, passes


def check_counts(sets):
    """the conditions the fixture is built to (every one asserted); returns per n the Counter of outcomes"""
    per_n = collections.defaultdict(collections.Counter)
    for key, (n, s, cases) in sets.items():
        for c in cases:
            assert max(c["gates"] + c["wires"] + c["chal"] + c["rand"]) < 17, (key, c["kind"], c["seed"])
            assert all(t in (0, 1, 2, 3, 255) for t in c["copies"][0::2]) and all(1 <= i <= n for i in c["copies"][1::2])
            if key == long_key(n):
                per_n[n]["proof" if is_proof(c["outcome"]) else c["outcome"].split()[0]] += 1
    assert sorted(per_n) == list(range(1, 17))
    for n, cnt in per_n.items():
        if n == 4:
            continue
        assert cnt["proof"] >= 8 and cnt["REM_T"] >= 8, (n, cnt)
        assert cnt["ACC"] >= (0 if n == 1 else 8), (n, cnt)
    assert per_n[1]["ACC"] == 0 and per_n[4]["ACC"] == 0          # acc_x(omega^n) is acc[0] = 1 there
    # n = 4
    four = sets[long_key(4)][2]
    proofs = [c for c in four if is_proof(c["outcome"])]
    ident = [x for k in range(3) for i in range(1, 5) for x in (k, i)]
    assert len(proofs) >= 150 and len({gen.circuit_bytes(c) for c in proofs}) >= 100
    assert sum(c["copies"] not in (ident, TOY_COPIES) for c in proofs) >= 60
    assert sum(any(c["copies"][2 * s] != s // 4 for s in range(12)) for c in proofs) >= 40
    assert sum(c["outcome"] == "REM_T" and c["kind"] == "perm" for c in four) >= 30
    assert sum(c["outcome"] == "REM_T" and c["kind"] in ("respect17", "respect3") for c in four) >= 10
    assert long_key(4, 0) in sets and any(is_proof(c["outcome"]) for c in sets[long_key(4, 0)][2])
    # GATE and COPY exits
    every = [(n, c) for n, s, cases in sets.values() for c in cases]
    gates = [(n, c) for n, c in every if c["outcome"].startswith("GATE")]
    assert len(gates) >= 10 and len({n for n, c in gates}) >= 3
    two = 0
    for n, c in gates:
        failing = [i for i in range(n) if (c["gates"][n + i] * c["wires"][i] + c["gates"][2 * n + i] * c["wires"][n + i] +
                                           c["gates"][3 * n + i] * c["wires"][2 * n + i] +
                                           c["gates"][i] * c["wires"][i] * c["wires"][n + i] + c["gates"][4 * n + i]) % 17]
        assert failing and c["outcome"] == "GATE %d" % failing[0]
        two += len(failing) == 2
    assert two >= 2 and any(n == 16 and c["outcome"] == "GATE 15" for n, c in gates)
    copies = [c for n, c in every if c["outcome"] == "COPY"]
    assert len(copies) >= 5 and {t for c in copies for t in c["copies"][0::2]} >= {3, 255}
    assert any(c["kind"] == "copy_gate" and c["outcome"].startswith("GATE") for n, c in every)
    # order of exits: short SRS at n = 2, 3, a_x with n + 2 and z_x with n + 3 coefficients
    for n in (2, 3):
        fails, passes = order_cases(sets, n)
        assert fails and passes
        low = {(c["kind"], c["seed"]): c["outcome"] for c in sets[key_of(n, n, 1)][2]}
        full = {(c["kind"], c["seed"]): c for c in sets[long_key(n)][2]}
        for k in fails + passes:
            assert full[k]["rand"][0] and full[k]["rand"][6], k
        assert all(low[k] == "SRS" and full[k]["outcome"] == "ACC" for k in fails)
        assert all(full[k]["outcome"] not in ("ACC", "SRS") for k in passes)
    return per_n
