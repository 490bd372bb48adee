"""Record tests/golden/prove_circuits.json from the REAL reference (oracle/_ref/libplonkref.so):
random circuits at n = 1..16 through srs_create + plonk_new(srs, n) + plonk_prove, each with the
proof it gave or the exit it took (ref_prove_n names the exit by the reference's own text).  Run
where the compiled reference exists:

    make -C oracle && python tests/golden/make_prove_circuits.py

Everything is seeded: a case is stored as (kind, seed) of gen.prove_circuit plus its outcome, under
the setup 'n/srs_n/srs_mode' it ran on, and a second run writes the same bytes.  The counts the file
is built to are asserted before it is written (tests/prove_circuit_cases.py check_counts; the CPU
test asserts them again on the loaded file).
"""
import collections
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import gen  # noqa: E402
import prove_circuit_cases as pc  # noqa: E402
from pyoracle import Reference  # noqa: E402

R = Reference()
SECRET = 2
BASE_KINDS = ("identity", "respect17", "respect3", "perm", "map", "degenerate", "mixed")
# n = 4: how many of each outcome to keep per kind (proofs / REM_T / SLICE)
FOUR = {"identity": (15, 3, 3), "respect17": (45, 8, 3), "respect3": (45, 8, 3), "perm": (25, 32, 3),
        "map": (15, 3, 3), "degenerate": (5, 3, 1), "mixed": (10, 3, 1)}


def run(n, kind, seed, srs_n, mode):
    c = gen.prove_circuit(n, kind, seed)
    return pc.outcome_text(*R.prove_n(n, c["gates"], c["copies"], c["wires"], c["chal"], c["rand"], SECRET, srs_n, mode))


def collect(n, srs_n, mode, caps, seeds):
    """per kind, seeds 0, 1, ... in order: a case is kept while its (kind, outcome) count is below caps(kind, what)"""
    cases = []
    for kind in BASE_KINDS:
        have = collections.Counter()
        for seed in range(seeds(kind)):
            out = run(n, kind, seed, srs_n, mode)
            what = "proof" if pc.is_proof(out) else out
            if have[what] < caps(kind, what):
                have[what] += 1
                cases.append([kind, seed, out])
    return cases


def main():
    cases = collections.OrderedDict()
    for n in range(1, 17):
        srs_n = 2 * n + 2
        if n == 4:
            caps = lambda kind, what: FOUR[kind][("proof", "REM_T", "SLICE").index(what)]   # noqa: E731
            got = collect(n, srs_n, 1, caps, lambda kind: 260)
        else:
            # proofs at n >= 5 need the degenerate kinds (a singular Vandermonde: h_pows_inv is matrix_inv's
            # Gauss-Jordan bytes there), a few per hundred draws at most n
            caps = lambda kind, what: 8 if (kind, what) == ("degenerate", "proof") else 3   # noqa: E731
            got = collect(n, srs_n, 1, caps, lambda kind: 1500 if kind == "degenerate" else 40)
        cases[pc.key_of(n, srs_n, 1)] = got
    cases[pc.long_key(4, 0)] = collect(4, 10, 0, lambda kind, what: 2, lambda kind: 40)
    # GATE and COPY exits, appended to the long setups of several n
    for n, kinds in ((1, ("gate",)), (2, ("gate", "gate2", "copy3")), (4, ("gate", "gate2", "gate_last", "copy3", "copy255", "copy_gate")),
                     (7, ("gate2", "copy255", "copy_gate")), (16, ("gate", "gate2", "gate_last", "copy3", "copy255", "copy_gate"))):
        for kind in kinds:
            for seed in range(2):
                cases[pc.long_key(n)].append([kind, seed, run(n, kind, seed, 2 * n + 2, 1)])
    # order of exits: circuits with b1 != 0 (a_x has n + 2 coefficients) and b7 != 0 (z_x has n + 3), on SRSs of
    # n + 1 and n + 2 points and on the long one
    for n in (2, 3):
        for want_acc in (True, False):
            kept = 0
            for seed in range(400):
                kind = ("perm+b1", "respect17+b1")[seed % 2]
                c = gen.prove_circuit(n, kind, seed)
                if not c["rand"][6]:
                    continue
                full = run(n, kind, seed, 2 * n + 2, 1)
                if (full == "ACC") != want_acc or full.startswith(("GATE", "SRS")):
                    continue
                mid, low = run(n, kind, seed, n + 1, 1), run(n, kind, seed, n, 1)
                assert mid == ("ACC" if want_acc else "SRS") and low == "SRS", (n, kind, seed, full, mid, low)
                cases[pc.long_key(n)].append([kind, seed, full])
                cases.setdefault(pc.key_of(n, n + 1, 1), []).append([kind, seed, mid])
                cases.setdefault(pc.key_of(n, n, 1), []).append([kind, seed, low])
                kept += 1
                if kept == 2:
                    break
            assert kept == 2
    setups = collections.OrderedDict()
    for key in cases:
        n, srs_n, mode = (int(x) for x in key.split("/"))
        setups[key] = {k: bytes(v).hex() for k, v in R.plonk_data(n, SECRET, srs_n, mode).items()}
    g = {
        "source": "reference srs_create + plonk_new(srs, n) + plonk_prove (src/plonk.h:53-118, 223-656) via oracle/_ref "
                  "ref_plonk_data / ref_prove_n, secret 2; srs_mode as in prove.json",
        "layout": "setups and cases are keyed 'n/srs_n/srs_mode'; a case is [kind, seed, outcome]: the circuit, challenges "
                  "and blinding are tests/golden/gen.py prove_circuit(n, kind, seed), the outcome the proof's 34 bytes in "
                  "hex or the reference's exit (GATE with the index of the unsatisfied gate, COPY, SRS, ACC, REM_T, SLICE, "
                  "REM_W1, REM_W2)",
        "setups": setups, "cases": cases,
    }
    per_n = pc.check_counts(pc.expand(g))
    one = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))  # noqa: E731
    path = os.path.join(HERE, "prove_circuits.json")
    with open(path, "w") as f:
        f.write('{\n "source": %s,\n "layout": %s,\n "setups": {\n' % (one(g["source"]), one(g["layout"])))
        f.write(",\n".join('  "%s": %s' % (k, one(v)) for k, v in setups.items()))
        f.write('\n },\n "cases": {\n')
        f.write(",\n".join('  "%s": [\n' % k + ",\n".join("   " + one(c) for c in v) + "\n  ]" for k, v in cases.items()))
        f.write("\n }\n}\n")
    total = sum(len(v) for v in cases.values())
    print("wrote prove_circuits.json: %d cases, %d bytes" % (total, os.path.getsize(path)))
    for n in sorted(per_n):
        print(" n = %2d: %s" % (n, dict(sorted(per_n[n].items()))))
    assert os.path.getsize(path) <= 225 * 1024


if __name__ == "__main__":
    main()
