#!/usr/bin/env python3
"""Golden answers of rounds 1-5 at the gate counts where the device prover's round-3 plan
switches (tile width, sum groups, transform field, the exact-range limit; the table in
tests/test_prove_large_gpu.py) from the CPU oracle (oracle/prove_ref.py over oracle.c): the
prove-shaped synthetic instance gen.prove_instance(n, seed, 2n + 8), non-strict (synthetic
polynomials leave remainders).  A case the reference exits on records the exit message instead
of a proof.  Writes tests/golden/prove_large.json; 2 .. 75 s of oracle time a case, one process
each (make_prove_2_20.py generalised; prove_2_20.json stays that script's).
    python tests/golden/make_prove_large.py [jobs]"""
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "oracle")]

# (n, seed): see the switch table in tests/test_prove_large_gpu.py
CASES = [(131072, 51), (262144, 51), (524288, 51), (600000, 52), (600000, 51), (1223336, 51), (1223337, 51),
         (1400000, 52), (1835006, 52), (1835007, 51), (2097152, 51), (3932158, 51)]


def run_case(case):
    """one golden entry: the oracle's proof (hex) or its exit message"""
    import gen
    from prove_ref import Prover as RefProver, ProveError
    from pyoracle import Oracle
    n, seed = case
    srs_len = 2 * n + 8
    polys, chal, rnd, zh, pts = gen.prove_instance(n, seed, srs_len)
    t = time.time()
    ref = RefProver(Oracle(), pts.tobytes(), n, z_h=zh.tobytes())
    proof = exit_msg = None
    try:
        proof = ref.rounds(polys, chal, rnd, strict=False).hex()
    except ProveError as e:
        exit_msg = str(e)
    return {"n": n, "seed": seed, "srs_len": srs_len, "proof": proof, "exit": exit_msg,
            "oracle_seconds": round(time.time() - t, 1)}


def main():
    jobs = int(sys.argv[1]) if len(sys.argv) > 1 else min(6, os.cpu_count() or 1)
    with ProcessPoolExecutor(jobs) as ex:
        cases = list(ex.map(run_case, CASES))
    out = {"note": "rounds 1-5 (plonk_prove, src/plonk.h:223-656) of gen.prove_instance(n, seed, srs_len), CPU "
                   "oracle, non-strict; exit: the reference's exit message where it gives no proof",
           "cases": cases}
    with open(os.path.join(HERE, "prove_large.json"), "w") as f:
        json.dump(out, f, indent=1)
    for c in cases:
        print(json.dumps(c))


if __name__ == "__main__":
    main()
