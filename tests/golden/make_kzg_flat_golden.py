"""Record tests/golden/kzg_flat.json from the compiled reference (oracle/_ref/libplonkref.so: the reference's
unmodified poly_eval, poly_divide and srs_eval_at_s behind oracle/ref_harness.c): the commitment and the opening
of single short polynomials, the values the flat batches return per polynomial.

    python tests/golden/make_kzg_flat_golden.py

Runs only where that library was built.  Each case stands alone: the rule SRS srs[i] = (2^i mod 17) G it was taken
over (as many points as the polynomial has coefficients), the coefficient bytes and z, and as results the
commitment srs_eval_at_s(srs, p), y = poly_eval(p, z) and the proof srs_eval_at_s(srs, q) with q the quotient of
poly_divide(p, {(17 - z) % 17, 1}).  Lengths sit on both sides of every boundary of the flat kernels (16, 32,
1024, 4096); the coefficients are seeded and canonical, their top one may be zero.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import gen  # noqa: E402

OUT = os.path.join(HERE, "kzg_flat.json")
SEED = 0x464C4154
# (length, z) pairs: every z on the short lengths, a few per long one
SHORT = (1, 2, 3, 15, 16, 17, 31, 32, 33)
LONG = (40, 63, 64, 65, 255, 256, 257, 1008, 1023, 1024, 1025, 2047, 2048, 4095, 4096)


def case_list():
    cases = [(n, (3 * i + 5 * k) % 17) for i, n in enumerate(SHORT) for k in range(2)]
    cases += [(n, z) for n, z in zip(LONG, (0, 1, 2, 16, 3, 0, 9, 4, 13, 5, 0, 6, 11, 7, 8))]
    cases += [(1, 0), (2, 0), (16, 0), (32, 0), (17, 16)]
    return cases


def rule_srs(n):
    return np.array([gen.KG[pow(2, i, 17)] for i in range(n)], np.uint8)


def coeffs_of(i, n):
    p = (gen.splitmix64(SEED + i, n) % np.uint64(17)).astype(np.uint8)
    if i % 5 == 3:
        p[-1] = 0            # an untrimmed top coefficient
    return p


def generate():
    from pyoracle import Reference
    ref = Reference()
    cases = []
    for i, (n, z) in enumerate(case_list()):
        p, srs = coeffs_of(i, n), rule_srs(n)
        q, _ = ref.poly_divide(p, [(17 - z) % 17, 1])
        cases.append({"srs": srs.tobytes().hex(), "coeffs": p.tobytes().hex(), "z": z,
                      "commit": ref.msm(srs, p).hex(), "y": ref.poly_eval(p, z),
                      "proof": ref.msm(srs[:len(q)], q).hex()})
    return {"source": "the compiled reference: poly_eval, poly_divide, srs_eval_at_s (src/poly.h, src/srs.h), unmodified",
            "cases": cases}


def main():
    with open(OUT, "w") as f:
        json.dump(generate(), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
