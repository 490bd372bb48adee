"""Record tests/golden/poly_mul_short.json from the REAL reference (oracle/_ref/libplonkref.so, the unmodified
reference headers compiled in place by oracle/Makefile): poly_mul (src/poly.h:106-122) of operands of at most
64 coefficients.

    make -C oracle && python tests/golden/make_poly_mul_short_golden.py

Runs only where the reference tree is present.  The file holds data only: per case a tag, the operand bytes
and the reference's trimmed product, all as hex.  Cases (tags): la, lb in {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33,
64} crossed sparsely ("t"), zero operands ("zero"), operands with trailing zeros, so that the product's top
is zero ("ztop"), and operands holding bytes >= 17, with 0xFF, 0xEE, 0xA5, 17, 33 and 34 among them ("raw").
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

OUT = os.path.join(HERE, "poly_mul_short.json")
SEED = 0x4D554C53
LENS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 64)
RAW = (0xFF, 0xEE, 0xA5, 17, 33, 34)


def cases():
    rng = np.random.default_rng(SEED)
    out = []

    def poly(n):
        p = rng.integers(0, 17, n).astype(np.uint8)
        p[-1] = int(rng.integers(1, 17))
        return p

    for i, la in enumerate(LENS):            # every length against itself, its neighbours in the list and 64
        for lb in sorted({la, LENS[(i + 1) % len(LENS)], LENS[(i + 5) % len(LENS)], 64}):
            out.append(("t", poly(la), poly(lb)))
    for la, lb in ((1, 1), (1, 9), (33, 1), (5, 64), (64, 64)):
        out.append(("zero", np.zeros(la, np.uint8), poly(lb)))
        out.append(("zero", poly(la), np.zeros(lb, np.uint8)))
    out.append(("zero", np.zeros(7, np.uint8), np.zeros(31, np.uint8)))
    for la, lb, za, zb in ((4, 4, 1, 0), (9, 33, 0, 5), (33, 9, 3, 2), (64, 64, 7, 1), (32, 2, 31, 0), (64, 5, 0, 4)):
        a, b = poly(la), poly(lb)
        a[la - za:] = 0
        b[lb - zb:] = 0
        out.append(("ztop", a, b))
    for k, fill in enumerate(RAW):
        la, lb = LENS[(2 * k + 3) % len(LENS)], LENS[(5 * k + 7) % len(LENS)]
        a, b = poly(la), poly(lb)
        a[rng.integers(0, la, 2)] = fill
        out.append(("raw", a, b))
        a, b = poly(lb), poly(la)
        b[rng.integers(0, la, 2)] = fill
        b[-1] = fill                         # 0xFF, 0xEE, 17 and 34 are 0 mod 17: a zero top
        out.append(("raw", a, b))
    out.append(("raw", np.full(64, 0xFF, np.uint8), np.full(64, 0xFF, np.uint8)))
    out.append(("raw", np.full(33, 0xA5, np.uint8), np.full(64, 0xA5, np.uint8)))
    out.append(("raw", np.array(RAW, np.uint8), np.array(RAW[::-1], np.uint8)))
    for _ in range(6):
        out.append(("raw", rng.integers(0, 256, int(rng.integers(1, 65))).astype(np.uint8),
                    rng.integers(0, 256, int(rng.integers(1, 65))).astype(np.uint8)))
    return out


def main():
    from pyoracle import Reference
    R = Reference()
    rec = []
    for tag, a, b in cases():
        assert 1 <= len(a) <= 64 and 1 <= len(b) <= 64
        rec.append({"tag": tag, "a": bytes(a).hex(), "b": bytes(b).hex(), "out": R.poly_mul(a, b).hex()})
    with open(OUT, "w") as f:
        json.dump({"source": "reference poly_mul src/poly.h:106-122, compiled unmodified; out trimmed as it returns it",
                   "cases": rec}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(rec), "cases")


if __name__ == "__main__":
    main()
