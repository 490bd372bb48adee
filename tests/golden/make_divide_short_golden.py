"""Record tests/golden/divide_short.json from the REAL reference (oracle/_ref/libplonkref.so, the unmodified
reference headers compiled in place by oracle/Makefile): poly_divide (src/poly.h:124-177) by divisors of
2 .. 17 coefficients.

    make -C oracle && python tests/golden/make_divide_short_golden.py

Runs only where the reference tree is present.  The file holds data only: per case a tag, the numerator
and divisor bytes and the reference's trimmed quotient and remainder, all as hex.  Numerators have at
most 64 coefficients.  Cases (tags): every degree t = 1 .. 16 at nl < dl, nl = dl, nl = dl + 1 and longer
("t"), d_0 = 0 ("d0"), d = lead x^t ("mono"), repeated roots ("rep"), vanishing polynomials of subsets of
GF(17) with x^16 - 1 among them ("zs"), every lead 1 .. 16 ("lead"), zero numerators ("zero"), exact
multiples ("exact"), quotients with a zero top ("ztop"), nl = 1 ("one") and numerators holding bytes >= 17,
0xFF and 0xEE among them ("raw": the host form's fallback).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

OUT = os.path.join(HERE, "divide_short.json")
SEED = 0x44495653


def pmul(a, b):
    return (np.convolve(np.asarray(a, np.int64), np.asarray(b, np.int64)) % 17).astype(np.uint8)


def from_roots(roots):
    p = np.array([1], np.uint8)
    for r in roots:
        p = pmul(p, [(17 - r) % 17, 1])
    return p


def cases():
    rng = np.random.default_rng(SEED)
    out = []

    def num(nl):
        return rng.integers(0, 17, nl).astype(np.uint8)

    def den(t, lead=None):
        d = rng.integers(0, 17, t + 1).astype(np.uint8)
        d[t] = int(rng.integers(1, 17)) if lead is None else lead
        return d

    for t in range(1, 17):
        dl = t + 1
        for nl in sorted({max(t - 1, 1), t, dl, dl + 1, dl + 2, int(rng.integers(dl + 3, 65)), 64}):
            out.append(("t", num(nl), den(t)))
        d = den(t)
        d[0] = 0
        out.append(("d0", num(int(rng.integers(dl, 65))), d))
        d = np.zeros(dl, np.uint8)
        d[t] = int(rng.integers(1, 17))
        out.append(("mono", num(int(rng.integers(dl, 65))), d))
        out.append(("rep", num(int(rng.integers(dl, 65))), from_roots([int(rng.integers(0, 17))] * t)))
        out.append(("zs", num(64), from_roots(rng.permutation(17)[:t].tolist())))
        out.append(("zero", np.zeros(int(rng.integers(1, 65)), np.uint8), den(t)))
        d = den(t)
        out.append(("exact", pmul(num(int(rng.integers(1, 65 - t))), d), d))
        n = num(64)
        n[64 - int(rng.integers(1, 8)):] = 0
        out.append(("ztop", n, den(t)))
        out.append(("one", num(1), den(t)))
        for fill in (0xFF, 0xEE, None):
            n = num(int(rng.integers(dl, 65)))
            k = rng.integers(0, len(n), 3)
            n[k] = rng.integers(17, 256, 3).astype(np.uint8) if fill is None else fill
            out.append(("raw", n, den(t)))
    out.append(("zs", num(64), from_roots(list(range(1, 17)))))          # x^16 - 1
    out.append(("zs", num(40), from_roots([0] + list(range(1, 16)))))
    out.append(("rep", num(50), from_roots([2, 2, 5, 5, 5, 11])))
    for lead in range(1, 17):
        out.append(("lead", num(30), den(3, lead)))
    out.append(("raw", np.full(64, 0xFF, np.uint8), den(16)))
    out.append(("raw", np.full(33, 0xEE, np.uint8), den(2)))
    return out


def main():
    from pyoracle import Reference
    R = Reference()
    rec = []
    for tag, n, d in cases():
        assert 1 <= len(n) <= 64 and 2 <= len(d) <= 17 and d[-1] != 0 and d.max() < 17
        q, r = R.poly_divide(n, d)
        rec.append({"tag": tag, "num": bytes(n).hex(), "den": bytes(d).hex(), "quot": q.hex(), "rem": r.hex()})
    assert bytes.fromhex([c for c in rec if c["tag"] == "zs"][-2]["den"]) == bytes([16] + [0] * 15 + [1])
    with open(OUT, "w") as f:
        json.dump({"source": "reference poly_divide src/poly.h:124-177, compiled unmodified; quot and rem trimmed as "
                             "it returns them", "cases": rec}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(rec), "cases")


if __name__ == "__main__":
    main()
