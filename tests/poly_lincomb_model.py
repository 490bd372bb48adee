"""The specification of plk_poly_lincomb (include/plonkhip.h, "poly linear combinations") in numpy: the
reference's byte formulas (src/hf.h:79-119) applied per coefficient over the untrimmed length
L = max(len + shift).  tests/test_poly_lincomb_cpu.py pins it to the reference's recorded outputs
(tests/golden/poly_lincomb.json); the GPU tests take their expected bytes from it."""
import numpy as np

RAW = 0xFF


def hf_add(a, b):
    s = (a.astype(np.uint16) + b.astype(np.uint16)).astype(np.uint8)      # uint8_t sum = a + b
    return np.where(s >= 17, s - np.uint8(17), s).astype(np.uint8)


def hf_sub(a, b):
    d = (a.astype(np.int8).astype(np.int16) - b.astype(np.int8).astype(np.int16)).astype(np.int8)   # int8_t diff
    d = np.where(d < 0, (d.astype(np.int16) + 17).astype(np.int8), d)
    return d.astype(np.uint8)


def hf_neg(a):
    return np.where(a == 0, 0, (17 - a.astype(np.int16)) & 0xFF).astype(np.uint8)


def hf_mul(a, b):
    return (a.astype(np.uint16) * np.asarray(b).astype(np.uint16) % 17).astype(np.uint8)


def term(p, shift=0, sub=0, scale=RAW, neg=0, twist=0):
    return {"p": p, "shift": shift, "sub": sub, "scale": scale, "neg": neg, "twist": twist}


def length(terms):
    return max(len(t["p"]) + t["shift"] for t in terms)


def lincomb(terms, add_hf=None):
    """the L untrimmed result bytes (uint8 array)"""
    L = length(terms)
    acc = None
    for i, t in enumerate(terms):
        v = np.asarray(t["p"], np.uint8).reshape(-1)
        if t["twist"]:
            v = hf_mul(v, np.array([pow(t["twist"], k, 17) for k in range(16)], np.uint8)[np.arange(v.size) % 16])
        if t["scale"] != RAW:
            v = hf_mul(v, np.uint8(t["scale"]))
        if t["neg"]:
            v = hf_neg(v)
        full = np.zeros(L, np.uint8)
        full[t["shift"]:t["shift"] + v.size] = v
        if i == 0:
            acc = full
        else:
            acc = hf_sub(acc, full) if t["sub"] else hf_add(acc, full)
    if add_hf is not None:
        acc[:1] = hf_add(acc[:1], np.array([add_hf], np.uint8))
    return acc


def nz(out):
    """index + 1 of the last non-zero byte, 0 when all are zero (the d_nz word)"""
    idx = np.flatnonzero(np.asarray(out))
    return int(idx[-1]) + 1 if idx.size else 0
