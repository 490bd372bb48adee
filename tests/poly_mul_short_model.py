"""The specification of plk_poly_mul_short_batch(_dev) in Python: the reference's poly_mul
(src/poly.h:106-122) folds hf_mul products (each reduced mod 17) with hf_add (which keeps a canonical sum
canonical, src/hf.h:79-109), so for EVERY input byte value the la + lb - 1 untrimmed bytes are
conv(a mod 17, b mod 17) mod 17, and the trimmed length is the index + 1 of the last non-zero byte."""
import numpy as np


def _u8(a):
    return np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a, np.uint8)


def product(a, b):
    """the la + lb - 1 untrimmed product bytes"""
    a, b = _u8(a).astype(np.int64) % 17, _u8(b).astype(np.int64) % 17
    if len(a) * len(b) <= 1 << 26:
        c = np.convolve(a, b)
    else:
        # the same integers by a real FFT: every sum is at most 16 x 16 x min(la, lb), far inside the exact
        # range of a double transform of this size; the distance to the nearest integer is asserted
        n = 1 << (len(a) + len(b) - 2).bit_length()
        f = np.fft.irfft(np.fft.rfft(a.astype(np.float64), n) * np.fft.rfft(b.astype(np.float64), n), n)[:len(a) + len(b) - 1]
        c = np.rint(f)
        assert float(np.abs(f - c).max()) < 0.05
        c = c.astype(np.int64)
    return (c % 17).astype(np.uint8).tobytes()


def product_rows(a, b):
    """row i of the result is product(a[i], b[i]) for 2-d arrays of equal-shape operands"""
    a, b = np.asarray(a, np.uint8).astype(np.int64) % 17, np.asarray(b, np.uint8).astype(np.int64) % 17
    out = np.zeros((a.shape[0], a.shape[1] + b.shape[1] - 1), np.int64)
    for j in range(b.shape[1]):
        out[:, j:j + a.shape[1]] += a * b[:, j:j + 1]
    return (out % 17).astype(np.uint8)


def trim(p):
    """index + 1 of the last non-zero byte, 0 when there is none (the d_nz word)"""
    nz = np.flatnonzero(_u8(p))
    return int(nz[-1]) + 1 if len(nz) else 0


def trimmed(p):
    """as plk_poly_mul returns it: at least one byte"""
    return bytes(p[:max(trim(p), 1)])
