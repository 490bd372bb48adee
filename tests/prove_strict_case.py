"""A strictly valid synthetic prover instance above n = 4 (shared by tests/test_prove_edges_gpu.py,
tests/test_prove_variants_cpu.py and tests/test_prove_variants_gpu.py).

q_c only moves the remainder of the t(x) division, so q_c = -(remainder at q_c = 0) makes a
prove-shaped random instance strictly valid, and one changed coefficient of q_c brings the
remainder exit back."""
import numpy as np

import gen
from prove_ref import Prover as RefProver

QC = 7


def ref_prover(oracle, pts, n, zh, cls=RefProver):
    return cls(oracle, np.ascontiguousarray(pts).tobytes(), n, z_h=zh.tobytes())


class Recording(RefProver):
    """remembers the remainder of its first division (t(x)'s) and the longest committed length"""
    rem = None
    longest = 0

    def divide(self, num, den):
        q, r = super().divide(num, den)
        if self.rem is None:
            self.rem = r
        return q, r

    def commit(self, p):
        self.longest = max(self.longest, len(p))
        return super().commit(p)


_STRICT = {}


def strict_case(oracle, n, seed):
    """a strictly valid synthetic instance: q_c = -(the t(x) remainder at q_c = 0), Z_H = x^n - 1
    having one more coefficient than q_c (once per module: 2^16 costs seconds of oracle time)"""
    if (n, seed) not in _STRICT:
        polys, chal, rnd, zh, pts = gen.prove_instance(n, seed, 2 * n + 8)
        polys = [p.copy() for p in polys]
        dense = polys[QC].copy()
        polys[QC] = np.zeros(n, np.uint8)
        rec = ref_prover(oracle, pts, n, zh, Recording)
        loose = rec.rounds(polys, chal, rnd, strict=False)
        r = np.zeros(n, np.int64)
        r[:len(rec.rem)] = rec.rem
        assert np.any(r) and len(rec.rem) <= n
        polys[QC] = ((17 - r) % 17).astype(np.uint8)
        ref = ref_prover(oracle, pts, n, zh, Recording)
        want = ref.rounds(polys, chal, rnd, strict=True)
        # q_c only moves the remainder: the same bytes with q_c = 0 and with the instance's dense q_c
        assert want == loose
        _STRICT[n, seed] = dict(n=n, polys=polys, chal=chal, rnd=rnd, zh=zh, pts=pts, want=want, lstar=ref.longest,
                                dense_qc=dense)
    return _STRICT[n, seed]
