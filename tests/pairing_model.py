"""Python model of the reference's pairing() (src/pairing.h:66-83) and of the KZG opening check
built on it, as csrc/pairing.hip computes them: the fixed schedule r = 2, 4, 8, 16, 17 of
pairing_f(17), one doubling chain p, 2p, 4p, 8p, 16p, the final power 600 = conj(f^5) f^95.

Encodings are plain ints: a G1 is (x, y, flag), a G2 (x, y), a GT (a, b) = a + b u with u^2 = -2.
Every formula is applied blindly, as the reference applies it: no curve or subgroup test, and
line() reads x and y whatever the flag says.  tests/golden/pairing.json pins the model to the
compiled reference; the tests use it for expected values at shapes the JSON does not hold."""
import functools

P = 101
R = 17
INV = [pow(v, P - 2, P) for v in range(P)]   # gf_inv: v^99, so inv(0) = 0
IDENTITY = (0, 0, 1)


def g1_double(a):
    x, y, inf = a
    if inf or y == 0:
        return IDENTITY
    m = 3 * x * x * INV[2 * y % P] % P
    m2 = m * m % P
    return ((m2 - 2 * x) % P, (m * ((3 * x - m2) % P) - y) % P, 0)


def g1_add(a, b):
    if a[2]:
        return b
    if b[2]:
        return a
    if a[0] == b[0]:
        return IDENTITY if (a[1] + b[1]) % P == 0 else g1_double(a)
    m = (b[1] - a[1]) * INV[(b[0] - a[0]) % P] % P
    xr = (m * m - a[0] - b[0]) % P
    return (xr, (m * ((a[0] - xr) % P) - a[1]) % P, 0)


def g1_neg(a):
    return a if a[2] else (a[0], -a[1] % P, 0)


def g1_mul(p, k):
    res, add = IDENTITY, p
    while k > 0:
        if k & 1:
            res = g1_add(res, add)
        add = g1_double(add)
        k >>= 1
    return res


def valid_g1(p):
    return p[0] < P and p[1] < P and p[2] < 2


def valid_g2(q):
    return q[0] < P and q[1] < P


def gt_mul(f, g):
    return ((f[0] * g[0] - 2 * f[1] * g[1]) % P, (f[0] * g[1] + f[1] * g[0]) % P)


def _term(a, b, q):
    """line(a, b) evaluated at q (src/pairing.h:19-29, 41-44)"""
    m, n = (b[0] - a[0]) % P, (b[1] - a[1]) % P
    c = (m * a[1] - n * a[0]) % P
    return ((q[0] * n + c) % P, q[1] * (-m % P) % P)


@functools.lru_cache(maxsize=None)
def pairing(p, q):
    """the reference's pairing(p, q) for a valid encoding pair (tuples; results are remembered)"""
    f = (1, 0)
    d = p
    for _ in range(4):            # r = 2, 4, 8, 16: rp = 2^k p, line(rp, 2 (-rp))
        f = gt_mul(gt_mul(f, f), _term(d, g1_double(g1_neg(d)), q))
        d = g1_double(d)
    f = gt_mul(f, _term(d, p, q))   # r = 17: line(16 p, p)
    f2 = gt_mul(f, f)
    f4 = gt_mul(f2, f2)
    f8 = gt_mul(f4, f4)
    f16 = gt_mul(f8, f8)
    f32 = gt_mul(f16, f16)
    f64 = gt_mul(f32, f32)
    f5 = gt_mul(f, f4)
    f95 = gt_mul(gt_mul(gt_mul(f5, f2), gt_mul(f8, f16)), f64)
    return gt_mul((f5[0], -f5[1] % P), f95)


def pairing_bytes(g1, g2):
    """two output bytes of plk_pairing_batch for one job: FF FF for an invalid encoding"""
    g1, g2 = tuple(g1), tuple(g2)
    if not (valid_g1(g1) and valid_g2(g2)):
        return (0xFF, 0xFF)
    return pairing(g1, g2)


def kzg_lhs(g, c, w, z, y):
    """L = C - y G + z W, built in the order the specification fixes"""
    return g1_add(g1_add(c, g1_neg(g1_mul(g, y))), g1_mul(w, z))


def kzg_verify(vk, c, w, z, y):
    """ok byte of plk_kzg_verify_batch for one job; vk = (g1, g2_1, g2_s), all valid"""
    c, w = tuple(c), tuple(w)
    if not (valid_g1(c) and valid_g1(w) and z < R and y < R):
        return 2
    g, h1, hs = (tuple(v) for v in vk)
    return 1 if pairing(kzg_lhs(g, c, w, z, y), h1) == pairing(w, hs) else 0
