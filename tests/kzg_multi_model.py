"""Python statement of the multi-point KZG opening and its verification (include/plonkhip.h, "KZG
multi-point openings"), on top of tests/kzg_fold_model.py, tests/divide_short_model.py and
tests/pairing_model.py: a helper of the tests, not a test.

    open    group (p_i, w_i, S_i as masks, u): ys[17 i + a] = p_i(a) for a in S_i, 0xFF elsewhere;
              q_i = the quotient of p_i by Z_i = prod_{a in S_i} (x - a) ({0} when len_i <= |S_i|);
              h = sum_i w_i q_i over Lh = max_i max(len_i - |S_i|, 1) untrimmed bytes;  W = [h trimmed];
              W' = the folded opening at u of (p_0 .. p_{k-1}, h) under multi_coeffs
    verify  r_i(u) by Lagrange over S_i from the claimed values, c = multi_coeffs, then the folded check on
            (C_0 .. C_{k-1}, W) with weights c, values (r_0(u) .. r_{k-1}(u), 0), z = u, proof W'

tests/golden/kzg_multi.json pins both to the compiled reference (tests/test_kzg_multi_cpu.py); the GPU tests
use the model for expected values at shapes the JSON does not hold."""
import numpy as np

import divide_short_model as D
import kzg_fold_model as F
import pairing_model as M

R = 17
MULTI_MAX = 15
FULL = (1 << R) - 1


def mask_ok(m):
    m = int(m)
    return m != 0 and m & ~FULL == 0 and m != FULL


def points(mask):
    return [a for a in range(R) if (int(mask) >> a) & 1]


def mask_of(pts):
    m = 0
    for a in pts:
        m |= 1 << int(a)
    return m


def from_roots(roots):
    """prod (x - r), low coefficient first"""
    z = [1]
    for r in roots:
        z = [((z[j - 1] if j else 0) - r * (z[j] if j < len(z) else 0)) % R for j in range(len(z) + 1)]
    return z


def vanish_at(mask, u):
    r = 1
    for a in points(mask):
        r = r * (u - a) % R
    return r


def multi_coeffs(sets, weights, u):
    """k + 1 bytes: c_i = w_i prod_{a in T \\ S_i} (u - a), then (17 - c_T) % 17"""
    T = 0
    for m in sets:
        T |= int(m)
    return [int(w) * vanish_at(T & ~int(m), u) % R for m, w in zip(sets, weights)] + [(R - vanish_at(T, u)) % R]


def quotient(p, mask):
    """max(len - t, 1) untrimmed bytes of p div Z_S (canonical p)"""
    p = [int(v) % R for v in np.asarray(p, dtype=np.uint8).tolist()]
    t = len(points(mask))
    if len(p) <= t:
        return np.zeros(1, np.uint8)
    if len(p) < 512:
        return np.frombuffer(D.long_divide(p, from_roots(points(mask)))[0], np.uint8)
    # long polynomials: the recurrence q[j] = p[j + t] - sum_{m < t} z[m] q[j + t - m] over numpy is still a
    # serial loop, so divide by one root at a time with the closed form of the suffix sums instead
    q = np.array(p, np.int64)
    for a in points(mask):
        q = _divide_linear(q, a)
    return q.astype(np.uint8)


def _divide_linear(p, a):
    """the quotient of p by x - a, len(p) - 1 coefficients: q[j] = sum_{i > j} p[i] a^(i - j - 1)"""
    n = p.size
    if a == 0:
        return p[1:].copy()
    pw = np.array([pow(a, i, R) for i in range(16)], np.int64)
    idx = np.arange(n)
    suf = np.cumsum((p * pw[idx % 16] % R)[::-1])[::-1] % R            # sum_{i >= j} p[i] a^i
    return suf[1:] * pw[(16 - idx[1:] % 16) % 16] % R                   # times a^-(j + 1)


def ys_row(p, mask):
    row = [0xFF] * R
    for a in points(mask):
        row[a] = eval_at(p, a)
    return row


def eval_at(p, a):
    p = np.asarray(p, dtype=np.uint8).astype(np.int64) % R
    if a == 0:
        return int(p[0])
    pw = np.array([pow(a, i, R) for i in range(16)], np.int64)
    return int((p * pw[np.arange(p.size) % 16] % R).sum() % R)


def h_of(polys, sets, weights):
    """h over Lh untrimmed bytes"""
    qs = [quotient(p, m) for p, m in zip(polys, sets)]
    return F.fold(qs, weights)


def open_multi(srs_pts, polys, sets, weights, u, msm=None):
    """(ys 17 k bytes, h, W, W') of one group; msm(points, scalars): the commitment (default the raw fold)"""
    msm = msm or F.msm
    ys = [v for p, m in zip(polys, sets) for v in ys_row(p, m)]
    h = h_of(polys, sets, weights)
    ht = F.trim(h)
    W = msm(srs_pts[:ht.size], ht)
    c = multi_coeffs(sets, weights, u)
    Ff = F.fold(list(polys) + [h], c)
    q = F.trim(F.quotient(Ff, u) if Ff.size < 512 else _divide_linear(Ff.astype(np.int64), u).astype(np.uint8))
    return ys, h, W, msm(srs_pts[:q.size], q)


def lagrange_at(mask, ys17, u):
    """r(u) from the 17-byte row of claimed values over the mask"""
    r = 0
    for a in points(mask):
        rest = int(mask) & ~(1 << a)
        r += int(ys17[a]) * vanish_at(rest, u) * pow(vanish_at(rest, a), R - 2, R)
    return r % R


def verify_multi(vk, commits, sets, weights, ys, u, proofs6):
    """ok byte of plk_kzg_verify_multi_batch for one job; commits: k 3-tuples, ys: 17 k bytes, proofs6: W, W'"""
    k = len(commits)
    commits = [tuple(int(v) for v in c) for c in commits]
    sets, weights = [int(m) for m in sets], [int(w) for w in weights]
    ys = [int(v) for v in ys]
    W, Wp = tuple(int(v) for v in proofs6[:3]), tuple(int(v) for v in proofs6[3:6])
    u = int(u)
    if not (all(M.valid_g1(c) for c in commits) and M.valid_g1(W) and M.valid_g1(Wp) and u < R and
            all(mask_ok(m) for m in sets) and all(w < R for w in weights) and
            all(ys[R * i + a] < R for i in range(k) for a in points(sets[i]))):
        return 2
    rs = [lagrange_at(sets[i], ys[R * i:R * i + R], u) for i in range(k)]
    return F.verify_fold(vk, commits + [W], multi_coeffs(sets, weights, u), rs + [0], u, Wp)


def verify_multi_batch(vk, k, commits, sets, weights, ys, us, proofs6):
    """n ok bytes; jobs repeat in the tiled batches the tests build, so results are remembered per distinct job"""
    c = np.asarray(commits, np.uint8).reshape(-1, k, 3)
    s = np.asarray(sets, np.uint32).reshape(-1, k)
    w = np.asarray(weights, np.uint8).reshape(-1, k)
    y = np.asarray(ys, np.uint8).reshape(-1, R * k)
    u = np.asarray(us, np.uint8).reshape(-1)
    p = np.asarray(proofs6, np.uint8).reshape(-1, 6)
    seen = {}
    out = np.zeros(u.size, np.uint8)
    for i in range(u.size):
        pts = [a for j in range(k) for a in (R * j + b for b in points(s[i, j]) if mask_ok(s[i, j]))]
        key = (c[i].tobytes(), s[i].tobytes(), w[i].tobytes(), y[i, pts].tobytes(), int(u[i]), p[i].tobytes())
        if key not in seen:
            seen[key] = verify_multi(vk, c[i].tolist(), s[i].tolist(), w[i].tolist(), y[i].tolist(), u[i], p[i].tolist())
        out[i] = seen[key]
    return out
