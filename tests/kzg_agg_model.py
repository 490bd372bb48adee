"""Python models of KZG aggregate verification (plk_kzg_verify_agg_batch*), built on pairing_model.py.

agg_raw   the specification loop of include/plonkhip.h: the reference's raw formulas applied blindly to one
          group, job by job.
agg_log   the log-domain formula of the fast path, vectorised in numpy for large regular inputs:
              sL = sum r (LOG C + (102 - (y lg) mod 102) + z LOG W) mod 102,  sW = sum r LOG W mod 102,
              ok = pairing(EXP[sL], g2_1) == pairing(EXP[sW], g2_s)
          with LOG / EXP built here from the model's own group law (a generator of order 102 found by search),
          not taken from the library.

A G1 is (x, y, flag), a job (C, W, z, y, r), a key (g1, g2_1, g2_s).  tests/golden/kzg_agg.json pins both
models to the compiled reference (tests/test_kzg_agg_cpu.py)."""
import functools

import numpy as np

import pairing_model as M

ORDER = 102
UNDECIDED = 3


def agg_raw(vk, jobs):
    """ok byte of one group: 1 / 0, or 2 when a byte of the group is invalid"""
    g, h1, hs = (tuple(int(v) for v in k) for k in vk)
    jobs = [(tuple(int(v) for v in c), tuple(int(v) for v in w), int(z), int(y), int(r)) for c, w, z, y, r in jobs]
    if not all(M.valid_g1(c) and M.valid_g1(w) and z < M.R and y < M.R and r < M.R for c, w, z, y, r in jobs):
        return 2
    acc_l = acc_w = M.IDENTITY
    for c, w, z, y, r in jobs:
        acc_l = M.g1_add(acc_l, M.g1_mul(M.kzg_lhs(g, c, w, z, y), r))
        acc_w = M.g1_add(acc_w, M.g1_mul(w, r))
    return 1 if M.pairing(acc_l, h1) == M.pairing(acc_w, hs) else 0


@functools.lru_cache(maxsize=None)
def group_tables():
    """(EXP, LOG): EXP[k] = k g0 as (x, y, flag) for the first affine point g0 of order 102 in (x, y) order;
    LOG[x, y, flag] = k for the 102 canonical encodings, -1 elsewhere"""
    pts = [(x, y, 0) for x in range(M.P) for y in range(M.P) if (y * y - x * x * x - 3) % M.P == 0]
    assert len(pts) == ORDER - 1

    def order(p):
        q, k = p, 1
        while not q[2]:
            q, k = M.g1_add(q, p), k + 1
        return k

    g0 = next(p for p in pts if order(p) == ORDER)
    exp, q = [], M.IDENTITY
    for _ in range(ORDER):
        exp.append(q)
        q = M.g1_add(q, g0)
    assert q == M.IDENTITY and len(set(exp)) == ORDER
    log = np.full((M.P, M.P, 2), -1, np.int64)
    for k, p in enumerate(exp):
        log[p] = k
    return exp, log


def logs_of(pts):
    """pts: k x 3 bytes -> (log or -1 where the encoding is valid but no canonical group element, valid mask)"""
    pts = np.asarray(pts, np.int64).reshape(-1, 3)
    valid = (pts[:, 0] < M.P) & (pts[:, 1] < M.P) & (pts[:, 2] < 2)
    safe = np.where(valid[:, None], pts, 0)
    return np.where(valid, group_tables()[1][safe[:, 0], safe[:, 1], safe[:, 2]], -1), valid


def agg_log(vk, m, commits, zs, ys, proofs, rs):
    """the ok bytes of plk_kzg_verify_agg_batch_dev for n groups of m jobs in flat arrays: 1 / 0, 2 for a
    group with an invalid byte, 3 (UNDECIDED) for a valid group that is not canonical or any valid group under
    a key whose g1 is not canonical"""
    g, h1, hs = (tuple(int(v) for v in k) for k in vk)
    exp = group_tables()[0]
    z, y, r = (np.asarray(a, np.int64).reshape(-1) for a in (zs, ys, rs))
    lc, vc = logs_of(commits)
    lw, vw = logs_of(proofs)
    n = z.size // m
    assert z.size == n * m and lc.size == n * m and lw.size == n * m and y.size == n * m and r.size == n * m
    invalid = ~(vc & vw & (z < M.R) & (y < M.R) & (r < M.R))
    lg = int(logs_of([g])[0][0])
    irregular = (lc < 0) | (lw < 0) | (lg < 0)
    s_l = (r * (lc + (ORDER - (y * lg) % ORDER) + z * lw)).reshape(n, m).sum(1) % ORDER
    s_w = (r * lw).reshape(n, m).sum(1) % ORDER
    invalid, irregular = invalid.reshape(n, m).any(1), irregular.reshape(n, m).any(1)
    return _verdicts(exp, h1, hs, s_l, s_w, invalid, irregular)


def _verdicts(exp, h1, hs, s_l, s_w, invalid, irregular):
    pairs, inv = np.unique(s_l * ORDER + s_w, return_inverse=True)   # at most 102^2 distinct pairings to compare
    eq = np.array([M.pairing(exp[p // ORDER], h1) == M.pairing(exp[p % ORDER], hs) for p in pairs.tolist()], np.uint8)
    return np.where(invalid, 2, np.where(irregular, UNDECIDED, eq[inv.reshape(-1)])).astype(np.uint8)


def agg_log_tiled(vk, m, commits, zs, ys, proofs, rs):
    """agg_log for ONE group of m jobs whose arrays are the given tile of t jobs repeated and cut off at m:
    the sums of m // t whole tiles and of the first m % t jobs (integers: the order does not matter)"""
    g, h1, hs = (tuple(int(v) for v in k) for k in vk)
    exp = group_tables()[0]
    z, y, r = (np.asarray(a, np.int64).reshape(-1) for a in (zs, ys, rs))
    t = z.size
    q, rem = divmod(m, t)
    lc, vc = logs_of(commits)
    lw, vw = logs_of(proofs)
    lg = int(logs_of([g])[0][0])
    used = slice(0, t if q else rem)
    invalid = ~(vc & vw & (z < M.R) & (y < M.R) & (r < M.R))[used]
    irregular = ((lc < 0) | (lw < 0) | (lg < 0))[used]
    t_l = r * (lc + (ORDER - (y * lg) % ORDER) + z * lw)
    t_w = r * lw
    s_l = (q * int(t_l.sum()) + int(t_l[:rem].sum())) % ORDER
    s_w = (q * int(t_w.sum()) + int(t_w[:rem].sum())) % ORDER
    return _verdicts(exp, h1, hs, np.array([s_l]), np.array([s_w]), np.array([invalid.any()]), np.array([irregular.any()]))


def agg_raw_flat(vk, m, commits, zs, ys, proofs, rs):
    """agg_raw over n groups of m jobs in flat arrays (the layout of the library call)"""
    c, w = np.asarray(commits).reshape(-1, 3), np.asarray(proofs).reshape(-1, 3)
    z, y, r = (np.asarray(a).reshape(-1) for a in (zs, ys, rs))
    n = z.size // m
    return np.array([agg_raw(vk, [(c[j], w[j], z[j], y[j], r[j]) for j in range(g * m, (g + 1) * m)]) for g in range(n)],
                    np.uint8)
