"""Python statement of the folded KZG opening and its verification (include/plonkhip.h, "KZG folded
openings"), on top of tests/pairing_model.py and numpy.

    open    group (p_0 .. p_{k-1}, w_0 .. w_{k-1}, z), L = the longest length:
              y_i = p_i(z);  F[j] = sum_i w_i p_i[j] mod 17 for j < L (nothing past a polynomial's own
              length, no trim);  q = max(L - 1, 1) untrimmed bytes of (F - F(z)) / (x - z);
              proof = the raw fold of g1_mul(srs[i], q[i]) over the trimmed quotient
    verify  C = the raw fold of g1_mul(C_i, w_i) from the identity, y = sum_i w_i y_i mod 17, then the
            check of pairing_model.kzg_verify on (C, z, y, W); 2 for an invalid byte in the job

tests/golden/kzg_fold.json pins both to the compiled reference (tests/test_kzg_fold_cpu.py); the GPU
tests use the model for expected values at shapes the JSON does not hold."""
import numpy as np

import pairing_model as M

R = 17
FOLD_MAX = 16


def fold(polys, weights):
    """F as L untrimmed bytes (always canonical: the products reduce)"""
    L = max(len(p) for p in polys)
    acc = np.zeros(L, np.int64)
    for p, w in zip(polys, weights):
        a = np.asarray(p, dtype=np.uint8).astype(np.int64)
        acc[:a.size] += int(w) % R * (a % R)
    return (acc % R).astype(np.uint8)


def poly_eval(p, z):
    y = 0
    for c in reversed(np.asarray(p, dtype=np.uint8).tolist()):
        y = (y * z + c) % R
    return y


def quotient(F, z):
    """max(L - 1, 1) untrimmed bytes of (F - F(z)) / (x - z): q[L-2] = F[L-1], q[j] = F[j+1] + z q[j+1]"""
    F = np.asarray(F, dtype=np.uint8).tolist()
    L = len(F)
    q = [0] * max(L - 1, 1)
    run = 0
    for j in range(L - 2, -1, -1):
        run = (F[j + 1] + z * run) % R
        q[j] = run
    return np.array(q, np.uint8)


def trim(a):
    a = np.asarray(a, dtype=np.uint8)
    n = a.size
    while n > 1 and a[n - 1] == 0:
        n -= 1
    return a[:n]


def msm(points, scalars):
    """srs_eval_at_s: the raw fold from the identity"""
    acc = M.IDENTITY
    for p, s in zip(points, scalars):
        acc = M.g1_add(acc, M.g1_mul(tuple(int(v) for v in p), int(s)))
    return acc


def open_fold(srs_pts, polys, weights, z):
    """(ys, F, proof 3-tuple) of one group"""
    F = fold(polys, weights)
    q = trim(quotient(F, z))
    return [poly_eval(p, z) for p in polys], F, msm(srs_pts[:q.size], q)


def fold_commitments(commits, weights):
    acc = M.IDENTITY
    for c, w in zip(commits, weights):
        acc = M.g1_add(acc, M.g1_mul(tuple(c), w))
    return acc


def verify_fold(vk, commits, weights, ys, z, proof):
    """ok byte of plk_kzg_verify_fold_batch for one job; commits: k 3-tuples, vk = (g1, g2_1, g2_s)"""
    commits = [tuple(int(v) for v in c) for c in commits]
    weights, ys = [int(v) for v in weights], [int(v) for v in ys]
    proof, z = tuple(int(v) for v in proof), int(z)
    if not (all(M.valid_g1(c) for c in commits) and M.valid_g1(proof) and z < R and
            all(w < R for w in weights) and all(y < R for y in ys)):
        return 2
    y = 0
    for w, yi in zip(weights, ys):
        y = (y + w * yi % R) % R
    return M.kzg_verify(vk, fold_commitments(commits, weights), proof, z, y)


def verify_fold_batch(vk, k, commits, weights, ys, zs, proofs):
    """n ok bytes; commits n k x 3, weights and ys n k, zs n, proofs n x 3 (numpy or lists).  Jobs repeat
    in the tiled batches the tests build, so results are remembered per distinct job."""
    c = np.asarray(commits, np.uint8).reshape(-1, k, 3)
    w = np.asarray(weights, np.uint8).reshape(-1, k)
    y = np.asarray(ys, np.uint8).reshape(-1, k)
    z = np.asarray(zs, np.uint8).reshape(-1)
    p = np.asarray(proofs, np.uint8).reshape(-1, 3)
    seen = {}
    out = np.zeros(z.size, np.uint8)
    for i in range(z.size):
        key = (c[i].tobytes(), w[i].tobytes(), y[i].tobytes(), int(z[i]), p[i].tobytes())
        if key not in seen:
            seen[key] = verify_fold(vk, c[i].tolist(), w[i].tolist(), y[i].tolist(), z[i], p[i].tolist())
        out[i] = seen[key]
    return out
