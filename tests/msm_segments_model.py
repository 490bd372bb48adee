"""Python statement of the segmented MSM (include/plonkhip.h, "Segmented MSM"; not a test module).

segment_fold   the specification: the reference's srs_eval_at_s fold (src/srs.h:53-68) over one segment,
               acc = g1_add(acc, g1_mul(P_i, s_i)) from the identity, with the raw g1_add / g1_mul of
               tests/pairing_model.py.  Those take field elements below 101 and a flag of 0 or 1; a segment that
               holds any other byte (a coordinate >= 101, a flag >= 2) is folded with the byte-level restatement
               of the same formulas in tests/g1_encoding_cases.py (py_add / py_double: gf_add, gf_sub and gf_mul
               on raw bytes as src/gf.h computes them), which agrees with pairing_model on its domain
               (tests/test_msm_segments_cpu.py checks that).
segments_host  plk_msm_g1_segments: (nseg, 3) bytes, every segment folded exactly.
segments_dev   plk_msm_g1_segments_dev: (nseg, 4) bytes {x, y, infinite, status} -- offsets read as min(o, total),
               status 2 and FF FF FF for a falling pair or an offset above total, status 1 and FF FF FF for a
               segment holding an encoding that is no canonical group element, else EXP[(sum s LOG) mod 102] with
               EXP / LOG built here from the model's own group law (numpy prefix sums: exact integers).

tests/golden/msm_segments.json pins segment_fold to the compiled reference."""
import functools

import numpy as np

import g1_encoding_cases as E
import pairing_model as M

ORDER = 102
IRREGULAR, BAD = 1, 2
FF = (0xFF, 0xFF, 0xFF)


def _byte_mul(p, k):
    """g1_mul (src/g1.h:91-103) on raw bytes"""
    res, add = M.IDENTITY, tuple(p)
    while k > 0:
        if k & 1:
            res = E.py_add(res, add)
        add = E.py_double(add)
        k >>= 1
    return res


def segment_fold(points, scalars):
    """the three bytes of srs_eval_at_s over these points (k x 3 bytes) and scalars (k bytes, any value)"""
    pts = [tuple(int(v) for v in p) for p in np.asarray(points, np.uint8).reshape(-1, 3)]
    sc = [int(s) for s in np.asarray(scalars, np.uint8).reshape(-1)]
    assert len(pts) == len(sc)
    acc = M.IDENTITY
    if all(M.valid_g1(p) for p in pts):
        for p, s in zip(pts, sc):
            acc = M.g1_add(acc, M.g1_mul(p, s))
    else:
        for p, s in zip(pts, sc):
            acc = E.py_add(acc, _byte_mul(p, s))
    return tuple(int(v) for v in acc)


def offsets_of(total, offsets=None, m=None):
    """the nseg + 1 offsets of a call as int64 (uniform: g m)"""
    if offsets is None:
        assert m and total % m == 0
        return np.arange(0, total + 1, m, dtype=np.int64)
    return np.asarray(offsets, np.int64).reshape(-1)


def segments_host(points, scalars, offsets=None, m=None):
    pts, sc = np.asarray(points, np.uint8).reshape(-1, 3), np.asarray(scalars, np.uint8).reshape(-1)
    o = offsets_of(sc.size, offsets, m)
    assert (np.diff(o) >= 0).all() and o[0] >= 0 and o[-1] <= sc.size
    return np.array([segment_fold(pts[a:b], sc[a:b]) for a, b in zip(o[:-1], o[1:])], np.uint8).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def group_tables():
    """(EXP (102, 3) uint8, LOG (256, 256) int64: the log of the affine point (x, y), -1 where there is none) for the
    first affine point of order 102 in (x, y) order -- the generator plk_dlog_generator names"""
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
    log = np.full((256, 256), -1, np.int64)
    for k, p in enumerate(exp):
        if not p[2]:
            log[p[0], p[1]] = k
    return np.array(exp, np.uint8), log


def logs_of(points):
    """the log of every canonical encoding ({0, 0, 1} is 0), -1 for every other triple of bytes"""
    pts = np.asarray(points, np.uint8).reshape(-1, 3).astype(np.int64)
    x, y, f = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.where(f == 0, group_tables()[1][x, y], np.where((x == 0) & (y == 0) & (f == 1), 0, -1))


def segments_dev(points, scalars, offsets=None, m=None):
    """(nseg, 4) uint8: what plk_msm_g1_segments_dev leaves in d_out4"""
    pts, sc = np.asarray(points, np.uint8).reshape(-1, 3), np.asarray(scalars, np.uint8).reshape(-1)
    total = sc.size
    exp = group_tables()[0]
    lg = logs_of(pts)
    bad_pref = np.concatenate([[0], np.cumsum(lg < 0)])
    sum_pref = np.concatenate([[0], np.cumsum(np.where(lg < 0, 0, lg) * sc.astype(np.int64))])
    o = offsets_of(total, offsets, m)
    a, b = o[:-1], o[1:]
    broken = (b < a) | (a > total) | (b > total)
    lo, hi = np.minimum(a, total), np.minimum(b, total)
    hi = np.maximum(hi, lo)                                      # (broken segments only: their sums are not used)
    irregular = (bad_pref[hi] - bad_pref[lo]) > 0
    out = np.zeros((a.size, 4), np.uint8)
    out[:, :3] = exp[(sum_pref[hi] - sum_pref[lo]) % ORDER]
    out[irregular] = FF + (IRREGULAR,)
    out[broken] = FF + (BAD,)
    return out
