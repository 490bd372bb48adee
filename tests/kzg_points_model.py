"""Python model of the KZG per-point openings (plk_kzg_open_points_batch*): the expansion into single
openings, the job order and the status rules of include/plonkhip.h.  Values come from the caller's oracle:
y = oracle.poly_eval(p, z), q = the quotient of oracle.poly_divide(p, [(17 - z) % 17, 1]), proof =
oracle.msm(srs[:len(q)], q) -- what tests/test_kzg_gpu.py::expect takes per (polynomial, z)."""
R = 17
FULL = (1 << R) - 1
CHUNK = 4096
FLAGGED_PROOF = b"\xff\xff\xff"


def mask_ok(m):
    """1 .. 17 points of GF(17): unlike the multi-point calls, all 17 bits is a set"""
    return m != 0 and (m & ~FULL) == 0


def points(mask):
    """the points of a set, ascending: the order of a polynomial's jobs"""
    return [a for a in range(R) if (mask >> a) & 1]


def mask_of(pts):
    m = 0
    for a in pts:
        m |= 1 << a
    return m


def count(sets):
    """J, or 0 when a mask is invalid (plk_kzg_points_count)"""
    if not sets or not all(mask_ok(m) for m in sets):
        return 0
    return sum(len(points(m)) for m in sets)


def expand(sets):
    """[(polynomial index, z)] in job order: job e = sum_{i' < i} popcount(S_i') + rank of a in S_i"""
    return [(i, a) for i, m in enumerate(sets) for a in points(m)]


def first_job(sets, i):
    return sum(len(points(m)) for m in sets[:i])


def chunks(n):
    return -(-n // CHUNK)


def workspace_words(lens, sets):
    """the words the header promises: per polynomial of more than one chunk, (points + non-zero points) x chunks"""
    return sum((len(points(m)) + len(points(m & ~1))) * chunks(n) for n, m in zip(lens, sets) if chunks(n) > 1)


def canonical(p):
    return all(int(b) < R for b in p)


def open_one(oracle, srs_pts, p, z):
    """(y, proof) of one opening through the oracle"""
    y = oracle.poly_eval(p, z)
    q, _ = oracle.poly_divide(p, [(R - z) % R, 1])
    return y, oracle.msm(srs_pts[:len(q)], q)


def open_points(oracle, srs_pts, polys, sets, cache=None, keys=None):
    """(zs, ys, proofs) flat in job order; cache / keys: a dict and one hashable key per polynomial that names
    its bytes, so tests that share polynomials compute each (polynomial, z) once"""
    zs, ys, proofs = [], [], []
    for i, a in expand(sets):
        k = None if cache is None or keys is None else (keys[i], a)
        if k is not None and k in cache:
            y, pf = cache[k]
        else:
            y, pf = open_one(oracle, srs_pts, polys[i], a)
            if k is not None:
                cache[k] = (y, pf)
        zs.append(a)
        ys.append(y)
        proofs.append(pf)
    return zs, ys, proofs


def dev_status(polys, sets, irregular=False):
    """d_status of the _dev form: every job of a polynomial with a byte >= 17 is 1, every job when the SRS is
    irregular, 0 otherwise"""
    return [1 if irregular or not canonical(polys[i]) else 0 for i, _ in expand(sets)]
