"""Deterministic G1 byte encodings for the MSM's decode and raw-fold kernels (not a test module).

tests/test_g1_encodings_gpu.py sends them through libplonkhip against the oracle;
tests/test_g1_encodings_cpu.py pins the builders and, for flag bytes 0 / 1, the oracle to the
compiled reference at the very same inputs.  A G1 is 3 bytes {x, y, flag}; 102 of the 2^24 triples
are canonical group elements, every other one is folded by the reference with its raw formulas.
Every builder is a pure function of its arguments: random parts come from a generator seeded by
the builder's name and arguments.  Builders that return expected values take the oracle
(pyoracle.Oracle) as their first argument.

The constants name the kernels' geometry (plonk.c_amd/csrc/msm.hip):

  msm_dlog_kernel          16-point groups (48 B, one v_perm_b32 position per point), the n mod 16
                           tail one point per thread of block 0; a single MSM whose threads have at
                           most one group takes half groups of 8
  msm_serial_fold_kernel   n < 8192; the prefix before the first irregular point as a log sum
  msm_fold_*_kernel        n >= 8192: chunks of max(2048, ceil(n / 256) rounded up to 1024) terms,
                           counted from the first irregular point
"""
import zlib

import numpy as np

import gen

GROUP = gen.all_points()                    # (102, 3): the identity, then the affine points in (x, y) order
IDENT = (0, 0, 1)
TWO_TORSION = (48, 0, 0)
SWEEP_ROWS = 32768                          # rows of one sweep launch: half of the 2^16 (x, y) of a flag byte
FOLD_CHUNKED_MIN = 8192                     # plk_msm_serial_launch: the chunked fold from this n on
BOUNDARY_N = 8192
BOUNDARY_L = 2048                           # chunk length at n = 8192
BIG_N = 2048 * 256 + 1                      # the first n whose chunk length grows past 2048 ...
BIG_L = 3072                                # ... ceil(n / 256) = 2049, rounded up to a multiple of 1024
PREFIX_N = 9000
PREFIX_POS = (0, 4095, 4096, PREFIX_N - 1)  # FOLD_T * FOLD_E = 16384 points per prefix step, 4096-term fold chunks

# the y values of the same-x family: around 0, 50, 101, 152, 202 and 255
Y47 = tuple(list(range(0, 6)) + list(range(47, 54)) + list(range(96, 107)) + list(range(149, 156)) +
            list(range(197, 207)) + list(range(250, 256)))
SAME_X = (0, 1, 48, 100, 101, 149, 255)
CHORD_YS = ((17, 60), (150, 233))           # (a.y, b.y): both below 101 / both at least 101
PAIR_FLAGS = (0, 1, 2, 255)


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def canonical_mask(triples):
    """True where a {x, y, flag} triple is a canonical group element: an affine point of
    y^2 = x^3 + 3 over GF(101) with both coordinates below 101 and flag 0, or the identity (0, 0, 1).
    Integer arithmetic on the bytes, no table: independent of the kernels' and the oracle's."""
    t = np.asarray(triples, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
    x, y, f = t[:, 0], t[:, 1], t[:, 2]
    affine = (f == 0) & (x < 101) & (y < 101) & ((y * y) % 101 == (x * x * x + 3) % 101)
    return affine | ((x == 0) & (y == 0) & (f == 1))


def _dedup_irregular(cands):
    seen, out = set(), []
    for c in cands:
        if all(0 <= v < 256 for v in c) and c not in seen:
            seen.add(c)
            out.append(c)
    arr = np.array(out, dtype=np.uint8)
    return arr[~canonical_mask(arr)]


def neighbours(p):
    """every single-field perturbation of the canonical point p that the near-miss list holds
    (values that leave the byte range are dropped later)"""
    x, y, f = (int(v) for v in p)
    if f == 1:
        return [(0, 0, fl) for fl in (0, 2, 3, 255)] + [(1, 0, 1), (0, 1, 1), (101, 0, 1), (0, 101, 1)]
    c = [(x ^ 1, y, 0), (x + 1, y, 0), (x - 1, y, 0), (x + 101, y, 0), (x + 202, y, 0)]
    c += [(x, y + 101, 0), (x, y + 202, 0)]
    # the negated y: as a field element ((x, 101 - y) is the inverse point, canonical, and drops out
    # again unless y = 0) and as a byte
    c += [(x, (101 - y) % 101, 0), (x, 101 - y, 0), (x, (256 - y) & 0xFF, 0)]
    c += [(x, y, fl) for fl in (1, 2, 3, 128, 254, 255)]
    return c


def near_misses():
    """(m, 3) uint8: encodings one field away from a canonical one, deduplicated, none canonical"""
    cands = []
    for p in GROUP:
        cands += neighbours(p)
    return _dedup_irregular(cands)


def near_misses_of(points):
    return _dedup_irregular([c for p in points for c in neighbours(p)])


# one affine point of full order, the identity and the 2-torsion point: every position is run for
# these and their near-misses
SPECIAL_POINTS = np.array([(1, 2, 0), IDENT, TWO_TORSION], dtype=np.uint8)


def special_candidates():
    """(m, 3): SPECIAL_POINTS and their near-misses"""
    return np.concatenate([SPECIAL_POINTS, near_misses_of(SPECIAL_POINTS)])


def control_and_near_misses():
    """(m, 3): the 102 canonical points (the control), then near_misses()"""
    return np.concatenate([GROUP, near_misses()])


def fillers(rng, shape):
    """(points shape + (3,), scalars shape): uniform over all 102 group elements, any scalar byte"""
    return GROUP[rng.integers(0, 102, shape)], rng.integers(0, 256, shape).astype(np.uint8)


def placed(name, cands, n, positions):
    """One n-point MSM per candidate: canonical fillers with candidate i at positions[i], scalar
    non-zero.  (points (m, n, 3), scalars (m, n))"""
    cands = np.asarray(cands, dtype=np.uint8).reshape(-1, 3)
    m = len(cands)
    rng = rng_for("placed/%s/%d" % (name, n))
    pts, sc = fillers(rng, (m, n))
    r = np.arange(m)
    pos = np.asarray(positions, dtype=np.int64)
    pts[r, pos] = cands
    sc[r, pos] = 1 + rng.integers(0, 255, m)
    return pts, sc


def expected_decode(oracle, pts, sc):
    """(irregular (m,) bool, log (m,) int, g1 (m, 3)): what msm_dlog_kernel must leave in the record
    of each row -- log and g1 only where the row is all canonical (irregular False)"""
    m, n = sc.shape
    irregular = ~canonical_mask(pts.reshape(-1, 3)).reshape(m, n).all(axis=1)
    logs = np.zeros(m, np.int64)
    g1 = np.zeros((m, 3), np.uint8)
    for r in np.flatnonzero(~irregular):
        lg, p = oracle.msm_dlog(pts[r], sc[r])
        assert lg is not None
        logs[r] = lg
        g1[r] = np.frombuffer(p, np.uint8)
    return irregular, logs, g1


def sweep_candidates(flag, half):
    """(32768, 3): x = 128 half + row // 256, y = row % 256, this flag byte"""
    v = half * SWEEP_ROWS + np.arange(SWEEP_ROWS)
    return np.stack([v >> 8, v & 0xFF, np.full(SWEEP_ROWS, flag)], axis=1).astype(np.uint8)


def sweep_rows(oracle, flag, half, n=16):
    """The 32,768 rows of one batched launch: 15 canonical fillers and the candidate
    sweep_candidates(flag, half)[row] at position row % 16 (n = 16), or a full group of fillers and
    the candidate in the tail at 16 + row % (n - 16) (n > 16).
    Returns (points (rows, n, 3), scalars (rows, n), irregular, log, g1) -- see expected_decode."""
    cands = sweep_candidates(flag, half)
    r = np.arange(SWEEP_ROWS)
    pos = r % 16 if n == 16 else 16 + r % (n - 16)
    pts, sc = placed("sweep/%d/%d" % (flag, half), cands, n, pos)
    # the fillers are group elements by construction, so the candidate alone decides the row
    irregular = ~canonical_mask(cands)
    reg = np.flatnonzero(~irregular)
    logs = np.zeros(SWEEP_ROWS, np.int64)
    g1 = np.zeros((SWEEP_ROWS, 3), np.uint8)
    if reg.size:
        _, logs[reg], g1[reg] = expected_decode(oracle, pts[reg], sc[reg])
    return pts, sc, irregular, logs, g1


def seeded_triples(flags, count, name="seeded"):
    """(count, 3) seeded triples with the flag byte drawn from `flags`"""
    rng = rng_for("%s/%d" % (name, count))
    t = rng.integers(0, 256, (count, 3)).astype(np.uint8)
    t[:, 2] = np.asarray(flags, dtype=np.uint8)[rng.integers(0, len(flags), count)]
    return t


# ------------------------------------------------------------------ pair families (raw arithmetic)
# Each family is (A (m, 3), T (m, 3), c (m,), want (m, 3)): want[i] = g1_add(A[i], g1_mul(T[i], c[i]))
# from the oracle.  As a fold: [A with scalar 1, T with scalar c] (the first term is adopted by the
# infinite accumulator), or [T with scalar c] alone where A is the identity.
def _family(oracle, A, T, c):
    A, T = np.ascontiguousarray(A, dtype=np.uint8), np.ascontiguousarray(T, dtype=np.uint8)
    c = np.ascontiguousarray(c, dtype=np.uint8)
    return A, T, c, oracle.g1_add_mul_many(A, T, c)


def pairs_same_x(oracle):
    """7 x 47 x 47 = 15,463 pairs with a.x == b.x: x over SAME_X, a.y and b.y over Y47, flags 0, c = 1
    (the branch add(a.y, b.y) == 0 ? identity : double(a), which never looks at b again)"""
    x, ay, by = np.meshgrid(SAME_X, Y47, Y47, indexing="ij")
    x, ay, by = x.reshape(-1), ay.reshape(-1), by.reshape(-1)
    z = np.zeros_like(x)
    return _family(oracle, np.stack([x, ay, z], 1), np.stack([x, by, z], 1), np.ones(x.size))


def pairs_chord(oracle, which):
    """all 65,536 (a.x, b.x) at the fixed (a.y, b.y) = CHORD_YS[which], flags 0, c = 1"""
    ax, bx = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    ax, bx = ax.reshape(-1), bx.reshape(-1)
    ay, by = CHORD_YS[which]
    z = np.zeros_like(ax)
    return _family(oracle, np.stack([ax, z + ay, z], 1), np.stack([bx, z + by, z], 1), np.ones(ax.size))


def flag_coordinate_pairs():
    """100 ((a.x, a.y), (b.x, b.y)): zeros, group elements, equal and opposite points, coordinates
    at and above 101, then seeded bytes"""
    fixed = [((0, 0), (0, 0)), ((0, 0), (1, 2)), ((1, 2), (0, 0)), ((1, 2), (1, 2)), ((1, 2), (1, 99)),
             ((1, 2), (68, 74)), ((48, 0), (48, 0)), ((48, 0), (1, 2)), ((200, 150), (200, 150)),
             ((200, 150), (200, 153)), ((101, 0), (0, 101)), ((0, 101), (101, 0)), ((102, 103), (1, 2)),
             ((1, 2), (102, 103)), ((255, 255), (255, 255)), ((255, 255), (0, 0)), ((3, 3), (3, 98)),
             ((3, 3), (5, 5)), ((100, 100), (201, 201)), ((202, 0), (0, 202))]
    rng = rng_for("flag_coordinate_pairs")
    rest = rng.integers(0, 256, (100 - len(fixed), 4))
    return fixed + [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in rest]


def pairs_flags(oracle):
    """a.flag, b.flag over PAIR_FLAGS x PAIR_FLAGS at the 100 flag_coordinate_pairs; c = 1, 1, 2, 255
    by the coordinate pair's index: 1,600 pairs"""
    A, T, c = [], [], []
    for fa in PAIR_FLAGS:
        for fb in PAIR_FLAGS:
            for j, ((ax, ay), (bx, by)) in enumerate(flag_coordinate_pairs()):
                A.append((ax, ay, fa))
                T.append((bx, by, fb))
                c.append((1, 1, 2, 255)[j % 4])
    return _family(oracle, A, T, c)


def pairs_mul(oracle):
    """A = the identity, T over the 102 canonical points and near_misses(), c over all 256 bytes (T
    major): a single-point fold returns the term g1_mul(T, c) itself"""
    base = control_and_near_misses()
    T = np.repeat(base, 256, axis=0)
    c = np.tile(np.arange(256), len(base))
    return _family(oracle, np.tile(np.array(IDENT), (len(T), 1)), T, c)


def pair_folds(family):
    """(points (m, n, 3), scalars (m, n)) of the folds that observe a family: n = 1 as [T, c] where
    every A is the identity, else n = 2 as [A, 1], [T, c]"""
    A, T, c, _ = family
    if (A == np.array(IDENT, np.uint8)).all():
        return T[:, None, :].copy(), c[:, None].copy()
    return np.stack([A, T], axis=1), np.stack([np.ones_like(c), c], axis=1)


# ------------------------------------------------------------------------ chunk-boundary layouts
def boundary_states():
    """(m, 3) start states S: the 102 group elements, off-curve states with x, y < 101, raw states
    with a coordinate >= 101 (no canonical state id: the resolve kernel re-folds the chunk they
    cross into), flagged states with coordinates.  About 1,000."""
    rng = rng_for("boundary_states")
    off = rng.integers(0, 101, (300, 2))
    off = np.concatenate([[(0, 0), (0, 1), (1, 0), (100, 100), (48, 1), (1, 3)], off])
    off = np.concatenate([off, np.zeros((len(off), 1), np.int64)], axis=1)
    off = off[~canonical_mask(off)]
    raw = rng.integers(0, 256, (300, 2))
    side = rng.integers(0, 3, 300)
    raw[side == 0, 0] = 101 + raw[side == 0, 0] % 155          # x >= 101 only
    raw[side == 0, 1] %= 101
    raw[side == 1, 1] = 101 + raw[side == 1, 1] % 155          # y >= 101 only
    raw[side == 1, 0] %= 101
    raw[side == 2] = 101 + raw[side == 2] % 155                # both
    raw = np.concatenate([[(101, 0), (0, 101), (255, 255), (101, 101), (102, 2), (1, 103)], raw])
    raw = np.concatenate([raw, np.zeros((len(raw), 1), np.int64)], axis=1)
    fl = rng.integers(0, 256, (290, 3))
    fl[:, 2] = np.array([1, 2, 255, 3, 128])[rng.integers(0, 5, 290)]
    fl = np.concatenate([[(1, 2, 1), (0, 0, 2), (0, 0, 255), (1, 0, 1), (0, 1, 1), (200, 150, 1), (1, 2, 2),
                          (1, 2, 255), (48, 0, 1), (0, 0, 3)], fl])
    s = np.concatenate([GROUP.astype(np.int64), off, raw, fl]).astype(np.uint8)
    return s


def boundary_cases():
    """(S (m, 3), T (m, 3, 3), c (m, 3)): a start state and the three terms that open the later
    chunks.  The terms mix canonical points, near-misses, raw bytes and flagged bytes; the
    scalars are 1 (the raw term itself), 0 (the identity), small and 255."""
    S = boundary_states()
    m = len(S)
    rng = rng_for("boundary_cases")
    nm = near_misses()
    kind = rng.integers(0, 4, (m, 3))
    T = np.zeros((m, 3, 3), np.uint8)
    T[kind == 0] = GROUP[rng.integers(0, 102, int((kind == 0).sum()))]
    T[kind == 1] = nm[rng.integers(0, len(nm), int((kind == 1).sum()))]
    k2 = int((kind == 2).sum())
    T[kind == 2] = np.concatenate([rng.integers(0, 256, (k2, 2)), np.zeros((k2, 1), np.int64)], axis=1)
    k3 = int((kind == 3).sum())
    T[kind == 3] = np.stack([rng.integers(0, 256, k3), rng.integers(0, 256, k3),
                             np.array([1, 2, 255])[rng.integers(0, 3, k3)]], axis=1)
    c = np.array([1, 1, 1, 0, 2, 3, 16, 255], np.uint8)[rng.integers(0, 8, (m, 3))]
    # every fourth case repeats the state as a term (a.x == b.x against a carried state) or negates it
    rep = np.arange(m) % 4 == 1
    T[rep, 0] = S[rep]
    c[rep, 0] = 1
    neg = np.arange(m) % 8 == 3
    T[neg, 1, 0] = S[neg, 0]
    T[neg, 1, 1] = ((101 - S[neg, 1].astype(np.int64)) % 101).astype(np.uint8)
    T[neg, 1, 2] = 0
    c[neg, 1] = 1
    return S, T, c


def boundary_layout(S, T, c, n=BOUNDARY_N, L=BOUNDARY_L, name="boundary_layout"):
    """(points (m, n, 3), scalars (m, n)): S at index 0 with scalar 1, T[:, j] at index L (j + 1) with
    scalar c[:, j], canonical identities (any scalar byte) everywhere else.  A state with a non-zero
    flag byte is "infinite" to g1_add, so the identity after it replaces it: such an S stands a
    second time at index L - 1, the last term of the first chunk, and crosses into the next chunk
    from there (index 0 still makes it the first irregular point, where the chunks start)."""
    S, T, c = (np.asarray(a, dtype=np.uint8) for a in (S, T, c))
    m = len(S)
    pts = np.empty((m, n, 3), np.uint8)
    pts[:] = np.array(IDENT, np.uint8)
    sc = rng_for("%s/%d" % (name, n)).integers(0, 256, (m, n)).astype(np.uint8)
    pts[:, 0] = S
    sc[:, 0] = 1
    flagged = S[:, 2] != 0
    pts[flagged, L - 1] = S[flagged]
    sc[flagged, L - 1] = 1
    for j in range(T.shape[1]):
        pts[:, L * (j + 1)] = T[:, j]
        sc[:, L * (j + 1)] = c[:, j]
    return pts, sc


def big_layout():
    """one layout at BIG_N points: a raw S at index 0 and eight terms at the chunk starts BIG_L j"""
    S = np.array([(200, 150, 0)], np.uint8)
    T = np.array([[(200, 150, 0), (1, 2, 0), (3, 3, 0), (9, 250, 1), (102, 103, 0), (1, 99, 0), (0, 0, 2),
                   (48, 101, 0)]], np.uint8)
    c = np.array([[1, 1, 2, 1, 255, 1, 1, 3]], np.uint8)
    pts, sc = boundary_layout(S, T, c, n=BIG_N, L=BIG_L, name="big_layout")
    return pts[0], sc[0]


def prefix_cases(cands, positions):
    """(points (m, 9000, 3), scalars (m, 9000)): one canonical 9,000-point input (the same fillers
    for every case), candidate i at positions[i] with a non-zero scalar"""
    cands = np.asarray(cands, dtype=np.uint8).reshape(-1, 3)
    m = len(cands)
    rng = rng_for("prefix_cases")
    bp, bs = fillers(rng, PREFIX_N)
    pts = np.repeat(bp[None], m, axis=0)
    sc = np.repeat(bs[None], m, axis=0)
    r = np.arange(m)
    pos = np.asarray(positions, dtype=np.int64)
    pts[r, pos] = cands
    sc[r, pos] = 1 + rng.integers(0, 255, m)
    return pts, sc


def srs_with(cand, pos, n=118):
    """an n-point SRS of canonical points (the 102 group elements cycled) holding cand at pos"""
    pts = GROUP[np.arange(n) % 102].copy()
    pts[pos] = cand
    return pts


# ------------------------------------------------- a Python restatement of the raw addition, for
# the sensitivity check of the same-x family (tests/test_g1_encodings_cpu.py)
def _fadd(a, b):
    s = a + b
    return (s - 101 if s >= 101 else s) & 0xFF


def _fsub(a, b):
    d = a - b
    return (d + 101 if d < 0 else d) & 0xFF


def _finv(a):
    return pow(a % 101, 99, 101)


def py_double(a):
    x, y, f = a
    if f or y == 0:
        return IDENT
    m = (3 * (x * x % 101) % 101) * _finv(2 * y % 101) % 101
    m2 = m * m % 101
    xr = _fsub(m2, 2 * x % 101)
    yr = _fsub(m * _fsub(3 * x % 101, m2) % 101, y)
    return (xr % 101, yr % 101, 0)


def py_add(a, b, same_x_uses_b=False):
    """g1_add on raw bytes as RawOps::addp restates it; same_x_uses_b: the mistake of doubling b
    instead of a in the a.x == b.x branch"""
    if a[2]:
        return tuple(b)
    if b[2]:
        return tuple(a)
    if a[0] == b[0]:
        if _fadd(a[1], b[1]) == 0:
            return IDENT
        return py_double(b if same_x_uses_b else a)
    m = _fsub(b[1], a[1]) * _finv(_fsub(b[0], a[0])) % 101
    xr = _fsub(_fsub(m * m % 101, a[0]), b[0])
    yr = _fsub(m * _fsub(a[0], xr) % 101, a[1])
    return (xr % 101, yr % 101, 0)
