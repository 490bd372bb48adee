"""Seeded inputs at the structural edges of polyops.hip (not a test module).

tests/test_polyops_edges_gpu.py runs them through libplonkhip against the oracle;
tests/test_polyops_edges_cpu.py pins the oracle to the compiled reference at the very same inputs.
Every case is built from an rng seeded by its own id, so a case does not depend on which cases were
built before it.  The constants name the kernels' geometry:

  poly_eval      one block per 64 KiB of the longest job, at most 64 blocks (grid stride beyond);
                 a launch takes 32 jobs; a block takes 256 chunks of 16 bytes per stride step
  binomial       one thread per chain up to a longest chain of 4096, the suffix scan in blocks of
                 4096 positions above; the later blocks' aggregates are summed 64 at a time
  constant       8192 blocks of 256 bytes, grid stride beyond
  matrix_mul     4096 blocks of 256 outputs, grid stride beyond
  matrix_inv     one block of 256 threads over n x 2n bytes
"""
import zlib

import numpy as np

EVAL_BLOCK = 65536          # bytes of the longest job per block
EVAL_MAX_BLOCKS = 64
EVAL_STEP = 4096            # bytes one block takes per grid-stride step (256 threads x 16)
EVAL_MAX_JOBS = 32          # PLK_EVAL_MAX_JOBS
SCAN_B = 4096               # chain positions per scan block; also the short / long switch


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def canon(rng, n):
    return rng.integers(0, 17, n).astype(np.uint8)


def raw(rng, n, lo=0, hi=256):
    return rng.integers(lo, hi, n).astype(np.uint8)


def canon_eval(p, x):
    """sum p[i] x^i mod 17 for canonical p, with integers (no byte arithmetic)"""
    xm = x % 17
    if xm == 0:
        return int(p[0]) if p.size else 0
    table = np.array([pow(xm, e, 17) for e in range(16)], np.int64)   # x^16 = 1
    return int((p.astype(np.int64) * table[np.arange(p.size) % 16]).sum() % 17)


def trimmed(b):
    """poly_new's trim: trailing zeros dropped, one coefficient kept"""
    b = bytes(b).rstrip(b"\x00")
    return b if b else b"\x00"


# --------------------------------------------------------------------------------- poly_eval
# x: residue 0 as the byte 0 and as non-zero bytes (17, 34, 255), order 1, order 2 (16), a
# generator (3), and a raw byte with a non-zero residue (18)
EVAL_XS = (0, 1, 3, 16, 17, 18, 34, 255)
EVAL_GEOMETRY_LENS = (65535, 65536, 65537, 131072, 131073, 64 * 65536, 64 * 65536 + 1, 65 * 65536 + 3)


def eval_geometry(length):
    """(polys, xs): one canonical polynomial of that length at every x of EVAL_XS"""
    p = canon(rng_for("eval_geometry/%d" % length), length)
    return [p] * len(EVAL_XS), list(EVAL_XS)


def eval_mixed():
    """jobs of length 0, 1, 2 and 17 beside one 64-block job, in both orders"""
    rng = rng_for("eval_mixed")
    polys = [canon(rng, n) for n in (0, 1, 2, 17, EVAL_MAX_BLOCKS * EVAL_BLOCK)]
    xs = [5, 18, 3, 255, 7]
    yield "short_first", polys, xs
    yield "long_first", polys[::-1], xs[::-1]


ONE_HOT_SMALL = tuple(range(41))
ONE_HOT_LARGE = (65535, 65536, 65537, (1 << 20) + 5)
ONE_HOT_XS = (0, 3, 16, 17, 20, 255)


def eval_one_hot(indices):
    """(polys, xs, expected): a single coefficient 1 at index i, once as the last coefficient and
    once followed by zeros up to a whole number of 16-byte chunks plus one more chunk; expected is
    x^i mod 17 from Python integers"""
    polys, xs, want = [], [], []
    for i in indices:
        for length in (i + 1, ((i + 16) & ~15) + 16):
            p = np.zeros(length, np.uint8)
            p[i] = 1
            for x in ONE_HOT_XS:
                polys.append(p)
                xs.append(x)
                want.append(1 if i == 0 else pow(x % 17, i, 17))
    return polys, xs, want


EVAL_JOB_COUNTS = (32, 33, 64, 65)
# the host call keeps a 256-byte slot per job (and one for the results) in its 16 KiB of mapped
# memory: 63 jobs is the most that path takes, in two launches (32 + 31)
EVAL_MAPPED_MAX_JOBS = 63


def eval_short_jobs(n):
    """n short jobs, 16 KiB in all at the most (lengths 0..200, raw bytes in every fourth)"""
    rng = rng_for("eval_short_jobs/%d" % n)
    polys = []
    for j in range(n):
        ln = int(rng.integers(0, 201))
        polys.append(raw(rng, ln) if j % 4 == 3 else canon(rng, ln))
    assert sum(p.size for p in polys) <= 16384
    return polys, [int(v) for v in rng.integers(0, 256, n)]


def eval_staged_jobs(n):
    """n jobs of 3000 bytes (beyond the mapped path whatever n is)"""
    rng = rng_for("eval_staged_jobs/%d" % n)
    return [canon(rng, 3000) for _ in range(n)], [int(v) for v in rng.integers(0, 256, n)]


def eval_dev_jobs(n):
    """n jobs for the device form: short ones, with a 2-block job in every launch of 32 (its slot
    moves from launch to launch)"""
    rng = rng_for("eval_dev_jobs/%d" % n)
    polys = []
    for j in range(n):
        ln = 70000 if j % EVAL_MAX_JOBS == (3 * (j // EVAL_MAX_JOBS)) % EVAL_MAX_JOBS else int(rng.integers(0, 301))
        polys.append(canon(rng, ln))
    return polys, [int(v) for v in rng.integers(0, 256, n)]


EVAL_RAW_LEN = 4 * EVAL_BLOCK - 5     # 4 blocks, the last chunk short


def eval_raw_four_blocks():
    """(id, poly, x) on a 4-block polynomial; block b of the launch takes the bytes
    [EVAL_STEP (b + 4 j), + EVAL_STEP).  Bytes 17..239 stay on the parallel path, a byte >= 240 at an
    index >= 1 sends the job to the serial loop."""
    L = EVAL_RAW_LEN
    rng = rng_for("eval_raw_four_blocks")
    base = canon(rng, L)

    def put(*pairs):
        p = base.copy()
        for i, b in pairs:
            p[i] = b
        return p

    for x in (3, 16, 255):
        yield "a_all_17_239/x%d" % x, raw(rng, L, 17, 240), x
        # Horner reaches index 1 with y x % 17 = 16 (x = 255: 0), the one value at which 16 + 240
        # wraps the uint8 sum while 16 + 239 does not: p[2] is chosen for it
        y3 = canon_eval(base[3:], x)
        c2 = (16 * pow(x % 17, 15, 17) - y3 * x) % 17
        yield "b_239_at_1/x%d" % x, put((1, 239), (2, c2)), x
        yield "b_240_at_1/x%d" % x, put((1, 240), (2, c2)), x
        yield "c_255_at_0/x%d" % x, put((0, 255)), x
    # a byte 255 wraps the uint8 sum unless Horner arrives with y x % 17 = 0: the coefficient above
    # it is chosen so that it does not (the last coefficient has nothing above it and cannot wrap, so
    # the tail case sits one below it, in the short last chunk)
    def wrapping(x, i):
        p = base.copy()
        if canon_eval(p[i + 1:], x) * x % 17 == 0:
            p[i + 1] = (int(p[i + 1]) + 1) % 17
        p[i] = 255
        return p

    for name, i in (("block0", 10), ("block2", 2 * EVAL_STEP + 100), ("block2_second_step", 6 * EVAL_STEP + 9),
                    ("third_64k", 2 * EVAL_BLOCK + 7), ("tail", L - 2)):
        yield "d_one_flag_%s" % name, wrapping(6, i), 6
    yield "e_every_block_flags", put(*[(EVAL_STEP * b + 17, 255) for b in range(4)]), 11


def eval_raw_all_255():
    return [np.full(1 << 20, 255, np.uint8)] * 2, [3, 255]


EVAL_UNALIGNED_OFFSETS = (1, 15)
EVAL_UNALIGNED_LENS = (16, 17, 31, 65536, 65537, 65551)   # len mod 16 in {0, 1, 15}


def eval_unaligned():
    """(base, jobs): jobs are (offset, length, x) views of one buffer; the second half of the buffer
    holds one byte >= 240, so the serial loop runs from an unaligned pointer too"""
    rng = rng_for("eval_unaligned")
    half = 65600
    base = canon(rng, 2 * half)
    base[half + 40000] = 251
    jobs = []
    for part in (0, half):
        for off in EVAL_UNALIGNED_OFFSETS:
            for ln in EVAL_UNALIGNED_LENS:
                jobs.append((part + off, ln, int(rng.integers(0, 256))))
    return base, jobs


def eval_tick_reuse():
    """three launches on one tick buffer: (polys, xs) of a 64-block launch with a flagged job, and of
    a 1-block clean launch over the same slots"""
    rng = rng_for("eval_tick_reuse")
    big = [canon(rng, EVAL_MAX_BLOCKS * EVAL_BLOCK), canon(rng, 40 * EVAL_BLOCK + 3), canon(rng, 9)]
    big[1][30 * EVAL_BLOCK] = 244
    small = [canon(rng, 1000), canon(rng, 65536), canon(rng, 0)]
    return (big, [3, 7, 255]), (small, [16, 18, 2])


def eval_null_job():
    """(polys, xs): a NULL polynomial of length 0 (None) between real jobs"""
    rng = rng_for("eval_null_job")
    return [canon(rng, 100), None, canon(rng, 70000)], [3, 9, 12]


def eval_all_host_arrays():
    """every (poly, x) above, for the CPU pin"""
    for L in EVAL_GEOMETRY_LENS:
        yield from zip(*eval_geometry(L))
    for _, polys, xs in eval_mixed():
        yield from zip(polys, xs)
    for idx in (ONE_HOT_SMALL, ONE_HOT_LARGE):
        polys, xs, _ = eval_one_hot(idx)
        yield from zip(polys, xs)
    for n in EVAL_JOB_COUNTS + (EVAL_MAPPED_MAX_JOBS, 5, 70):
        for make in (eval_short_jobs, eval_staged_jobs, eval_dev_jobs):
            yield from zip(*make(n))
    for _, p, x in eval_raw_four_blocks():
        yield p, x
    yield from zip(*eval_raw_all_255())
    base, jobs = eval_unaligned()
    for off, ln, x in jobs:
        yield base[off:off + ln], x
    for polys, xs in eval_tick_reuse():
        yield from zip(polys, xs)
    polys, xs = eval_null_job()
    yield from ((np.zeros(0, np.uint8) if p is None else p, x) for p, x in zip(polys, xs))


# ------------------------------------------------------------------------------- poly_divide
def binomial(m, d0, lead):
    den = np.zeros(m + 1, np.uint8)
    den[0], den[m] = d0, lead
    return den


def _binom_case(name, m, lq, rng=None, d0=None, lead=None):
    rng = rng or rng_for(name)
    d0 = int(rng.integers(0, 17)) if d0 is None else d0
    lead = int(rng.integers(1, 17)) if lead is None else lead
    return name, canon(rng, lq + m), binomial(m, d0, lead), 2


def divide_switch():
    """longest chain ceil(lq / m) = 4096 (one thread per chain), then 4097 twice (the scan): with one
    chain one longer than the others, and with every chain at 4097"""
    for m in (1, 2, 3, 5, 16, 17, 64):
        for lq in (SCAN_B * m, SCAN_B * m + 1, (SCAN_B + 1) * m):
            yield _binom_case("switch/m%d/lq%d" % (m, lq), m, lq)


def divide_scan_blocks():
    """two scan blocks exactly, one position into a third, 66 aggregates (the carry loop wraps past
    64), and chains of uneven length"""
    for m, lq in ((1, 8192), (1, 8193), (1, 65 * SCAN_B + 5), (3, 3 * 5000 + 1), (3, 3 * 5000 + 2)):
        yield _binom_case("scan/m%d/lq%d" % (m, lq), m, lq)


def divide_multipliers(path):
    """all 17 x 16 (d0, lead): A = -d0 / lead takes every value, 0 included"""
    m, nl = (2, 600) if path == "short" else (1, 4200)
    rng = rng_for("multipliers/" + path)
    num = canon(rng, nl)
    for d0 in range(17):
        for lead in range(1, 17):
            yield "mult/%s/d0=%d/lead=%d" % (path, d0, lead), num, binomial(m, d0, lead), 2


def divide_short_blocks():
    """the one-thread-per-chain kernel: threads with a remainder coefficient and no quotient
    (nl < 2 m), and chain counts on both sides of one block of 256 threads"""
    for m, nl in [(300, v) for v in (301, 450, 599, 600, 601)] + [(m, 4 * m + 7) for m in (255, 256, 257)]:
        yield _binom_case("short_blocks/m%d/nl%d" % (m, nl), m, nl - m)


def divide_raw_numerator(shape, oracle):
    """one numerator byte >= 17 (17, 200, 255): in the remainder region only, at num[m - 1], inside a
    chain in scan block 1, at the very end.  'long': lq = 4096 m + 1, where scan block 1 holds one
    position, num[nl - 1]; 'long_mid': lq = 4200 m, the byte at position 4150 of the middle chain;
    'short': m = 64, nl = 3000 (a chain's middle instead of the scan block).

    Where the loop's bytes differ from arithmetic mod 17 (raw_numerator_is_sensitive): the int8
    difference keeps a byte's residue until a +17 carries it past 255, so 255 changes the quotient
    below it, 200 only where m - 1 zero divisor bytes pass over it first, 17 never; in the remainder
    region a byte >= 17 comes out as it is when nothing is subtracted from it, so q[0] and q[m - 1]
    are made zero here (num[m] and num[2 m - 1] chosen for it)."""
    m, kind = shape
    if kind == "long":
        lq = SCAN_B * m + 1
        places = (0, m - 1, (SCAN_B + 1) * m, lq + m - 1)
    elif kind == "long_mid":
        lq = 4200 * m
        places = (m // 2 + 4151 * m,)
    else:
        lq = 3000 - m
        places = (0, m - 1, m // 2 + 20 * m, lq + m - 1)
    name = "raw_num/m%d/%s" % (m, kind)
    rng = rng_for(name)
    base = canon(rng, lq + m)
    den = binomial(m, int(rng.integers(1, 17)), int(rng.integers(1, 17)))
    q = oracle.poly_divide(base, den)[0].ljust(lq, b"\x00")
    for r in {0, m - 1}:
        base[r + m] = (int(base[r + m]) - int(den[m]) * q[r]) % 17
    for at in sorted(set(places)):
        for b in (17, 200, 255):
            num = base.copy()
            num[at] = b
            yield "%s/at%d/byte%d" % (name, at, b), num, den, 2


def raw_numerator_is_sensitive(name, m, nl):
    """whether the reference's bytes for that case differ from the division of num mod 17 (a missed
    flag would show): see divide_raw_numerator"""
    at, byte = int(name.split("/at")[1].split("/")[0]), int(name.split("byte")[1])
    if at < m:
        return True
    if at >= nl - m:          # consumed before any subtraction reaches it: only its residue counts
        return False
    return byte == 255 or (byte == 200 and m >= 5)


DIVIDE_RAW_SHAPES = ((1, "long"), (1, "long_mid"), (17, "long"), (17, "long_mid"), (64, "short"))


def divide_trim(oracle):
    """quotients with a zero tail longer than the trim's 16 KiB window, an all-zero quotient, and
    exact divisions (num = q den from the oracle's product: rem = {0})"""
    for m in (3, 16):            # chains of 13333 (scan) and 2499 (one thread per chain)
        name = "trim/top_zero/m%d" % m
        rng = rng_for(name)
        num = canon(rng, 40000)
        num[20000:] = 0
        num[19999] = 1
        yield name, num, binomial(m, int(rng.integers(1, 17)), int(rng.integers(1, 17))), 2
        name = "trim/zero_quotient/m%d" % m
        rng = rng_for(name)
        num = np.zeros(40000, np.uint8)
        num[:m] = rng.integers(1, 17, m)
        yield name, num, binomial(m, int(rng.integers(1, 17)), int(rng.integers(1, 17))), 2
    for m, lq in ((64, 3000), (2, 10000)):
        name = "trim/exact/m%d" % m
        rng = rng_for(name)
        q = canon(rng, lq)
        q[-1] = 1 + int(rng.integers(0, 16))
        den = binomial(m, int(rng.integers(1, 17)), int(rng.integers(1, 17)))
        num = np.frombuffer(oracle.poly_mul(q, den), np.uint8)
        assert num.size == lq + m
        yield name, num, den, 2


def divide_constant():
    """past the constant kernel's 8192 blocks x 256 bytes; every byte value"""
    num = raw(rng_for("constant"), (1 << 21) + 5)
    for lead in (1, 5, 16):
        yield "constant/lead%d" % lead, num, np.array([lead], np.uint8), 1


def divide_trivial():
    """nl < dl for a binomial divisor of 65 bytes: canonical and raw numerators"""
    den = binomial(64, 16, 1)
    for nl in (1, 64):
        rng = rng_for("trivial/%d" % nl)
        yield "trivial/nl%d/canonical" % nl, canon(rng, nl), den, 0
        yield "trivial/nl%d/raw" % nl, raw(rng, nl, 1), den, 0


def divide_device_shapes():
    """(id, num, den) for the device form: one thread per chain, the scan, a constant"""
    rng = rng_for("divide_device")
    yield "short", canon(rng, 3000), binomial(64, 16, 1)
    yield "long", canon(rng, 3 * 5000 + 5), binomial(3, 5, 7)
    yield "constant", raw(rng, 70001), np.array([5], np.uint8)
    num = canon(rng, 3 * 5000 + 5)
    num[9001] = 255        # (changes the quotient below it: divide_raw_numerator)
    yield "long_raw", num, binomial(3, 5, 7)


def divide_groups(oracle):
    """name -> a callable giving (id, num, den, path) cases; every host-form case"""
    g = {
        "switch": divide_switch,
        "scan_blocks": divide_scan_blocks,
        "multipliers_short": lambda: divide_multipliers("short"),
        "multipliers_long": lambda: divide_multipliers("long"),
        "short_blocks": divide_short_blocks,
        "trim": lambda: divide_trim(oracle),
        "constant": divide_constant,
        "trivial": divide_trivial,
    }
    for shape in DIVIDE_RAW_SHAPES:
        g["raw_numerator_m%d_%s" % shape] = lambda shape=shape: divide_raw_numerator(shape, oracle)
    return g


DIVIDE_GROUPS = ("switch", "scan_blocks", "multipliers_short", "multipliers_long", "short_blocks", "trim", "constant",
                 "trivial") + tuple("raw_numerator_m%d_%s" % s for s in DIVIDE_RAW_SHAPES)


# ---------------------------------------------------------------------------------- matrices
MATRIX_MUL_SHAPES = ((33, 70, 5), (256, 1, 256), (1, 5000, 1), (4, 0, 4), (1025, 3, 1024))


def matrix_mul_case(m, k, n):
    rng = rng_for("matrix_mul/%d/%d/%d" % (m, k, n))
    return raw(rng, m * k), raw(rng, k * n)


MATRIX_INV_SIZES = (18, 64, 127, 128, 129, 255, 256, 257, 300)
MATRIX_INV_VARIANTS = ("lu", "permutation", "equal_rows", "zero_column", "rank1", "zero")


def matrix_inv_case(n, variant):
    """n x n canonical bytes (row-major, flat).  'lu' is invertible by construction, 'permutation'
    too (the cyclic shift: every elimination step but the last swaps); the others are singular."""
    rng = rng_for("matrix_inv/%d/%s" % (n, variant))
    if variant == "lu":
        lo = np.tril(rng.integers(0, 17, (n, n)), -1) + np.eye(n, dtype=np.int64)
        up = np.triu(rng.integers(0, 17, (n, n)), 1) + np.diag(rng.integers(1, 17, n))
        mat = lo.astype(np.int64) @ up.astype(np.int64) % 17
    elif variant == "permutation":
        mat = np.roll(np.eye(n, dtype=np.int64), 1, axis=1)     # row i = e_(i + 1 mod n)
    elif variant == "equal_rows":
        mat = rng.integers(0, 17, (n, n))
        mat[n - 2] = mat[n // 3]
    elif variant == "zero_column":
        mat = rng.integers(0, 17, (n, n))
        mat[:, n // 3] = 0
    elif variant == "rank1":
        mat = np.outer(rng.integers(1, 17, n), rng.integers(1, 17, n)) % 17
    else:
        mat = np.zeros((n, n), np.int64)
    return np.ascontiguousarray(mat.astype(np.uint8)).reshape(-1)


INTERPOLATE_CASES = ((1, "random"), (17, "random"), (17, "zero"), (64, "random"), (64, "tail_rows_zero"),
                     (300, "random"), (300, "tail_rows_zero"), (2000, "random"))


def interpolate_case(n, variant):
    """(matrix, values): canonical matrix, raw value bytes; 'tail_rows_zero': the last 40 rows are
    zero, so the output is trimmed by 40 coefficients at least"""
    rng = rng_for("interpolate/%d/%s" % (n, variant))
    mat = canon(rng, n * n).reshape(n, n)
    if variant == "tail_rows_zero":
        mat[n - 40:] = 0
    elif variant == "zero":
        mat[:] = 0
    return mat.reshape(-1), raw(rng, n)
