"""The chunked form of division by a short divisor, in plain Python: a helper of
the tests, not a test.

`long_divide` is the recurrence one coefficient at a time -- for canonical bytes the reference's loop
(src/poly.h:124-177).  `divide_chunked` is what plonk.c_amd/csrc/divshort.hip runs, with its geometry as
parameters: the divisor padded to T states (D = d x^s over the numerator a x^s), spans of `chunk`
coefficients cut from virtual index 0 up, `threads` spans to a block, every run acting on the state as
R -> R x^n mod D + (run mod D), multiplication by x^n as the n-th power of the companion matrix, inclusive
Kogge-Stone scans over the spans of a block and over the blocks of the job (`threads` blocks a round, the
running state folded into the round's first item), then each span walked from its incoming state.  Nothing
is inverted but the divisor's lead."""
P = 17


def bucket_of(dl):
    return 2 if dl <= 3 else 4 if dl <= 5 else 8 if dl <= 9 else 16


def trim(p):
    n = len(p)
    while n and p[n - 1] == 0:
        n -= 1
    return n


def long_divide(num, den):
    """(quot, rem) untrimmed: max(nl - dl + 1, 1) and min(dl - 1, nl) bytes"""
    num, den = [int(v) for v in num], [int(v) for v in den]
    nl, t = len(num), len(den) - 1
    inv = pow(den[t], P - 2, P)
    R = [0] * t
    q = [0] * max(nl - t, 1)
    for i in range(nl - 1, -1, -1):
        c = inv * R[t - 1] % P
        if i < nl - t:
            q[i] = c
        R = [(num[i] - c * den[0]) % P] + [(R[j - 1] - c * den[j]) % P for j in range(1, t)]
    return bytes(q), bytes(R[:min(t, nl)])


def _matmul(a, b):
    n = len(a)
    return [[sum(a[i][l] * b[l][m] for l in range(n)) % P for m in range(n)] for i in range(n)]


def _matpow(c, e):
    n = len(c)
    r = [[int(i == m) for m in range(n)] for i in range(n)]
    while e:
        if e & 1:
            r = _matmul(r, c)
        c = _matmul(c, c)
        e >>= 1
    return r


def _vecmat(u, m, v):
    """u m + v"""
    n = len(u)
    return [(sum(u[j] * m[j][k] for j in range(n)) + v[k]) % P for k in range(n)]


def _scan(items, power):
    """inclusive scan, item 0 first: out_i = out_{i-1} x^n + item_i, by doubling; power(l) = x^(n 2^l)"""
    v = [list(x) for x in items]
    lv = 0
    while (1 << lv) < len(v):
        d = 1 << lv
        m = power(lv)
        v = [_vecmat(v[i - d], m, v[i]) if i >= d else v[i] for i in range(len(v))]
        lv += 1
    return v


def divide_chunked(num, den, chunk, threads=4, T=None):
    num, den = [int(v) for v in num], [int(v) for v in den]
    nl, t = len(num), len(den) - 1
    T = t if T is None else T
    assert T >= t >= 1 and den[t] % P and chunk >= 1 and threads >= 1
    s = T - t
    inv = pow(den[t], P - 2, P)
    D = [0] * s + den[:t]                                        # d x^s without its lead
    comp = [[int(m == i + 1) for m in range(T)] for i in range(T - 1)] + [[(-inv * D[m]) % P for m in range(T)]]
    block = chunk * threads
    nch = -(-(nl + s) // block)
    a = lambda v: num[v - s] if s <= v < nl + s else 0           # noqa: E731  the numerator at virtual index v
    ql = max(nl - t, 0)
    quot = [0] * max(ql, 1)

    def walk(S, vtop, store):
        for v in range(vtop, vtop - chunk, -1):
            c = inv * S[T - 1] % P
            if store and v < ql:
                quot[v] = c
            S = [(a(v) - c * D[0]) % P] + [(S[j - 1] - c * D[j]) % P for j in range(1, T)]
        return S

    cache = {}

    def power(n, lv):                                            # x^(n 2^lv), by squaring as the kernels do
        if (n, lv) not in cache:
            cache[n, lv] = _matpow(comp, n) if lv == 0 else _matmul(power(n, lv - 1), power(n, lv - 1))
        return cache[n, lv]

    tpow = lambda lv: power(chunk, lv)                           # noqa: E731
    bpow = lambda lv: power(block, lv)                           # noqa: E731
    tops = lambda k: [k * block + block - 1 - i * chunk for i in range(threads)]   # noqa: E731  thread 0: the top

    # phase 1: chunk aggregates (chunk 0's is not needed)
    agg = {k: _scan([walk([0] * T, vt, False) for vt in tops(k)], tpow)[-1] for k in range(1, nch)}
    # phase 2: carries, item i = chunk nch - 1 - i
    carry, run = {nch - 1: [0] * T}, None
    for i0 in range(0, nch - 1, threads):
        items = [agg[nch - 1 - i] for i in range(i0, min(i0 + threads, nch - 1))]
        if run is not None:
            items[0] = _vecmat(run, bpow(0), items[0])
        inc = _scan(items, bpow)
        for j, v in enumerate(inc):
            carry[nch - 2 - (i0 + j)] = v
        run = inc[-1]
    # phase 3: apply
    S = low = None
    for k in range(nch):
        items = [walk([0] * T, vt, False) for vt in tops(k)]
        items[0] = _vecmat(carry[k], tpow(0), items[0])
        inc = _scan(items, tpow)
        for i, vt in enumerate(tops(k)):
            S = walk(inc[i - 1] if i else carry[k], vt, True)
            assert S == inc[i]
        if k == 0:
            low = S                                              # the state below virtual index 0: r x^s
    return bytes(quot), bytes(low[s:s + min(t, nl)])
