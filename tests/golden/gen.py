"""Seeded synthetic inputs shared by the golden-fixture script, the tests and bench.py.

Counter-based SplitMix64 (vectorised numpy, bit-stable across platforms):
    r_i = mix(seed + (i + 1) * 0x9E3779B97F4A7C15),  i = 0, 1, ...
Every stream is a pure function of (seed, n).
"""
import numpy as np

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)

# kG for k = 0..16 on y^2 = x^3 + 3 over GF(101), G = (1, 2) (src/g1.h:22-24);
# pinned by tests/golden/g1.json (k = 0 is the identity {0, 0, 1}).
KG = [(0, 0, 1), (1, 2, 0), (68, 74, 0), (26, 45, 0), (65, 98, 0), (12, 32, 0), (32, 42, 0),
      (91, 35, 0), (18, 49, 0), (18, 52, 0), (91, 66, 0), (32, 59, 0), (12, 69, 0),
      (65, 3, 0), (26, 56, 0), (68, 27, 0), (1, 99, 0)]


def splitmix64(seed, n, offset=0):
    with np.errstate(over="ignore"):
        i = np.arange(offset + 1, offset + n + 1, dtype=np.uint64)
        z = np.uint64(seed) + i * _GOLD
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def all_points():
    """The 102 elements of E(F101) as canonical 3-byte encodings, identity first, then
    affine points in (x, y) order."""
    pts = [(0, 0, 1)]
    for x in range(101):
        rhs = (x * x * x + 3) % 101
        for y in range(101):
            if (y * y) % 101 == rhs:
                pts.append((x, y, 0))
    return np.array(pts, dtype=np.uint8)


def msm_inputs(seed, n, kind="subgroup"):
    """(points[n,3] uint8, scalars[n] uint8).

    kind = "subgroup": points kG, k uniform in [1,16]; scalars uniform in [0,16]
    kind = "full":     points uniform over all 102 group elements (identity and the
                       2-torsion point (48,0) included); scalars uniform in [0,16]
    kind = "bytes":    subgroup points; scalars uniform over all 256 byte values
                       (g1_mul takes the raw HF byte as a uint64 scalar, src/srs.h:63)
    """
    r = splitmix64(seed, 2 * n)
    rp, rs = r[:n], r[n:]
    if kind in ("subgroup", "bytes"):
        table = np.array(KG[1:], dtype=np.uint8)
        pts = table[(rp % np.uint64(16)).astype(np.int64)]
    elif kind == "full":
        table = all_points()
        pts = table[(rp % np.uint64(102)).astype(np.int64)]
    else:
        raise ValueError(kind)
    if kind == "bytes":
        sc = (rs & np.uint64(0xFF)).astype(np.uint8)
    else:
        sc = (rs % np.uint64(17)).astype(np.uint8)
    return np.ascontiguousarray(pts), np.ascontiguousarray(sc)


def poly_inputs(seed, la, lb, lead_nonzero=True, modulus=17):
    """Two coefficient vectors (uint8) with entries uniform in [0, modulus)."""
    r = splitmix64(seed, la + lb)
    a = (r[:la] % np.uint64(modulus)).astype(np.uint8)
    b = (r[la:] % np.uint64(modulus)).astype(np.uint8)
    if lead_nonzero:
        if la:
            a[-1] = 1 + a[-1] % 16
        if lb:
            b[-1] = 1 + b[-1] % 16
    return a, b


def digest(c):
    """SHA-256 of the raw bytes, hex -- the fixture digest for long outputs."""
    import hashlib
    return hashlib.sha256(np.asarray(c, dtype=np.uint8).tobytes()).hexdigest()


CIRCUIT_KINDS = ("identity", "respect17", "respect3", "perm", "map", "degenerate", "mixed",
                 "gate", "gate2", "gate_last", "copy3", "copy255", "copy_gate")


def _draw(r, count, modulus):
    """the next `count` values of the stream r (a list holding one array) reduced mod `modulus`"""
    out = (r[0][:count] % np.uint64(modulus)).astype(np.int64)
    r[0] = r[0][count:]
    return out


def _shuffle(r, items):
    """a uniform permutation of `items`: ordered by fresh 64-bit keys (stable, so bit-exact anywhere)"""
    keys = r[0][:len(items)]
    r[0] = r[0][len(items):]
    return [items[i] for i in np.argsort(keys, kind="stable")]


def prove_circuit(n, kind, seed):
    """One n-gate circuit with challenges and blinding, a pure function of (n, kind, seed): the dict of
    tests/golden/prove.json's cases (gates 5n: q_m q_l q_r q_o q_c; copies 6n: c_a c_b c_c as (type, index)
    pairs; wires 3n: a b c; chal 5; rand 9).  All bytes canonical (< 17, copy types 0-2 except where the kind
    says otherwise, copy indices 1..n).  Every gate holds by construction: selectors, a and b random, c solved
    through q_o where q_o != 0 and q_c solved otherwise.

    kind (one of CIRCUIT_KINDS, optionally followed by "+b1" for a blinding scalar b1 != 0 and plain challenges):
      identity   every wire slot its own copy
      respect17  a random permutation inside each class of equal wire values over all 3n slots, wires from 17 values
      respect3   the same with a, b and the free c from 3 values: large classes that cross columns
      perm       an arbitrary permutation of the 3n slots
      map        an arbitrary map of the 3n slots (not injective)
      degenerate zero selectors, constant wires, identity copies, beta = 0 in half the draws
      mixed      zero selectors, wires constant per column, identity or value-respecting copies
      gate / gate2 / gate_last   "respect17" with one wire c changed at a random gate / at two gates / at gate n - 1
      copy3 / copy255 / copy_gate  "respect17" with one copy type set to 3 / to 255 / to 3 and one gate failing too
    Challenges and blinding are uniform, with beta = 0, gamma = 0, beta = gamma = 0, b7 = b8 = b9 = 0 and all
    blinding zero each mixed in at one draw in sixteen."""
    base, _, mod = kind.partition("+")
    assert mod in ("", "b1") and 1 <= n <= 16
    r = [splitmix64(int(seed) * 1000003 + 4099 * n + CIRCUIT_KINDS.index(base), 16 * n + 64)]
    p = 17
    sel = _draw(r, 5 * n, p).reshape(5, n)
    q_m, q_l, q_r, q_o, q_c = sel
    vals = 3 if base == "respect3" else p
    a, b, c = _draw(r, 3 * n, vals).reshape(3, n)
    if vals == 3:                                   # three values spread over the field, not 0 1 2
        spread = _draw(r, 3, p)
        a, b, c = spread[a], spread[b], spread[c]
    else:
        _draw(r, 3, p)
    if base in ("degenerate", "mixed"):
        sel[:] = 0
        col = _draw(r, 3, p)
        if base == "degenerate":
            col[:] = col[0]
        a, b, c = (np.full(n, v, np.int64) for v in col)
    else:
        _draw(r, 3, p)
    rest = (q_l * a + q_r * b + q_m * (a * b % p)) % p
    for i in range(n):
        if q_o[i]:
            c[i] = (p - (rest[i] + q_c[i]) % p) * pow(int(q_o[i]), p - 2, p) % p
        else:
            q_c[i] = (p - rest[i]) % p
    wires = np.concatenate([a, b, c])
    slots = list(range(3 * n))
    how = {"identity": "identity", "degenerate": "identity", "perm": "perm", "map": "map"}.get(base, "respect")
    pick = _draw(r, 1, 2)[0]
    if base == "mixed" and pick:
        how = "identity"
    if how == "identity":
        _shuffle(r, slots)
        target = slots
    elif how == "perm":
        target = _shuffle(r, slots)
    elif how == "map":
        target = [int(x) for x in _draw(r, 3 * n, 3 * n)]
    else:
        order = _shuffle(r, slots)                  # class members in a random order: source -> next member
        target = list(slots)
        for v in range(p):
            cls = [s for s in slots if wires[s] == v]
            img = [s for s in order if wires[s] == v]
            for s, t in zip(cls, img):
                target[s] = t
    copies = [x for t in target for x in (t // n, t % n + 1)]
    extra = _draw(r, 8, 1 << 30)
    wires = [int(x) for x in wires]
    if base in ("gate", "gate2", "gate_last", "copy_gate"):
        g = n - 1 if base == "gate_last" else int(extra[0] % n)
        hit = {g, int(extra[1] % n)} if base == "gate2" else {g}
        for i in hit:                               # the changed c must count: q_o = 1 at that gate, c off by 1..16
            sel[3][i] = 1
            wires[2 * n + i] = int((p - (rest[i] + q_c[i]) % p) % p + 1 + extra[2] % 16) % p
    if base in ("copy3", "copy255", "copy_gate"):
        copies[2 * int(extra[3] % (3 * n))] = 255 if base == "copy255" else 3
    chal = [int(x) for x in _draw(r, 5, p)]
    rand = [int(x) for x in _draw(r, 9, p)]
    variant = int(_draw(r, 1, 16)[0])
    if mod == "b1":
        rand[0] = 1 + rand[0] % 16
    elif base == "degenerate":
        if variant < 8:
            chal[1] = 0
    elif variant == 0:
        chal[1] = 0
    elif variant == 1:
        chal[2] = 0
    elif variant == 2:
        chal[1] = chal[2] = 0
    elif variant == 3:
        rand[6] = rand[7] = rand[8] = 0
    elif variant == 4:
        rand = [0] * 9
    return {"gates": [int(x) for x in sel.reshape(-1)], "copies": copies, "wires": wires, "chal": chal, "rand": rand}


def circuit_bytes(c):
    """the 14n bytes of one prove_batch entry: q_m q_l q_r q_o q_c | copy_a copy_b copy_c | a b c"""
    return bytes(c["gates"]) + bytes(c["copies"]) + bytes(c["wires"])


def prove_instance(n, seed, srs_len):
    """Prove-shaped synthetic instance (rounds 1-5 at n gates): 13 random 'interpolated'
    polynomials of length n, challenges / blinding scalars, Z_H = x^n - 1, an SRS over the whole
    group (tests/test_prove_gpu.py, tests/golden/make_prove_2_20.py, bench.py)."""
    r = splitmix64(seed, 13 * n + 64)
    polys = [(r[i * n:(i + 1) * n] % np.uint64(17)).astype(np.uint8) for i in range(13)]
    chal = [int(x % np.uint64(17)) for x in r[13 * n:13 * n + 5]]
    rnd = [int(x % np.uint64(17)) for x in r[13 * n + 5:13 * n + 14]]
    chal[3] = max(chal[3], 2)            # z: avoid the degenerate z in {0, 1}
    zh = np.zeros(n + 1, np.uint8)
    zh[0], zh[n] = 16, 1
    pts, _ = msm_inputs(seed ^ 0x5A5A, srs_len, "full")
    return polys, chal, rnd, zh, pts
