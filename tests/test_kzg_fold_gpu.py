"""KZG folded openings (plk_kzg_open_fold_batch*, plk_kzg_verify_fold_batch*) on the GPU.

Openings: expected values are the composition the header specifies, over the oracle as
tests/test_kzg_gpu.py builds it -- y_i = oracle.poly_eval(p_i, z), F from numpy
(tests/kzg_fold_model.py), q = the quotient of oracle.poly_divide(F, [(17 - z) % 17, 1]),
proof = oracle.msm(srs[:len(q)], q).  Verification: the reference's recorded verdicts
(tests/golden/kzg_fold.json) and the Python model pinned to them by tests/test_kzg_fold_cpu.py.
Everything is exact: bytes are compared for equality."""
import numpy as np
import pytest

import gen
import kzg_fold_model as F
from conftest import load_golden

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 15, 16, 17, 255, 257, 4095, 4096, 4097, 8193, 3 * 4096 + 5, 65537]
ZS = [0, 1, 2, 5, 16]
KS = [1, 2, 3, 9, 16]
SRS_N = 65537
REC = 2176
GUARD = 32
BUDGET = 32            # polynomials per launch (csrc/kzg.hip FOLD_POLYS)


@pytest.fixture(scope="module")
def srs_pts():
    pts, _ = gen.msm_inputs(0x5125, SRS_N, "full")     # identity and the 2-torsion point included
    return pts


@pytest.fixture(scope="module")
def srs(hip, srs_pts):
    with hip.Srs(srs_pts) as s:
        assert len(s) == SRS_N and not s.irregular
        yield s


_POLY = {}


def poly(seed, n):
    """a canonical polynomial, computed once and left unchanged"""
    if (seed, n) not in _POLY:
        a, _ = gen.poly_inputs(seed, n, 0)
        a.setflags(write=False)
        _POLY[(seed, n)] = a
    return _POLY[(seed, n)]


def trim(q):
    return bytes(F.trim(np.frombuffer(bytes(q), np.uint8)))


_EXPECT = {}


def expect(oracle, pts, polys, weights, z, key=None):
    """(ys, trimmed quotient bytes, proof) of the specified composition; cached by key"""
    if key is not None and key in _EXPECT:
        return _EXPECT[key]
    Fb = F.fold(polys, weights)
    q, _ = oracle.poly_divide(Fb, [(17 - z) % 17, 1])
    r = ([oracle.poly_eval(p, z) for p in polys], bytes(q), oracle.msm(pts[:len(q)], q))
    if key is not None:
        _EXPECT[key] = r
    return r


def starts(groups):
    s = [0]
    for g in groups:
        s.append(s[-1] + len(g))
    return s


def open_dev(hip, srs, groups, weights, zs, want_quots=True, offset=0, qoffset=0, stream=None, state=None):
    """plk_kzg_open_fold_batch_dev over torch buffers -> ([[y]], [record dicts], [quotient bytes or None], state);
    want_quots: True, False or a per-group list; offset / qoffset: polynomials / quotients start that many
    bytes past a 16-byte boundary; state: (records, workspace) to reuse without re-initialising.  Guard
    bytes behind ys, every quotient and the records are checked."""
    import torch
    flat = [p for g in groups for p in g]
    lens = [len(p) for p in flat]
    st = starts(groups)
    ng = len(groups)
    wq = want_quots if isinstance(want_quots, list) else [bool(want_quots)] * ng
    dp = []
    for p in flat:
        t = torch.zeros(len(p) + 32, dtype=torch.uint8, device="cuda")
        t[offset:offset + len(p)] = torch.from_numpy(np.array(p, dtype=np.uint8)).cuda()
        assert t.data_ptr() % 16 == 0
        dp.append(t[offset:])
    Ls = [max(len(p) for p in g) for g in groups]
    dq = [torch.full((qoffset + max(L - 1, 1) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")[qoffset:] if w else None
          for L, w in zip(Ls, wq)]
    ys = torch.full((len(flat) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    if state is None:
        res = torch.zeros(ng * REC + GUARD, dtype=torch.uint8, device="cuda")
        res[ng * REC:] = 0xEE
        # the workspace needs no initialisation: hand it over dirty
        work = torch.full((hip.kzg_fold_workspace(lens, st),), 0xA5, dtype=torch.uint8, device="cuda")
    else:
        res, work = state
    torch.cuda.synchronize()
    hip.kzg_open_fold_dev(srs, dp, lens, [w for g in weights for w in g], st, zs, ys, res,
                          quots=dq if any(wq) else None, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    assert (r[ng * REC:] == 0xEE).all(), "wrote past the records"
    recs = [hip.parse_result(r[i * REC:(i + 1) * REC]) for i in range(ng)]
    quots = []
    for L, q in zip(Ls, dq):
        if q is None:
            quots.append(None)
            continue
        h = q.cpu().numpy()
        assert (h[max(L - 1, 1):] == 0xEE).all(), "wrote past max(L - 1, 1) quotient bytes"
        quots.append(bytes(h[:max(L - 1, 1)]))
    hy = ys.cpu().numpy()
    assert (hy[len(flat):] == 0xEE).all(), "wrote past the ys"
    return [[int(v) for v in hy[st[g]:st[g + 1]]] for g in range(ng)], recs, quots, (res, work)


def check_dev(out, exp, wq=None):
    dys, recs, quots, _ = out
    wq = [True] * len(exp) if wq is None else wq
    for g, e in enumerate(exp):
        assert dys[g] == e[0], g
        assert recs[g]["irregular"] == 0 and recs[g]["g1"] == e[2], g
        assert (quots[g] is None) == (not wq[g]), g
        if wq[g]:
            assert trim(quots[g]) == e[1], g


# ------------------------------------------------------------------ shapes
def sweep_groups():
    """k in KS with mixed lengths (the longest never first where k > 1), then the degenerate weights"""
    L = LENGTHS
    lens = [[4097], [15, 65537], [2, 8193, 1], [16, 17, 255, 3 * 4096 + 5, 257, 4095, 4096, 1, 2],
            [L[(5 * i + 3) % 13] for i in range(16)],
            [4096, 4097, 300], [4097, 4097], [1, 1], [257, 3 * 4096 + 5, 17]]
    assert [len(g) for g in lens[:5]] == KS and sorted(set(lens[4])) == sorted(L) and lens[4][0] != 65537
    groups = [[poly(200 + 16 * g + i, n) for i, n in enumerate(ln)] for g, ln in enumerate(lens)]
    weights = [[(3 + 5 * i + g) % 17 for i in range(len(ln))] for g, ln in enumerate(lens)]
    weights[3][2] = weights[4][0] = weights[4][7] = 0        # some zero weights
    weights[5] = [0, 0, 0]                                   # all zero: F = 0, the proof is the identity
    groups[6][1] = groups[6][0]                              # w p + (17 - w) p: F cancels to zero
    weights[6] = [6, 11]
    weights[8] = [4, 0, 9]                                   # the longest polynomial drops out: F shorter than L
    return groups, weights


@pytest.mark.parametrize("z", ZS)
def test_open_shape_sweep(hip, oracle, srs, srs_pts, z):
    groups, weights = sweep_groups()
    zs = [z] * len(groups)
    exp = [expect(oracle, srs_pts, g, w, z, key=("sweep", i, z)) for i, (g, w) in enumerate(zip(groups, weights))]
    assert exp[5][2] == exp[6][2] == bytes([0, 0, 1]) and exp[7][1] == bytes([0])
    ys, proofs = hip.kzg_open_fold(srs, groups, weights, zs)
    assert ys == [e[0] for e in exp]
    assert proofs == [e[2] for e in exp]
    wq = [i % 2 == 0 for i in range(len(groups))]           # quotients for every other group only
    check_dev(open_dev(hip, srs, groups, weights, zs, want_quots=wq), exp, wq)


def test_single_polynomial_weight_one_is_the_plain_opening(hip, srs):
    polys = [poly(100 + n, n) for n in LENGTHS]
    zs = [ZS[i % len(ZS)] for i in range(len(polys))]
    ys1, proofs1 = hip.kzg_open(srs, polys, zs)
    ys, proofs = hip.kzg_open_fold(srs, [[p] for p in polys], [[1]] * len(polys), zs)
    assert [y[0] for y in ys] == ys1 and proofs == proofs1


def test_launch_boundaries_70_groups(hip, oracle, srs, srs_pts):
    """mixed k: the polynomial total crosses the per-launch budget many times; a group is never split"""
    rng = np.random.default_rng(70)
    small = [1, 2, 15, 16, 17, 255, 257, 4095, 4096, 4097, 8193]
    ks = [int(KS[i]) for i in rng.integers(0, len(KS), 70)]
    ks[0], ks[1], ks[2] = 16, 16, 1                          # 16 + 16 fills a launch exactly; the next starts with 1
    assert sum(ks) > 6 * BUDGET
    groups = [[poly(300 + j, small[int(i)]) for j, i in enumerate(rng.integers(0, len(small), k))] for k in ks]
    weights = [[int(v) for v in rng.integers(0, 17, k)] for k in ks]
    zs = [ZS[int(i)] for i in rng.integers(0, len(ZS), 70)]
    ys, proofs = hip.kzg_open_fold(srs, groups, weights, zs)
    dys, recs, quots, _ = open_dev(hip, srs, groups, weights, zs)
    for g in range(70):
        y1, p1 = hip.kzg_open_fold(srs, [groups[g]], [weights[g]], [zs[g]])
        assert (ys[g], proofs[g]) == (y1[0], p1[0]), g
        e = expect(oracle, srs_pts, groups[g], weights[g], zs[g])
        assert (ys[g], proofs[g]) == (e[0], e[2]), g
        assert dys[g] == e[0] and recs[g]["irregular"] == 0 and recs[g]["g1"] == e[2], g
        assert trim(quots[g]) == e[1], g


# ------------------------------------------------------------------ slow paths
@pytest.mark.parametrize("where", ["first", "middle", "chunk_1", "last"])
def test_non_canonical_coefficient_bytes(hip, oracle, srs, srs_pts, where):
    n = 9000
    pos = {"first": 0, "middle": 3001, "chunk_1": 4100, "last": n - 1}[where]
    bad = poly(31, n).copy()
    bad[pos] = 200
    mid = [poly(34, 5000), bad, poly(35, 17)]
    left, right = [poly(32, 4500), poly(36, 4097)], [poly(33, n)]
    groups, weights = [left, mid, right], [[3, 16], [5, 7, 1], [9]]
    for z in (0, 5):
        zs = [z, z, z]
        # host form = the composition: ys through the eval path, the proof that of the plain opening of F
        Fb = F.fold(mid, weights[1])
        assert np.array_equal(Fb, F.fold([mid[0], bad % 17, mid[2]], weights[1]))
        _, pf = hip.kzg_open(srs, [Fb], [z])
        ys, proofs = hip.kzg_open_fold(srs, groups, weights, zs)
        assert ys[1] == [hip.poly_eval(p, z) for p in mid] and proofs[1] == pf[0], (where, z)
        el, er = expect(oracle, srs_pts, left, weights[0], z), expect(oracle, srs_pts, right, weights[2], z)
        assert (ys[0], proofs[0]) == (el[0], el[2]) and (ys[2], proofs[2]) == (er[0], er[2])
        # device form: that group flagged, its quotient bytes still exact, its neighbours exact
        dys, recs, quots, _ = open_dev(hip, srs, groups, weights, zs)
        assert recs[1]["irregular"] > 0, (where, z)
        q, _ = oracle.poly_divide(Fb, [(17 - z) % 17, 1])
        assert trim(quots[1]) == bytes(q), (where, z)
        assert recs[0]["irregular"] == 0 and recs[0]["g1"] == el[2] and dys[0] == el[0] and trim(quots[0]) == el[1]
        assert recs[2]["irregular"] == 0 and recs[2]["g1"] == er[2] and dys[2] == er[0] and trim(quots[2]) == er[1]


def test_irregular_srs(hip, oracle):
    n = 5000
    pts, _ = gen.msm_inputs(0x1229, n + 100, "full")
    pts = pts.copy()
    pts[2500] = (3, 3, 0)                              # off-curve
    groups = [[poly(42, 600), poly(41, n), poly(43, 4097)], [poly(44, 17)]]
    weights = [[2, 9, 16], [0]]
    with hip.Srs(pts) as s:
        assert s.irregular
        for z in (0, 7):
            exp = [expect(oracle, pts, g, w, z) for g, w in zip(groups, weights)]
            ys, proofs = hip.kzg_open_fold(s, groups, weights, [z, z])
            assert ys == [e[0] for e in exp] and proofs == [e[2] for e in exp], z
            dys, recs, quots, _ = open_dev(hip, s, groups, weights, [z, z])
            assert all(r["irregular"] > 0 for r in recs)
            assert dys == ys and [trim(q) for q in quots] == [e[1] for e in exp]   # exact whatever the SRS


def test_srs_boundary(hip, oracle):
    n = 4100
    pts, _ = gen.msm_inputs(0xB0, n, "full")
    with hip.Srs(pts) as s:
        g, w = [poly(64, 300), poly(61, n + 1)], [5, 3]        # L - 1 == srs_len
        e = expect(oracle, pts, g, w, 4)
        assert len(e[1]) == n
        ys, proofs = hip.kzg_open_fold(s, [g], [w], [4])
        assert (ys[0], proofs[0]) == (e[0], e[2])
        check_dev(open_dev(hip, s, [g], [w], [4]), [e])
        over = [poly(64, 300), poly(62, n + 2)]
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open_fold(s, [over], [[5, 0]], [4])        # on the lengths as given, whatever the weights
        assert err.value.code == hip.PLK_ERR_RANGE and "degree exceeds SRS size" in str(err.value)
        with pytest.raises(hip.PlonkHipError) as err:
            open_dev(hip, s, [over], [w], [4])
        assert err.value.code == hip.PLK_ERR_RANGE


# ------------------------------------------------------------------ the device API
def api_case(oracle, srs_pts):
    groups = [[poly(117, 17), poly(500, 4097)], [poly(501, 8193), poly(502, 4096), poly(503, 3 * 4096 + 5)], [poly(504, 300)]]
    weights = [[1, 16], [7, 0, 12], [3]]
    zs = [2, 0, 16]
    exp = [expect(oracle, srs_pts, g, w, z, key=("api", i)) for i, (g, w, z) in enumerate(zip(groups, weights, zs))]
    return groups, weights, zs, exp


def test_device_api_unaligned_polynomials_and_quotients(hip, oracle, srs, srs_pts):
    groups, weights, zs, exp = api_case(oracle, srs_pts)
    for off in range(1, 16):
        check_dev(open_dev(hip, srs, groups, weights, zs, offset=off, qoffset=16 - off), exp)
        check_dev(open_dev(hip, srs, groups, weights, zs, offset=0, qoffset=off), exp)


def test_device_api_state_and_streams(hip, oracle, srs, srs_pts):
    import torch
    groups, weights, zs, exp = api_case(oracle, srs_pts)
    # quotients wanted for some groups only
    part = [False, True, False]
    check_dev(open_dev(hip, srs, groups, weights, zs, want_quots=part), exp, part)
    # two calls back to back on the same records and (dirty) workspace, nothing re-initialised
    first = open_dev(hip, srs, groups, weights, zs, want_quots=False)
    check_dev(first, exp, [False] * 3)
    second = open_dev(hip, srs, groups, weights, zs, want_quots=False, state=first[3])
    check_dev(second, exp, [False] * 3)
    assert second[:2] == first[:2]                             # a repeated call gives identical bytes
    # a non-default stream
    check_dev(open_dev(hip, srs, groups, weights, zs, stream=torch.cuda.Stream()), exp)


def test_two_streams_with_distinct_workspaces(hip, oracle, srs, srs_pts):
    import torch
    groups, weights, zs, exp = api_case(oracle, srs_pts)
    flat = [p for g in groups for p in g]
    lens, st = [len(p) for p in flat], starts(groups)
    dp = [torch.from_numpy(np.array(p, dtype=np.uint8)).cuda() for p in flat]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(2):
        outs.append((torch.full((len(flat),), 0xEE, dtype=torch.uint8, device="cuda"),
                     torch.zeros(len(groups) * REC, dtype=torch.uint8, device="cuda"),
                     torch.full((hip.kzg_fold_workspace(lens, st),), 0xA5, dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    for (ys, res, work), s in zip(outs, (s1, s2)):
        hip.kzg_open_fold_dev(srs, dp, lens, [w for g in weights for w in g], st, zs, ys, res, work=work, stream=s)
    s1.synchronize()
    s2.synchronize()
    for ys, res, _ in outs:
        r = res.cpu().numpy()
        assert [hip.parse_result(r[i * REC:(i + 1) * REC])["g1"] for i in range(len(groups))] == [e[2] for e in exp]
        assert ys.cpu().numpy().tolist() == [y for e in exp for y in e[0]]


def test_larger_case_k9_ragged(hip, oracle):
    n = (1 << 18) + 5
    pts, _ = gen.msm_inputs(0x1A26E, n, "full")
    lens = [n - 4096 * 3, 1 << 17, n, 4097, n - 1, 1 << 18, 17, n - 16, 12345]
    g = [poly(700 + i, m) for i, m in enumerate(lens)]
    w = [1, 5, 16, 0, 3, 9, 11, 2, 7]
    e = expect(oracle, pts, g, w, 3)
    with hip.Srs(pts) as s:
        ys, proofs = hip.kzg_open_fold(s, [g], [w], [3])
        assert ys == [e[0]] and proofs == [e[2]]
        check_dev(open_dev(hip, s, [g], [w], [3]), [e])


# ------------------------------------------------------------------ verification
class Gold:
    """tests/golden/kzg_fold.json joined with its inputs, which are rebuilt from the recorded seeds"""

    def __init__(self):
        import make_kzg_fold_golden as mk
        self.raw = load_golden("kzg_fold.json")
        self.key = bytes.fromhex(self.raw["key"])
        _, verify, self.cases = mk.expand(self.raw)
        self.rows = {k: verify[k][0] for k in KS}
        self.bits = {k: verify[k][1] for k in KS}

    def std(self, k):
        """the rows recorded under the s = 2 key, and their verdicts"""
        m = (self.rows[k][:, :7] == np.frombuffer(self.key, np.uint8)).all(1)
        return self.rows[k][m], self.bits[k][m]


@pytest.fixture(scope="module")
def gold():
    return Gold()


def vk_of(hip, b):
    b = bytes(b)
    return hip.KzgVk(b[0:3], b[3:5], b[5:7])


def columns(rows, k):
    """(commits n k x 3, weights n k, ys n k, zs n, proofs n x 3) of recorded rows"""
    ent = rows[:, 7:7 + 5 * k].reshape(-1, k, 5)
    return (np.ascontiguousarray(ent[:, :, :3]), np.ascontiguousarray(ent[:, :, 3]), np.ascontiguousarray(ent[:, :, 4]),
            np.ascontiguousarray(rows[:, -1]), np.ascontiguousarray(rows[:, 7 + 5 * k:10 + 5 * k]))


def on_device(a, offset=0):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    t = torch.full((offset + a.size + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[offset:offset + a.size] = torch.from_numpy(a.copy()).cuda()
    return t[offset:]


def verify_dev(hip, vk, k, cols, offset=0, stream=None):
    import torch
    n = cols[3].size
    d = [on_device(a, offset) for a in cols]
    ok = torch.full((offset + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")[offset:]
    torch.cuda.synchronize()
    hip.kzg_verify_fold_dev(vk, k, d[0], d[1], d[2], d[3], d[4], n, ok, stream=stream)
    torch.cuda.synchronize()
    h = ok.cpu().numpy()
    assert (h[n:] == 0xEE).all(), "wrote past the output"
    return h[:n].copy()


def verify_both(hip, vk, k, cols, form, offset=0):
    return hip.kzg_verify_fold(vk, k, *cols) if form == "host" else verify_dev(hip, vk, k, cols, offset)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("k", KS)
def test_verify_every_golden_job(hip, gold, k, form):
    """the jobs under the s = 2 key in one call; the jobs carrying their own key one call each"""
    rows, bits = gold.std(k)
    got = verify_both(hip, vk_of(hip, gold.key), k, columns(rows, k), form)
    bad = np.flatnonzero(got != bits)
    assert bad.size == 0 and 0 < bits.sum() < bits.size, (bad[:8], rows[bad[:8]].tolist())
    own = np.flatnonzero((gold.rows[k][:, :7] != np.frombuffer(gold.key, np.uint8)).any(1))
    assert own.size >= 50
    for i in own:
        r = gold.rows[k][i:i + 1]
        assert verify_both(hip, vk_of(hip, r[0, :7]), k, columns(r, k), form)[0] == gold.bits[k][i], (k, int(i))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256 + 1])
def test_verify_batch_sizes(hip, gold, n):
    """the recorded jobs tiled; the largest wraps the grid-stride loop; expectations from the model"""
    k = 3
    rows, _ = gold.std(k)
    base = model_std(gold, k)
    reps = -(-n // len(rows))
    tiled = np.tile(rows, (reps, 1))[:n]
    exp = np.tile(base, reps)[:n]
    assert np.array_equal(verify_dev(hip, vk_of(hip, gold.key), k, columns(tiled, k)), exp)
    if n <= 257:
        assert np.array_equal(hip.kzg_verify_fold(vk_of(hip, gold.key), k, *columns(tiled, k)), exp)


def F_key(gold):
    b = tuple(gold.key)
    return (b[0:3], b[3:5], b[5:7])


_MODEL = {}


def model_std(gold, k):
    """the model's verdicts of the rows recorded under the s = 2 key, computed once"""
    if k not in _MODEL:
        rows, bits = gold.std(k)
        _MODEL[k] = F.verify_fold_batch(F_key(gold), k, *columns(rows, k))
        assert np.array_equal(_MODEL[k], bits) and 0 < bits.sum() < bits.size
    return _MODEL[k]


# (column of the 7 + 5 k + 4 byte row relative to an entry or the tail, value)
ENTRY_INVALID = {"c_x_101": (0, 101), "c_y_255": (1, 255), "c_flag_2": (2, 2), "weight_17": (3, 17), "weight_255": (3, 255),
                 "y_17": (4, 17)}
TAIL_INVALID = {"w_x_255": (0, 255), "w_y_101": (1, 101), "w_flag_2": (2, 2), "z_17": (3, 17), "z_255": (3, 255)}


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("kind", sorted(ENTRY_INVALID) + sorted(TAIL_INVALID))
def test_verify_invalid_byte(hip, gold, kind, k):
    """at the first and at the last entry of a job, for the first job, a block's last and the batch's last"""
    rows, _ = gold.std(k)
    base = np.tile(rows, (2, 1))[:257].copy()
    vk = F_key(gold)
    exp0 = np.tile(model_std(gold, k), 2)[:257]
    for entry in sorted({0, k - 1}):
        jobs, exp = base.copy(), exp0.copy()
        for pos in (0, 255, 256):
            if kind in ENTRY_INVALID:
                col, val = ENTRY_INVALID[kind]
                jobs[pos, 7 + 5 * entry + col] = val
            else:
                col, val = TAIL_INVALID[kind]
                jobs[pos, 7 + 5 * k + col] = val
            exp[pos] = 2
        assert F.verify_fold_batch(vk, k, *columns(jobs[:1], k))[0] == 2
        for form in ("host", "dev"):
            assert np.array_equal(verify_both(hip, vk_of(hip, gold.key), k, columns(jobs, k), form), exp), (form, entry)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_verify_unaligned_device_buffers_and_guards(hip, gold, offset):
    for k in (2, 16):
        rows, bits = gold.std(k)
        assert np.array_equal(verify_dev(hip, vk_of(hip, gold.key), k, columns(rows, k), offset), bits)


def test_verify_non_default_stream_and_repeat(hip, gold):
    import torch
    rows, bits = gold.std(9)
    cols = columns(rows, 9)
    vk = vk_of(hip, gold.key)
    first = verify_dev(hip, vk, 9, cols, stream=torch.cuda.Stream())
    assert np.array_equal(first, bits)
    assert np.array_equal(verify_dev(hip, vk, 9, cols), first)
    assert np.array_equal(hip.kzg_verify_fold(vk, 9, *cols), first)


# ------------------------------------------------------------------ end to end with commit and open, s = 2
def unhex(s):
    return list(bytes.fromhex(s))


def test_end_to_end_commit_open_verify(hip, gold):
    """the library's commitments and folded openings are the reference's, every honest group is accepted,
    and an altered y_i, weight or proof gets the model's (= the reference's recorded) verdict -- over GF(17)
    one alteration in 17 is accepted by arithmetic"""
    cases = gold.cases
    srs_pts = np.array(unhex(gold.raw["srs"]), np.uint8).reshape(-1, 3)
    vk, key = vk_of(hip, gold.key), F_key(gold)
    groups = [[np.array(p, np.uint8) for p in c["polys"]] for c in cases]
    weights = [c["weights"] for c in cases]
    zs = [c["z"] for c in cases]
    with hip.Srs(srs_pts) as srs:
        assert not srs.irregular
        commits = [hip.kzg_commit(srs, g) for g in groups]
        ys, proofs = hip.kzg_open_fold(srs, groups, weights, zs)
    rejected = 0
    for n, c in enumerate(cases):
        k = len(groups[n])
        assert [tuple(x) for x in commits[n]] == c["commits"], n
        assert ys[n] == c["ys"] and tuple(proofs[n]) == c["proof"], n
        variants = c["variants"]                                   # honest, one y_i, one weight, the proof altered
        assert variants[0] == (weights[n], ys[n], tuple(proofs[n])), n
        cols = (np.array([c["commits"]] * 4, np.uint8), np.array([v[0] for v in variants], np.uint8),
                np.array([v[1] for v in variants], np.uint8), np.array([zs[n]] * 4, np.uint8),
                np.array([v[2] for v in variants], np.uint8))
        model = F.verify_fold_batch(key, k, *cols)
        assert "".join(str(int(b)) for b in model) == c["bits"] and model[0] == 1, n
        for form in ("host", "dev"):
            assert np.array_equal(verify_both(hip, vk, k, cols, form), model), (n, form)
        rejected += int((model[1:] == 0).sum())
    assert rejected > 2 * len(cases)
