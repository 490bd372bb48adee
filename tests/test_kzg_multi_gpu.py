"""KZG multi-point openings (plk_kzg_open_multi_batch*, plk_kzg_verify_multi_batch*) on the GPU.

Openings: expected values come from tests/kzg_multi_model.py (numpy; pinned to the compiled reference by
tests/test_kzg_multi_cpu.py) with the commitments folded by the oracle, and from the composition of the
library's own host calls that the header names as the specification.  Verification: the reference's recorded
verdicts (tests/golden/kzg_multi.json) and the model.  Everything is exact: bytes are compared for equality."""
import numpy as np
import pytest

import gen
import kzg_multi_model as MM
from conftest import load_golden

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 15, 16, 17, 255, 257, 4095, 4096, 4097, 8193, 3 * 4096 + 5, 65537]
SRS_N = 65537
REC = 2176
GUARD = 32
PER_LAUNCH = 4         # whole groups per launch (csrc/kzg_multi.hip MULTI_GROUPS)
FULL = MM.FULL
Z, ZW = 3, 12          # a point and its image under omega = 4
NONZERO16 = FULL & ~1
LOW16 = 0xFFFF         # {0 .. 15}


def rule_srs(n):
    """the golden file's rule, srs[i] = (2^i mod 17) G: a well-formed SRS for s = 2"""
    kg = np.array(gen.KG, np.uint8)
    return np.ascontiguousarray(kg[[pow(2, i % 8, 17) for i in range(n)]])    # (2 has order 8 mod 17)


@pytest.fixture(scope="module")
def srs_pts():
    return rule_srs(SRS_N)


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


def seeded_masks(seed, n):
    import make_kzg_multi_golden as mk
    r = [int(v >> np.uint64(8)) for v in gen.splitmix64(seed, 3 * n)]
    return [mk.random_mask(r[3 * i], r[3 * i + 1], r[3 * i + 2] % 3) for i in range(n)]


_EXPECT = {}


def expect(oracle, pts, polys, sets, weights, u, key=None):
    """(17-byte rows, h untrimmed, W + W' 6 bytes) of the model, the commitments folded by the oracle"""
    if key is not None and key in _EXPECT:
        return _EXPECT[key]
    ys, h, W, Wp = MM.open_multi(pts, polys, sets, weights, u, msm=lambda p, s: bytes(oracle.msm(p, s)))
    k = len(polys)
    r = ([bytes(ys[17 * i:17 * i + 17]) for i in range(k)], bytes(h), W + Wp)
    if key is not None:
        _EXPECT[key] = r
    return r


def compose(hip, srs, polys, sets, weights, u):
    """the header's specification through the library's own host calls -> (rows, h over Lh, W + W')"""
    rows = [bytes(hip.poly_eval(p, a) if (m >> a) & 1 else 0xFF for a in range(17)) for p, m in zip(polys, sets)]
    dens = [hip.poly_from_roots(MM.points(m)) for m in sets]
    qs = [q for q, _ in hip.poly_divide_short_batch(polys, dens)]
    lh = max(max(len(p) - len(MM.points(m)), 1) for p, m in zip(polys, sets))
    hb, hl = hip.poly_lincomb(([hip.lc_term(q, scale=w) for q, w in zip(qs, weights)], None))
    h = np.zeros(lh, np.uint8)
    h[:len(hb)] = np.frombuffer(hb, np.uint8)
    W = hip.kzg_commit(srs, [h[:hl]])[0]
    c = hip.kzg_multi_coeffs(sets, weights, u)
    _, pf = hip.kzg_open_fold(srs, [list(polys) + [h]], [c], [u])
    return rows, bytes(h), W + pf[0]


def starts(groups):
    s = [0]
    for g in groups:
        s.append(s[-1] + len(g))
    return s


def lh_of(g, s):
    return max(max(len(p) - len(MM.points(m)), 1) for p, m in zip(g, s))


def open_dev(hip, srs, groups, sets, weights, us, want_hs=True, offset=0, hoffset=0, stream=None, state=None):
    """plk_kzg_open_multi_batch_dev over torch buffers -> ([[row]], [record dicts, two per group], [h or None], state);
    want_hs: True, False or a per-group list; offset / hoffset: polynomials / h buffers start that many bytes past
    a 16-byte boundary; state: (records, workspace) to reuse without re-initialising.  Guard bytes behind ys, every
    h and the records are checked."""
    import torch
    flat = [p for g in groups for p in g]
    fsets = [m for s in sets for m in s]
    lens = [len(p) for p in flat]
    st = starts(groups)
    ng = len(groups)
    wh = want_hs if isinstance(want_hs, list) else [bool(want_hs)] * ng
    dp = []
    for p in flat:
        t = torch.zeros(len(p) + 32, dtype=torch.uint8, device="cuda")
        t[offset:offset + len(p)] = torch.from_numpy(np.array(p, dtype=np.uint8)).cuda()
        assert t.data_ptr() % 16 == 0
        dp.append(t[offset:])
    Ls = [lh_of(g, s) for g, s in zip(groups, sets)]
    dh = [torch.full((hoffset + L + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")[hoffset:] if w else None
          for L, w in zip(Ls, wh)]
    ys = torch.full((17 * len(flat) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    if state is None:
        res = torch.zeros(2 * ng * REC + GUARD, dtype=torch.uint8, device="cuda")
        res[2 * ng * REC:] = 0xEE
        # the workspace needs no initialisation: hand it over dirty
        work = torch.full((hip.kzg_multi_workspace(lens, fsets, st),), 0xA5, dtype=torch.uint8, device="cuda")
    else:
        res, work = state
    torch.cuda.synchronize()
    hip.kzg_open_multi_dev(srs, dp, lens, fsets, [w for g in weights for w in g], st, us, ys, res,
                           hs=dh if any(wh) else None, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    assert (r[2 * ng * REC:] == 0xEE).all(), "wrote past the records"
    recs = [hip.parse_result(r[i * REC:(i + 1) * REC]) for i in range(2 * ng)]
    hs = []
    for L, q in zip(Ls, dh):
        if q is None:
            hs.append(None)
            continue
        b = q.cpu().numpy()
        assert (b[L:] == 0xEE).all(), "wrote past Lh bytes of h"
        hs.append(bytes(b[:L]))
    hy = ys.cpu().numpy()
    assert (hy[17 * len(flat):] == 0xEE).all(), "wrote past the ys"
    rows = [[bytes(hy[17 * i:17 * i + 17]) for i in range(st[g], st[g + 1])] for g in range(ng)]
    return rows, recs, hs, (res, work)


def check_dev(out, exp, wh=None):
    rows, recs, hs, _ = out
    wh = [True] * len(exp) if wh is None else wh
    for g, e in enumerate(exp):
        assert rows[g] == e[0], g
        assert recs[2 * g]["irregular"] == 0 and recs[2 * g + 1]["irregular"] == 0, g
        assert recs[2 * g]["g1"] + recs[2 * g + 1]["g1"] == e[2], g
        assert (hs[g] is None) == (not wh[g]), g
        if wh[g]:
            assert hs[g] == e[1], g


# ------------------------------------------------------------------ shapes
def sweep_groups():
    """k in {1, 2, 9, 15} with ragged lengths (the longest never first where k > 1) and every kind of set, then the
    degenerate weights"""
    L = LENGTHS
    lens = [[4097], [15, 65537], [8193, 1], [16, 17, 255, 3 * 4096 + 5, 257, 4095, 4096, 1, 2],
            [L[(5 * i + 3) % 13] for i in range(15)],
            [4096, 4097, 300], [4097, 4097], [1, 1], [257, 3 * 4096 + 5, 17]]
    sets = [[1], [1 << 5, 1 | 1 << 5], [1 << Z | 1 << ZW, NONZERO16],
            [1 << 5, LOW16, 1 << Z | 1 << ZW, NONZERO16, 0b101, 1, LOW16, 1 << 7, 0b110],
            seeded_masks(0x5E75, 15),
            [1 | 1 << 5, 1 << 5, 1], [1 << Z | 1 << ZW] * 2, [1, 1 << 5], [0b1001, 1 << 16, LOW16]]
    assert [len(g) for g in lens[:5]] == [1, 2, 2, 9, 15] and sorted(set(lens[4])) == sorted(L) and lens[4][0] != 65537
    # len <= t (1 and 2 against sixteen points and a pair), len = t + 1 (17 against {0 .. 15}), len = 1
    assert (lens[3][1], sets[3][1]) == (17, LOW16) and (lens[3][7], lens[3][8]) == (1, 2) and lens[8][2] == 17
    groups = [[poly(200 + 16 * g + i, n) for i, n in enumerate(ln)] for g, ln in enumerate(lens)]
    weights = [[(3 + 5 * i + g) % 17 or 1 for i in range(len(ln))] for g, ln in enumerate(lens)]
    weights[3][2] = weights[4][0] = weights[4][7] = 0        # some zero weights
    weights[5] = [0, 0, 0]                                   # all zero: h = 0, W is the identity
    groups[6][1] = groups[6][0]                              # w p + (17 - w) p over one set: h cancels to zero
    weights[6] = [6, 11]
    weights[8] = [4, 0, 9]                                   # the longest polynomial drops out of h
    return groups, sets, weights


def u_of(sets, kind):
    T = 0
    for m in sets:
        T |= m
    if kind == "zero":
        return 0
    inside, outside = MM.points(T), MM.points(FULL & ~T)
    if kind == "inside":
        return inside[-1]
    return outside[-1] if outside else inside[0]


@pytest.mark.parametrize("ukind", ["zero", "inside", "outside"])
def test_open_shape_sweep(hip, oracle, srs, srs_pts, ukind):
    groups, sets, weights = sweep_groups()
    us = [u_of(s, ukind) for s in sets]
    exp = [expect(oracle, srs_pts, g, s, w, u, key=("sweep", i, u))
           for i, (g, s, w, u) in enumerate(zip(groups, sets, weights, us))]
    assert exp[5][2][:3] == exp[6][2][:3] == bytes([0, 0, 1]) and exp[7][1] == bytes([0])
    rows, proofs = hip.kzg_open_multi(srs, groups, sets, weights, us)
    assert rows == [e[0] for e in exp]
    assert proofs == [e[2] for e in exp]
    wh = [i % 2 == 0 for i in range(len(groups))]           # h for every other group only
    check_dev(open_dev(hip, srs, groups, sets, weights, us, want_hs=wh), exp, wh)


def test_every_set_at_one_point_is_the_folded_opening(hip, srs):
    groups = [[poly(100 + n, n) for n in LENGTHS[3:12]], [poly(120, 4097)], [poly(121, 1), poly(122, 300)]]
    weights = [[(2 + 3 * i) % 17 for i in range(9)], [5], [1, 16]]
    zs = [5, 0, 16]
    ys1, proofs1 = hip.kzg_open_fold(srs, groups, weights, zs)
    rows, proofs = hip.kzg_open_multi(srs, groups, [[1 << z] * len(g) for g, z in zip(groups, zs)], weights, [7, 7, 0])
    for g, z in enumerate(zs):
        assert [r[z] for r in rows[g]] == ys1[g] and proofs[g][:3] == proofs1[g], g
        assert all(set(r[:z] + r[z + 1:]) == {0xFF} for r in rows[g]), g


def test_launch_boundaries_11_groups(hip, oracle, srs, srs_pts):
    """more groups than a launch carries, not a multiple of it, mixed k; a group is never split"""
    rng = np.random.default_rng(11)
    small = [1, 2, 15, 16, 17, 255, 257, 4095, 4096, 4097, 8193]
    ks = [15, 15, 15, 15, 1, 9, 2, 15, 1, 1, 3]
    assert len(ks) > 2 * PER_LAUNCH and len(ks) % PER_LAUNCH
    groups = [[poly(300 + j, small[int(i)]) for j, i in enumerate(rng.integers(0, len(small), k))] for k in ks]
    sets = [seeded_masks(0xB0 + g, k) for g, k in enumerate(ks)]
    weights = [[int(v) for v in rng.integers(0, 17, k)] for k in ks]
    us = [int(v) for v in rng.integers(0, 17, len(ks))]
    rows, proofs = hip.kzg_open_multi(srs, groups, sets, weights, us)
    drows, recs, hs, _ = open_dev(hip, srs, groups, sets, weights, us)
    for g in range(len(ks)):
        e = expect(oracle, srs_pts, groups[g], sets[g], weights[g], us[g])
        assert (rows[g], proofs[g]) == (e[0], e[2]), g
        assert drows[g] == e[0] and hs[g] == e[1] and recs[2 * g]["g1"] + recs[2 * g + 1]["g1"] == e[2], g
        assert recs[2 * g]["irregular"] == 0 and recs[2 * g + 1]["irregular"] == 0, g


# ------------------------------------------------------------------ the golden record
class Gold:
    """tests/golden/kzg_multi.json joined with its inputs, which are rebuilt from the recorded seeds"""

    def __init__(self):
        import make_kzg_multi_golden as mk
        self.mk = mk
        self.raw = load_golden("kzg_multi.json")
        self.key = bytes.fromhex(self.raw["key"])
        self.srs = np.array(list(bytes.fromhex(self.raw["srs"])), np.uint8).reshape(-1, 3)
        self.opened, verify, self.cases = mk.expand(self.raw)
        self.rows = {k: verify[k][0] for k in verify}
        self.bits = {k: verify[k][1] for k in verify}

    def std(self, k):
        """the rows recorded under the s = 2 key, and their verdicts"""
        m = (self.rows[k][:, :7] == np.frombuffer(self.key, np.uint8)).all(1)
        return self.rows[k][m], self.bits[k][m]


@pytest.fixture(scope="module")
def gold():
    return Gold()


def test_open_every_golden_group(hip, gold):
    og = gold.opened
    groups = [[np.array(p, np.uint8) for p in g["polys"]] for g in og]
    sets, weights, us = [g["sets"] for g in og], [g["weights"] for g in og], [g["u"] for g in og]
    with hip.Srs(gold.srs) as s:
        rows, proofs = hip.kzg_open_multi(s, groups, sets, weights, us)
        drows, recs, hs, _ = open_dev(hip, s, groups, sets, weights, us)
    for i, g in enumerate(og):
        assert proofs[i] == bytes(g["W"] + g["Wp"]), i
        assert recs[2 * i]["g1"] + recs[2 * i + 1]["g1"] == proofs[i] and drows[i] == rows[i], i
        assert recs[2 * i]["irregular"] == 0 and recs[2 * i + 1]["irregular"] == 0, i
        assert gold.mk.digest(b"".join(rows[i]), MM.F.trim(np.frombuffer(hs[i], np.uint8)).tolist()) == g["digest"], i


# ------------------------------------------------------------------ slow paths
@pytest.mark.parametrize("where", ["first", "chunk_1", "last"])
def test_non_canonical_coefficient_bytes(hip, oracle, srs, srs_pts, where):
    n = 9000
    pos = {"first": 0, "chunk_1": 4100, "last": n - 1}[where]
    bad = poly(31, n).copy()
    bad[pos] = 200
    mid = [poly(34, 5000), bad, poly(35, 17)]
    left, right = [poly(32, 4500), poly(36, 4097)], [poly(33, n)]
    groups, weights = [left, mid, right], [[3, 16], [5, 7, 1], [9]]
    sets = [[1 << Z | 1 << ZW, 1], [0b100001, 1 << Z | 1 << ZW, LOW16], [NONZERO16]]
    us = [4, 5, 0]
    # host form = the composition called through the library itself
    rows, proofs = hip.kzg_open_multi(srs, groups, sets, weights, us)
    crow, _, cproof = compose(hip, srs, mid, sets[1], weights[1], us[1])
    assert rows[1] == crow and proofs[1] == cproof, where
    el = expect(oracle, srs_pts, left, sets[0], weights[0], us[0], key=("nc", 0))
    er = expect(oracle, srs_pts, right, sets[2], weights[2], us[2], key=("nc", 2))
    assert (rows[0], proofs[0]) == (el[0], el[2]) and (rows[2], proofs[2]) == (er[0], er[2])
    # device form: both records of that group flagged, its neighbours exact
    drows, recs, hs, _ = open_dev(hip, srs, groups, sets, weights, us)
    assert recs[2]["irregular"] > 0 and recs[3]["irregular"] > 0, where
    for g, e in ((0, el), (2, er)):
        assert recs[2 * g]["irregular"] == 0 and recs[2 * g + 1]["irregular"] == 0
        assert drows[g] == e[0] and hs[g] == e[1] and recs[2 * g]["g1"] + recs[2 * g + 1]["g1"] == e[2]


def test_irregular_srs(hip, oracle):
    n = 5000
    pts, _ = gen.msm_inputs(0x1229, n + 100, "full")
    pts = pts.copy()
    pts[2500] = (3, 3, 0)                              # off-curve
    groups = [[poly(42, 600), poly(41, n), poly(43, 4097)], [poly(44, 17)]]
    sets, weights, us = [[1, 1 << Z | 1 << ZW, 0b1110], [LOW16]], [[2, 9, 16], [0]], [7, 0]
    with hip.Srs(pts) as s:
        assert s.irregular
        exp = [expect(oracle, pts, g, m, w, u) for g, m, w, u in zip(groups, sets, weights, us)]
        rows, proofs = hip.kzg_open_multi(s, groups, sets, weights, us)
        assert rows == [e[0] for e in exp] and proofs == [e[2] for e in exp]
        drows, recs, hs, _ = open_dev(hip, s, groups, sets, weights, us)
        assert all(r["irregular"] > 0 for r in recs)
        assert drows == rows and hs == [e[1] for e in exp]           # exact whatever the SRS


def test_srs_boundary(hip, oracle):
    n = 4100
    pts, _ = gen.msm_inputs(0xB0, n, "full")
    with hip.Srs(pts) as s:
        g, m, w = [poly(64, 300), poly(61, n + 1)], [0b11, 1 << 5], [5, 3]        # Lh == srs_len
        e = expect(oracle, pts, g, m, w, 4)
        assert len(e[1]) == n
        rows, proofs = hip.kzg_open_multi(s, [g], [m], [w], [4])
        assert (rows[0], proofs[0]) == (e[0], e[2])
        check_dev(open_dev(hip, s, [g], [m], [w], [4]), [e])
        for over, om in (([poly(64, 300), poly(62, n + 2)], m),               # Lh one more
                         ([poly(64, 300), poly(62, n + 2)], [0b11, LOW16])):  # Lh fits, the fold's L - 1 does not
            with pytest.raises(hip.PlonkHipError) as err:
                hip.kzg_open_multi(s, [over], [om], [[5, 0]], [4])            # on the lengths as given
            assert err.value.code == hip.PLK_ERR_RANGE and "degree exceeds SRS size" in str(err.value)
            with pytest.raises(hip.PlonkHipError) as err:
                open_dev(hip, s, [over], [om], [w], [4])
            assert err.value.code == hip.PLK_ERR_RANGE


# ------------------------------------------------------------------ the device API
def api_case(oracle, srs_pts):
    groups = [[poly(117, 17), poly(500, 4097)], [poly(501, 8193), poly(502, 4096), poly(503, 3 * 4096 + 5)], [poly(504, 300)]]
    sets = [[1, 1 << Z | 1 << ZW], [NONZERO16, 0b100001, 1 << 9], [LOW16]]
    weights = [[1, 16], [7, 0, 12], [3]]
    us = [2, 0, 16]
    exp = [expect(oracle, srs_pts, g, m, w, u, key=("api", i)) for i, (g, m, w, u) in enumerate(zip(groups, sets, weights, us))]
    return groups, sets, weights, us, exp


@pytest.mark.parametrize("off", [1, 7, 15])
def test_device_api_unaligned_polynomials_and_h(hip, oracle, srs, srs_pts, off):
    groups, sets, weights, us, exp = api_case(oracle, srs_pts)
    check_dev(open_dev(hip, srs, groups, sets, weights, us, offset=off, hoffset=16 - off), exp)
    check_dev(open_dev(hip, srs, groups, sets, weights, us, offset=0, hoffset=off), exp)


def test_device_api_state_and_streams(hip, oracle, srs, srs_pts):
    import torch
    groups, sets, weights, us, exp = api_case(oracle, srs_pts)
    part = [False, True, False]                                # h wanted for some groups only
    check_dev(open_dev(hip, srs, groups, sets, weights, us, want_hs=part), exp, part)
    # two calls back to back on the same records and (dirty) workspace, nothing re-initialised
    first = open_dev(hip, srs, groups, sets, weights, us, want_hs=False)
    check_dev(first, exp, [False] * 3)
    second = open_dev(hip, srs, groups, sets, weights, us, want_hs=False, state=first[3])
    check_dev(second, exp, [False] * 3)
    assert second[:2] == first[:2]                             # a repeated call gives identical bytes
    check_dev(open_dev(hip, srs, groups, sets, weights, us, stream=torch.cuda.Stream()), exp)


def test_two_streams_with_distinct_workspaces(hip, oracle, srs, srs_pts):
    import torch
    groups, sets, weights, us, exp = api_case(oracle, srs_pts)
    flat = [p for g in groups for p in g]
    fsets = [m for s in sets for m in s]
    lens, st = [len(p) for p in flat], starts(groups)
    dp = [torch.from_numpy(np.array(p, dtype=np.uint8)).cuda() for p in flat]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(2):
        outs.append((torch.full((17 * len(flat),), 0xEE, dtype=torch.uint8, device="cuda"),
                     torch.zeros(2 * len(groups) * REC, dtype=torch.uint8, device="cuda"),
                     torch.full((hip.kzg_multi_workspace(lens, fsets, st),), 0xA5, dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    for (ys, res, work), s in zip(outs, (s1, s2)):
        hip.kzg_open_multi_dev(srs, dp, lens, fsets, [w for g in weights for w in g], st, us, ys, res, work=work, stream=s)
    s1.synchronize()
    s2.synchronize()
    for ys, res, _ in outs:
        r = res.cpu().numpy()
        got = [hip.parse_result(r[i * REC:(i + 1) * REC])["g1"] for i in range(2 * len(groups))]
        assert [got[2 * g] + got[2 * g + 1] for g in range(len(groups))] == [e[2] for e in exp]
        assert bytes(ys.cpu().numpy()) == b"".join(row for e in exp for row in e[0])


def test_larger_case_plonk_sets_against_the_composition(hip):
    """9 polynomials of 2^18 coefficients, eight at {z} and one at {z, z omega}: the fused call against the
    composition of the library's own calls"""
    n = 1 << 18
    pts = rule_srs(n)
    g = [poly(700 + i, n) for i in range(9)]
    m = [1 << Z] * 8 + [1 << Z | 1 << ZW]
    w = [1, 5, 16, 2, 3, 9, 11, 4, 7]
    with hip.Srs(pts) as s:
        crow, ch, cproof = compose(hip, s, g, m, w, 6)
        rows, proofs = hip.kzg_open_multi(s, [g], [m], [w], [6])
        assert rows[0] == crow and proofs[0] == cproof
        drows, recs, hs, _ = open_dev(hip, s, [g], [m], [w], [6])
        assert drows[0] == crow and hs[0] == ch and recs[0]["g1"] + recs[1]["g1"] == cproof
        assert recs[0]["irregular"] == 0 and recs[1]["irregular"] == 0


# ------------------------------------------------------------------ verification
def vk_of(hip, b):
    b = bytes(b)
    return hip.KzgVk(b[0:3], b[3:5], b[5:7])


def key_tuple(gold):
    b = tuple(gold.key)
    return (b[0:3], b[3:5], b[5:7])


def columns(rows, k):
    """(commits n k x 3, sets n k, weights n k, ys n k x 17, us n, proofs n x 6) of recorded rows"""
    ent = rows[:, 7:7 + 25 * k].reshape(-1, k, 25)
    sets = np.ascontiguousarray(ent[:, :, 3:7]).view("<u4").reshape(-1, k)
    return (np.ascontiguousarray(ent[:, :, :3]), sets, np.ascontiguousarray(ent[:, :, 7]),
            np.ascontiguousarray(ent[:, :, 8:25]), np.ascontiguousarray(rows[:, -1]),
            np.ascontiguousarray(rows[:, 7 + 25 * k:13 + 25 * k]))


def on_device(a, offset=0):
    import torch
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.full((offset + a.size + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[offset:offset + a.size] = torch.from_numpy(a.copy()).cuda()
    return t[offset:]


def verify_dev(hip, vk, k, cols, offset=0, stream=None):
    """every buffer offset bytes past a 16-byte boundary, except the masks (4-byte aligned: 4 offset)"""
    import torch
    n = cols[4].size
    d = [on_device(a, 4 * offset if i == 1 else offset) for i, a in enumerate(cols)]
    ok = torch.full((offset + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")[offset:]
    torch.cuda.synchronize()
    hip.kzg_verify_multi_dev(vk, k, d[0], d[1], d[2], d[3], d[4], d[5], n, ok, stream=stream)
    torch.cuda.synchronize()
    h = ok.cpu().numpy()
    assert (h[n:] == 0xEE).all(), "wrote past the output"
    return h[:n].copy()


def verify_both(hip, vk, k, cols, form, offset=0):
    return hip.kzg_verify_multi(vk, k, *cols) if form == "host" else verify_dev(hip, vk, k, cols, offset)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("k", [1, 2, 3, 9, 15])
def test_verify_every_golden_job(hip, gold, k, form):
    """the jobs under the s = 2 key in one call; the jobs carrying their own key one call each"""
    rows, bits = gold.std(k)
    got = verify_both(hip, vk_of(hip, gold.key), k, columns(rows, k), form)
    bad = np.flatnonzero(got != bits)
    assert bad.size == 0 and 0 < bits.sum() < bits.size, bad[:8]
    own = np.flatnonzero((gold.rows[k][:, :7] != np.frombuffer(gold.key, np.uint8)).any(1))
    assert own.size >= 50
    for i in own:
        r = gold.rows[k][i:i + 1]
        assert verify_both(hip, vk_of(hip, r[0, :7]), k, columns(r, k), form)[0] == gold.bits[k][i], (k, int(i))


@pytest.mark.parametrize("n", [1, 255, 256, 257, (1 << 19) + 1])
def test_verify_batch_sizes(hip, gold, n):
    """the recorded jobs tiled; the largest wraps the grid-stride loop"""
    k = 3
    rows, bits = gold.std(k)
    reps = -(-n // len(rows))
    tiled = np.tile(rows, (reps, 1))[:n]
    exp = np.tile(bits, reps)[:n]
    assert np.array_equal(verify_dev(hip, vk_of(hip, gold.key), k, columns(tiled, k)), exp)
    if n <= 257:
        assert np.array_equal(hip.kzg_verify_multi(vk_of(hip, gold.key), k, *columns(tiled, k)), exp)


# (column of the 7 + 25 k + 7 byte row relative to an entry or the tail, value); the y column is set at the
# first point of the entry's set by the test
ENTRY_INVALID = {"c_x_101": (0, 101), "c_y_255": (1, 255), "c_flag_2": (2, 2), "mask_0": (3, None), "mask_bit17": (5, 0x02),
                 "mask_all17": (3, None), "weight_17": (7, 17), "weight_255": (7, 255), "y_17": (8, 17)}
TAIL_INVALID = {"w_x_255": (0, 255), "w_flag_2": (2, 2), "wp_y_101": (4, 101), "wp_flag_2": (5, 2), "u_17": (6, 17),
                "u_255": (6, 255)}


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("kind", sorted(ENTRY_INVALID) + sorted(TAIL_INVALID))
def test_verify_invalid_byte(hip, gold, kind, k):
    """at the first and at the last entry of a job, for the first job, a block's last and the batch's last"""
    rows, bits = gold.std(k)
    base = np.tile(rows, (2, 1))[:257].copy()
    exp0 = np.tile(bits, 2)[:257]
    for entry in sorted({0, k - 1}):
        jobs, exp = base.copy(), exp0.copy()
        for pos in (0, 255, 256):
            e0 = 7 + 25 * entry
            if kind == "mask_0":
                jobs[pos, e0 + 3:e0 + 7] = 0
            elif kind == "mask_all17":
                jobs[pos, e0 + 3:e0 + 7] = (0xFF, 0xFF, 0x01, 0)
            elif kind == "y_17":
                mask = int.from_bytes(bytes(jobs[pos, e0 + 3:e0 + 7]), "little")
                jobs[pos, e0 + 8 + MM.points(mask)[0]] = 17
            elif kind in ENTRY_INVALID:
                col, val = ENTRY_INVALID[kind]
                jobs[pos, e0 + col] = val
            else:
                col, val = TAIL_INVALID[kind]
                jobs[pos, 7 + 25 * k + col] = val
            exp[pos] = 2
        cols = columns(jobs[:1], k)
        assert MM.verify_multi_batch(key_tuple(gold), k, *cols)[0] == 2
        for form in ("host", "dev"):
            assert np.array_equal(verify_both(hip, vk_of(hip, gold.key), k, columns(jobs, k), form), exp), (form, entry)


def test_verify_ignores_bytes_off_the_set(hip, gold):
    k = 3
    rows, bits = gold.std(k)
    jobs = rows.copy()
    for r in jobs:
        for i in range(k):
            mask = int.from_bytes(bytes(r[7 + 25 * i + 3:7 + 25 * i + 7]), "little")
            for a in range(17):
                if not (mask >> a) & 1:
                    r[7 + 25 * i + 8 + a] = 0xFF
    for form in ("host", "dev"):
        assert np.array_equal(verify_both(hip, vk_of(hip, gold.key), k, columns(jobs, k), form), bits), form


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_verify_unaligned_device_buffers_and_guards(hip, gold, offset):
    for k in (2, 15):
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
    assert np.array_equal(hip.kzg_verify_multi(vk, 9, *cols), first)


# ------------------------------------------------------------------ end to end with commit and open, s = 2
def test_completeness_seeded_groups(hip, gold):
    """what the opener produces for random groups over an SRS built from s = 2, the verifier accepts"""
    groups_in = gold.mk.random_groups(0xC0817E7E, 40)
    vk = vk_of(hip, gold.key)
    groups = [[np.array(p, np.uint8) for p in g[0]] for g in groups_in]
    sets, weights, us = [g[1] for g in groups_in], [g[2] for g in groups_in], [g[3] for g in groups_in]
    with hip.Srs(gold.srs) as srs:
        commits = [hip.kzg_commit(srs, g) for g in groups]
        rows, proofs = hip.kzg_open_multi(srs, groups, sets, weights, us)
    for n in range(len(groups)):
        k = len(groups[n])
        cols = (np.frombuffer(b"".join(commits[n]), np.uint8), np.array(sets[n], np.uint32), np.array(weights[n], np.uint8),
                np.frombuffer(b"".join(rows[n]), np.uint8), np.array([us[n]], np.uint8), np.frombuffer(proofs[n], np.uint8))
        for form in ("host", "dev"):
            assert verify_both(hip, vk, k, cols, form).tolist() == [1], (n, form)


def test_end_to_end_tampering(hip, gold):
    """the library's commitments and openings are the reference's; the honest job is accepted and one altered
    value, mask, W, W' or commitment gets the model's (= the reference's recorded) byte.  u lies outside T and the
    weights are non-zero, so an altered value, W or commitment moves the left-hand side and the byte is 0 by
    arithmetic, not by accident of the 17-element group"""
    cases = gold.cases
    vk, key = vk_of(hip, gold.key), key_tuple(gold)
    groups = [[np.array(p, np.uint8) for p in c["polys"]] for c in cases]
    sets, weights, us = [c["sets"] for c in cases], [c["weights"] for c in cases], [c["u"] for c in cases]
    with hip.Srs(gold.srs) as srs:
        commits = [hip.kzg_commit(srs, g) for g in groups]
        rows, proofs = hip.kzg_open_multi(srs, groups, sets, weights, us)
    for n, c in enumerate(cases):
        k = len(groups[n])
        assert [tuple(x) for x in commits[n]] == c["commits"] and proofs[n] == bytes(c["W"] + c["Wp"]), n
        ys = list(b"".join(rows[n]))
        variants = gold.mk.e2e_variants(n, sets[n], ys, c["commits"], c["W"], c["Wp"])
        cols = (np.array([v[2] for v in variants], np.uint8), np.array([v[0] for v in variants], np.uint32),
                np.array([weights[n]] * 6, np.uint8), np.array([v[1] for v in variants], np.uint8),
                np.array([us[n]] * 6, np.uint8), np.array([list(v[3]) + list(v[4]) for v in variants], np.uint8))
        model = MM.verify_multi_batch(key, k, *cols)
        assert "".join(str(int(b)) for b in model) == c["bits"], n
        assert model[0] == 1 and model[1] == model[3] == model[5] == 0, n
        for form in ("host", "dev"):
            assert np.array_equal(verify_both(hip, vk, k, cols, form), model), (n, form)
