"""KZG commit and open over a resident SRS (plk_srs_* / plk_kzg_*) on the GPU.

Expected values are the composition the header specifies, over the oracle: y = oracle.poly_eval(p, z),
q = the quotient of oracle.poly_divide(p, [(17 - z) % 17, 1]), proof = oracle.msm(srs[:len(q)], q) --
the raw serial fold.  Everything is exact: bytes are compared for equality."""
import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 5, 65537]
ZS = [0, 1, 2, 5, 16]
SRS_N = 65537
REC = 2176


@pytest.fixture(scope="module")
def srs_pts():
    pts, _ = gen.msm_inputs(0x5125, SRS_N, "full")     # identity and the 2-torsion point included
    return pts


@pytest.fixture(scope="module")
def srs(hip, srs_pts):
    with hip.Srs(srs_pts) as s:
        assert len(s) == SRS_N and not s.irregular
        yield s


def poly(seed, n):
    a, _ = gen.poly_inputs(seed, n, 0)
    return a


def trim(q):
    q = bytes(q)
    n = len(q)
    while n > 1 and q[n - 1] == 0:
        n -= 1
    return q[:n]


_EXPECT = {}


def expect(oracle, pts, p, z, key=None):
    """(y, trimmed quotient bytes, proof) of the specified composition; cached by key"""
    if key is not None and key in _EXPECT:
        return _EXPECT[key]
    y = oracle.poly_eval(p, z)
    q, _ = oracle.poly_divide(p, [(17 - z) % 17, 1])
    r = (y, q, oracle.msm(pts[:len(q)], q))
    if key is not None:
        _EXPECT[key] = r
    return r


def open_dev(hip, srs, polys, zs, want_quots=True, offset=0, stream=None, state=None):
    """plk_kzg_open_batch_dev over torch buffers -> (ys, [result dicts], [quotient bytes or None]);
    want_quots: True, False or a per-job list; offset: the polynomials start that many bytes past a
    16-byte boundary; state: (records, workspace) to reuse without re-initialising"""
    import torch
    n = len(polys)
    lens = [len(p) for p in polys]
    wq = want_quots if isinstance(want_quots, list) else [bool(want_quots)] * n
    dp = []
    for p in polys:
        t = torch.zeros(len(p) + 32, dtype=torch.uint8, device="cuda")
        t[offset:offset + len(p)] = torch.from_numpy(np.ascontiguousarray(p, dtype=np.uint8)).cuda()
        assert t.data_ptr() % 16 == 0
        dp.append(t[offset:])
    dq = [torch.full((max(l - 1, 1) + 16,), 0xEE, dtype=torch.uint8, device="cuda") if w else None
          for l, w in zip(lens, wq)]
    ys = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    if state is None:
        res = torch.zeros(n * REC, dtype=torch.uint8, device="cuda")
        # the workspace needs no initialisation: hand it over dirty
        work = torch.full((hip.kzg_workspace(lens),), 0xA5, dtype=torch.uint8, device="cuda")
    else:
        res, work = state
    torch.cuda.synchronize()
    hip.kzg_open_dev(srs, dp, lens, zs, ys, res, quots=dq if any(wq) else None, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    recs = [hip.parse_result(r[i * REC:(i + 1) * REC]) for i in range(n)]
    quots = []
    for l, q in zip(lens, dq):
        if q is None:
            quots.append(None)
            continue
        h = q.cpu().numpy()
        assert (h[max(l - 1, 1):] == 0xEE).all(), "wrote past max(len - 1, 1) quotient bytes"
        quots.append(bytes(h[:max(l - 1, 1)]))
    return [int(v) for v in ys.cpu().numpy()], recs, quots, (res, work)


@pytest.mark.parametrize("z", ZS)
def test_open_shape_sweep(hip, oracle, srs, srs_pts, z):
    polys = [poly(100 + n, n) for n in LENGTHS]
    exp = [expect(oracle, srs_pts, p, z, key=(len(p), z)) for p in polys]
    ys, proofs = hip.kzg_open(srs, polys, [z] * len(polys))
    assert ys == [e[0] for e in exp]
    assert proofs == [e[2] for e in exp]
    dys, recs, quots, _ = open_dev(hip, srs, polys, [z] * len(polys))
    assert dys == [e[0] for e in exp]
    for n, r, q, e in zip(LENGTHS, recs, quots, exp):
        assert r["irregular"] == 0 and r["g1"] == e[2], (n, z)
        assert trim(q) == e[1], (n, z)


def test_mixed_batch_of_70_equals_one_job_per_call(hip, oracle, srs, srs_pts):
    rng = np.random.default_rng(70)
    lens = [LENGTHS[i] for i in rng.integers(0, len(LENGTHS) - 1, 70)]   # (65537 once, below)
    lens[33] = 65537
    zs = [ZS[i] for i in rng.integers(0, len(ZS), 70)]
    polys = [poly(100 + n, n) for n in lens]
    ys, proofs = hip.kzg_open(srs, polys, zs)
    dys, recs, quots, _ = open_dev(hip, srs, polys, zs)
    for b in range(70):
        y1, p1 = hip.kzg_open(srs, [polys[b]], [zs[b]])
        assert (ys[b], proofs[b]) == (y1[0], p1[0]), b
        e = expect(oracle, srs_pts, polys[b], zs[b], key=(lens[b], zs[b]))
        assert (ys[b], proofs[b]) == (e[0], e[2]), b
        assert dys[b] == e[0] and recs[b]["irregular"] == 0 and recs[b]["g1"] == e[2], b
        assert trim(quots[b]) == e[1], b


def test_degenerate_polynomials(hip, oracle, srs, srs_pts):
    tail = poly(9, 5000).copy()
    tail[4097:] = 0                                    # trailing zeros above a non-zero coefficient
    tail[4096] = 3
    polys = [np.zeros(1, np.uint8), np.zeros(300, np.uint8), np.zeros(4097, np.uint8),
             np.array([7], np.uint8), np.array([7, 0, 0, 0], np.uint8), tail]
    for z in (0, 3, 16):
        exp = [expect(oracle, srs_pts, p, z) for p in polys]
        ys, proofs = hip.kzg_open(srs, polys, [z] * len(polys))
        assert ys == [e[0] for e in exp] and proofs == [e[2] for e in exp], z
        dys, recs, quots, _ = open_dev(hip, srs, polys, [z] * len(polys))
        assert dys == ys and [r["g1"] for r in recs] == proofs, z
        assert [trim(q) for q in quots] == [e[1] for e in exp], z
    assert hip.kzg_commit(srs, polys) == [oracle.msm(srs_pts[:len(p)], p) for p in polys]


@pytest.mark.parametrize("where", ["first", "middle", "chunk_boundary", "last"])
def test_non_canonical_coefficient_bytes(hip, oracle, srs, srs_pts, where):
    n = 9000
    pos = {"first": 0, "middle": 5001, "chunk_boundary": 4096, "last": n - 1}[where]
    bad = poly(31, n).copy()
    bad[pos] = 200
    left, right = poly(32, 4500), poly(33, n)
    for z in (0, 5):
        # host form = the public entry points composed
        y = hip.poly_eval(bad, z)
        q, _ = hip.poly_divide(bad, [(17 - z) % 17, 1])
        proof = hip.msm_g1(srs_pts[:len(q)], q)
        ys, proofs = hip.kzg_open(srs, [left, bad, right], [z, z, z])
        assert (ys[1], proofs[1]) == (y, proof), (where, z)
        el, er = expect(oracle, srs_pts, left, z), expect(oracle, srs_pts, right, z)
        assert (ys[0], proofs[0]) == (el[0], el[2]) and (ys[2], proofs[2]) == (er[0], er[2])
        # device form: that job flagged, its canonical neighbours exact
        dys, recs, _, _ = open_dev(hip, srs, [left, bad, right], [z, z, z], want_quots=False)
        assert recs[1]["irregular"] > 0, (where, z)
        assert recs[0]["irregular"] == 0 and recs[0]["g1"] == el[2] and dys[0] == el[0]
        assert recs[2]["irregular"] == 0 and recs[2]["g1"] == er[2] and dys[2] == er[0]


@pytest.mark.parametrize("where", ["first", "middle", "last_used", "beyond"])
def test_irregular_srs(hip, oracle, where):
    import torch
    n = 5000
    pts, _ = gen.msm_inputs(0x1229, n + 100, "full")
    pts = pts.copy()
    p = poly(41, n).copy()
    p[n - 40:] = 0                                     # trimmed quotient length n - 41
    p[n - 41] = 9
    pos = {"first": 0, "middle": 2500, "last_used": n - 42, "beyond": n - 41}[where]
    pts[pos] = (3, 3, 0)                               # off-curve
    small = poly(42, 600)
    with hip.Srs(pts) as s:
        assert s.irregular and len(s) == n + 100
        for z in (0, 7):
            polys = [p, small]
            exp = [expect(oracle, pts, x, z) for x in polys]
            assert len(exp[0][1]) == n - 41
            ys, proofs = hip.kzg_open(s, polys, [z, z])
            assert ys == [e[0] for e in exp] and proofs == [e[2] for e in exp], (where, z)
            dys, recs, quots, _ = open_dev(hip, s, polys, [z, z])
            assert all(r["irregular"] > 0 for r in recs)
            assert dys == ys and [trim(q) for q in quots] == [e[1] for e in exp]   # exact whatever the SRS
        assert hip.kzg_commit(s, [p, small]) == [oracle.msm(pts[:len(x)], x) for x in (p, small)]
        res = torch.zeros(2 * REC, dtype=torch.uint8, device="cuda")
        dp = [torch.from_numpy(x).cuda() for x in (p, small)]
        hip.kzg_commit_dev(s, dp, [len(p), len(small)], res)
        r = res.cpu().numpy()
        assert all(hip.parse_result(r[i * REC:(i + 1) * REC])["irregular"] > 0 for i in range(2))


def test_commit_ragged_batch_all_byte_values(hip, oracle, srs, srs_pts):
    import torch
    lens = [1, 16, 17, 4097, (1 << 16) + 1]
    polys = [gen.msm_inputs(50 + n, n, "bytes")[1] for n in lens]
    exp = [oracle.msm(srs_pts[:n], p) for n, p in zip(lens, polys)]
    assert hip.kzg_commit(srs, polys) == exp
    assert [hip.msm_g1(srs_pts[:n], p) for n, p in zip(lens, polys)] == exp
    for offset in (0, 1):
        bufs = [torch.zeros(n + 32, dtype=torch.uint8, device="cuda") for n in lens]
        for t, p in zip(bufs, polys):
            t[offset:offset + len(p)] = torch.from_numpy(p).cuda()
        res = torch.zeros(len(lens) * REC, dtype=torch.uint8, device="cuda")
        hip.kzg_commit_dev(srs, [t[offset:] for t in bufs], lens, res)
        r = res.cpu().numpy()
        recs = [hip.parse_result(r[i * REC:(i + 1) * REC]) for i in range(len(lens))]
        assert [x["g1"] for x in recs] == exp and all(x["irregular"] == 0 for x in recs), offset


def test_srs_boundary(hip, oracle):
    n = 4100
    pts, _ = gen.msm_inputs(0xB0, n, "full")
    with hip.Srs(pts) as s:
        p = poly(61, n + 1)                            # len - 1 == srs_len
        e = expect(oracle, pts, p, 4)
        ys, proofs = hip.kzg_open(s, [p], [4])
        assert (ys[0], proofs[0]) == (e[0], e[2])
        dys, recs, _, _ = open_dev(hip, s, [p], [4])
        assert dys[0] == e[0] and recs[0]["g1"] == e[2] and recs[0]["irregular"] == 0
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open(s, [poly(62, n + 2)], [4])
        assert err.value.code == hip.PLK_ERR_RANGE and "degree exceeds SRS size" in str(err.value)
        with pytest.raises(hip.PlonkHipError) as err:
            open_dev(hip, s, [poly(62, n + 2)], [4])
        assert err.value.code == hip.PLK_ERR_RANGE
        c = poly(63, n)                                # len == srs_len
        assert hip.kzg_commit(s, [c]) == [oracle.msm(pts, c)]
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_commit(s, [p])
        assert err.value.code == hip.PLK_ERR_RANGE
    with hip.Srs(pts[:1]) as s1:                       # a one-point SRS opens up to two coefficients
        for x in ([5], [5, 6]):
            e = expect(oracle, pts, np.array(x, np.uint8), 3)
            assert hip.kzg_open(s1, [x], [3]) == ([e[0]], [e[2]])
        with pytest.raises(hip.PlonkHipError):
            hip.kzg_open(s1, [[5, 6, 7]], [3])


def test_device_api(hip, oracle, srs, srs_pts):
    import torch
    lens = [17, 4096, 4097, 8193, 3 * 4096 + 5]
    zs = [0, 2, 5, 16, 0]
    polys = [poly(100 + n, n) for n in lens]
    exp = [expect(oracle, srs_pts, p, z, key=(len(p), z)) for p, z in zip(polys, zs)]

    def check(out, wq):
        dys, recs, quots, _ = out
        assert dys == [e[0] for e in exp]
        assert [r["g1"] for r in recs] == [e[2] for e in exp] and all(r["irregular"] == 0 for r in recs)
        for q, w, e in zip(quots, wq, exp):
            assert (q is None) == (not w)
            if w:
                assert trim(q) == e[1]

    # polynomial pointers one byte past a 16-byte boundary: the byte-wise loads
    check(open_dev(hip, srs, polys, zs, offset=1), [True] * 5)
    # quotients wanted for some jobs only
    part = [True, False, True, False, False]
    check(open_dev(hip, srs, polys, zs, want_quots=part), part)
    # two calls back to back on the same records and workspace, nothing re-initialised
    first = open_dev(hip, srs, polys, zs, want_quots=False)
    check(first, [False] * 5)
    check(open_dev(hip, srs, polys, zs, want_quots=False, state=first[3]), [False] * 5)
    # a non-default stream
    check(open_dev(hip, srs, polys, zs, stream=torch.cuda.Stream()), [True] * 5)


def test_large_case(hip, oracle):
    n = (1 << 20) + 3
    pts, _ = gen.msm_inputs(0x1A26E, n, "full")
    polys = [poly(71, n), poly(72, n)]
    exp = [expect(oracle, pts, p, 3) for p in polys]
    with hip.Srs(pts) as s:
        ys, proofs = hip.kzg_open(s, polys, [3, 3])
        assert ys == [e[0] for e in exp] and proofs == [e[2] for e in exp]
        dys, recs, quots, _ = open_dev(hip, s, polys, [3, 3])
        assert dys == ys and [r["g1"] for r in recs] == proofs
        assert [trim(q) for q in quots] == [e[1] for e in exp]
