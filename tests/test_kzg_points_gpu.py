"""KZG per-point openings (plk_kzg_open_points_batch*) on the GPU.

Expected values are the expansion of tests/kzg_points_model.py over the oracle: per (polynomial, z) the
composition tests/test_kzg_gpu.py::expect takes -- oracle.poly_eval, the quotient of oracle.poly_divide by
[(17 - z) % 17, 1], oracle.msm over the SRS prefix -- in the job order of the header.  Everything is exact:
bytes are compared for equality, in the host form and in the _dev form.  The _dev form gets a dirty workspace
(0xA5) and outputs with 0xEE on both sides."""
import numpy as np
import pytest

import gen
import kzg_points_model as PM
from conftest import load_golden

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 15, 16, 17, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 5, 65537]
SRS_N = 65537
GUARD = 32
FULL = PM.FULL
FLAG = PM.FLAGGED_PROOF


def seeded_masks(seed, n):
    """n valid masks of 1 .. 17 points"""
    r = gen.splitmix64(seed, n)
    out = []
    for v in r:
        m = int(v >> np.uint64(8)) & FULL
        out.append(m if m else 1 << (int(v) % 17))
    return out


MASKS = [1, 1 << 16, 0b11, FULL & ~1, FULL] + seeded_masks(0x9017, 2)


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
    """seeded canonical coefficients, built once and never modified (tests copy before editing)"""
    if (seed, n) not in _POLY:
        _POLY[seed, n] = gen.poly_inputs(seed, n, 0)[0]
    return _POLY[seed, n]


def by_len(n):
    return poly(100 + n, n)


_CACHE = {}


def expect(oracle, pts, polys, sets, keys=None):
    """(zs, ys, proofs) of the model; keys name shared polynomials (each (polynomial, z) is computed once)"""
    return PM.open_points(oracle, pts, polys, sets, cache=_CACHE, keys=keys)


def guarded(n, offset=0):
    """n output bytes `offset` bytes past a 16-byte boundary, 0xEE all over and on both sides"""
    import torch
    t = torch.full((16 + offset + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t, 16 + offset


def taken(buf, n):
    t, pre = buf
    h = t.cpu().numpy()
    assert (h[:pre] == 0xEE).all() and (h[pre + n:] == 0xEE).all(), "wrote outside the output"
    return h[pre:pre + n].copy()


def points_dev(hip, srs, polys, sets, offset=0, out_offset=0, stream=None, work=None, want_zs=True):
    """plk_kzg_open_points_batch_dev over torch buffers -> (zs or None, ys, [proof bytes], status, work);
    offset: the polynomials start that many bytes past a 16-byte boundary; out_offset: the outputs do;
    work: a workspace to reuse without re-initialising"""
    import torch
    lens = [len(p) for p in polys]
    dp = []
    for p in polys:
        t = torch.zeros(len(p) + 32, dtype=torch.uint8, device="cuda")
        t[offset:offset + len(p)] = torch.from_numpy(np.ascontiguousarray(p, dtype=np.uint8)).cuda()
        assert t.data_ptr() % 16 == 0
        dp.append(t[offset:])
    J = hip.kzg_points_count(sets)
    assert J == PM.count(sets) > 0
    zs, ys, st, pf = (guarded(k, out_offset) for k in (J, J, J, 3 * J))
    ws = hip.kzg_points_workspace(lens, sets)
    assert (ws == 0) == all(n <= PM.CHUNK for n in lens)
    if work is None and ws:
        work = torch.full((ws,), 0xA5, dtype=torch.uint8, device="cuda")   # needs no initialisation: hand it over dirty
    torch.cuda.synchronize()
    hip.kzg_open_points_dev(srs, dp, lens, sets, zs[0][zs[1]:] if want_zs else None, ys[0][ys[1]:], pf[0][pf[1]:],
                            st[0][st[1]:], work=work if ws else None, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    z = taken(zs, J if want_zs else 0)
    p = taken(pf, 3 * J)
    return (z.tolist() if want_zs else None, taken(ys, J).tolist(), [bytes(p[3 * e:3 * e + 3]) for e in range(J)],
            taken(st, J).tolist(), work)


def check_dev(out, exp):
    zs, ys, proofs, status, _ = out
    assert status == [0] * len(exp[0])
    assert zs is None or zs == exp[0]
    assert ys == exp[1]
    assert proofs == exp[2]


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("rot", range(len(MASKS)))
def test_shape_sweep(hip, oracle, srs, srs_pts, rot):
    assert all(PM.mask_ok(m) for m in MASKS) and len(set(MASKS)) == len(MASKS)
    polys = [by_len(n) for n in LENGTHS]
    sets = [MASKS[(i + rot) % len(MASKS)] for i in range(len(LENGTHS))]
    exp = expect(oracle, srs_pts, polys, sets, keys=LENGTHS)
    assert exp[0] == [a for m in sets for a in PM.points(m)]
    assert hip.kzg_open_points(srs, polys, sets) == exp
    check_dev(points_dev(hip, srs, polys, sets), exp)


# ------------------------------------------------------------------ 2. batches and launch cuts
def mixed_batch(hip, n):
    """n polynomials, single-chunk and multi-chunk ones side by side in every launch, seeded masks"""
    pool = [1, 2, 16, 17, 255, 257, 4095, 4096, 4097, 8193]
    r = gen.splitmix64(0xBA7C, n)
    lens = [pool[int(v % np.uint64(len(pool)))] for v in r]
    L = hip.PLK_KZG_POINTS_LAUNCH_POLYS
    for first in range(0, n, L):                          # every launch holds both kinds
        if first + 1 < n:
            lens[first], lens[first + 1] = 8193, 3
    return lens, seeded_masks(0xBA7D, n)


def test_one_call_equals_one_polynomial_calls(hip, oracle, srs, srs_pts):
    L = hip.PLK_KZG_POINTS_LAUNCH_POLYS
    n = 2 * L + 1
    lens, sets = mixed_batch(hip, n)
    polys = [by_len(k) for k in lens]
    exp = expect(oracle, srs_pts, polys, sets, keys=lens)
    got = hip.kzg_open_points(srs, polys, sets)
    assert got == exp
    check_dev(points_dev(hip, srs, polys, sets), exp)
    for i in range(n):
        e0, t = PM.first_job(sets, i), len(PM.points(sets[i]))
        one = hip.kzg_open_points(srs, [polys[i]], [sets[i]])
        assert one == tuple(x[e0:e0 + t] for x in got), i


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_batch_sizes_around_one_launch(hip, oracle, srs, srs_pts, delta):
    n = hip.PLK_KZG_POINTS_LAUNCH_POLYS + delta
    lens, sets = mixed_batch(hip, 2 * hip.PLK_KZG_POINTS_LAUNCH_POLYS + 1)
    lens, sets = lens[:n], sets[:n]
    polys = [by_len(k) for k in lens]
    exp = expect(oracle, srs_pts, polys, sets, keys=lens)
    assert hip.kzg_open_points(srs, polys, sets) == exp
    check_dev(points_dev(hip, srs, polys, sets), exp)


# ------------------------------------------------------------------ 3. the specification read literally
def test_equals_kzg_open_on_the_expanded_list(hip, srs):
    tail = poly(9, 5000).copy()
    tail[4097:] = 0                                    # trailing zeros above a non-zero coefficient
    tail[4096] = 3
    polys = [np.zeros(1, np.uint8), np.zeros(300, np.uint8), np.zeros(4097, np.uint8), np.array([7], np.uint8),
             np.array([7, 0, 0, 0], np.uint8), tail, by_len(8193), by_len(255)]
    sets = [FULL, 0b1001, FULL, FULL, 1 | 1 << 16, FULL, 0b110, 1]
    jobs = PM.expand(sets)
    ys, proofs = hip.kzg_open(srs, [polys[i] for i, _ in jobs], [z for _, z in jobs])
    exp = ([z for _, z in jobs], ys, proofs)
    assert hip.kzg_open_points(srs, polys, sets) == exp
    check_dev(points_dev(hip, srs, polys, sets), exp)
    # len == 1: the identity proof and y = the coefficient
    e0 = PM.first_job(sets, 3)
    assert ys[e0:e0 + 17] == [7] * 17 and set(proofs[e0:e0 + 17]) == {bytes([0, 0, 1])}


# ------------------------------------------------------------------ 4. the carry beyond 257 chunks
def test_more_than_257_chunks(hip, oracle):
    n = 258 * 4096 + 5
    pts, _ = gen.msm_inputs(0x258C, n, "full")
    p = poly(81, n)
    sets = [0b11 | 1 << 16]
    exp = PM.open_points(oracle, pts, [p], sets)
    assert PM.chunks(n) == 259 and exp[0] == [0, 1, 16]
    with hip.Srs(pts) as s:
        assert hip.kzg_open_points(s, [p], sets) == exp
        check_dev(points_dev(hip, s, [p], sets), exp)


def test_carries_across_three_scan_tiles(hip, oracle):
    """the carries of a point are formed 1024 chunks at a time from the top down: 2050 chunks are three tiles
    (the last of two words), so every hand-over between tiles is taken"""
    n = 2049 * 4096 + 5
    pts, _ = gen.msm_inputs(0x2049, n, "full")
    p = poly(82, n)
    sets = [1 << 3 | 1 << 16]
    exp = PM.open_points(oracle, pts, [p], sets)
    assert PM.chunks(n) == 2050
    with hip.Srs(pts) as s:
        check_dev(points_dev(hip, s, [p], sets), exp)


# ------------------------------------------------------------------ 5. coefficient bytes >= 17
@pytest.mark.parametrize("where", ["first", "chunk_boundary", "last"])
def test_non_canonical_coefficient_bytes(hip, oracle, srs, srs_pts, where):
    n = 9000
    pos = {"first": 0, "chunk_boundary": 4096, "last": n - 1}[where]
    bad = poly(31, n).copy()
    bad[pos] = 200
    left, right = poly(32, 4500), poly(33, n)
    polys, sets = [left, bad, right], [0b100101, 1 | 1 << 5 | 1 << 16, FULL]
    exp = expect(oracle, srs_pts, [left, left, right], sets, keys=["nc_l", "nc_l", "nc_r"])
    lo, hi = PM.first_job(sets, 1), PM.first_job(sets, 2)
    # host form = the public entry points composed
    zs, ys, proofs = hip.kzg_open_points(srs, polys, sets)
    assert zs == exp[0]
    for e, z in zip(range(lo, hi), PM.points(sets[1])):
        q, _ = hip.poly_divide(bad, [(17 - z) % 17, 1])
        assert (ys[e], proofs[e]) == (hip.poly_eval(bad, z), hip.msm_g1(srs_pts[:len(q)], q)), (where, z)
    assert ys[:lo] == exp[1][:lo] and proofs[:lo] == exp[2][:lo]
    assert ys[hi:] == exp[1][hi:] and proofs[hi:] == exp[2][hi:]
    # device form: every job of that polynomial flagged, its canonical neighbours exact
    dz, dy, dp, st, _ = points_dev(hip, srs, polys, sets)
    assert st == PM.dev_status(polys, sets) and sum(st) == hi - lo and st[lo:hi] == [1] * (hi - lo)
    assert dz == exp[0]
    assert dp[lo:hi] == [FLAG] * (hi - lo)
    assert dy[:lo] == exp[1][:lo] and dp[:lo] == exp[2][:lo]
    assert dy[hi:] == exp[1][hi:] and dp[hi:] == exp[2][hi:]


# ------------------------------------------------------------------ 6. an SRS without log form
def test_irregular_srs(hip, oracle):
    n = 5000
    pts, _ = gen.msm_inputs(0x1229, n + 100, "full")
    pts = pts.copy()
    pts[2500] = (3, 3, 0)                              # off-curve
    polys, sets = [poly(41, n), poly(42, 600), poly(43, 4097)], [0b1000011, FULL, 1 << 9]
    exp = PM.open_points(oracle, pts, polys, sets)
    with hip.Srs(pts) as s:
        assert s.irregular
        assert hip.kzg_open_points(s, polys, sets) == exp
        dz, dy, dp, st, _ = points_dev(hip, s, polys, sets)
        assert st == PM.dev_status(polys, sets, irregular=True) == [1] * len(exp[0])
        assert dz == exp[0] and dy == exp[1]           # exact whatever the SRS
        assert dp == [FLAG] * len(exp[0])


# ------------------------------------------------------------------ 7. the SRS boundary
def test_srs_boundary(hip, oracle):
    n = 4100
    pts, _ = gen.msm_inputs(0xB0, n, "full")
    sets = [0b10001 | 1 << 16]
    with hip.Srs(pts) as s:
        p = poly(61, n + 1)                            # len - 1 == srs_len
        exp = PM.open_points(oracle, pts, [p], sets)
        assert hip.kzg_open_points(s, [p], sets) == exp
        check_dev(points_dev(hip, s, [p], sets), exp)
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open_points(s, [by_len(17), poly(62, n + 2)], [1, 2])
        assert err.value.code == hip.PLK_ERR_RANGE and "degree exceeds SRS size" in str(err.value)
        with pytest.raises(hip.PlonkHipError) as err:
            points_dev(hip, s, [poly(62, n + 2)], [FULL])
        assert err.value.code == hip.PLK_ERR_RANGE and "degree exceeds SRS size" in str(err.value)
    with hip.Srs(pts[:1]) as s1:                       # a one-point SRS opens up to two coefficients
        for x in ([5], [5, 6]):
            x = np.array(x, np.uint8)
            exp = PM.open_points(oracle, pts, [x], [FULL])
            assert hip.kzg_open_points(s1, [x], [FULL]) == exp
            check_dev(points_dev(hip, s1, [x], [FULL]), exp)
        with pytest.raises(hip.PlonkHipError):
            hip.kzg_open_points(s1, [[5, 6, 7]], [FULL])


# ------------------------------------------------------------------ 8. device rules
def test_device_api(hip, oracle, srs, srs_pts):
    import torch
    lens = [17, 4096, 4097, 8193, 3 * 4096 + 5]
    sets = [FULL, MASKS[5], 0b11, FULL, MASKS[6]]
    polys = [by_len(n) for n in lens]
    exp = expect(oracle, srs_pts, polys, sets, keys=lens)
    # polynomial pointers one byte past a 16-byte boundary (the byte-wise loads), outputs at odd offsets
    check_dev(points_dev(hip, srs, polys, sets, offset=1), exp)
    check_dev(points_dev(hip, srs, polys, sets, offset=1, out_offset=3), exp)
    check_dev(points_dev(hip, srs, polys, sets, out_offset=1), exp)
    # two calls back to back on the same workspace, nothing re-initialised
    first = points_dev(hip, srs, polys, sets)
    check_dev(first, exp)
    check_dev(points_dev(hip, srs, polys, sets, work=first[4]), exp)
    # the workspace left by a call of another shape
    check_dev(points_dev(hip, srs, polys[::-1], sets[::-1], work=first[4]),
              expect(oracle, srs_pts, polys[::-1], sets[::-1], keys=lens[::-1]))
    # a non-default stream
    check_dev(points_dev(hip, srs, polys, sets, stream=torch.cuda.Stream()), exp)
    # d_zs = NULL
    out = points_dev(hip, srs, polys, sets, want_zs=False)
    assert out[0] is None
    check_dev(out, exp)


# ------------------------------------------------------------------ 9. producer to verifier without the host
def test_openings_feed_the_verify_calls_on_the_device(hip):
    import torch

    import kzg_agg_model as A
    import pairing_model as M
    raw = load_golden("kzg_multi.json")
    kb = tuple(bytes.fromhex(raw["key"]))
    key = (kb[0:3], kb[3:5], kb[5:7])
    vk = hip.KzgVk(*key)
    g = np.array(list(bytes.fromhex(raw["srs"])), np.uint8).reshape(-1, 3)
    assert len(g) == 48 and all((g[i] == g[i % 8]).all() for i in range(48))   # (2^8 = 1 mod 17)
    pts = np.ascontiguousarray(np.tile(g[:8], (1025, 1))[:8200])
    lens = [17, 4097, 8193]
    polys = [poly(0xE2E + n, n) for n in lens]
    sets = [FULL] * 3
    m, J = 17, 51
    r = (gen.splitmix64(0x9E2E, J) % np.uint64(16)).astype(np.uint8) + np.uint8(1)
    with hip.Srs(pts) as s:
        assert not s.irregular
        dp = [torch.from_numpy(p).cuda() for p in polys]
        res = torch.zeros(3 * 2176, dtype=torch.uint8, device="cuda")
        hip.kzg_commit_dev(s, dp, lens, res)
        commits = res.view(3, 2176)[:, 16:19].repeat_interleave(m, dim=0).contiguous()   # the commitment per job
        zs, ys, st, pf = (torch.full((k,), 0xEE, dtype=torch.uint8, device="cuda") for k in (J, J, J, 3 * J))
        work = torch.full((hip.kzg_points_workspace(lens, sets),), 0xA5, dtype=torch.uint8, device="cuda")
        hip.kzg_open_points_dev(s, dp, lens, sets, zs, ys, pf, st, work=work)
        d_r = torch.from_numpy(r).cuda()
        ok1 = torch.full((J,), 0xEE, dtype=torch.uint8, device="cuda")
        okm = torch.full((3,), 0xEE, dtype=torch.uint8, device="cuda")
        ws = hip.kzg_verify_agg_workspace(m, 3)
        awork = torch.full((ws,), 0xA5, dtype=torch.uint8, device="cuda") if ws else None

        def verdicts():
            hip.kzg_verify_dev(vk, commits, zs, ys, pf, J, ok1)
            hip.kzg_verify_agg_dev(vk, m, commits, zs, ys, pf, d_r, 3, okm, work=awork)
            torch.cuda.synchronize()
            return ok1.cpu().numpy().tolist(), okm.cpu().numpy().tolist()

        assert verdicts() == ([1] * J, [1] * 3)
        assert st.cpu().numpy().tolist() == [0] * J and zs.cpu().numpy().tolist() == list(range(17)) * 3
        c, w = commits.cpu().numpy(), pf.cpu().numpy().reshape(-1, 3)
        z = zs.cpu().numpy()
        ct, wt = [tuple(int(v) for v in p) for p in c], [tuple(int(v) for v in p) for p in w]
        for j in (0, 20, 50):
            ys[j] = (ys[j] + 1) % 17
            y = ys.cpu().numpy()
            exp1 = [M.kzg_verify(key, ct[e], wt[e], int(z[e]), int(y[e])) for e in range(J)]
            expm = A.agg_raw_flat(key, m, c, z, y, w, r).tolist()
            assert exp1[j] == 0 and sum(exp1) == J - 1
            assert verdicts() == (exp1, expm), j
            ys[j] = (ys[j] + 16) % 17
