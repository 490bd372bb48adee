"""KZG flat batches (plk_kzg_commit_flat*, plk_kzg_open_flat*) on the GPU.

Expected values come from tests/kzg_flat_model.py (pinned to the oracle and to the reference's recorded values by
tests/test_kzg_flat_cpu.py) and, for the first polynomials of every list, from the library's own
plk_kzg_commit_batch / plk_kzg_open_batch on the expanded list, which is the specification.  Everything is exact:
bytes are compared for equality.  Every _dev output starts dirty (0xEE) with guard bytes on both sides."""
import numpy as np
import pytest

import devbuf
import gen
import kzg_flat_model as FM
from conftest import load_golden

pytestmark = pytest.mark.gpu

SRS_N = 4097
LANE_M = [1, 2, 3, 15, 16, 17, 31, 32]
WAVE_M = [33, 63, 64, 65, 255, 256, 257, 1008, 1023, 1024]
BLOCK_M = [1025, 2047, 2048, 4095, 4096]
FLAG = list(FM.FLAGGED)
SPEC_POLYS = 24          # polynomials per list also taken through plk_kzg_open_batch / plk_kzg_commit_batch


@pytest.fixture(scope="module")
def srs_pts():
    pts, _ = gen.msm_inputs(0xF1A7, SRS_N, "full")     # identity and the 2-torsion point included
    return pts


@pytest.fixture(scope="module")
def srs(hip, srs_pts):
    with hip.Srs(srs_pts) as s:
        assert len(s) == SRS_N and not s.irregular
        yield s


def coeffs(seed, n):
    return (gen.splitmix64(0xC0EF + seed, n) % np.uint64(17)).astype(np.uint8)


def npoly_for(m):
    """not a multiple of the plan's polynomials per block, at least three blocks, every z = g mod 17 met"""
    per = FM.plan(m, 1)["per_block"]
    n = {256: 2 * 256 + 37, 4: 4 * 8 + 3, 1: 19}[per]
    assert n >= 17 and -(-n // per) >= 3 and (per == 1 or n % per)
    return n


def flat_dev(hip, srs, co, m, npoly, zs=None, offsets=None, commits=True, in_res=0, out_res=1, stream=None):
    """one _dev call over guarded buffers -> dict(status, ys, proofs, commits) of numpy arrays; the coefficient
    array starts in_res bytes past a 16-byte boundary, every output out_res bytes past one"""
    import torch
    co = np.ascontiguousarray(co, np.uint8)
    cb, cv = devbuf.place(co, in_res, poison="raw")
    d_off = None if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, np.uint32).view(np.int32)).cuda()
    opening = zs is not None
    outs = {"status": devbuf.place_out(npoly, out_res)}
    if commits:
        outs["commits"] = devbuf.place_out(3 * npoly, out_res)
    if opening:
        zb, zv = devbuf.place(np.asarray(zs, np.uint8), out_res, poison="raw")
        outs["ys"] = devbuf.place_out(npoly, out_res)
        outs["proofs"] = devbuf.place_out(3 * npoly, out_res)
    torch.cuda.synchronize()
    v = {k: b[1] for k, b in outs.items()}
    if opening:
        hip.kzg_open_flat_dev(srs, cv, co.size, d_off, m, npoly, zv, v["ys"], v["proofs"], v.get("commits"), v["status"],
                              stream=stream)
    else:
        hip.kzg_commit_flat_dev(srs, cv, co.size, d_off, m, npoly, v["commits"], v["status"], stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    res = {"ys": None, "proofs": None, "commits": None}
    for k, (backing, view) in outs.items():
        assert devbuf.guards_intact(backing, view), "wrote outside " + k
        h = view.cpu().numpy().copy()
        res[k] = h.reshape(-1, 3) if k in ("proofs", "commits") else h
    return res


def check(got, exp, what=""):
    """every byte the header specifies"""
    assert got["status"].tolist() == exp["status"].tolist(), what
    for k in ("proofs", "commits"):
        assert (got[k] is None) == (exp[k] is None), (what, k)
        if exp[k] is not None:
            assert np.array_equal(got[k], exp[k]), (what, k, np.nonzero((got[k] != exp[k]).any(axis=1))[0][:8])
    if exp["ys"] is not None:
        e = exp["ys_exact"]
        assert np.array_equal(got["ys"][e], exp["ys"][e]), (what, "ys")


def spec(hip, srs, polys, zs):
    """the specification: plk_kzg_commit_batch / plk_kzg_open_batch on the expanded list"""
    ys, proofs = hip.kzg_open(srs, polys, zs)
    return ys, [list(p) for p in proofs], [list(c) for c in hip.kzg_commit(srs, polys)]


def check_spec(hip, srs, got, polys, zs, idx):
    ys, proofs, commits = spec(hip, srs, [polys[i] for i in idx], [int(zs[i]) for i in idx])
    assert got["ys"][idx].tolist() == ys
    assert got["proofs"][idx].tolist() == proofs
    assert got["commits"][idx].tolist() == commits


# ------------------------------------------------------------------ 1. uniform lengths, every path
@pytest.mark.parametrize("m", LANE_M + WAVE_M + BLOCK_M)
def test_uniform(hip, srs, srs_pts, m):
    npoly = npoly_for(m)
    plan = hip.kzg_flat_plan(m, npoly)
    assert plan == FM.plan(m, npoly) and plan["blocks"] >= 3 and plan["launches"] == 1
    assert plan["path"] == (0 if m in LANE_M else 1 if m in WAVE_M else 2)
    co = coeffs(m, m * npoly)
    zs = np.arange(npoly) % 17
    exp = FM.flat_dev(co, m, npoly, srs_pts, zs)
    assert exp["status"].sum() == 0
    got = flat_dev(hip, srs, co, m, npoly, zs, in_res=0, out_res=0)
    check(got, exp, "open")
    check_spec(hip, srs, got, FM.expanded(co, m, npoly), zs, list(range(min(SPEC_POLYS, npoly))))
    # without commitments, and commitments alone
    check(flat_dev(hip, srs, co, m, npoly, zs, commits=False), FM.flat_dev(co, m, npoly, srs_pts, zs, want_commits=False), "no commits")
    check(flat_dev(hip, srs, co, m, npoly), FM.flat_dev(co, m, npoly, srs_pts), "commit")
    # the host forms
    ys, proofs, commits = hip.kzg_open_flat(srs, co, zs, m=m, commits=True)
    assert np.array_equal(ys, exp["ys"]) and np.array_equal(proofs, exp["proofs"]) and np.array_equal(commits, exp["commits"])
    assert np.array_equal(hip.kzg_commit_flat(srs, co, m=m), exp["commits"])


def test_length_one_is_the_identity_proof(hip, srs, srs_pts):
    co = np.arange(34, dtype=np.uint8) % 17
    got = flat_dev(hip, srs, co, 1, 34, np.arange(34) % 17)
    assert got["ys"].tolist() == co.tolist() and got["status"].sum() == 0
    assert got["proofs"].tolist() == [[0, 0, 1]] * 34


# ------------------------------------------------------------------ 2. the grid-stride loop
@pytest.mark.parametrize("m", [1, 33, 1025])
def test_grid_stride(hip, srs, srs_pts, m):
    """npoly just above polynomials per block x blocks: the last polynomials are a block's second turn"""
    per = FM.plan(m, 1)["per_block"]
    npoly = per * 2048 + 1 + per // 2
    plan = hip.kzg_flat_plan(m, npoly)
    assert plan["blocks"] == 2048 and plan["per_block"] * plan["blocks"] < npoly
    co = coeffs(0x651D + m, m * npoly)
    zs = (np.arange(npoly) * 7 + 3) % 17
    check(flat_dev(hip, srs, co, m, npoly, zs), FM.flat_dev(co, m, npoly, srs_pts, zs), "grid stride")


# ------------------------------------------------------------------ 3. ragged lists
def ragged_list(m, seed):
    """(coeffs, offsets, zs, bad indices): lengths 1 .. m mixed; one empty polynomial, a falling offset, an offset
    above total, a polynomial of m + 1 coefficients, a z byte of 17 and one of 255"""
    r = gen.splitmix64(0x4A66 + seed, 48)
    lens = [1 + int(v % np.uint64(m)) for v in r]
    lens[:8] = [1, m, 2, max(m - 1, 1), min(16, m), min(17, m), min(15, m), m]
    lens[20] = m + 1                                   # one coefficient too long
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(off[-1])
    off = off.tolist()
    off.insert(12, off[12])                            # polynomial 12 is empty
    bad = {12, 21}                                     # (the long one moved up by one)
    off[30] = off[29] - 1                              # polynomial 29 falls; 30 starts lower and is a longer polynomial
    bad.add(29)
    if off[31] - off[30] > m:
        bad.add(30)
    off[40] = total + 5                                # polynomials 39 and 40: an offset above total (40 falls too)
    bad |= {39, 40}
    off[45] = 0xFFFFFFFF
    bad |= {44, 45}
    npoly = len(off) - 1
    zs = (np.arange(npoly) * 5 + 1) % 17
    zs[3], zs[17] = 17, 255
    bad |= {3, 17}
    return coeffs(0x4A67 + seed, total), np.array(off, np.uint32), zs.astype(np.uint8), sorted(bad)


@pytest.mark.parametrize("m", [32, 1024, 4096])
def test_ragged(hip, srs, srs_pts, m):
    co, off, zs, bad = ragged_list(m, m)
    npoly = off.size - 1
    exp = FM.flat_dev(co, m, npoly, srs_pts, zs, offsets=off)
    assert np.nonzero(exp["status"])[0].tolist() == bad and (exp["status"][bad] == FM.BAD).all()
    got = flat_dev(hip, srs, co, m, npoly, zs, offsets=off)
    check(got, exp, "ragged open")
    assert got["proofs"][bad].tolist() == [FLAG] * len(bad) and got["commits"][bad].tolist() == [FLAG] * len(bad)
    # the neighbours against the specification
    good = [g for g in range(npoly) if g not in bad]
    polys = {g: co[int(off[g]):int(off[g + 1])] for g in good}
    assert {1, m} <= {len(p) for p in polys.values()}
    ys, proofs, commits = spec(hip, srs, [polys[g] for g in good], [int(zs[g]) for g in good])
    assert got["ys"][good].tolist() == ys and got["proofs"][good].tolist() == proofs and got["commits"][good].tolist() == commits
    # commitments alone: no z, so only the broken segments are flagged
    expc = FM.flat_dev(co, m, npoly, srs_pts, offsets=off)
    assert np.nonzero(expc["status"])[0].tolist() == [g for g in bad if g not in (3, 17)]
    check(flat_dev(hip, srs, co, m, npoly, offsets=off), expc, "ragged commit")
    # the host form refuses the list, and takes its valid part
    with pytest.raises(hip.PlonkHipError) as err:
        hip.kzg_open_flat(srs, co, zs, offsets=off, m=m)
    assert err.value.code == hip.PLK_ERR_ARG
    goff = np.concatenate([[0], np.cumsum([len(polys[g]) for g in good])]).astype(np.uint32)
    gco = np.concatenate([polys[g] for g in good])
    hy, hp, hc = hip.kzg_open_flat(srs, gco, zs[good], offsets=goff, m=m, commits=True)
    assert hy.tolist() == ys and hp.tolist() == proofs and hc.tolist() == commits
    assert hip.kzg_commit_flat(srs, gco, offsets=goff, m=m).tolist() == commits


# ------------------------------------------------------------------ 4. coefficient bytes >= 17
@pytest.mark.parametrize("m", [32, 700, 3000])
def test_non_canonical_bytes(hip, srs, srs_pts, m):
    """a byte >= 17 at the first byte, at coefficients 15 and 16 (a lane boundary) and at the last byte, each in a
    polynomial of its own: the opening is flagged, the commitment exact, the neighbours exact"""
    npoly = 13
    co = coeffs(0xBAD + m, m * npoly).copy()
    where = {1: 0, 4: 15, 7: 16, 10: m - 1}
    for g, (pos, byte) in zip(where, zip(where.values(), (17, 200, 255, 18))):
        co[g * m + pos] = byte
    zs = np.arange(npoly) % 17
    exp = FM.flat_dev(co, m, npoly, srs_pts, zs)
    assert np.nonzero(exp["status"])[0].tolist() == sorted(where) and (exp["status"][sorted(where)] == FM.IRREGULAR).all()
    got = flat_dev(hip, srs, co, m, npoly, zs)
    check(got, exp, "non-canonical")
    assert got["proofs"][sorted(where)].tolist() == [FLAG] * 4
    polys = FM.expanded(co, m, npoly)
    ys, proofs, commits = spec(hip, srs, polys, zs.tolist())     # (exact for every byte: the host forms' composition)
    assert got["commits"].tolist() == commits
    good = [g for g in range(npoly) if g not in where]
    assert got["ys"][good].tolist() == [ys[g] for g in good] and got["proofs"][good].tolist() == [proofs[g] for g in good]
    # commitments alone take any byte
    gc = flat_dev(hip, srs, co, m, npoly)
    assert gc["status"].sum() == 0 and gc["commits"].tolist() == commits
    # the host forms are exact for every byte
    hy, hp, hc = hip.kzg_open_flat(srs, co, zs, m=m, commits=True)
    assert hy.tolist() == ys and hp.tolist() == proofs and hc.tolist() == commits
    assert hip.kzg_commit_flat(srs, co, m=m).tolist() == commits


# ------------------------------------------------------------------ 5. an SRS without log form
def test_irregular_srs(hip, srs_pts):
    pts = srs_pts[:2100].copy()
    pts[7] = (3, 3, 0)                                 # off-curve
    with hip.Srs(pts) as s:
        assert s.irregular
        for m, npoly in ((20, 300), (100, 9), (2000, 5)):
            co = coeffs(0x1229 + m, m * npoly)
            zs = np.arange(npoly) % 17
            exp = FM.flat_dev(co, m, npoly, pts, zs)
            assert (exp["status"] == FM.IRREGULAR).all() and exp["ys_exact"].all()
            got = flat_dev(hip, s, co, m, npoly, zs)
            check(got, exp, m)
            assert (got["proofs"] == 0xFF).all() and (got["commits"] == 0xFF).all()
            assert got["ys"].tolist() == FM.flat_dev(co, m, npoly, srs_pts, zs)["ys"].tolist()   # exact whatever the SRS
            gc = flat_dev(hip, s, co, m, npoly)
            assert (gc["status"] == FM.IRREGULAR).all() and (gc["commits"] == 0xFF).all()
            # the host forms: exact through plk_kzg_open_batch / plk_kzg_commit_batch
            k = min(npoly, 6)
            polys = FM.expanded(co, m, npoly)[:k]
            ys, proofs, commits = spec(hip, s, polys, zs[:k].tolist())
            hy, hp, hc = hip.kzg_open_flat(s, co[:k * m], zs[:k], m=m, commits=True)
            assert hy.tolist() == ys and hp.tolist() == proofs and hc.tolist() == commits
            assert hip.kzg_commit_flat(s, co[:k * m], m=m).tolist() == commits


# ------------------------------------------------------------------ 6. the SRS boundary
@pytest.mark.parametrize("n", [16, 40, 1040])
def test_srs_boundary(hip, srs_pts, n):
    pts = srs_pts[:n]
    npoly = 21
    with hip.Srs(pts) as s:
        zs = np.arange(npoly) % 17
        co = coeffs(0xB0 + n, n * npoly)                     # m == plk_srs_len commits
        check(flat_dev(hip, s, co, n, npoly), FM.flat_dev(co, n, npoly, pts), "commit at the bound")
        check(flat_dev(hip, s, co, n, npoly, zs), FM.flat_dev(co, n, npoly, pts, zs), "open with commitments at the bound")
        co = coeffs(0xB1 + n, (n + 1) * npoly)               # m == plk_srs_len + 1 opens without commitments
        got = flat_dev(hip, s, co, n + 1, npoly, zs, commits=False)
        check(got, FM.flat_dev(co, n + 1, npoly, pts, zs, want_commits=False), "open one past")
        ys, proofs = hip.kzg_open(s, FM.expanded(co, n + 1, npoly), zs.tolist())
        assert got["ys"].tolist() == ys and got["proofs"].tolist() == [list(p) for p in proofs]
        hy, hp = hip.kzg_open_flat(s, co, zs, m=n + 1)
        assert hy.tolist() == ys and hp.tolist() == [list(p) for p in proofs]
        for call in (lambda: flat_dev(hip, s, co, n + 1, npoly),                    # commit one past
                     lambda: flat_dev(hip, s, co, n + 1, npoly, zs),                # open one past, commitments asked for
                     lambda: hip.kzg_commit_flat(s, co, m=n + 1),
                     lambda: hip.kzg_open_flat(s, co, zs, m=n + 1, commits=True),
                     lambda: flat_dev(hip, s, coeffs(1, (n + 2) * 3), n + 2, 3, [1, 2, 3], commits=False),
                     lambda: hip.kzg_open_flat(s, coeffs(1, (n + 2) * 3), [1, 2, 3], m=n + 2)):
            with pytest.raises(hip.PlonkHipError) as err:
                call()
            assert err.value.code == hip.PLK_ERR_RANGE and "degree exceeds SRS size" in str(err.value)
        # the ragged form is bound by m as given, whatever the lengths are
        off = np.array([0, 3, 5], np.uint32)
        with pytest.raises(hip.PlonkHipError) as err:
            flat_dev(hip, s, coeffs(2, 5), n + 1, 2, offsets=off)
        assert err.value.code == hip.PLK_ERR_RANGE


# ------------------------------------------------------------------ 7. alignment and guard bytes
@pytest.mark.parametrize("m,ragged", [(32, False), (16, False), (48, False), (1100, False), (32, True), (300, True)])
def test_alignment_and_guards(hip, srs, srs_pts, m, ragged):
    npoly = 260 if m <= 32 else 23
    zs = np.arange(npoly) % 17
    if ragged:
        lens = 1 + (gen.splitmix64(0xA119 + m, npoly) % np.uint64(m)).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    else:
        off = None
    co = coeffs(0xA11 + m, int(off[-1]) if ragged else m * npoly)
    exp = FM.flat_dev(co, m, npoly, srs_pts, zs, offsets=off)
    assert exp["status"].sum() == 0
    base = flat_dev(hip, srs, co, m, npoly, zs, offsets=off, in_res=0, out_res=0)
    check(base, exp, "aligned")
    for res in range(16):
        got = flat_dev(hip, srs, co, m, npoly, zs, offsets=off, in_res=res, out_res=2 * (res % 8) + 1)
        for k in ("status", "ys", "proofs", "commits"):
            assert np.array_equal(got[k], base[k]), (res, k)
    gc = flat_dev(hip, srs, co, m, npoly, offsets=off, in_res=5, out_res=3)
    assert np.array_equal(gc["commits"], base["commits"]) and gc["status"].sum() == 0


# ------------------------------------------------------------------ 8. repeatability and streams
@pytest.mark.parametrize("m", [24, 500, 2500])
def test_repeatability_and_streams(hip, srs, srs_pts, m):
    import torch
    npoly = 700 if m <= 32 else 37
    co = coeffs(0x5712 + m, m * npoly)
    zs = (np.arange(npoly) * 3) % 17
    exp = FM.flat_dev(co, m, npoly, srs_pts, zs)
    a = flat_dev(hip, srs, co, m, npoly, zs)
    b = flat_dev(hip, srs, co, m, npoly, zs)
    check(a, exp)
    for k in ("status", "ys", "proofs", "commits"):
        assert np.array_equal(a[k], b[k]), k
    # two calls in flight on two streams, distinct outputs
    d_co = torch.from_numpy(co).cuda()
    d_zs = torch.from_numpy(zs.astype(np.uint8)).cuda()
    outs = [[torch.full((k,), 0xEE, dtype=torch.uint8, device="cuda") for k in (npoly, 3 * npoly, 3 * npoly, npoly)] for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for st, (ys, pr, cm, status) in zip(streams, outs):
        hip.kzg_open_flat_dev(srs, d_co, co.size, None, m, npoly, d_zs, ys, pr, cm, status, stream=st)
    for st in streams:
        st.synchronize()
    torch.cuda.synchronize()
    for ys, pr, cm, status in outs:
        assert np.array_equal(ys.cpu().numpy(), a["ys"]) and np.array_equal(status.cpu().numpy(), a["status"])
        assert np.array_equal(pr.cpu().numpy().reshape(-1, 3), a["proofs"])
        assert np.array_equal(cm.cpu().numpy().reshape(-1, 3), a["commits"])


# ------------------------------------------------------------------ 9. producer to verifier without the host
@pytest.mark.parametrize("m", [24, 100, 1500])
def test_openings_feed_the_verify_calls_on_the_device(hip, m):
    import torch
    g = load_golden("pairing.json")
    vk = hip.KzgVk((1, 2, 0), bytes.fromhex(g["g2_multiples"]["1"]), bytes.fromhex(g["g2_multiples"]["2"]))
    pts = np.ascontiguousarray(FM.rule_srs(m))            # srs[i] = (2^i mod 17) G: s = 2
    group, ngroups = 4, 9
    npoly = group * ngroups
    co = coeffs(0xE2E + m, m * npoly).copy()
    flagged = 14
    co[flagged * m + m // 2] = 99                         # one polynomial with a byte >= 17
    zs = np.arange(npoly) % 17
    rs = (gen.splitmix64(0x9E2E + m, npoly) % np.uint64(16)).astype(np.uint8) + np.uint8(1)
    with hip.Srs(pts) as s:
        assert not s.irregular
        d_co, d_zs, d_rs = (torch.from_numpy(np.ascontiguousarray(x, np.uint8)).cuda() for x in (co, zs, rs))
        ys, status, ok1 = (torch.full((npoly,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(3))
        pr, cm = (torch.full((3 * npoly,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
        okg = torch.full((ngroups,), 0xEE, dtype=torch.uint8, device="cuda")
        ws = hip.kzg_verify_agg_workspace(group, ngroups)
        awork = torch.full((ws,), 0xA5, dtype=torch.uint8, device="cuda") if ws else None
        hip.kzg_open_flat_dev(s, d_co, co.size, None, m, npoly, d_zs, ys, pr, cm, status)

        def verdicts():
            hip.kzg_verify_dev(vk, cm, d_zs, ys, pr, npoly, ok1)
            hip.kzg_verify_agg_dev(vk, group, cm, d_zs, ys, pr, d_rs, ngroups, okg, work=awork)
            torch.cuda.synchronize()
            return ok1.cpu().numpy().tolist(), okg.cpu().numpy().tolist()

        exp1 = [1] * npoly
        exp1[flagged] = 2                                  # FF FF FF is answered with 2, never with an accept
        expg = [1] * ngroups
        expg[flagged // group] = 2
        assert status.cpu().numpy().tolist() == [1 if i == flagged else 0 for i in range(npoly)]
        assert verdicts() == (exp1, expg)
        for j in (0, 21, npoly - 1):                       # one y changed on the device
            ys[j] = (ys[j] + 1) % 17
            e1, eg = list(exp1), list(expg)
            e1[j], eg[j // group] = 0, 0                   # (its weight is non-zero and the group's other jobs hold)
            assert verdicts() == (e1, eg), j
            ys[j] = (ys[j] + 16) % 17
        assert verdicts() == (exp1, expg)


# ------------------------------------------------------------------ 10. errors with a live handle
def test_errors_with_a_live_handle(hip, srs):
    import torch
    co = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for kw, code in ((dict(total=64, m=16, npoly=0), hip.PLK_ERR_ARG), (dict(total=0, m=16, npoly=4), hip.PLK_ERR_ARG),
                     (dict(total=64, m=0, npoly=4), hip.PLK_ERR_ARG), (dict(total=63, m=16, npoly=4), hip.PLK_ERR_ARG),
                     (dict(total=4097, m=4097, npoly=1), hip.PLK_ERR_RANGE), (dict(total=1 << 32, m=4096, npoly=1 << 20), hip.PLK_ERR_RANGE),
                     (dict(total=(1 << 30) + 1, m=1, npoly=(1 << 30) + 1), hip.PLK_ERR_RANGE)):
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_commit_flat_dev(srs, co, kw["total"], None, kw["m"], kw["npoly"], out, out)
        assert err.value.code == code, kw
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open_flat_dev(srs, co, kw["total"], None, kw["m"], kw["npoly"], out, out, out, None, out)
        assert err.value.code == code, kw
    with pytest.raises(hip.PlonkHipError) as err:
        hip.kzg_open_flat_dev(srs, co, 64, None, 16, 4, out, out, None, None, out)
    assert err.value.code == hip.PLK_ERR_ARG
