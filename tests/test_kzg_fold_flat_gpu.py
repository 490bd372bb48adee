"""KZG flat folded openings (plk_kzg_open_fold_flat*) on the GPU.

Expected values come from tests/kzg_fold_flat_model.py (pinned to kzg_fold_model, the oracle and through them to
the reference's recorded values by tests/test_kzg_fold_flat_cpu.py) and, for the first groups of every list, from
the library's own plk_kzg_open_fold_batch / plk_kzg_commit_batch on the expanded groups, which is the
specification.  Everything is exact: bytes are compared for equality.  Every _dev output starts dirty (0xEE) with
guard bytes on both sides."""
import numpy as np
import pytest

import devbuf
import gen
import kzg_flat_model as FM
import kzg_fold_flat_model as FF
import kzg_fold_model as F
from conftest import load_golden

pytestmark = pytest.mark.gpu

SRS_N = 4097
FLAG = list(FF.FLAGGED)
SPEC_GROUPS = 24          # groups per list also taken through plk_kzg_open_fold_batch / plk_kzg_commit_batch
LANE_M, LANE_K = [1, 2, 15, 16, 17, 31, 32], [1, 2, 3, 16]
WAVE_M, WAVE_K = [33, 64, 65, 255, 1008, 1023, 1024], [1, 4, 5, 9, 16]
BLOCK_M, BLOCK_K = [1025, 2048, 4095, 4096], [1, 9, 16]


def pairs(ms, ks):
    """every m with two values of k, every k with at least one m"""
    out = [(m, ks[(i + j) % len(ks)]) for i, m in enumerate(ms) for j in (0, 1)]
    assert {k for _, k in out} == set(ks)
    return out


UNIFORM = pairs(LANE_M, LANE_K) + pairs(WAVE_M, WAVE_K) + pairs(BLOCK_M, BLOCK_K)


@pytest.fixture(scope="module")
def srs_pts():
    pts, _ = gen.msm_inputs(0xF1A7, SRS_N, "full")     # identity and the 2-torsion point included: all 102 elements
    return pts


@pytest.fixture(scope="module")
def srs(hip, srs_pts):
    with hip.Srs(srs_pts) as s:
        assert len(s) == SRS_N and not s.irregular
        yield s


def coeffs(seed, n):
    return (gen.splitmix64(0xF01D + seed, n) % np.uint64(17)).astype(np.uint8)


def weights_for(seed, n):
    """values 0 .. 16, zeros among them"""
    w = (gen.splitmix64(0x3E16 + seed, n) % np.uint64(17)).astype(np.uint8)
    w[::7] = 0
    return w


def ngroups_for(m):
    """not a multiple of the plan's groups per block, at least three blocks, every z = g mod 17 met"""
    per = FF.plan(m, 1, 1)["per_block"]
    n = {256: 2 * 256 + 37, 4: 4 * 8 + 3, 1: 19}[per]
    assert n >= 17 and -(-n // per) >= 3 and (per == 1 or n % per)
    return n


def fold_dev(hip, srs, co, m, k, ng, w, zs, offsets=None, commits=True, in_res=0, out_res=1, stream=None):
    """one _dev call over guarded buffers -> dict(status, ys, proofs, commits) of numpy arrays; the coefficient
    array starts in_res bytes past a 16-byte boundary, every output out_res bytes past one"""
    import torch
    co = np.ascontiguousarray(co, np.uint8)
    cb, cv = devbuf.place(co, in_res, poison="raw")
    wb, wv = devbuf.place(np.asarray(w, np.uint8), out_res, poison="raw")
    zb, zv = devbuf.place(np.asarray(zs, np.uint8), out_res, poison="raw")
    d_off = None if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, np.uint32).view(np.int32)).cuda()
    outs = {"status": devbuf.place_out(ng, out_res), "ys": devbuf.place_out(k * ng, out_res),
            "proofs": devbuf.place_out(3 * ng, out_res)}
    if commits:
        outs["commits"] = devbuf.place_out(3 * k * ng, out_res)
    torch.cuda.synchronize()
    v = {n: b[1] for n, b in outs.items()}
    hip.kzg_open_fold_flat_dev(srs, cv, co.size, d_off, m, k, ng, wv, zv, v["ys"], v["proofs"], v.get("commits"), v["status"],
                               stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    res = {"commits": None}
    for n, (backing, view) in outs.items():
        assert devbuf.guards_intact(backing, view), "wrote outside " + n
        h = view.cpu().numpy().copy()
        res[n] = h.reshape(-1, 3) if n in ("proofs", "commits") else h
    return res


def check(got, exp, what=""):
    """every byte the header specifies"""
    assert got["status"].tolist() == exp["status"].tolist(), what
    for n in ("proofs", "commits"):
        assert (got[n] is None) == (exp[n] is None), (what, n)
        if exp[n] is not None:
            assert np.array_equal(got[n], exp[n]), (what, n, np.nonzero((got[n] != exp[n]).any(axis=1))[0][:8])
    e = exp["ys_exact"]
    assert np.array_equal(got["ys"][e], exp["ys"][e]), (what, "ys", np.nonzero(got["ys"] != exp["ys"])[0][:8])


def spec(hip, srs, groups, weights, zs):
    """the specification: plk_kzg_open_fold_batch / plk_kzg_commit_batch on the expanded groups ->
    (ys flat, proofs, commits flat)"""
    ys, proofs = hip.kzg_open_fold(srs, groups, [list(map(int, w)) for w in weights], [int(z) for z in zs])
    commits = hip.kzg_commit(srs, [p for g in groups for p in g])
    return [y for g in ys for y in g], [list(p) for p in proofs], [list(c) for c in commits]


def check_spec(hip, srs, got, groups, w, zs, k, idx, commits=True):
    ys, proofs, cm = spec(hip, srs, [groups[g] for g in idx], [w[k * g:k * (g + 1)] for g in idx], [zs[g] for g in idx])
    e = [k * g + i for g in idx for i in range(k)]
    assert got["ys"][e].tolist() == ys
    assert got["proofs"][idx].tolist() == proofs
    if commits:
        assert got["commits"][e].tolist() == cm


# ------------------------------------------------------------------ 1. uniform lengths, every path
@pytest.mark.parametrize("m,k", UNIFORM)
def test_uniform(hip, srs, srs_pts, m, k):
    ng = ngroups_for(m)
    plan = hip.kzg_fold_flat_plan(m, k, ng)
    assert plan == FF.plan(m, k, ng) and plan["blocks"] >= 3 and plan["launches"] == 1
    assert plan["path"] == (0 if m in LANE_M else 1 if m in WAVE_M else 2)
    co = coeffs(100 * m + k, m * k * ng)
    w = weights_for(100 * m + k, k * ng)
    zs = np.arange(ng) % 17
    exp = FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs)
    assert exp["status"].sum() == 0
    got = fold_dev(hip, srs, co, m, k, ng, w, zs, in_res=0, out_res=0)
    check(got, exp, "open")
    check_spec(hip, srs, got, FF.expanded(co, m, k, ng), w, zs, k, list(range(min(SPEC_GROUPS, ng))))
    # without commitments
    check(fold_dev(hip, srs, co, m, k, ng, w, zs, commits=False),
          FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs, want_commits=False), "no commits")
    # the host form
    ys, proofs, commits = hip.kzg_open_fold_flat(srs, co, k, w, zs, m=m, commits=True)
    assert np.array_equal(ys, exp["ys"]) and np.array_equal(proofs, exp["proofs"]) and np.array_equal(commits, exp["commits"])
    ys, proofs = hip.kzg_open_fold_flat(srs, co, k, w, zs, m=m)
    assert np.array_equal(ys, exp["ys"]) and np.array_equal(proofs, exp["proofs"])


# ------------------------------------------------------------------ 2. degenerate groups
def degenerate_list(m, z):
    """groups of two: plain, all weights zero, the cancelling pair (p, p under 1 and 16), F cancelling only its top
    coefficients, every polynomial shorter than m, L = 1, plain"""
    p = coeffs(0xDE6 + m, m)
    p[-1] = 5
    top = p.copy()
    top[:m // 3 + 1] = coeffs(0xDE7 + m, m // 3 + 1)          # equal above m // 3: F keeps degree <= m // 3
    top[m // 3] = (int(p[m // 3]) + 1) % 17
    groups = [[coeffs(1 + m, m), coeffs(2 + m, max(m // 2, 1))], [p, coeffs(3 + m, m - 1)], [p, p], [p, top],
              [coeffs(4 + m, m // 2 + 1), coeffs(5 + m, 3)], [np.array([5], np.uint8), np.array([7], np.uint8)],
              [coeffs(6 + m, 17), coeffs(7 + m, m)]]
    weights = np.array([3, 4, 0, 0, 1, 16, 1, 16, 2, 9, 3, 4, 16, 1], np.uint8)
    polys = [q for g in groups for q in g]
    off = np.concatenate([[0], np.cumsum([len(q) for q in polys])]).astype(np.uint32)
    return groups, np.concatenate(polys), off, weights, np.full(len(groups), z, np.uint8)


@pytest.mark.parametrize("m", [32, 1024, 4096])
def test_degenerate_groups(hip, srs, srs_pts, m):
    for z in (0, 1, 6):
        groups, co, off, w, zs = degenerate_list(m, z)
        ng = len(groups)
        exp = FF.fold_flat_dev(co, m, 2, ng, srs_pts, w, zs, offsets=off)
        assert exp["status"].sum() == 0
        assert exp["proofs"][[1, 2, 5]].tolist() == [[0, 0, 1]] * 3          # F = 0, F = 0, L = 1: the identity proof
        got = fold_dev(hip, srs, co, m, 2, ng, w, zs, offsets=off)
        check(got, exp, ("degenerate", z))
        check_spec(hip, srs, got, groups, w, zs, 2, list(range(ng)))
        # F's top cancels: the proof is that of the short F itself
        Fb = F.trim(F.fold(groups[3], [1, 16]))
        assert Fb.size == m // 3 + 1
        ys, proofs = hip.kzg_open(srs, [Fb], [z])
        assert got["proofs"][3].tolist() == list(proofs[0])
        hy, hp, hc = hip.kzg_open_fold_flat(srs, co, 2, w, zs, offsets=off, m=m, commits=True)
        assert np.array_equal(hy, exp["ys"]) and np.array_equal(hp, exp["proofs"]) and np.array_equal(hc, exp["commits"])


def test_length_one_is_the_identity_proof(hip, srs, srs_pts):
    k, ng = 3, 40
    co = np.arange(k * ng, dtype=np.uint8) % 17
    w = weights_for(1, k * ng)
    got = fold_dev(hip, srs, co, 1, k, ng, w, np.arange(ng) % 17)
    assert got["ys"].tolist() == co.tolist() and got["status"].sum() == 0
    assert got["proofs"].tolist() == [[0, 0, 1]] * ng
    assert got["commits"].tolist() == FM.commit_rows(co.reshape(-1, 1), FM.srs_logs(srs_pts)).tolist()


# ------------------------------------------------------------------ 3. the grid-stride loop
@pytest.mark.parametrize("m,k", [(1, 2), (33, 2), (1025, 2)])
def test_grid_stride(hip, srs, srs_pts, m, k):
    """ngroups just above groups per block x blocks: the last groups are a block's second turn"""
    per = FF.plan(m, k, 1)["per_block"]
    ng = per * 2048 + 1 + per // 2
    plan = hip.kzg_fold_flat_plan(m, k, ng)
    assert plan["blocks"] == 2048 and plan["per_block"] * plan["blocks"] < ng
    co = coeffs(0x651D + m, m * k * ng)
    w = weights_for(0x651D + m, k * ng)
    zs = (np.arange(ng) * 7 + 3) % 17
    check(fold_dev(hip, srs, co, m, k, ng, w, zs), FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs), "grid stride")


# ------------------------------------------------------------------ 4. ragged lists
RAGGED_K = 3


def ragged_list(m, seed):
    """(coeffs, offsets, weights, zs, bad groups): 21 groups of three, lengths 1 .. m mixed inside the groups; one
    group each with an empty polynomial, a falling offset, an offset above total, an offset of 0xFFFFFFFF, a
    polynomial of m + 1 coefficients, z = 17, z = 255, a weight of 17 and a weight of 255, every one between valid
    neighbours"""
    k, ng = RAGGED_K, 21
    r = gen.splitmix64(0x4A66 + seed, k * ng)
    lens = [1 + int(v % np.uint64(m)) for v in r]
    lens[:9] = [1, m, 2, max(m - 1, 1), min(16, m), min(17, m), min(15, m), m, m]
    lens[k * 2 + 1] = 0                                  # group 2: an empty polynomial
    lens[k * 10 + 2] = m + 1                             # group 10: one coefficient too long
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(off[-1])
    off[k * 4 + 1] = off[k * 4] - 1                      # group 4: its first polynomial falls
    off[k * 6 + 1] = total + 5                           # group 6: an offset above total (and the next polynomial falls)
    off[k * 8 + 2] = 0xFFFFFFFF                          # group 8
    zs = (np.arange(ng) * 5 + 1) % 17
    zs[12], zs[14] = 17, 255
    w = weights_for(0x4A67 + seed, k * ng)
    w[k * 16], w[k * 18 + 2] = 17, 255
    return coeffs(0x4A68 + seed, total), off.astype(np.uint32), w, zs.astype(np.uint8), [2, 4, 6, 8, 10, 12, 14, 16, 18]


@pytest.mark.parametrize("m", [32, 1024, 4096])
def test_ragged(hip, srs, srs_pts, m):
    k = RAGGED_K
    co, off, w, zs, bad = ragged_list(m, m)
    ng = zs.size
    exp = FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs, offsets=off)
    assert np.nonzero(exp["status"])[0].tolist() == bad and (exp["status"][bad] == FF.BAD).all()
    got = fold_dev(hip, srs, co, m, k, ng, w, zs, offsets=off)
    check(got, exp, "ragged")
    assert got["proofs"][bad].tolist() == [FLAG] * len(bad)
    assert (got["ys"].reshape(ng, k)[bad] == 0xFF).all() and (got["commits"].reshape(ng, k, 3)[bad] == 0xFF).all()
    check(fold_dev(hip, srs, co, m, k, ng, w, zs, offsets=off, commits=False),
          FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs, offsets=off, want_commits=False), "ragged, no commits")
    # the neighbours against the specification
    good = [g for g in range(ng) if g not in bad]
    groups = {g: [co[int(off[e]):int(off[e + 1])] for e in range(k * g, k * (g + 1))] for g in good}
    assert {1, m} <= {len(p) for g in good for p in groups[g]}
    check_spec(hip, srs, got, groups, w, zs, k, good)
    # the host form refuses the list, and takes its valid part
    with pytest.raises(hip.PlonkHipError) as err:
        hip.kzg_open_fold_flat(srs, co, k, w, zs, offsets=off, m=m)
    assert err.value.code == hip.PLK_ERR_ARG
    polys = [p for g in good for p in groups[g]]
    goff = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.uint32)
    e = [k * g + i for g in good for i in range(k)]
    hy, hp, hc = hip.kzg_open_fold_flat(srs, np.concatenate(polys), k, w[e], zs[good], offsets=goff, m=m, commits=True)
    assert np.array_equal(hy, got["ys"][e]) and np.array_equal(hp, got["proofs"][good]) and np.array_equal(hc, got["commits"][e])


# ------------------------------------------------------------------ 5. coefficient bytes >= 17
@pytest.mark.parametrize("m", [32, 700, 3000])
def test_non_canonical_bytes(hip, srs, srs_pts, m):
    """a byte >= 17 at the first byte, at coefficients 15 and 16 (a lane boundary) and at the last byte, in the first
    and in the last polynomial of a group: the group is flagged, its commitments exact, the neighbours exact"""
    k, ng = 3, 17
    co = coeffs(0xBAD + m, m * k * ng).copy()
    cases = [(pos, i) for pos in (0, 15, 16, m - 1) for i in (0, k - 1)]
    flagged = list(range(1, 17, 2))
    for g, (pos, i), byte in zip(flagged, cases, (17, 200, 255, 18, 100, 17, 254, 99)):
        co[(k * g + i) * m + pos] = byte
    w = weights_for(0xBAD + m, k * ng)
    zs = np.arange(ng) % 17
    exp = FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs)
    assert np.nonzero(exp["status"])[0].tolist() == flagged and (exp["status"][flagged] == FF.IRREGULAR).all()
    got = fold_dev(hip, srs, co, m, k, ng, w, zs)
    check(got, exp, "non-canonical")
    assert got["proofs"][flagged].tolist() == [FLAG] * len(flagged)
    groups = FF.expanded(co, m, k, ng)
    ys, proofs, commits = spec(hip, srs, groups, w.reshape(ng, k), zs)      # (exact for every byte: the host calls)
    assert got["commits"].tolist() == commits
    good = [g for g in range(ng) if g not in flagged]
    e = [k * g + i for g in good for i in range(k)]
    assert got["ys"][e].tolist() == [ys[j] for j in e] and got["proofs"][good].tolist() == [proofs[g] for g in good]
    # the host form is exact for every byte
    hy, hp, hc = hip.kzg_open_fold_flat(srs, co, k, w, zs, m=m, commits=True)
    assert hy.tolist() == ys and hp.tolist() == proofs and hc.tolist() == commits


# ------------------------------------------------------------------ 6. an SRS without log form
def test_irregular_srs(hip, srs_pts):
    pts = srs_pts[:2100].copy()
    pts[7] = (3, 3, 0)                                 # off-curve
    with hip.Srs(pts) as s:
        assert s.irregular
        for m, k, ng in ((20, 3, 300), (100, 5, 9), (2000, 2, 5)):
            co = coeffs(0x1229 + m, m * k * ng)
            w = weights_for(0x1229 + m, k * ng)
            zs = np.arange(ng) % 17
            exp = FF.fold_flat_dev(co, m, k, ng, pts, w, zs)
            assert (exp["status"] == FF.IRREGULAR).all() and exp["ys_exact"].all()
            got = fold_dev(hip, s, co, m, k, ng, w, zs)
            check(got, exp, m)
            assert (got["proofs"] == 0xFF).all() and (got["commits"] == 0xFF).all()
            assert got["ys"].tolist() == FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs)["ys"].tolist()   # exact whatever the SRS
            # the host form: exact through plk_kzg_open_fold_batch / plk_kzg_commit_batch
            n = min(ng, 6)
            groups = FF.expanded(co, m, k, ng)[:n]
            ys, proofs, commits = spec(hip, s, groups, w[:k * n].reshape(n, k), zs[:n])
            hy, hp, hc = hip.kzg_open_fold_flat(s, co[:k * n * m], k, w[:k * n], zs[:n], m=m, commits=True)
            assert hy.tolist() == ys and hp.tolist() == proofs and hc.tolist() == commits


# ------------------------------------------------------------------ 7. the SRS boundary
@pytest.mark.parametrize("n", [16, 40, 1040])
def test_srs_boundary(hip, srs_pts, n):
    pts = srs_pts[:n]
    k, ng = 3, 21
    with hip.Srs(pts) as s:
        zs = np.arange(ng) % 17
        w = weights_for(0xB0 + n, k * ng)
        co = coeffs(0xB0 + n, n * k * ng)                    # m == plk_srs_len, with commitments
        check(fold_dev(hip, s, co, n, k, ng, w, zs), FF.fold_flat_dev(co, n, k, ng, pts, w, zs), "at the bound")
        co = coeffs(0xB1 + n, (n + 1) * k * ng)              # m - 1 == plk_srs_len opens without commitments
        got = fold_dev(hip, s, co, n + 1, k, ng, w, zs, commits=False)
        check(got, FF.fold_flat_dev(co, n + 1, k, ng, pts, w, zs, want_commits=False), "one past")
        ys, proofs = hip.kzg_open_fold(s, FF.expanded(co, n + 1, k, ng), w.reshape(ng, k).tolist(), zs.tolist())
        assert got["ys"].tolist() == [y for g in ys for y in g] and got["proofs"].tolist() == [list(p) for p in proofs]
        hy, hp = hip.kzg_open_fold_flat(s, co, k, w, zs, m=n + 1)
        assert np.array_equal(hy, got["ys"]) and np.array_equal(hp, got["proofs"])
        small = coeffs(1, (n + 2) * k)
        for call in (lambda: fold_dev(hip, s, co, n + 1, k, ng, w, zs),                  # one past, commitments asked for
                     lambda: hip.kzg_open_fold_flat(s, co, k, w, zs, m=n + 1, commits=True),
                     lambda: fold_dev(hip, s, small, n + 2, k, 1, w[:k], [1], commits=False),
                     lambda: hip.kzg_open_fold_flat(s, small, k, w[:k], [1], m=n + 2)):
            with pytest.raises(hip.PlonkHipError) as err:
                call()
            assert err.value.code == hip.PLK_ERR_RANGE and "degree exceeds SRS size" in str(err.value)
        # the ragged form is bound by m as given, whatever the lengths are
        off = np.array([0, 3, 5, 6], np.uint32)
        with pytest.raises(hip.PlonkHipError) as err:
            fold_dev(hip, s, coeffs(2, 6), n + 2, k, 1, w[:k], [1], offsets=off, commits=False)
        assert err.value.code == hip.PLK_ERR_RANGE


# ------------------------------------------------------------------ 8. alignment and guard bytes
@pytest.mark.parametrize("m,ragged", [(32, False), (16, False), (1100, False), (32, True), (300, True), (2500, True)])
def test_alignment_and_guards(hip, srs, srs_pts, m, ragged):
    k = 3
    ng = 260 if m <= 32 else 11
    zs = np.arange(ng) % 17
    w = weights_for(0xA11 + m, k * ng)
    if ragged:
        lens = 1 + (gen.splitmix64(0xA119 + m, k * ng) % np.uint64(m)).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    else:
        off = None
    co = coeffs(0xA11 + m, int(off[-1]) if ragged else m * k * ng)
    exp = FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs, offsets=off)
    assert exp["status"].sum() == 0
    base = fold_dev(hip, srs, co, m, k, ng, w, zs, offsets=off, in_res=0, out_res=0)
    check(base, exp, "aligned")
    for res in (0, 1, 5, 15):
        got = fold_dev(hip, srs, co, m, k, ng, w, zs, offsets=off, in_res=res, out_res=(res + 4) % 16 if res else 0)
        for n in ("status", "ys", "proofs", "commits"):
            assert np.array_equal(got[n], base[n]), (res, n)
        got = fold_dev(hip, srs, co, m, k, ng, w, zs, offsets=off, in_res=(res + 8) % 16, out_res=res)
        for n in ("status", "ys", "proofs", "commits"):
            assert np.array_equal(got[n], base[n]), (res, n)


# ------------------------------------------------------------------ 9. repeatability and streams
@pytest.mark.parametrize("m", [24, 500, 2500])
def test_repeatability_and_streams(hip, srs, srs_pts, m):
    import torch
    k = 5
    ng = 700 if m <= 32 else 37
    co = coeffs(0x5712 + m, m * k * ng)
    w = weights_for(0x5712 + m, k * ng)
    zs = ((np.arange(ng) * 3) % 17).astype(np.uint8)
    exp = FF.fold_flat_dev(co, m, k, ng, srs_pts, w, zs)
    a = fold_dev(hip, srs, co, m, k, ng, w, zs)
    b = fold_dev(hip, srs, co, m, k, ng, w, zs)
    check(a, exp)
    for n in ("status", "ys", "proofs", "commits"):
        assert np.array_equal(a[n], b[n]), n
    # two calls in flight on two streams, distinct outputs
    d_co, d_w, d_zs = (torch.from_numpy(x).cuda() for x in (co, w, zs))
    outs = [[torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for n in (k * ng, 3 * ng, 3 * k * ng, ng)] for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for st, (ys, pr, cm, status) in zip(streams, outs):
        hip.kzg_open_fold_flat_dev(srs, d_co, co.size, None, m, k, ng, d_w, d_zs, ys, pr, cm, status, stream=st)
    for st in streams:
        st.synchronize()
    torch.cuda.synchronize()
    for ys, pr, cm, status in outs:
        assert np.array_equal(ys.cpu().numpy(), a["ys"]) and np.array_equal(status.cpu().numpy(), a["status"])
        assert np.array_equal(pr.cpu().numpy().reshape(-1, 3), a["proofs"])
        assert np.array_equal(cm.cpu().numpy().reshape(-1, 3), a["commits"])


# ------------------------------------------------------------------ 10. producer to verifier without the host
@pytest.mark.parametrize("m", [24, 100, 1500])
def test_openings_feed_the_fold_verifier_on_the_device(hip, m):
    import torch
    g = load_golden("pairing.json")
    vk = hip.KzgVk((1, 2, 0), bytes.fromhex(g["g2_multiples"]["1"]), bytes.fromhex(g["g2_multiples"]["2"]))
    pts = np.ascontiguousarray(FM.rule_srs(m))            # srs[i] = (2^i mod 17) G: s = 2
    k, ng = 9, 9
    co = coeffs(0xE2E + m, m * k * ng).copy()
    flagged = 4
    co[(k * flagged + 3) * m + m // 2] = 99               # one group with a byte >= 17
    zs = (np.arange(ng) % 14 + 3).astype(np.uint8)        # (never s = 2: there a changed weight goes unnoticed)
    assert 2 not in zs.tolist()
    w = (gen.splitmix64(0x9E2E + m, k * ng) % np.uint64(16)).astype(np.uint8) + np.uint8(1)   # non-zero: every y counts
    with hip.Srs(pts) as s:
        assert not s.irregular
        d_co, d_zs, d_w = (torch.from_numpy(np.ascontiguousarray(x, np.uint8)).cuda() for x in (co, zs, w))
        ys = torch.full((k * ng,), 0xEE, dtype=torch.uint8, device="cuda")
        cm = torch.full((3 * k * ng,), 0xEE, dtype=torch.uint8, device="cuda")
        pr = torch.full((3 * ng,), 0xEE, dtype=torch.uint8, device="cuda")
        status, ok = (torch.full((ng,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
        hip.kzg_open_fold_flat_dev(s, d_co, co.size, None, m, k, ng, d_w, d_zs, ys, pr, cm, status)

        def verdicts():
            hip.kzg_verify_fold_dev(vk, k, cm, d_w, ys, d_zs, pr, ng, ok)    # the five arrays as they stand
            torch.cuda.synchronize()
            return ok.cpu().numpy().tolist()

        exp = [1] * ng
        exp[flagged] = 2                                   # FF FF FF is answered with 2, never with an accept
        assert status.cpu().numpy().tolist() == [1 if i == flagged else 0 for i in range(ng)]
        assert verdicts() == exp
        for j in (0, 3 * k + 2, k * ng - 1):               # one y changed on the device
            ys[j] = (ys[j] + 1) % 17
            e = list(exp)
            e[j // k] = 0
            assert verdicts() == e, j
            ys[j] = (ys[j] + 16) % 17
        assert verdicts() == exp
        # one weight changed on the device: noticed wherever p_j(s) != p_j(z)
        polys = FM.expanded(co, m, k * ng)
        for grp in (0, 7):
            j = next(e for e in range(k * grp, k * grp + k) if F.poly_eval(polys[e], 2) != F.poly_eval(polys[e], int(zs[grp])))
            d_w[j] = d_w[j] % 16 + 1
            e = list(exp)
            e[grp] = 0
            assert verdicts() == e, j
            d_w[j] = int(w[j])
        assert verdicts() == exp


# ------------------------------------------------------------------ 11. linearity on the device
@pytest.mark.parametrize("m,k", [(20, 9), (300, 5), (2000, 3)])
def test_proof_is_the_weighted_fold_of_the_single_proofs(hip, m, k):
    """proofs == the repacked words of plk_msm_g1_segments_dev(proofs3 of plk_kzg_open_flat_dev over the expanded
    polynomials with z repeated, weights, m = k).  The identity needs an SRS inside the subgroup of order 17
    (kzg_flat_model.rule_srs): F's bytes are reduced mod 17, and sum_i w_i (q_ij P_j) = (sum_i w_i q_ij mod 17) P_j
    only where 17 P_j = 0 -- over all 102 elements the two sides differ by multiples of 17 P_j."""
    with hip.Srs(np.ascontiguousarray(FM.rule_srs(m))) as srs:
        assert not srs.irregular
        _linearity(hip, srs, m, k, 50)


def _linearity(hip, srs, m, k, ng):
    import torch
    co = coeffs(0x11E + m, m * k * ng)
    w = weights_for(0x11E + m, k * ng)
    zs = (np.arange(ng) % 17).astype(np.uint8)
    d_co, d_w, d_zs, d_zx = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (co, w, zs, np.repeat(zs, k)))

    def dirty(n):
        return torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")

    ys, pr, st = dirty(k * ng), dirty(3 * ng), dirty(ng)
    hip.kzg_open_fold_flat_dev(srs, d_co, co.size, None, m, k, ng, d_w, d_zs, ys, pr, None, st)
    ys1, pr1, st1, out4 = dirty(k * ng), dirty(3 * k * ng), dirty(k * ng), dirty(4 * ng)
    hip.kzg_open_flat_dev(srs, d_co, co.size, None, m, k * ng, d_zx, ys1, pr1, None, st1)
    ws = hip.msm_g1_segments_workspace(k * ng, k, ng, False)
    work = dirty(ws) if ws else None
    hip.msm_g1_segments_dev(pr1, d_w, k * ng, None, k, ng, out4, work=work)
    torch.cuda.synchronize()
    words = out4.cpu().numpy().reshape(ng, 4)
    assert st.cpu().numpy().sum() == 0 and st1.cpu().numpy().sum() == 0 and words[:, 3].sum() == 0
    assert np.array_equal(pr.cpu().numpy().reshape(ng, 3), words[:, :3])
    assert np.array_equal(ys.cpu().numpy(), ys1.cpu().numpy())


# ------------------------------------------------------------------ 12. errors with a live handle
def test_errors_with_a_live_handle(hip, srs):
    import torch
    co = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    A, R = hip.PLK_ERR_ARG, hip.PLK_ERR_RANGE
    for kw, code in ((dict(total=64, m=16, k=2, ng=0), A), (dict(total=64, m=16, k=0, ng=2), A), (dict(total=0, m=16, k=2, ng=2), A),
                     (dict(total=64, m=0, k=2, ng=2), A), (dict(total=63, m=16, k=2, ng=2), A), (dict(total=17 * 16, m=16, k=17, ng=1), A),
                     (dict(total=4097, m=4097, k=1, ng=1), R), (dict(total=1 << 32, m=4096, k=16, ng=1 << 16), R),
                     (dict(total=(1 << 30) + 16, m=1, k=16, ng=(1 << 26) + 1), R)):
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open_fold_flat_dev(srs, co, kw["total"], None, kw["m"], kw["k"], kw["ng"], out, out, out, out, None, out)
        assert err.value.code == code, kw
    for drop in range(6):                                   # coeffs, weights, zs, ys, proofs3, status
        a = [co, out, out, out, out, out]
        a[drop] = None
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open_fold_flat_dev(srs, a[0], 64, None, 16, 2, 2, a[1], a[2], a[3], a[4], None, a[5])
        assert err.value.code == A and "required" in str(err.value), drop
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.PlonkHipError) as err:
        hip.kzg_open_fold_flat_dev(srs, co, 64, off.data_ptr() + 2, 16, 2, 2, out, out, out, out, None, out)
    assert err.value.code == A and "4-byte aligned" in str(err.value)
