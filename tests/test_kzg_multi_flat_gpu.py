"""KZG flat multi-point openings (plk_kzg_open_multi_flat*) on the GPU.

Expected values come from tests/kzg_multi_flat_model.py (pinned to kzg_multi_model and through it to the
reference's recorded values by tests/test_kzg_multi_flat_cpu.py) and, for the first groups of every list, from the
library's own plk_kzg_open_multi_batch / plk_kzg_commit_batch on the expanded groups, which is the specification.
Everything is exact: bytes are compared for equality.  Every _dev output starts dirty (0xEE) with guard bytes on
both sides."""
import numpy as np
import pytest

import devbuf
import gen
import kzg_flat_model as FM
import kzg_multi_flat_model as MF
import kzg_multi_model as MM
from conftest import load_golden

pytestmark = pytest.mark.gpu

SRS_N = 4097
FLAG6 = [0xFF] * 6
IDENTITY = [0, 0, 1]
SPEC_GROUPS = 12          # groups per list also taken through plk_kzg_open_multi_batch / plk_kzg_commit_batch
PAIR = MM.mask_of([3, 6])                                    # {z, z omega} for z = 3, omega = 2
UNIFORM = [(1, 1), (1, 5), (2, 2), (15, 4), (16, 9), (17, 5), (32, 15), (32, 2), (33, 1), (33, 9), (48, 4), (1024, 15),
           (1024, 2), (1025, 5), (1025, 9), (4096, 15), (4096, 1)]
assert {m for m, _ in UNIFORM} == {1, 2, 15, 16, 17, 32, 33, 48, 1024, 1025, 4096}
assert {k for _, k in UNIFORM} == {1, 2, 4, 5, 9, 15} and {(32, 15), (1024, 15), (4096, 15)} <= set(UNIFORM)


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
    return (gen.splitmix64(0x3F17 + seed, n) % np.uint64(17)).astype(np.uint8)


def weights_for(seed, n):
    """values 0 .. 16, zeros among them"""
    w = (gen.splitmix64(0x3E16 + seed, n) % np.uint64(17)).astype(np.uint8)
    w[::7] = 0
    return w


def sets_for(seed, k, ng):
    """(ng, k) masks drawn per polynomial from {0}, one non-zero point, the PLONK pair, sixteen points and a random
    set; every third group only from the first three, so that its T leaves points outside"""
    r = np.random.default_rng(0x5E75 + seed)
    out = np.zeros((ng, k), np.uint32)
    for g in range(ng):
        for i in range(k):
            kind = (g + i) % (3 if g % 3 == 0 else 5)
            if kind == 0:
                out[g, i] = 1
            elif kind == 1:
                out[g, i] = 1 << int(r.integers(1, 17))
            elif kind == 2:
                out[g, i] = PAIR
            elif kind == 3:
                out[g, i] = MM.FULL & ~(1 << int(r.integers(0, 17)))
            else:
                out[g, i] = MM.mask_of(r.choice(17, int(r.integers(1, 17)), replace=False))
    return out


def ngroups_for(m):
    """not a multiple of the plan's groups per block, at least three blocks, every u = g mod 17 met"""
    per = MF.plan(m, 1, 1)["per_block"]
    n = {256: 2 * 256 + 37, 4: 4 * 8 + 3, 1: 19}[per]
    assert n >= 17 and -(-n // per) >= 3 and (per == 1 or n % per)
    return n


def multi_dev(hip, srs, co, m, k, ng, sets, w, us, offsets=None, commits=True, in_res=0, out_res=1, stream=None):
    """one _dev call over guarded buffers -> dict(status, ys, proofs, commits) of numpy arrays; the coefficient
    array starts in_res bytes past a 16-byte boundary, every output (and the weights and us) out_res bytes past one"""
    import torch
    co = np.ascontiguousarray(co, np.uint8)
    cb, cv = devbuf.place(co, in_res, poison="raw")
    wb, wv = devbuf.place(np.asarray(w, np.uint8), out_res, poison="raw")
    ub, uv = devbuf.place(np.asarray(us, np.uint8), out_res, poison="raw")
    d_sets = torch.from_numpy(np.ascontiguousarray(sets, np.uint32).reshape(-1).view(np.int32)).cuda()
    d_off = None if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, np.uint32).view(np.int32)).cuda()
    outs = {"status": devbuf.place_out(ng, out_res), "ys": devbuf.place_out(17 * k * ng, out_res),
            "proofs": devbuf.place_out(6 * ng, out_res)}
    if commits:
        outs["commits"] = devbuf.place_out(3 * k * ng, out_res)
    torch.cuda.synchronize()
    v = {n: b[1] for n, b in outs.items()}
    hip.kzg_open_multi_flat_dev(srs, cv, co.size, d_off, m, k, ng, d_sets, wv, uv, v["ys"], v["proofs"], v.get("commits"),
                                v["status"], stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    res = {"commits": None}
    shape = {"proofs": (-1, 6), "commits": (-1, 3), "ys": (-1, 17), "status": (-1,)}
    for n, (backing, view) in outs.items():
        assert devbuf.guards_intact(backing, view), "wrote outside " + n
        res[n] = view.cpu().numpy().copy().reshape(shape[n])
    return res


def check(got, exp, k, what=""):
    """every byte the header specifies"""
    assert got["status"].tolist() == exp["status"].tolist(), what
    for n in ("proofs", "commits"):
        assert (got[n] is None) == (exp[n] is None), (what, n)
        if exp[n] is not None:
            assert np.array_equal(got[n], exp[n]), (what, n, np.nonzero((got[n] != exp[n]).any(axis=1))[0][:8])
    e = np.repeat(exp["ys_exact"], k)
    assert np.array_equal(got["ys"][e], exp["ys"][e]), (what, "ys", np.nonzero((got["ys"] != exp["ys"]).any(axis=1))[0][:8])


def spec(hip, srs, groups, sets, weights, us):
    """the specification: plk_kzg_open_multi_batch / plk_kzg_commit_batch on the expanded groups ->
    (ys rows flat, proofs, commits flat)"""
    rows, proofs = hip.kzg_open_multi(srs, groups, [[int(v) for v in s] for s in sets], [[int(v) for v in w] for w in weights],
                                      [int(u) for u in us])
    commits = hip.kzg_commit(srs, [p for g in groups for p in g])
    return [list(r) for g in rows for r in g], [list(p) for p in proofs], [list(c) for c in commits]


def check_spec(hip, srs, got, groups, sets, w, us, k, idx, commits=True):
    sets, w = np.asarray(sets).reshape(-1, k), np.asarray(w).reshape(-1, k)
    ys, proofs, cm = spec(hip, srs, [groups[g] for g in idx], [sets[g] for g in idx], [w[g] for g in idx], [us[g] for g in idx])
    e = [k * g + i for g in idx for i in range(k)]
    assert got["ys"][e].tolist() == ys
    assert got["proofs"][idx].tolist() == proofs
    if commits:
        assert got["commits"][e].tolist() == cm


def check_host(hip, srs, exp, co, k, sets, w, us, offsets=None, m=None):
    ys, proofs, commits = hip.kzg_open_multi_flat(srs, co, k, sets, w, us, offsets=offsets, m=m, commits=True)
    assert np.array_equal(ys, exp["ys"]) and np.array_equal(proofs, exp["proofs"]) and np.array_equal(commits, exp["commits"])
    ys, proofs = hip.kzg_open_multi_flat(srs, co, k, sets, w, us, offsets=offsets, m=m)
    assert np.array_equal(ys, exp["ys"]) and np.array_equal(proofs, exp["proofs"])


def tiled(distinct, ng):
    """(index of the distinct group each of the ng groups repeats)"""
    return np.arange(ng) % distinct


# ------------------------------------------------------------------ 1. uniform lengths, every path
@pytest.mark.parametrize("m,k", UNIFORM)
def test_uniform(hip, srs, srs_pts, m, k):
    ng = ngroups_for(m)
    plan = hip.kzg_multi_flat_plan(m, k, ng)
    assert plan == MF.plan(m, k, ng) and plan["blocks"] >= 3 and plan["launches"] == 1
    assert plan["path"] == (0 if m <= 32 else 1 if m <= 1024 else 2)
    # 34 distinct groups (two turns of u = 0 .. 16 under different sets), repeated where the path wants many groups
    d = min(ng, 34)
    t = tiled(d, ng)
    co = coeffs(100 * m + k, m * k * d).reshape(d, m * k)[t].reshape(-1)
    w = weights_for(100 * m + k, k * d).reshape(d, k)[t].reshape(-1)
    sets = sets_for(100 * m + k, k, d)[t]
    us = (np.arange(d) % 17)[t]
    T = np.bitwise_or.reduce(sets[:d], axis=1)
    inside = ((T >> us[:d].astype(np.uint32)) & 1).astype(bool)
    assert (us[:d] == 0).any() and inside.any() and (~inside).any()
    exp = MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us)
    assert exp["status"].sum() == 0
    got = multi_dev(hip, srs, co, m, k, ng, sets, w, us, in_res=0, out_res=0)
    check(got, exp, k, "open")
    check_spec(hip, srs, got, MF.expanded(co, m, k, ng), sets, w, us, k, list(range(min(SPEC_GROUPS, ng))))
    # without commitments
    check(multi_dev(hip, srs, co, m, k, ng, sets, w, us, commits=False),
          MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us, want_commits=False), k, "no commits")
    check_host(hip, srs, exp, co, k, sets, w, us, m=m)


# ------------------------------------------------------------------ 2. degenerate groups
def degenerate_list(m, u):
    """groups of two: plain; every len_i <= |S_i|; all weights zero; the cancelling pair (p, p under w and 17 - w on
    one set); T = all 17 points with both sets smaller; both sets {z}; h cancelling only its top; plain"""
    p = coeffs(0xDE6 + m, m)
    p[-1] = 5
    top = p.copy()
    top[:m // 3 + 1] = coeffs(0xDE7 + m, m // 3 + 1)          # equal above m // 3: the difference has degree m // 3
    top[m // 3] = (int(p[m // 3]) + 1) % 17
    lo, hi = MM.mask_of(range(0, 9)), MM.mask_of(range(8, 17))
    groups = [[coeffs(1 + m, m), coeffs(2 + m, max(m // 2, 1))], [coeffs(3 + m, 2), coeffs(4 + m, 5)], [p, coeffs(5 + m, m - 1)],
              [p, p], [coeffs(6 + m, m), coeffs(7 + m, max(m - 3, 1))], [coeffs(8 + m, m), coeffs(9 + m, max(m // 2, 1))], [p, top],
              [coeffs(10 + m, 17), coeffs(11 + m, m)]]
    sets = np.array([[PAIR, 1 << 5], [0b110, MM.mask_of([0, 2, 7, 9, 16])], [PAIR, 1], [0b10110, 0b10110], [lo, hi],
                     [1 << 6, 1 << 6], [1 << 4, 1 << 4], [MM.FULL & ~2, 1]], np.uint32)
    weights = np.array([3, 4, 5, 6, 0, 0, 5, 12, 2, 9, 3, 4, 1, 16, 16, 1], np.uint8)
    polys = [q for g in groups for q in g]
    off = np.concatenate([[0], np.cumsum([len(q) for q in polys])]).astype(np.uint32)
    return groups, np.concatenate(polys), off, sets, weights, np.full(len(groups), u, np.uint8)


@pytest.mark.parametrize("m", [32, 1024, 4096])
def test_degenerate_groups(hip, srs, srs_pts, m):
    for u in (0, 6, 11):
        groups, co, off, sets, w, us = degenerate_list(m, u)
        ng = len(groups)
        exp = MF.multi_flat_dev(co, m, 2, ng, srs_pts, sets, w, us, offsets=off)
        assert exp["status"].sum() == 0
        assert exp["proofs"][[1, 2, 3], :3].tolist() == [IDENTITY] * 3        # h = 0: the identity
        got = multi_dev(hip, srs, co, m, 2, ng, sets, w, us, offsets=off)
        check(got, exp, 2, ("degenerate", u))
        check_spec(hip, srs, got, groups, sets, w, us, 2, list(range(ng)))
        check_host(hip, srs, exp, co, 2, sets, w, us, offsets=off, m=m)
        # every set {z}: W is the folded proof of (p_0, p_1) at z under w, W' that of (p_0, p_1, h) at u under c
        g, z = 5, 6
        ys, pr = hip.kzg_open_fold_flat(srs, np.concatenate(groups[g]), 2, w[2 * g:2 * g + 2], [z],
                                        offsets=[0, len(groups[g][0]), len(groups[g][0]) + len(groups[g][1])], m=m)
        assert got["proofs"][g, :3].tolist() == pr[0].tolist()
        assert got["ys"][[2 * g, 2 * g + 1], z].tolist() == ys.tolist()
        h = MM.h_of(groups[g], sets[g], w[2 * g:2 * g + 2])
        three = groups[g] + [h]
        off3 = np.concatenate([[0], np.cumsum([len(q) for q in three])]).astype(np.uint32)
        c = hip.kzg_multi_coeffs([int(v) for v in sets[g]], w[2 * g:2 * g + 2], u)
        _, pr = hip.kzg_open_fold_flat(srs, np.concatenate(three), 3, c, [u], offsets=off3, m=m)
        assert got["proofs"][g, 3:].tolist() == pr[0].tolist()


def test_length_one(hip, srs, srs_pts):
    """m = 1: every quotient is {0}, both proofs the identity, every value the constant"""
    k, ng = 3, 40
    co = np.arange(k * ng, dtype=np.uint8) % 17
    w = weights_for(1, k * ng)
    sets = sets_for(1, k, ng)
    got = multi_dev(hip, srs, co, 1, k, ng, sets, w, np.arange(ng) % 17)
    assert got["status"].sum() == 0 and got["proofs"].tolist() == [IDENTITY * 2] * ng
    on = ((sets.reshape(-1, 1) >> np.arange(17, dtype=np.uint32)) & 1).astype(bool)
    assert np.array_equal(got["ys"], np.where(on, co[:, None], 0xFF))
    assert got["commits"].tolist() == FM.commit_rows(co.reshape(-1, 1), FM.srs_logs(srs_pts)).tolist()
    check_host(hip, srs, got, co, k, sets, w, np.arange(ng) % 17, m=1)


# ------------------------------------------------------------------ 3. the grid-stride loop
@pytest.mark.parametrize("m,k", [(1, 2), (33, 2), (1025, 2)])
def test_grid_stride(hip, srs, srs_pts, m, k):
    """ngroups just above groups per block x blocks: the last groups are a block's second turn.  Expected values
    from 17 distinct groups, tiled."""
    per = MF.plan(m, k, 1)["per_block"]
    ng = per * 2048 + 1 + per // 2
    plan = hip.kzg_multi_flat_plan(m, k, ng)
    assert plan["blocks"] == 2048 and plan["per_block"] * plan["blocks"] < ng
    d = 17
    t = tiled(d, ng)
    co = coeffs(0x651D + m, m * k * d).reshape(d, -1)
    w = weights_for(0x651D + m, k * d).reshape(d, k)
    sets = sets_for(0x651D + m, k, d)
    us = (np.arange(d) * 7 + 3) % 17
    e = MF.multi_flat_dev(co.reshape(-1), m, k, d, srs_pts, sets, w, us)
    assert e["status"].sum() == 0
    got = multi_dev(hip, srs, co[t].reshape(-1), m, k, ng, sets[t], w[t].reshape(-1), us[t])
    assert got["status"].sum() == 0
    assert np.array_equal(got["proofs"], e["proofs"][t])
    assert np.array_equal(got["ys"].reshape(ng, k, 17), e["ys"].reshape(d, k, 17)[t])
    assert np.array_equal(got["commits"].reshape(ng, k, 3), e["commits"].reshape(d, k, 3)[t])


# ------------------------------------------------------------------ 4. ragged lists
RAGGED_K = 3
RAGGED_BAD = [2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22]


def ragged_list(m, seed):
    """(coeffs, offsets, sets, weights, us): 25 groups of three, lengths 1 .. m mixed inside the groups, o_0 = 5 and
    unused bytes behind the last polynomial; one group each with an empty polynomial, a falling offset, an offset
    above total, an offset of 0xFFFFFFFF, a polynomial of m + 1 coefficients, u = 17, a weight of 17, a weight of
    255, mask 0, a mask with bit 17 and the full mask, every one between valid neighbours"""
    k, ng = RAGGED_K, 25
    r = gen.splitmix64(0x4A66 + seed, k * ng)
    lens = [1 + int(v % np.uint64(m)) for v in r]
    lens[:9] = [1, m, 2, max(m - 1, 1), min(16, m), min(17, m), min(15, m), m, m]
    lens[k * 2 + 1] = 0                                  # group 2: an empty polynomial
    lens[k * 10 + 2] = m + 1                             # group 10: one coefficient too long
    off = 5 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(off[-1]) + 9
    off[k * 4 + 1] = off[k * 4] - 1                      # group 4: its first polynomial falls
    off[k * 6 + 1] = total + 5                           # group 6: an offset above total (and the next polynomial falls)
    off[k * 8 + 2] = 0xFFFFFFFF                          # group 8
    us = (np.arange(ng) * 5 + 1) % 17
    us[12] = 17
    w = weights_for(0x4A67 + seed, k * ng)
    w[k * 14], w[k * 16 + 2] = 17, 255
    sets = sets_for(0x4A69 + seed, k, ng)
    sets[18, 1], sets[20, 2], sets[22, 0] = 0, PAIR | 1 << 17, MM.FULL
    return coeffs(0x4A68 + seed, total), off.astype(np.uint32), sets, w, us.astype(np.uint8)


@pytest.mark.parametrize("m", [32, 1024, 4096])
def test_ragged(hip, srs, srs_pts, m):
    k, bad = RAGGED_K, RAGGED_BAD
    co, off, sets, w, us = ragged_list(m, m)
    ng = us.size
    exp = MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us, offsets=off)
    assert np.nonzero(exp["status"])[0].tolist() == bad and (exp["status"][bad] == MF.BAD).all()
    got = multi_dev(hip, srs, co, m, k, ng, sets, w, us, offsets=off)
    check(got, exp, k, "ragged")
    assert got["proofs"][bad].tolist() == [FLAG6] * len(bad)
    assert (got["ys"].reshape(ng, -1)[bad] == 0xFF).all() and (got["commits"].reshape(ng, k, 3)[bad] == 0xFF).all()
    check(multi_dev(hip, srs, co, m, k, ng, sets, w, us, offsets=off, commits=False),
          MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us, offsets=off, want_commits=False), k, "ragged, no commits")
    # the neighbours against the specification
    good = [g for g in range(ng) if g not in bad]
    groups = {g: [co[int(off[e]):int(off[e + 1])] for e in range(k * g, k * (g + 1))] for g in good}
    assert {1, m} <= {len(p) for g in good for p in groups[g]}
    check_spec(hip, srs, got, groups, sets, w, us, k, good)
    # the host form refuses the list, and takes its valid part
    with pytest.raises(hip.PlonkHipError) as err:
        hip.kzg_open_multi_flat(srs, co, k, sets, w, us, offsets=off, m=m)
    assert err.value.code == hip.PLK_ERR_ARG
    polys = [p for g in good for p in groups[g]]
    goff = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.uint32)
    e = [k * g + i for g in good for i in range(k)]
    hy, hp, hc = hip.kzg_open_multi_flat(srs, np.concatenate(polys), k, sets[good], w[e], us[good], offsets=goff, m=m, commits=True)
    assert np.array_equal(hy, got["ys"][e]) and np.array_equal(hp, got["proofs"][good]) and np.array_equal(hc, got["commits"][e])


@pytest.mark.parametrize("m", [32, 100, 2000])
def test_device_byte_bad_causes_uniform(hip, srs, srs_pts, m):
    """mask 0, a mask with bit 17, the full mask, weight 17, u 200: each in a group between two good neighbours"""
    k, ng = 2, 11
    co = coeffs(0xBADB + m, m * k * ng)
    sets = sets_for(0xBADB + m, k, ng)
    w = weights_for(0xBADB + m, k * ng)
    us = (np.arange(ng) % 17).astype(np.uint8)
    sets[1, 0], sets[3, 1], sets[5, 0] = 0, 1 << 17 | 1, MM.FULL
    w[k * 7 + 1] = 17
    us[9] = 200
    bad = [1, 3, 5, 7, 9]
    exp = MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us)
    assert np.nonzero(exp["status"])[0].tolist() == bad and (exp["status"][bad] == MF.BAD).all()
    got = multi_dev(hip, srs, co, m, k, ng, sets, w, us)
    check(got, exp, k, "device bytes")
    assert got["proofs"][bad].tolist() == [FLAG6] * 5 and (got["ys"].reshape(ng, -1)[bad] == 0xFF).all()
    assert (got["commits"].reshape(ng, k, 3)[bad] == 0xFF).all()
    good = [g for g in range(ng) if g not in bad]
    check_spec(hip, srs, got, MF.expanded(co, m, k, ng), sets, w, us, k, good)
    with pytest.raises(hip.PlonkHipError) as err:
        hip.kzg_open_multi_flat(srs, co, k, sets, w, us, m=m)
    assert err.value.code == hip.PLK_ERR_ARG


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
    sets = sets_for(0xBAD + m, k, ng)
    us = np.arange(ng) % 17
    exp = MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us)
    assert np.nonzero(exp["status"])[0].tolist() == flagged and (exp["status"][flagged] == MF.IRREGULAR).all()
    got = multi_dev(hip, srs, co, m, k, ng, sets, w, us)
    check(got, exp, k, "non-canonical")
    assert got["proofs"][flagged].tolist() == [FLAG6] * len(flagged)
    groups = MF.expanded(co, m, k, ng)
    ys, proofs, commits = spec(hip, srs, groups, sets, w.reshape(ng, k), us)      # (exact for every byte: the host calls)
    assert got["commits"].tolist() == commits
    good = [g for g in range(ng) if g not in flagged]
    e = [k * g + i for g in good for i in range(k)]
    assert got["ys"][e].tolist() == [ys[j] for j in e] and got["proofs"][good].tolist() == [proofs[g] for g in good]
    # the host form is exact for every byte
    hy, hp, hc = hip.kzg_open_multi_flat(srs, co, k, sets, w, us, m=m, commits=True)
    assert hy.tolist() == ys and hp.tolist() == proofs and hc.tolist() == commits


# ------------------------------------------------------------------ 6. an SRS without log form
def test_irregular_srs(hip, srs_pts):
    pts = srs_pts[:2100].copy()
    pts[7] = (3, 3, 0)                                 # off-curve
    with hip.Srs(pts) as s:
        assert s.irregular
        for m, k, ng in ((20, 3, 300), (100, 5, 9), (2000, 2, 5)):
            d = min(ng, 20)
            t = tiled(d, ng)
            co = coeffs(0x1229 + m, m * k * d).reshape(d, -1)[t].reshape(-1)
            w = weights_for(0x1229 + m, k * d).reshape(d, k)[t].reshape(-1)
            sets = sets_for(0x1229 + m, k, d)[t]
            us = (np.arange(d) % 17)[t]
            exp = MF.multi_flat_dev(co, m, k, ng, pts, sets, w, us)
            assert (exp["status"] == MF.IRREGULAR).all() and exp["ys_exact"].all()
            got = multi_dev(hip, s, co, m, k, ng, sets, w, us)
            check(got, exp, k, m)
            assert (got["proofs"] == 0xFF).all() and (got["commits"] == 0xFF).all()
            assert np.array_equal(got["ys"], MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us)["ys"])   # exact whatever the SRS
            # the host form: exact through plk_kzg_open_multi_batch / plk_kzg_commit_batch
            n = min(ng, 6)
            groups = MF.expanded(co, m, k, ng)[:n]
            ys, proofs, commits = spec(hip, s, groups, sets[:n], w[:k * n].reshape(n, k), us[:n])
            hy, hp, hc = hip.kzg_open_multi_flat(s, co[:k * n * m], k, sets[:n], w[:k * n], us[:n], m=m, commits=True)
            assert hy.tolist() == ys and hp.tolist() == proofs and hc.tolist() == commits


# ------------------------------------------------------------------ 7. the SRS boundary
@pytest.mark.parametrize("n", [16, 40, 1040])
def test_srs_boundary(hip, srs_pts, n):
    pts = srs_pts[:n]
    k, ng = 3, 21
    with hip.Srs(pts) as s:
        us = np.arange(ng) % 17
        w = weights_for(0xB0 + n, k * ng)
        sets = sets_for(0xB0 + n, k, ng)
        co = coeffs(0xB0 + n, n * k * ng)                    # m == plk_srs_len, with commitments
        check(multi_dev(hip, s, co, n, k, ng, sets, w, us), MF.multi_flat_dev(co, n, k, ng, pts, sets, w, us), k, "at the bound")
        co = coeffs(0xB1 + n, (n + 1) * k * ng)              # max(m - 1, 1) == plk_srs_len opens without commitments
        got = multi_dev(hip, s, co, n + 1, k, ng, sets, w, us, commits=False)
        check(got, MF.multi_flat_dev(co, n + 1, k, ng, pts, sets, w, us, want_commits=False), k, "one past")
        rows, proofs = hip.kzg_open_multi(s, MF.expanded(co, n + 1, k, ng), sets.tolist(), w.reshape(ng, k).tolist(), us.tolist())
        assert got["ys"].tolist() == [list(r) for g in rows for r in g] and got["proofs"].tolist() == [list(p) for p in proofs]
        hy, hp = hip.kzg_open_multi_flat(s, co, k, sets, w, us, m=n + 1)
        assert np.array_equal(hy, got["ys"]) and np.array_equal(hp, got["proofs"])
        small = coeffs(1, (n + 2) * k)
        for call in (lambda: multi_dev(hip, s, co, n + 1, k, ng, sets, w, us),            # one past, commitments asked for
                     lambda: hip.kzg_open_multi_flat(s, co, k, sets, w, us, m=n + 1, commits=True),
                     lambda: multi_dev(hip, s, small, n + 2, k, 1, sets[:1], w[:k], [1], commits=False),   # one point fewer
                     lambda: hip.kzg_open_multi_flat(s, small, k, sets[:1], w[:k], [1], m=n + 2)):
            with pytest.raises(hip.PlonkHipError) as err:
                call()
            assert err.value.code == hip.PLK_ERR_RANGE and "degree exceeds SRS size" in str(err.value)
        # the ragged form is bound by m as given, whatever the lengths are
        off = np.array([0, 3, 5, 6], np.uint32)
        with pytest.raises(hip.PlonkHipError) as err:
            multi_dev(hip, s, coeffs(2, 6), n + 2, k, 1, sets[:1], w[:k], [1], offsets=off, commits=False)
        assert err.value.code == hip.PLK_ERR_RANGE


# ------------------------------------------------------------------ 8. alignment and guard bytes
@pytest.mark.parametrize("m,ragged", [(32, False), (16, False), (1100, False), (32, True), (300, True), (2500, True)])
def test_alignment_and_guards(hip, srs, srs_pts, m, ragged):
    k = 3
    ng = 260 if m <= 32 else 11
    us = np.arange(ng) % 17
    w = weights_for(0xA11 + m, k * ng)
    sets = sets_for(0xA11 + m, k, ng)
    if ragged:
        lens = 1 + (gen.splitmix64(0xA119 + m, k * ng) % np.uint64(m)).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    else:
        off = None
    co = coeffs(0xA11 + m, int(off[-1]) if ragged else m * k * ng)
    exp = MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us, offsets=off)
    assert exp["status"].sum() == 0
    base = multi_dev(hip, srs, co, m, k, ng, sets, w, us, offsets=off, in_res=0, out_res=0)
    check(base, exp, k, "aligned")
    for res in (1, 7, 15):
        got = multi_dev(hip, srs, co, m, k, ng, sets, w, us, offsets=off, in_res=res, out_res=(res + 4) % 16)
        for n in ("status", "ys", "proofs", "commits"):
            assert np.array_equal(got[n], base[n]), (res, n)
        got = multi_dev(hip, srs, co, m, k, ng, sets, w, us, offsets=off, in_res=(res + 8) % 16, out_res=res)
        for n in ("status", "ys", "proofs", "commits"):
            assert np.array_equal(got[n], base[n]), (res, n)


# ------------------------------------------------------------------ 9. repeatability and streams
@pytest.mark.parametrize("m", [24, 500, 2500])
def test_repeatability_and_streams(hip, srs, srs_pts, m):
    import torch
    k = 5
    ng = 700 if m <= 32 else 37
    d = min(ng, 37)
    t = tiled(d, ng)
    co = coeffs(0x5712 + m, m * k * d).reshape(d, -1)[t].reshape(-1)
    w = weights_for(0x5712 + m, k * d).reshape(d, k)[t].reshape(-1)
    sets = np.ascontiguousarray(sets_for(0x5712 + m, k, d)[t])
    us = ((np.arange(d) * 3) % 17).astype(np.uint8)[t]
    exp = MF.multi_flat_dev(co, m, k, ng, srs_pts, sets, w, us)
    a = multi_dev(hip, srs, co, m, k, ng, sets, w, us)
    b = multi_dev(hip, srs, co, m, k, ng, sets, w, us, stream=torch.cuda.Stream())
    check(a, exp, k)
    for n in ("status", "ys", "proofs", "commits"):
        assert np.array_equal(a[n], b[n]), n
    # two calls in flight on two streams, distinct outputs
    d_co, d_w, d_us = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (co, w, us))
    d_sets = torch.from_numpy(sets.reshape(-1).view(np.int32)).cuda()
    outs = [[torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for n in (17 * k * ng, 6 * ng, 3 * k * ng, ng)] for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for st, (ys, pr, cm, status) in zip(streams, outs):
        hip.kzg_open_multi_flat_dev(srs, d_co, co.size, None, m, k, ng, d_sets, d_w, d_us, ys, pr, cm, status, stream=st)
    for st in streams:
        st.synchronize()
    torch.cuda.synchronize()
    for ys, pr, cm, status in outs:
        assert np.array_equal(ys.cpu().numpy().reshape(-1, 17), a["ys"]) and np.array_equal(status.cpu().numpy(), a["status"])
        assert np.array_equal(pr.cpu().numpy().reshape(-1, 6), a["proofs"])
        assert np.array_equal(cm.cpu().numpy().reshape(-1, 3), a["commits"])


# ------------------------------------------------------------------ 10. producer to verifier without the host
@pytest.mark.parametrize("m", [24, 100, 1500])
def test_openings_feed_the_multi_verifier_on_the_device(hip, m):
    import torch
    g = load_golden("pairing.json")
    vk = hip.KzgVk((1, 2, 0), bytes.fromhex(g["g2_multiples"]["1"]), bytes.fromhex(g["g2_multiples"]["2"]))
    pts = np.ascontiguousarray(FM.rule_srs(m))            # srs[i] = (2^i mod 17) G: s = 2
    k, ng = 9, 9
    co = coeffs(0xE2E + m, m * k * ng).copy()
    flagged = 4
    co[(k * flagged + 3) * m + m // 2] = 99               # one group with a byte >= 17
    # PLONK's shape: eight polynomials at {z}, one at {z, z omega}; u outside T, weights non-zero: every value counts
    zs = [3, 5, 6, 7, 10, 11, 12, 14, 1]
    sets = np.array([[1 << z] * 8 + [1 << z | 1 << (2 * z % 17)] for z in zs], np.uint32)
    us = np.array([next(u for u in list(range(4 + i, 17)) + list(range(4, 4 + i)) if not (sets[i, 8] >> u) & 1)
                   for i in range(ng)], np.uint8)
    w = (gen.splitmix64(0x9E2E + m, k * ng) % np.uint64(16)).astype(np.uint8) + np.uint8(1)
    with hip.Srs(pts) as s:
        assert not s.irregular
        d_co, d_us, d_w = (torch.from_numpy(np.ascontiguousarray(x, np.uint8)).cuda() for x in (co, us, w))
        d_sets = torch.from_numpy(sets.reshape(-1).view(np.int32)).cuda()
        ys = torch.full((17 * k * ng,), 0xEE, dtype=torch.uint8, device="cuda")
        cm = torch.full((3 * k * ng,), 0xEE, dtype=torch.uint8, device="cuda")
        pr = torch.full((6 * ng,), 0xEE, dtype=torch.uint8, device="cuda")
        status, ok = (torch.full((ng,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
        hip.kzg_open_multi_flat_dev(s, d_co, co.size, None, m, k, ng, d_sets, d_w, d_us, ys, pr, cm, status)

        def verdicts():
            hip.kzg_verify_multi_dev(vk, k, cm, d_sets, d_w, ys, d_us, pr, ng, ok)    # the six arrays as they stand
            torch.cuda.synchronize()
            return ok.cpu().numpy().tolist()

        exp = [1] * ng
        exp[flagged] = 2                                   # FF FF FF is answered with 2, never with an accept
        assert status.cpu().numpy().tolist() == [1 if i == flagged else 0 for i in range(ng)]
        assert verdicts() == exp
        # one value at a point of a set changed on the device: the first polynomial of group 0 at z, the pair's
        # second point in group 3, the last polynomial of the last group
        for e, a in ((0, zs[0]), (3 * k + 8, 2 * zs[3] % 17), (k * ng - 1, zs[8])):
            j = 17 * e + a
            assert int(ys[j]) < 17
            ys[j] = (ys[j] + 1) % 17
            want = list(exp)
            want[e // k] = 0
            assert verdicts() == want, (e, a)
            ys[j] = (ys[j] + 16) % 17
        assert verdicts() == exp


# ------------------------------------------------------------------ 11. the reference's recorded groups
def test_golden_groups_through_the_flat_forms(hip):
    import make_kzg_multi_golden as mk
    raw = load_golden("kzg_multi.json")
    pts = np.array(list(bytes.fromhex(raw["srs"])), np.uint8).reshape(-1, 3)
    opened, _, _ = mk.expand(raw)
    by_k = {}
    for g in opened:
        if max(len(p) for p in g["polys"]) <= FM.FLAT_MAX:
            by_k.setdefault(len(g["polys"]), []).append(g)
    assert sum(len(v) for v in by_k.values()) >= 1
    with hip.Srs(pts) as s:
        for k, gs in sorted(by_k.items()):
            polys = [np.array(p, np.uint8) for g in gs for p in g["polys"]]
            off = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.uint32)
            co = np.concatenate(polys)
            m = max(len(p) for p in polys)
            sets = np.array([g["sets"] for g in gs], np.uint32)
            w = np.array([g["weights"] for g in gs], np.uint8).reshape(-1)
            us = np.array([g["u"] for g in gs], np.uint8)
            got = multi_dev(hip, s, co, m, k, len(gs), sets, w, us, offsets=off)
            hy, hp = hip.kzg_open_multi_flat(s, co, k, sets, w, us, offsets=off, m=m)
            assert got["status"].sum() == 0 and np.array_equal(hy, got["ys"]) and np.array_equal(hp, got["proofs"])
            for i, g in enumerate(gs):
                assert got["proofs"][i].tolist() == list(g["W"]) + list(g["Wp"]), (k, i)
                h = MM.F.trim(MM.h_of(g["polys"], g["sets"], g["weights"])).tolist()
                assert mk.digest(got["ys"][k * i:k * (i + 1)].tobytes(), h) == g["digest"], (k, i)


# ------------------------------------------------------------------ 12. errors with a live handle
def test_errors_with_a_live_handle(hip, srs):
    import torch
    co = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(128, dtype=torch.uint8, device="cuda")
    sets = torch.full((8,), 2, dtype=torch.int32, device="cuda")
    A, R = hip.PLK_ERR_ARG, hip.PLK_ERR_RANGE
    for kw, code in ((dict(total=64, m=16, k=2, ng=0), A), (dict(total=64, m=16, k=0, ng=2), A), (dict(total=0, m=16, k=2, ng=2), A),
                     (dict(total=64, m=0, k=2, ng=2), A), (dict(total=63, m=16, k=2, ng=2), A), (dict(total=16 * 16, m=16, k=16, ng=1), A),
                     (dict(total=4097, m=4097, k=1, ng=1), R), (dict(total=1 << 32, m=4096, k=8, ng=1 << 17), R),
                     (dict(total=(1 << 30) + 8, m=1, k=8, ng=(1 << 27) + 1), R)):
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open_multi_flat_dev(srs, co, kw["total"], None, kw["m"], kw["k"], kw["ng"], sets, out, out, out, out, None, out)
        assert err.value.code == code, kw
    for drop in range(7):                                   # coeffs, sets, weights, us, ys, proofs6, status
        a = [co, sets, out, out, out, out, out]
        a[drop] = None
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open_multi_flat_dev(srs, a[0], 64, None, 16, 2, 2, a[1], a[2], a[3], a[4], a[5], None, a[6])
        assert err.value.code == A and "required" in str(err.value), drop
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    for o, st in ((off.data_ptr() + 2, sets), (None, sets.data_ptr() + 2)):
        with pytest.raises(hip.PlonkHipError) as err:
            hip.kzg_open_multi_flat_dev(srs, co, 64, o, 16, 2, 2, st, out, out, out, out, None, out)
        assert err.value.code == A and "4-byte aligned" in str(err.value)
    if torch.cuda.device_count() > 1:                       # a call from another device
        with torch.cuda.device(1):
            with pytest.raises(hip.PlonkHipError) as err:
                hip.kzg_open_multi_flat_dev(srs, co, 64, None, 16, 2, 2, sets, out, out, out, out, None, out)
        assert err.value.code == A
