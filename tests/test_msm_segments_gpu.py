"""Segmented MSM (plk_msm_g1_segments*) on the GPU.

Expected values are the reference's bytes recorded in tests/golden/msm_segments.json and the Python model of
tests/msm_segments_model.py (pinned to that file by tests/test_msm_segments_cpu.py); where an input holds a flag
byte the reference's bool cannot take, the host form is compared with plk_msm_g1 on the same segment, which is what
the header promises.  Everything is exact: bytes are compared for equality.  Sizes come from the plan (T = the
points of one block tile), so a changed tile still meets its edges."""
import numpy as np
import pytest

import devbuf
import g1_encoding_cases as E
import gen
import make_msm_segments_golden as mk
import msm_segments_model as S
from conftest import load_golden

pytestmark = pytest.mark.gpu

LANE, PREFIX = 0, 1
FFI = (0xFF, 0xFF, 0xFF, S.IRREGULAR)


# ------------------------------------------------------------------ inputs, shared and never modified
class Pool:
    """seeded canonical points over all 102 group elements with scalar bytes over 0..255; every test takes a slice (copies)"""

    def __init__(self, n=1 << 16):
        self.pts, self.sc = E.fillers(E.rng_for("msm_segments/pool"), n)
        assert {tuple(p) for p in self.pts[:4096].tolist()} == {tuple(p) for p in gen.all_points().tolist()}
        assert len(set(self.sc[:4096].tolist())) == 256

    def take(self, n, start=0):
        assert start + n <= self.sc.size
        return self.pts[start:start + n].copy(), self.sc[start:start + n].copy()


@pytest.fixture(scope="module")
def pool():
    return Pool()


@pytest.fixture(scope="module")
def T(hip):
    t = hip.msm_g1_segments_plan(1 << 20, 0, 1, 1)["tile"]
    assert t % 16 == 0 and 3 * t + 37 <= 1 << 16
    return t


def dev_offsets(off):
    import torch
    return torch.from_numpy(np.asarray(off, np.int64).astype(np.uint32).view(np.int32).copy()).cuda()


def work_for(hip, total, m, nseg, ragged):
    import torch
    ws = hip.msm_g1_segments_workspace(total, m, nseg, ragged)
    assert (ws == 0) == (hip.msm_g1_segments_plan(total, m, nseg, ragged)["launches"] == 1)
    return torch.full((ws,), 0xEE, dtype=torch.uint8, device="cuda") if ws else None


def seg_dev(hip, pts, sc, offsets=None, m=None, rp=0, rs=0, ro=0, guard=devbuf.GUARD, work=None, stream=None):
    """(nseg, 4) bytes of one _dev call: points and scalars at residues rp, rs mod 16 inside raw poison, out at residue
    ro with 0xEE guards checked afterwards, the workspace full of 0xEE unless one is passed"""
    import torch
    pts, sc = np.ascontiguousarray(pts, np.uint8).reshape(-1, 3), np.ascontiguousarray(sc, np.uint8).reshape(-1)
    total = sc.size
    ragged = offsets is not None
    nseg = len(offsets) - 1 if ragged else total // m
    _, dp = devbuf.place(pts, rp, guard=3 * guard, poison="raw")
    _, ds = devbuf.place(sc, rs, guard=guard, poison="raw")
    bo, do = devbuf.place_out(4 * nseg, ro)
    dof = dev_offsets(offsets) if ragged else None
    if work is None:
        work = work_for(hip, total, 0 if ragged else m, nseg, ragged)
    torch.cuda.synchronize()
    hip.msm_g1_segments_dev(dp, ds, total, dof, 0 if ragged else m, nseg, do, work=work, stream=stream)
    torch.cuda.synchronize()
    assert devbuf.guards_intact(bo, do), "wrote outside the 4 nseg output bytes"
    return do.cpu().numpy().reshape(nseg, 4).copy()


def check_dev(hip, pts, sc, offsets=None, m=None, **kw):
    exp = S.segments_dev(pts, sc, offsets, m)
    got = seg_dev(hip, pts, sc, offsets, m, **kw)
    bad = np.flatnonzero((got != exp).any(1))
    assert bad.size == 0, (bad[:8], got[bad[:4]], exp[bad[:4]])
    return got


# ------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("kind", ["random", "irregular"])
def test_golden_lists(hip, kind):
    """the reference's bytes from the host form for both lists; from the _dev form with status 0 for the canonical
    list, status 1 and FF FF FF for every segment of the irregular one"""
    g = load_golden("msm_segments.json")["lists"][kind]
    pts, sc, off = mk.list_inputs(kind)
    exp = np.frombuffer(bytes.fromhex(g["out3"]), np.uint8).reshape(-1, 3)
    assert np.array_equal(S.segments_host(pts, sc, off), exp)
    assert np.array_equal(hip.msm_g1_segments(pts, sc, offsets=off), exp)
    got = check_dev(hip, pts, sc, off)
    if kind == "random":
        assert np.array_equal(got[:, :3], exp) and not got[:, 3].any()
    else:
        assert (got == FFI).all()


# ------------------------------------------------------------------ lane path
@pytest.mark.parametrize("m", [1, 2, 9, 16, 17, 32])
def test_lane_path(hip, pool, m):
    for nseg in (1, 63, 64, 65, 1000):
        p = hip.msm_g1_segments_plan(m * nseg, m, nseg, 0)
        assert p["path"] == LANE and p["launches"] == 1 and hip.msm_g1_segments_workspace(m * nseg, m, nseg, 0) == 0
        pts, sc = pool.take(m * nseg, start=nseg)
        got = check_dev(hip, pts, sc, m=m)
        assert not got[:, 3].any()
        if nseg == 65:
            assert np.array_equal(hip.msm_g1_segments(pts, sc, m=m), got[:, :3])
            assert np.array_equal(S.segments_host(pts, sc, m=m), got[:, :3])


# ------------------------------------------------------------------ prefix path, uniform
@pytest.mark.parametrize("shape", ["33x5", "T-1x3", "Tx3", "T+1x3", "3T+37x1"])
def test_prefix_path_uniform(hip, pool, T, shape):
    m, nseg = {"33x5": (33, 5), "T-1x3": (T - 1, 3), "Tx3": (T, 3), "T+1x3": (T + 1, 3), "3T+37x1": (3 * T + 37, 1)}[shape]
    p = hip.msm_g1_segments_plan(m * nseg, m, nseg, 0)
    assert p["path"] == PREFIX and p["launches"] == 3 and p["tile"] == T
    pts, sc = pool.take(m * nseg, start=7)
    got = check_dev(hip, pts, sc, m=m)
    assert not got[:, 3].any()
    assert np.array_equal(hip.msm_g1_segments(pts, sc, m=m), got[:, :3])


# ------------------------------------------------------------------ prefix path, ragged
def edge_lists(T):
    """two lists over total = 3 T + 37 (offsets rise, so one list cannot hold both a segment ending at T and one
    that spans it): A starts at 0 with an empty segment and one of length 1, ends segments at 15, 16, 17, has
    lengths 32 and 33, an empty segment in the middle, ends at T - 1, T, T + 1, covers a whole tile and parts of its
    neighbours, and is empty at total; B covers two whole tiles and parts of their neighbours"""
    total = 3 * T + 37
    a = [0, 0, 1, 15, 16, 17, 49, 82, 82, T - 1, T, T + 1, 3 * T + 20, total, total]
    b = [0, T - 7, 3 * T + 5, total]
    return total, a, b


def test_prefix_path_ragged_edges(hip, pool, T):
    total, a, b = edge_lists(T)
    lens = np.diff(a).tolist()
    assert lens[:2] == [0, 1] and {32, 33} <= set(lens) and lens.count(0) == 3 and a[-2:] == [total, total]
    pts, sc = pool.take(total, start=3)
    for off in (a, b):
        assert hip.msm_g1_segments_plan(total, 0, len(off) - 1, 1)["path"] == PREFIX
        got = check_dev(hip, pts, sc, off)
        assert not got[:, 3].any()
        assert np.array_equal(hip.msm_g1_segments(pts, sc, offsets=off), got[:, :3])
        assert np.array_equal(S.segments_host(pts, sc, off), got[:, :3])
    empty = [g for g, n in enumerate(lens) if n == 0]
    assert (check_dev(hip, pts, sc, a)[empty] == (0, 0, 1, 0)).all()


def test_bytes_outside_the_segments_do_not_matter(hip, pool, T):
    """the first offset is not 0 and the last is below total; the points and scalars outside are non-canonical poison"""
    total = 2 * T + 100
    pts, sc = pool.take(total, start=11)
    off = [21, 30, 70, T + 3, 2 * T + 50]
    clean = S.segments_dev(pts, sc, off)
    pts[:21], sc[:21] = devbuf.RAW, devbuf.RAW
    pts[2 * T + 50:], sc[2 * T + 50:] = devbuf.RAW, devbuf.RAW
    assert not E.canonical_mask(pts[:21]).any()
    got = check_dev(hip, pts, sc, off)
    assert np.array_equal(got, clean) and not got[:, 3].any()
    assert np.array_equal(hip.msm_g1_segments(pts, sc, offsets=off), clean[:, :3])


def test_one_segment_lists(hip, pool, T):
    for total in (1, 33, T + 5):
        pts, sc = pool.take(total, start=total)
        whole = check_dev(hip, pts, sc, [0, total])
        assert whole[0, 3] == 0 and bytes(whole[0, :3]) == hip.msm_g1(pts, sc)
        for at in (0, total // 2, total):
            assert check_dev(hip, pts, sc, [at, at]).tolist() == [[0, 0, 1, 0]]


# ------------------------------------------------------------------ irregular encodings
def test_every_near_miss_flags_its_segment_only(hip):
    """every near-miss encoding of tests/g1_encoding_cases.py, alternately at the first and at the last point of a
    segment of its own (lengths on both sides of the direct-sum switch), clean segments on both sides"""
    cands = np.concatenate([E.near_misses(), E.seeded_triples((0, 1, 2, 255), 300, "msm_segments")])
    cands = cands[~E.canonical_mask(cands)]
    lens = np.array([20, 40, 33, 32, 50, 1, 16, 17])[np.arange(3 * len(cands)) % 8]
    off = np.concatenate([[0], np.cumsum(lens)])
    pts, sc = E.fillers(E.rng_for("msm_segments/near"), int(off[-1]))
    hold = 3 * np.arange(len(cands)) + 1
    pos = np.where(np.arange(len(cands)) % 2 == 0, off[hold], off[hold + 1] - 1)
    pts[pos] = cands
    got = check_dev(hip, pts, sc, off)
    status = np.zeros(len(lens), np.uint8)
    status[hold] = S.IRREGULAR
    assert np.array_equal(got[:, 3], status) and (got[hold] == FFI).all()


EDGE_CANDS = [(5, 5, 0), (1, 2, 1), (0, 0, 0), (0, 0, 2), (1, 2, 255), (101, 2, 0), (1, 103, 0), (255, 255, 255)]


@pytest.mark.parametrize("length", [20, 40], ids=["direct", "prefix"])
def test_bad_point_next_to_a_segment_edge(hip, pool, T, length):
    """a bad point at o_g - 1 or at o_{g+1} must not flag g: boundaries at chunk edges (the bad point at an index that
    is 15 and 0 mod 16) and at tile edges, segments summed directly and as prefix differences; the host form of the
    flagged segment is plk_msm_g1 of its bytes"""
    total = 2 * T + 200
    for i, b in enumerate((48, 64, T, 2 * T, T + 16)):
        off = [3, b - length, b, b + length, total - 5]
        for j, at in enumerate((b - 1, b)):
            cand = EDGE_CANDS[(2 * i + j) % len(EDGE_CANDS)]
            pts, sc = pool.take(total, start=5 * i)
            clean = S.segments_dev(pts, sc, off)
            pts[at] = cand
            sc[at] = 1 + sc[at] % 255
            got = check_dev(hip, pts, sc, off)
            exp = clean.copy()
            exp[1 + j] = FFI
            assert np.array_equal(got, exp), (b, at, cand)
            host = hip.msm_g1_segments(pts, sc, offsets=off)
            assert np.array_equal(np.delete(host, 1 + j, 0), np.delete(clean[:, :3], 1 + j, 0))
            lo, hi = off[1 + j], off[2 + j]
            assert bytes(host[1 + j]) == hip.msm_g1(pts[lo:hi], sc[lo:hi]), (b, at, cand)


def test_lane_path_flags_the_holding_segment_only(hip, pool):
    for m in (1, 9, 16, 32):
        pts, sc = pool.take(5 * m, start=m)
        clean = S.segments_dev(pts, sc, m=m)
        for at, g in ((2 * m, 2), (3 * m - 1, 2), (0, 0), (5 * m - 1, 4)):
            p2 = pts.copy()
            p2[at] = EDGE_CANDS[(at + m) % len(EDGE_CANDS)]
            exp = clean.copy()
            exp[g] = FFI
            assert np.array_equal(check_dev(hip, p2, sc, m=m), exp), (m, at)
            host = hip.msm_g1_segments(p2, sc, m=m)
            assert np.array_equal(np.delete(host, g, 0), np.delete(clean[:, :3], g, 0))
            assert bytes(host[g]) == hip.msm_g1(p2[g * m:(g + 1) * m], sc[g * m:(g + 1) * m])


# ------------------------------------------------------------------ bad offsets
def test_bad_offsets_mark_their_segments_only(hip, pool, T):
    """a falling pair and offsets above total give status 2 for exactly those segments; the arrays lie inside a larger
    allocation of non-canonical poison (the guard exceeds the largest excess), so a missing clamp shows as wrong bytes
    or a wrong status, never as a read outside an allocation"""
    for total in (100, T + 40):
        pts, sc = pool.take(total, start=9)
        off = [0, 10, 5, 50, total + 30, total + 10, total, total, total - 40, total + 1, total - 3, total]
        assert max(off) - total < devbuf.GUARD
        exp = S.segments_dev(pts, sc, off)
        assert exp[:, 3].tolist() == [0, 2, 0, 2, 2, 2, 0, 2, 2, 2, 0]
        got = check_dev(hip, pts, sc, off)
        assert np.array_equal(got[:, 3], exp[:, 3]) and (got[exp[:, 3] == 2, :3] == 0xFF).all()
        for g in (0, 2, 6, 10):
            assert np.array_equal(got[g, :3], S.segments_host(pts, sc, [off[g], off[g + 1]])[0])
    huge = [0, 0xFFFFFFFF, 7, 0x80000000, 100]
    pts, sc = pool.take(100)
    assert check_dev(hip, pts, sc, huge)[:, 3].tolist() == [2, 2, 2, 2]


# ------------------------------------------------------------------ placement
@pytest.mark.parametrize("residue", range(16))
def test_points_and_scalars_at_every_residue(hip, pool, T, residue):
    rs = (5 * residue + 1) % 16 if residue else 0
    pts, sc = pool.take(T + 100, start=residue)
    off = [0, 1, 17, 60, T + 3, T + 100]
    for ro in (0, residue % 4):
        check_dev(hip, pts, sc, off, rp=residue, rs=rs, ro=ro)
        check_dev(hip, pts[:64 * 16], sc[:64 * 16], m=16, rp=residue, rs=rs, ro=ro)
        check_dev(hip, pts[:70 * 9], sc[:70 * 9], m=9, rp=rs, rs=residue, ro=ro)


@pytest.mark.parametrize("ro", [0, 1, 2, 3])
def test_output_at_every_residue(hip, pool, T, ro):
    pts, sc = pool.take(T + 100, start=ro)
    check_dev(hip, pts, sc, [0, 1, 17, 60, T + 3, T + 100], ro=ro)
    check_dev(hip, pts[:320], sc[:320], m=32, ro=ro)
    check_dev(hip, pts[:330], sc[:330], m=33, ro=ro)


def test_workspace_reused_and_runs_identical(hip, pool, T):
    """one 0xEE-filled workspace and one stream for two different lists and a repeat of the first"""
    import torch
    total = 3 * T + 37
    _, a, b = edge_lists(T)
    pa, sa = pool.take(total, start=1)
    pb, sb = pool.take(total, start=2)
    pb[T + 9] = (5, 5, 0)
    ws = max(hip.msm_g1_segments_workspace(total, 0, len(o) - 1, 1) for o in (a, b))
    work = torch.full((ws,), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    first = check_dev(hip, pa, sa, a, work=work, stream=s)
    other = check_dev(hip, pb, sb, b, work=work, stream=s)
    assert other[:, 3].tolist() == [0, 1, 0]
    again = check_dev(hip, pa, sa, a, work=work, stream=s)
    assert np.array_equal(first, again)
    assert np.array_equal(check_dev(hip, pa, sa, a, rp=3, rs=5), first)


# ------------------------------------------------------------------ through the public API
def subgroup_srs(n):
    g1 = load_golden("g1.json")["kG_k0_17"]
    return np.array([list(bytes.fromhex(g1[pow(2, i, 17)])) for i in range(n)], np.uint8)


def test_weighted_sums_of_commitments_are_commitments_of_weighted_sums(hip):
    """segments of the k = 9 commitments under weights w < 17 equal plk_kzg_commit_batch of plk_poly_lincomb of the
    polynomials under the same weights (an SRS inside the subgroup of order 17, where the coefficients act mod 17)"""
    k, groups, n = 9, 300, 40
    polys = [gen.poly_inputs(0x5E6 + i, n - i, 0)[0] for i in range(k)]
    w = (gen.splitmix64(0x5E7, groups * k) % np.uint64(17)).astype(np.uint8).reshape(groups, k)
    w[0], w[1] = 0, 16
    with hip.Srs(subgroup_srs(n)) as srs:
        assert not srs.irregular
        commits = np.array([list(c) for c in hip.kzg_commit(srs, polys)], np.uint8)
        combos = [hip.poly_lincomb(([hip.lc_term(p, scale=int(s)) for p, s in zip(polys, row)], -1))[0] for row in w]
        exp = np.array([list(c) for c in hip.kzg_commit(srs, combos)], np.uint8)
    assert len({tuple(r) for r in exp.tolist()}) > 10 and tuple(exp[0]) == (0, 0, 1)
    pts, sc = np.tile(commits, (groups, 1)), w.reshape(-1)
    assert np.array_equal(hip.msm_g1_segments(pts, sc, m=k), exp)
    got = check_dev(hip, pts, sc, m=k)
    assert np.array_equal(got[:, :3], exp) and not got[:, 3].any()
    off = np.arange(0, groups * k + 1, k)
    assert np.array_equal(check_dev(hip, pts, sc, off), got)


def test_dev_words_feed_the_verify_call_without_the_host(hip):
    """C_a + C_b from the _dev form, copied from stride 4 to 3 bytes on the device, is accepted by
    plk_kzg_verify_batch_dev with the library's opening of p_a + p_b; a flagged segment (FF FF FF) is answered with 2"""
    import torch
    n, pairs = 24, 12
    polys = [gen.poly_inputs(0x5E8 + i, n - i % 3, 0)[0] for i in range(2 * pairs)]
    zs = [(3 * i + 1) % 17 for i in range(pairs)]
    g2 = load_golden("pairing.json")["g2_multiples"]
    vk = hip.KzgVk((1, 2, 0), bytes.fromhex(g2["1"]), bytes.fromhex(g2["2"]))
    with hip.Srs(subgroup_srs(n)) as srs:
        commits = np.array([list(c) for c in hip.kzg_commit(srs, polys)], np.uint8)
        sums = []
        for i in range(pairs):
            s = np.zeros(n, np.uint8)
            for p in (polys[2 * i], polys[2 * i + 1]):
                s[:p.size] = (s[:p.size] + p) % 17
            sums.append(s)
        ys, proofs = hip.kzg_open(srs, sums, zs)
    commits[2 * (pairs - 1)] = (5, 5, 0)                       # the last pair holds an off-curve commitment
    sc = np.ones(2 * pairs, np.uint8)
    out4 = torch.full((4 * pairs,), 0xEE, dtype=torch.uint8, device="cuda")
    dp, ds = torch.from_numpy(commits.reshape(-1)).cuda(), torch.from_numpy(sc).cuda()
    hip.msm_g1_segments_dev(dp, ds, 2 * pairs, None, 2, pairs, out4)
    c3 = out4.view(pairs, 4)[:, :3].contiguous()
    dz, dy = torch.tensor(zs, dtype=torch.uint8).cuda(), torch.tensor(ys, dtype=torch.uint8).cuda()
    dw = torch.from_numpy(np.array([list(p) for p in proofs], np.uint8).reshape(-1)).cuda()
    ok = torch.full((pairs,), 0xEE, dtype=torch.uint8, device="cuda")
    hip.kzg_verify_dev(vk, c3, dz, dy, dw, pairs, ok)
    torch.cuda.synchronize()
    assert out4.view(pairs, 4)[:, 3].cpu().tolist() == [0] * (pairs - 1) + [1]
    assert ok.cpu().tolist() == [1] * (pairs - 1) + [2]
