"""The batched MSM launch (plk_msm_g1_batch_dev -> msm_dlog_kernel with blockIdx.y = the row) and what
follows it on the multi-GPU path (gpu_ops.records_to_partials, finish_sharded, plk_msm_finalize_dev),
against the oracle's serial fold at the smallest shapes where each piece can go wrong.

The ticketed finish (msm_finish_xy, plk_msm_finish.h) derives a block's shard, the shard's block
count and the number of arriving shards from (row * X + x) mod PLK_MSM_SHARDS, X = blocks per row.  A
mistake there crashes nothing: a record keeps the previous launch's point, completes early with a
partial sum, or keeps non-zero internal words that corrupt the next launch reusing it.  So every
launch here goes through run_batch, which checks that each record is all zero outside
log / irregular / g1 afterwards, and every test first asserts through plk_msm_plan (the launch's own
helper) that it ran the blocks per row it means to run.

Everything that is not a row byte in the device buffers is 0xFF: a point read from it is an
irregular encoding, so `irregular == 0` on every row also says nothing was read outside the rows
(the padding control shows a read of the pad is seen).
"""
import numpy as np
import pytest

import gen
from plonkhip import dist

pytestmark = pytest.mark.gpu

SHAPE_A = 37461      # 2341 groups of 16 + a 5-point tail: 256-thread blocks, up to 10 blocks per row
SHAPE_B = 1059785    # 66236 groups + a 9-point tail: 512-thread blocks
SHAPE_C = 135205     # 8450 groups + a 5-point tail: 256-thread blocks, up to 34 (past the 16 ticket shards)
POISON = 0xFF
TAIL_PAD = 64        # poison after the last row
GUARD = 256          # poison after the records array / an output
STALE = 0x5A         # written over log / irregular / g1 before every launch
IDENT = bytes([0, 0, 1])


def _round16(v):
    return (v + 15) & ~15


def _dev():
    import torch
    return torch.device("cuda:0")


def _upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(_dev())


def new_records(hip, batch, fill=0):
    """batch result records (zeroed) followed by GUARD poison bytes, one uint8 device tensor"""
    import torch
    buf = torch.full((batch * hip.MSM_RESULT_BYTES + GUARD,), fill, dtype=torch.uint8, device=_dev())
    buf[batch * hip.MSM_RESULT_BYTES:] = POISON
    return buf


def records_view(hip, records, batch):
    return records[:batch * hip.MSM_RESULT_BYTES].view(batch, hip.MSM_RESULT_BYTES)


def check_records(hip, records, batch):
    """parsed records; asserts the guard after them is intact and every record is zero outside
    log / irregular / g1[0..2] (top, g1[3], pad and the whole shard array: the re-arming)"""
    R = hip.MSM_RESULT_BYTES
    host = records.cpu().numpy()
    assert host.size == batch * R + GUARD
    assert (host[batch * R:] == POISON).all(), "guard after the records overwritten"
    rec = host[:batch * R].reshape(batch, R)
    dirty = np.flatnonzero(rec[:, :hip.MSM_LOG_OFFSET].any(axis=1) | rec[:, hip.MSM_G1_OFFSET + 3:].any(axis=1))
    assert dirty.size == 0, ("records with non-zero internal words after the launch", dirty[:8].tolist())
    logs = rec[:, hip.MSM_LOG_OFFSET:hip.MSM_LOG_OFFSET + 4].copy().view("<u4").reshape(-1)
    irr = rec[:, hip.MSM_IRREGULAR_OFFSET:hip.MSM_IRREGULAR_OFFSET + 4].copy().view("<u4").reshape(-1)
    g1 = rec[:, hip.MSM_G1_OFFSET:hip.MSM_G1_OFFSET + 3]
    return [{"log": int(logs[b]), "irregular": int(irr[b]), "g1": bytes(g1[b])} for b in range(batch)]


def run_batch(hip, rows, pstride, sstride, base_off=(0, 0), records=None, n=None, batch=None):
    """ONE plk_msm_g1_batch_dev launch over rows = [(points[n, 3], scalars[n]), ...] laid out at
    base + b * stride in one device buffer each for points and scalars; every other byte of the
    buffers (before an offset base, between rows, TAIL_PAD after the last row) is POISON.  With a
    stride of 0 the rows must agree (one SRS / one scalar vector).  n / batch: launch with other
    values than the layout's (the padding control, many records over one row).  records: reuse
    these (new_records) without re-initialising their internal words.  Returns check_records'
    parsed records."""
    import torch
    rn = rows[0][1].size
    n = rn if n is None else n
    batch = len(rows) if batch is None else batch
    poff, soff = base_off
    hp = np.full(poff + (len(rows) - 1) * pstride + 3 * rn + TAIL_PAD, POISON, np.uint8)
    hs = np.full(soff + (len(rows) - 1) * sstride + rn + TAIL_PAD, POISON, np.uint8)
    for b, (p, s) in enumerate(rows):
        assert p.shape == (rn, 3) and s.shape == (rn,)
        hp[poff + b * pstride:poff + b * pstride + 3 * rn] = p.reshape(-1)
        hs[soff + b * sstride:soff + b * sstride + rn] = s
    # every byte the launch may read lies inside the buffers (rows beyond the layout: stride 0 only)
    last = batch - 1 if batch > 1 else 0
    assert poff + last * pstride + 3 * n <= hp.size and soff + last * sstride + n <= hs.size
    dp, ds = _upload(hp), _upload(hs)
    assert dp.data_ptr() % 16 == 0 and ds.data_ptr() % 16 == 0
    if records is None:
        records = new_records(hip, batch)
    # stale answers in the output fields (the internal words stay as the last launch left them): a
    # record the launch never completes shows them instead of an earlier launch's right answer
    records_view(hip, records, batch)[:, hip.MSM_LOG_OFFSET:hip.MSM_G1_OFFSET + 3] = STALE
    hip.msm_g1_batch_dev(dp.data_ptr() + poff, pstride, ds.data_ptr() + soff, sstride, n, batch, records,
                         torch.cuda.current_stream())
    torch.cuda.synchronize()
    return check_records(hip, records, batch)


def make_row(oracle, kind, seed, n):
    """(points, scalars) of one row; besides gen.msm_inputs' kinds: all-identity points, all-zero
    scalars, and "max": every point the group element of discrete log 101 with every scalar 255"""
    if kind in ("subgroup", "full", "bytes"):
        return gen.msm_inputs(seed, n, kind)
    pts, sc = gen.msm_inputs(seed, n, "full")
    if kind == "identity":
        return np.tile(np.array([0, 0, 1], np.uint8), (n, 1)), sc.copy()
    if kind == "zero":
        return pts, np.zeros(n, np.uint8)
    assert kind == "max"
    top = [p for p in gen.all_points() if oracle.dlog(p) == 101]
    assert len(top) == 1
    return np.tile(top[0], (n, 1)), np.full(n, 255, np.uint8)


def want_of(oracle, rows):
    """per row (G1 bytes of the serial fold, discrete log) -- the log only for canonical rows"""
    return [(oracle.msm(p, s), oracle.msm_dlog(p, s)[0]) for p, s in rows]


def assert_rows(got, want, ctx=None):
    for b, (g, (g1, lg)) in enumerate(zip(got, want)):
        assert g["irregular"] == 0, (ctx, b, g)
        assert g["g1"] == g1, (ctx, b, g, g1.hex())
        assert g["log"] == lg, (ctx, b, g, lg)


KINDS = ("subgroup", "full", "bytes", "identity", "zero", "max")


@pytest.fixture(scope="module")
def rows_a(hip, oracle):
    """11 rows of shape A cycling through KINDS, their oracle answers, and ONE records array that
    every launch of test_blocks_per_row_1_to_9 reuses without re-initialising"""
    rows = [make_row(oracle, KINDS[b % len(KINDS)], 0xA00 + b, SHAPE_A) for b in range(11)]
    want = want_of(oracle, rows)
    assert want[3][0] == IDENT and want[4][0] == IDENT
    assert len({w[0] for w in want}) >= 6          # the rows do not all agree
    return {"rows": rows, "want": want, "records": new_records(hip, 11)}


@pytest.mark.parametrize("X", range(1, 10))
def test_blocks_per_row_1_to_9(hip, rows_a, X):
    """X = 1..9 blocks per row over rows 0..10: below the shard count every shard has one block of
    the row or none, X shards arrive, and the row's first shard is (row * X) mod 16 -- every
    (X, row) pair there.  The records carry over from one geometry to the next (the parametrized
    cases run in order on one array; only the output fields are overwritten in between)."""
    rows, want, records = rows_a["rows"], rows_a["want"], rows_a["records"]
    pstride, sstride = _round16(3 * SHAPE_A), _round16(SHAPE_A)
    variants = [{}]
    if X == 1:
        variants.append({"MSM_GROUPS": 4})
    if X == 3:
        variants.append({"MSM_THREADS": 1024})
    for extra in variants:
        with hip.options(MSM_MAX_BLOCKS=11 * X, **extra):
            plan = hip.msm_plan(SHAPE_A, 11)
            assert plan["blocks"] == X and plan["half"] == 0, plan
            assert plan["threads"] == extra.get("MSM_THREADS", 256), plan
            assert plan["groups"] == (4 if extra.get("MSM_GROUPS") else (2 if X <= 4 and not extra else 1)), plan
            got = run_batch(hip, rows, pstride, sstride, records=records)
        assert_rows(got, want, (X, extra))
    # the byte-wise form of the same launch (odd strides), on the same records
    with hip.options(MSM_MAX_BLOCKS=11 * X):
        plan = hip.msm_plan(SHAPE_A, 11, aligned=False)
        assert (plan["threads"], plan["blocks"], plan["groups"], plan["half"]) == (256, X, 1, 0), plan
        got = run_batch(hip, rows, 3 * SHAPE_A + 1, SHAPE_A + 3, records=records)
    assert_rows(got, want, (X, "byte-wise"))


@pytest.mark.parametrize("X", (15, 16, 17, 33))
def test_blocks_per_row_around_the_shard_count(hip, oracle, X):
    """PLK_MSM_SHARDS is 16: from X = 17 a shard holds several blocks of one row, at X = 15 / 17 the
    row's first shard moves with the row index; 5 rows, so rows start in shards 0, X, 2X, ... mod 16"""
    kinds = ("full", "bytes", "subgroup", "max", "full")
    rows = [make_row(oracle, kinds[b], 0xC00 + b, SHAPE_C) for b in range(5)]
    with hip.options(MSM_MAX_BLOCKS=5 * X):
        plan = hip.msm_plan(SHAPE_C, 5)
        assert (plan["threads"], plan["blocks"]) == (256, X), plan
        records = new_records(hip, 5)
        got = run_batch(hip, rows, _round16(3 * SHAPE_C), _round16(SHAPE_C), records=records)
        assert_rows(got, want_of(oracle, rows), X)
        # the same records again, the rows in another order: nothing may survive from the first launch
        got = run_batch(hip, rows[::-1], _round16(3 * SHAPE_C), _round16(SHAPE_C), records=records)
        assert_rows(got, want_of(oracle, rows[::-1]), (X, "reversed"))


@pytest.fixture(scope="module")
def rows_b(oracle):
    kinds = ("full", "bytes", "full")
    rows = [make_row(oracle, kinds[b], 0xB00 + b, SHAPE_B) for b in range(3)]
    return rows, want_of(oracle, rows)


@pytest.mark.parametrize("X", (3, 7))
def test_512_thread_rows(hip, rows_b, X):
    rows, want = rows_b
    with hip.options(MSM_MAX_BLOCKS=3 * X):
        plan = hip.msm_plan(SHAPE_B, 3)
        assert (plan["threads"], plan["blocks"], plan["groups"]) == (512, X, 2), plan
        got = run_batch(hip, rows, _round16(3 * SHAPE_B), _round16(SHAPE_B))
    assert_rows(got, want, X)


@pytest.fixture(scope="module")
def pool_a(oracle):
    """8 distinct rows of shape A and their oracle answers, repeated cyclically for large batches"""
    kinds = ("subgroup", "full", "bytes", "full", "max", "bytes", "identity", "full")
    rows = [make_row(oracle, kinds[b], 0xD00 + b, SHAPE_A) for b in range(8)]
    return rows, want_of(oracle, rows)


@pytest.mark.parametrize("batch,blocks", [(2, 10), (64, 8), (100, 5), (160, 10)])
def test_default_geometry(hip, pool_a, batch, blocks):
    rows, want = pool_a
    plan = hip.msm_plan(SHAPE_A, batch)
    assert (plan["threads"], plan["blocks"], plan["half"]) == (256, blocks, 0), plan
    got = run_batch(hip, [rows[b % 8] for b in range(batch)], _round16(3 * SHAPE_A), _round16(SHAPE_A))
    assert_rows(got, [want[b % 8] for b in range(batch)], batch)


@pytest.mark.parametrize("n", (0, 1, 15, 16, 17, 255))
def test_tiny_rows(hip, oracle, n):
    rows = [make_row(oracle, KINDS[b % 3], 0xE00 + 16 * n + b, n) for b in range(9)]
    if n:
        rows[4] = (rows[4][0], np.full(n, 255, np.uint8))
    assert hip.msm_plan(n, 9)["blocks"] == 1
    records = new_records(hip, 9)
    got = run_batch(hip, rows, _round16(3 * n), _round16(n), records=records)
    if n == 0:
        assert got == [{"log": 0, "irregular": 0, "g1": IDENT}] * 9
    assert_rows(got, want_of(oracle, rows), n)
    # contiguous rows (stride = row: the byte-wise form unless n is a multiple of 16)
    assert_rows(run_batch(hip, rows, 3 * n, n, records=records), want_of(oracle, rows), (n, "contiguous"))


@pytest.fixture(scope="module")
def rows5(oracle):
    kinds = ("full", "bytes", "subgroup", "bytes", "full")
    rows = [make_row(oracle, kinds[b], 0xF00 + b, SHAPE_A) for b in range(5)]
    return rows, want_of(oracle, rows)


PADDED = (_round16(3 * SHAPE_A) + 32, _round16(SHAPE_A) + 16)


@pytest.mark.parametrize("case", ["padded", "odd", "points_base_off_1", "scalars_base_off_5"])
def test_strides_and_alignment(hip, rows5, case):
    rows, want = rows5
    n = SHAPE_A
    aligned = case == "padded"
    pstride, sstride = (3 * n + 1, n + 3) if case == "odd" else PADDED
    off = {"points_base_off_1": (1, 0), "scalars_base_off_5": (0, 5)}.get(case, (0, 0))
    plan = hip.msm_plan(n, 5, aligned)
    assert (plan["threads"], plan["blocks"], plan["half"]) == (256, 10, 0), plan
    if not aligned:
        assert plan["groups"] == 1, plan
    assert_rows(run_batch(hip, rows, pstride, sstride, base_off=off), want, case)


def test_one_srs_many_scalar_rows(hip, oracle, rows5):
    """points_stride = 0: every row reads the same points"""
    rows, _ = rows5
    pts = rows[1][0]
    shared = [(pts, s) for _, s in rows]
    assert_rows(run_batch(hip, shared, 0, PADDED[1]), want_of(oracle, shared), "pstride 0")
    # ... and one scalar vector against many point rows
    sc = rows[1][1]
    shared = [(p, sc) for p, _ in rows]
    assert_rows(run_batch(hip, shared, PADDED[0], 0), want_of(oracle, shared), "sstride 0")


def test_single_row_ignores_strides(hip, rows5):
    rows, want = rows5
    plan = hip.msm_plan(SHAPE_A, 1)
    assert (plan["blocks"], plan["half"]) == (20, 1), plan      # aligned bases: the half-group form
    assert_rows(run_batch(hip, rows[:1], 7, 13), want[:1], "batch 1, strides 7 / 13")
    assert hip.msm_plan(SHAPE_A, 1, aligned=False)["blocks"] == 10
    assert_rows(run_batch(hip, rows[:1], 1 << 40, 3, base_off=(3, 1)), want[:1], "batch 1, misaligned bases")


def test_padding_control_poison_is_seen(hip, rows5):
    """the padded layout launched with n + 1 points: each row's last point is the poison triple
    {0xFF, 0xFF, 0xFF} right behind it, so every row must report it"""
    rows, _ = rows5
    got = run_batch(hip, rows, PADDED[0], PADDED[1], n=SHAPE_A + 1)
    assert all(g["irregular"] > 0 for g in got), got


@pytest.mark.parametrize("layout", ["aligned", "odd"])
def test_irregular_rows(hip, oracle, rows_a, layout):
    """irregular points in 3 of 11 rows (inside a full group, in the 5-point tail, as the first
    point): exactly those rows are flagged, the others are right, and finish_sharded repairs the
    three through the exact serial fold"""
    n = SHAPE_A
    rows = [(p.copy(), s.copy()) for p, s in rows_a["rows"]]
    for b, idx, raw in ((3, 16 * 1000 + 7, (3, 3, 0)), (7, n - 2, (7, 7, 1)), (10, 0, (200, 150, 0))):
        rows[b][0][idx] = raw
        rows[b][1][idx] = 5
    assert n - 2 >= (n >> 4) << 4
    bad = {3, 7, 10}
    want = [rows_a["want"][b] if b not in bad else (oracle.msm(*rows[b]), None) for b in range(11)]
    pstride, sstride = (3 * n + 1, n + 3) if layout == "odd" else (_round16(3 * n), _round16(n))
    assert hip.msm_plan(n, 11, layout == "aligned")["blocks"] == 10
    records = new_records(hip, 11)
    got = run_batch(hip, rows, pstride, sstride, records=records)
    assert {b for b in range(11) if got[b]["irregular"] > 0} == bad, got
    assert_rows([got[b] for b in range(11) if b not in bad], [want[b] for b in range(11) if b not in bad], layout)
    ops = dist.gpu_ops(hip)
    part = ops.records_to_partials(records_view(hip, records, 11))
    out, folded = dist.finish_sharded(part, n, ops, lambda b: (_upload(rows[b][0]), _upload(rows[b][1])))
    assert folded == 3
    assert dist.g1_bytes(out) == [w[0] for w in want]


def test_batch_limits(hip, oracle):
    import torch
    R = hip.MSM_RESULT_BYTES
    pts, sc = gen.msm_inputs(0x11, 16, "bytes")
    dp, ds = _upload(pts), _upload(sc)
    st = torch.cuda.current_stream()
    records = new_records(hip, 2, fill=0xA5)
    before = records.cpu().numpy().copy()
    for batch in (0, -1):                                  # no-ops
        hip.msm_g1_batch_dev(dp, 48, ds, 16, 16, batch, records, st)
    with pytest.raises(hip.PlonkHipError) as e:       # refused before any launch
        hip.msm_g1_batch_dev(dp, 0, ds, 0, 16, 65536, records, st)
    assert e.value.code == hip.PLK_ERR_RANGE
    torch.cuda.synchronize()
    assert (records.cpu().numpy() == before).all()
    del records
    # the largest batch: 65535 records (143 MB) over one 16-point row
    assert hip.msm_plan(16, 65535)["blocks"] == 1
    got = run_batch(hip, [(pts, sc)], 0, 0, batch=65535)
    assert len(got) == 65535 and R * 65535 > 142 * 10 ** 6
    want = {"log": oracle.msm_dlog(pts, sc)[0], "irregular": 0, "g1": oracle.msm(pts, sc)}
    wrong = [b for b, g in enumerate(got) if g != want]
    assert not wrong, (len(wrong), wrong[:8], got[wrong[0]], want)


def _finalize(hip, logs_ptr, batch, stride):
    """plk_msm_finalize_dev into a poisoned out4 with a guard: returns the batch x 4 bytes"""
    import torch
    out = torch.full((4 * batch + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    hip.msm_finalize_dev(logs_ptr, batch, stride, out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[4 * batch:] == POISON).all(), "guard after out4 overwritten"
    return host[:4 * batch].reshape(batch, 4)


def _exp4(oracle, k):
    return oracle.dlog_exp(k % 102) + b"\0"


def test_finalize_every_log_and_reduction(hip, oracle):
    import torch
    ks = list(range(102)) + [102, 203, 8 * 101, 2 ** 31 - 1]
    logs = torch.tensor(ks, dtype=torch.int32, device=_dev())
    got = _finalize(hip, logs.data_ptr(), len(ks), 1)
    assert [bytes(r) for r in got] == [_exp4(oracle, k) for k in ks]
    assert bytes(got[0]) == IDENT + b"\0"
    # the kernel reduces an UNSIGNED word: 2^32 - 1 = 33 (mod 102), 2^31 = 26
    logs = torch.tensor([-1, -(2 ** 31)], dtype=torch.int32, device=_dev())
    assert [bytes(r) for r in _finalize(hip, logs.data_ptr(), 2, 1)] == [_exp4(oracle, 2 ** 32 - 1),
                                                                          _exp4(oracle, 2 ** 31)]


@pytest.mark.parametrize("batch", (1, 256, 257, 1000))
def test_finalize_batch_sizes(hip, oracle, batch):
    """the launch uses 256-thread blocks: one block, exactly one, one more thread, several"""
    import torch
    ks = (gen.splitmix64(0xF1 + batch, batch) % np.uint64(1 << 20)).astype(np.int64)
    logs = torch.from_numpy(ks.astype(np.int32)).to(_dev())
    got = _finalize(hip, logs.data_ptr(), batch, 1)
    table = [_exp4(oracle, k) for k in range(102)]
    assert [bytes(r) for r in got] == [table[int(k) % 102] for k in ks]
    # batch <= 0: nothing written
    out = torch.full((8,), POISON, dtype=torch.uint8, device=_dev())
    hip.msm_finalize_dev(logs, 0, 1, out, torch.cuda.current_stream())
    hip.msm_finalize_dev(logs, -3, 1, out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()


def test_finalize_strided_over_partials_and_records(hip, oracle):
    """stride 2 over records_to_partials' [batch, 2] tensor, and stride MSM_RESULT_BYTES / 4 over the
    log words of a real records array: both give the points the launch itself wrote"""
    batch, n = 9, 255
    rows = [make_row(oracle, KINDS[b % 3], 0x700 + b, n) for b in range(batch)]
    records = new_records(hip, batch)
    got = run_batch(hip, rows, _round16(3 * n), _round16(n), records=records)
    want = want_of(oracle, rows)
    assert_rows(got, want)
    assert len({w[1] for w in want}) > 4
    g1 = [w[0] + b"\0" for w in want]
    part = dist.gpu_ops(hip).records_to_partials(records_view(hip, records, batch))
    assert tuple(part.shape) == (batch, 2) and part.is_contiguous()
    assert part.cpu().numpy().tolist() == [[w[1], 0] for w in want]
    assert [bytes(r) for r in _finalize(hip, part.data_ptr(), batch, 2)] == g1
    assert hip.MSM_RESULT_BYTES % 4 == 0
    got = _finalize(hip, records.data_ptr() + hip.MSM_LOG_OFFSET, batch, hip.MSM_RESULT_BYTES // 4)
    assert [bytes(r) for r in got] == g1
    check_records(hip, records, batch)                     # read only


@pytest.mark.parametrize("count", (1, 8, 16))
def test_combine_sums_above_the_group_order(hip, oracle, count):
    import torch
    ks = [101 - (i % 3) for i in range(count)]
    assert count == 1 or sum(ks) > 102
    logs = torch.tensor(ks, dtype=torch.int32, device=_dev())
    out = torch.full((3 + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    hip.msm_combine_dev(logs, count, out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert bytes(host[:3]) == oracle.dlog_exp(sum(ks) % 102)
    assert (host[3:] == POISON).all()


def _strided_predicate(ps_list, ss_list):
    """gpu_ops.partials' own test for "one launch": constant positive strides"""
    ps, ss = ps_list[1] - ps_list[0], ss_list[1] - ss_list[0]
    return ps > 0 and ss > 0 and all(p == ps_list[0] + b * ps for b, p in enumerate(ps_list)) and \
        all(s == ss_list[0] + b * ss for b, s in enumerate(ss_list))


def test_gpu_ops_partials_strided_and_per_row(hip, rows5):
    """views of one buffer (one batched launch) and separately allocated rows (msm_g1_dev per row)
    give the same partials tensor, the oracle's logs; sharded_msm with no group gives its bytes"""
    import torch
    rows, want = rows5
    n = SHAPE_A
    ops = dist.gpu_ops(hip)
    bp = _upload(np.stack([p.reshape(-1) for p, _ in rows]))
    bs = _upload(np.stack([s for _, s in rows]))
    vp = [bp[3 * n * b:3 * n * (b + 1)] for b in range(5)]
    vs = [bs[n * b:n * (b + 1)] for b in range(5)]
    assert _strided_predicate([t.data_ptr() for t in vp], [t.data_ptr() for t in vs])
    # separately allocated, with spacers of growing size between them: no constant stride
    keep, sp, ss = [], [], []
    for b, (p, s) in enumerate(rows):
        sp.append(_upload(p))
        keep.append(torch.empty(4096 * (b + 1) * (b + 1), dtype=torch.uint8, device=_dev()))
        ss.append(_upload(s))
    assert not _strided_predicate([t.data_ptr() for t in sp], [t.data_ptr() for t in ss])
    a = ops.partials(vp, vs)
    b = ops.partials(sp, ss)
    torch.cuda.synchronize()
    assert a.dtype == torch.int32 and tuple(a.shape) == (5, 2)
    assert a.cpu().numpy().tolist() == [[w[1], 0] for w in want]
    assert torch.equal(a, b)
    for shards in ((vp, vs), (sp, ss)):
        out, folded = dist.sharded_msm(shards[0], shards[1], n, ops)
        assert folded == 0 and dist.g1_bytes(out) == [w[0] for w in want]
        assert not out[:, 3].any()
    # one row: the batch == 1 branch
    assert ops.partials(sp[2:3], ss[2:3]).cpu().numpy().tolist() == [[want[2][1], 0]]


@pytest.mark.parametrize("world", (2, 3, 8))
def test_simulated_world_on_one_gpu(hip, oracle, rows_a, world):
    """point-range shards of 6 rows, one "rank" after the other on one GPU: the partials added on
    the device, exp of the sum = the whole row's fold; an irregular point in the last rank's range
    raises the summed irregular column for its row only"""
    import torch
    n = SHAPE_A
    rows = [(p.copy(), s.copy()) for p, s in rows_a["rows"][:6]]
    flagged = 4
    lo_last, _ = dist.shard_range(n, world - 1, world)
    rows[flagged][0][lo_last + 11] = (3, 3, 0)
    rows[flagged][1][lo_last + 11] = 9
    ops = dist.gpu_ops(hip)
    total = torch.zeros((6, 2), dtype=torch.int32, device=_dev())
    per_rank_irr = []
    for rank in range(world):
        lo, hi = dist.shard_range(n, rank, world)
        m = hi - lo
        bp = _upload(np.stack([p[lo:hi].reshape(-1) for p, _ in rows]))
        bs = _upload(np.stack([s[lo:hi] for _, s in rows]))
        part = ops.partials([bp[3 * m * b:3 * m * (b + 1)] for b in range(6)],
                            [bs[m * b:m * (b + 1)] for b in range(6)])
        per_rank_irr.append(part[:, 1].cpu().numpy().tolist())
        total += part
    host = total.cpu().numpy()
    assert [b for b in range(6) if host[b, 1] != 0] == [flagged]
    assert all(not any(irr) for irr in per_rank_irr[:-1])
    out = ops.exp(total[:, 0] % dist.GROUP_ORDER)
    got = dist.g1_bytes(out)
    for b in range(6):
        if b != flagged:
            assert got[b] == rows_a["want"][b][0], (world, b)
    assert ops.fold(_upload(rows[flagged][0]), _upload(rows[flagged][1])) == oracle.msm(*rows[flagged])
