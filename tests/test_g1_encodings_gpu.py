"""Every G1 byte encoding through the MSM's decode and raw-fold kernels (plonk.c_amd/csrc/msm.hip).

The canonical / irregular decision is one subtract against the 512-entry table built in capi.hip;
a missed flag crashes nothing, it returns EXP[log] for bytes that are no group element.  Here every
one of the 2^24 encodings is presented to msm_dlog_kernel once (batched rows, the candidate at
position row % 16 among canonical fillers), the encodings one field away from a canonical one
(g1_encoding_cases.near_misses) go to every other kernel that decodes the table, and the raw
arithmetic RawOps::addp / dbl / mulp is observed one addition at a time -- a fold of one pair has
nothing after the addition that could merge a wrong value back -- and at the chunk boundaries of
the long fold.  Everything compares bytes or flags for equality against the oracle
(tests/test_g1_encodings_cpu.py pins the same expectations to the compiled reference).

Records: one shared buffer of 65,536 plk_msm_result_t.  Before a set of launches the output fields
log / irregular / g1 of the records it uses are overwritten with a stale pattern, so a record no
launch completed shows; only those 12 bytes per record are read back (a strided device view).
"""
import numpy as np
import pytest

import g1_encoding_cases as ge

pytestmark = pytest.mark.gpu

MAX_RECORDS = 65536
STALE = 0x5A
POISON = 0xFF                    # every pad byte of a device buffer: a point read from it is irregular


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(_dev())


def _round16(v):
    return (v + 15) & ~15


@pytest.fixture(scope="module")
def records(hip):
    import torch
    return torch.zeros(MAX_RECORDS * hip.MSM_RESULT_BYTES, dtype=torch.uint8, device=_dev())


def _arm(hip, records, m):
    assert m <= MAX_RECORDS
    records.view(MAX_RECORDS, hip.MSM_RESULT_BYTES)[:m, hip.MSM_LOG_OFFSET:hip.MSM_G1_OFFSET + 4] = STALE


def _fields(hip, records, m):
    """(log, irregular, g1 (m, 3)) of the first m records: 12 bytes each cross the bus"""
    import torch
    torch.cuda.synchronize()
    v = records.view(MAX_RECORDS, hip.MSM_RESULT_BYTES)[:m, hip.MSM_LOG_OFFSET:hip.MSM_G1_OFFSET + 4]
    h = v.contiguous().cpu().numpy()
    return h[:, 0:4].copy().view("<u4").reshape(-1), h[:, 4:8].copy().view("<u4").reshape(-1), h[:, 8:11]


def _rows_on_device(pts, sc, off):
    """rows of n points at a 16-byte multiple stride, the bases `off` bytes past a 16-byte boundary,
    POISON everywhere else.  (points tensor, scalars tensor, points stride, scalars stride)"""
    m, n = sc.shape
    ps, ss = _round16(3 * n), _round16(n)
    hp = np.full((m, ps), POISON, np.uint8)
    hs = np.full((m, ss), POISON, np.uint8)
    hp[:, :3 * n] = pts.reshape(m, 3 * n)
    hs[:, :n] = sc
    pad = np.full(64, POISON, np.uint8)
    dp = _up(np.concatenate([pad[:off], hp.reshape(-1), pad]))
    ds = _up(np.concatenate([pad[:off], hs.reshape(-1), pad]))
    assert dp.data_ptr() % 16 == 0 and ds.data_ptr() % 16 == 0
    return dp, ds, ps, ss


def _assert_decode(got, irregular, logs, g1, ctx):
    glog, girr, gg1 = got
    bad = np.flatnonzero((girr > 0) != irregular)
    assert bad.size == 0, (ctx, "irregular flag wrong at rows", bad[:8].tolist(), girr[bad[:8]].tolist())
    assert (girr <= 1).all(), (ctx, "irregular is 0 or 1")
    reg = ~irregular
    assert np.array_equal(glog[reg], logs[reg]), (ctx, "log")
    assert np.array_equal(gg1[reg], g1[reg]), (ctx, "g1")


# ------------------------------------------------------------------ decode, exhaustive (batched form)
def _sweep(hip, oracle, records, flag, half, n=16, off=0):
    import torch
    pts, sc, irregular, logs, g1 = ge.sweep_rows(oracle, flag, half, n)
    rows = ge.SWEEP_ROWS
    plan = hip.msm_plan(n, rows, aligned=(off == 0))
    assert (plan["threads"], plan["blocks"], plan["half"]) == (256, 1, 0), plan     # one block per row
    dp, ds, ps, ss = _rows_on_device(pts, sc, off)
    _arm(hip, records, rows)
    hip.msm_g1_batch_dev(dp.data_ptr() + off, ps, ds.data_ptr() + off, ss, n, rows, records,
                         torch.cuda.current_stream())
    _assert_decode(_fields(hip, records, rows), irregular, logs, g1, (flag, half, n, off))
    return int((~irregular).sum())


@pytest.mark.parametrize("f0", range(0, 256, 16))
def test_decode_every_encoding(hip, oracle, records, f0):
    """all 2^16 (x, y) of 16 flag bytes: 32 launches of 32,768 rows, 2^20 encodings per item, 2^24 in all"""
    regular = sum(_sweep(hip, oracle, records, flag, half) for flag in range(f0, f0 + 16) for half in (0, 1))
    assert regular == (102 if f0 == 0 else 0)


@pytest.mark.parametrize("flag", [0, 1])
def test_decode_every_encoding_bytewise(hip, oracle, records, flag):
    """the byte-wise form of the kernel: the bases one byte past a 16-byte boundary"""
    assert sum(_sweep(hip, oracle, records, flag, half, off=1) for half in (0, 1)) == (101, 1)[flag]


@pytest.mark.parametrize("flag", [0, 1])
def test_decode_every_encoding_in_the_tail(hip, oracle, records, flag):
    """n = 21: one full group of fillers, the candidate among the 5 tail points at row % 5"""
    assert sum(_sweep(hip, oracle, records, flag, half, n=21) for half in (0, 1)) == (101, 1)[flag]


# ------------------------------------------------ decode, near-misses on the other paths
def _cycled(n):
    """(candidates, positions): the control and near_misses() with the position cycling over the
    list, then SPECIAL_POINTS and their near-misses at every position"""
    base = ge.control_and_near_misses()
    sp = ge.special_candidates()
    cands = np.concatenate([base, np.repeat(sp, n, axis=0)])
    pos = np.concatenate([np.arange(len(base)) % n, np.tile(np.arange(n), len(sp))])
    return cands, pos


@pytest.mark.parametrize("n,off", [(16, 0), (16, 1), (40, 0), (40, 1)])
def test_near_misses_single_launch(hip, oracle, records, n, off):
    """plk_msm_g1_dev, one launch and one record per candidate: the half-group form (aligned) and
    the byte-wise form; n = 40 is two groups (four half groups) and an 8-point tail"""
    import torch
    plan = hip.msm_plan(n, 1, aligned=(off == 0))
    assert plan["half"] == (1 if off == 0 else 0), plan
    cands, pos = _cycled(n)
    pts, sc = ge.placed("single", cands, n, pos)
    irregular, logs, g1 = ge.expected_decode(oracle, pts, sc)
    assert np.array_equal(irregular, ~ge.canonical_mask(cands))
    m = len(cands)
    dp, ds, ps, ss = _rows_on_device(pts, sc, off)
    _arm(hip, records, m)
    st = torch.cuda.current_stream().cuda_stream
    p0, s0, r0, R = dp.data_ptr() + off, ds.data_ptr() + off, records.data_ptr(), hip.MSM_RESULT_BYTES
    for i in range(m):
        hip.msm_g1_dev(p0 + i * ps, s0 + i * ss, n, r0 + i * R, st)
    _assert_decode(_fields(hip, records, m), irregular, logs, g1, (n, off))
    print("near-miss single launches n=%d off=%d: %d (%d irregular)" % (n, off, m, int(irregular.sum())))


@pytest.mark.parametrize("n", [1, 16, 17])
def test_near_misses_host_msm(hip, oracle, n):
    """plk_msm_g1 from host buffers: the flag makes it take the raw fold, whose bytes are the oracle's"""
    cands, pos = _cycled(n)
    pts, sc = ge.placed("host/%d" % n, cands, n, pos)
    want = oracle.msm_many(pts, sc)
    for i in range(len(cands)):
        assert hip.msm_g1(pts[i], sc[i]) == bytes(want[i]), (n, i, cands[i].tolist(), int(pos[i]))


@pytest.mark.parametrize("part", range(4))
def test_near_misses_srs_flag(hip, part):
    """srs_log_kernel: a 118-point SRS (7 groups and 6) holding one near-miss is irregular"""
    nm = ge.near_misses()
    for i in range(part, len(nm), 4):
        with hip.Srs(ge.srs_with(nm[i], i % 118)) as s:
            assert s.irregular and len(s) == 118, (i, nm[i].tolist())
    for j, c in enumerate(ge.special_candidates()[3:]):
        for pos in range(part, 118, 4 * 3):
            with hip.Srs(ge.srs_with(c, pos)) as s:
                assert s.irregular, (c.tolist(), pos)


def test_canonical_srs_rotations_and_unit_commits(hip):
    """the 102 canonical points at each rotation mod 16: not irregular, and the commitment of the
    unit vector e_i over the log form is point i's own 3 bytes"""
    units = [np.concatenate([np.zeros(i, np.uint8), np.ones(1, np.uint8)]) for i in range(102)]
    for rot in range(16):
        pts = np.roll(ge.GROUP, rot, axis=0)
        with hip.Srs(pts) as s:
            assert not s.irregular, rot
            assert hip.kzg_commit(s, units) == [bytes(p) for p in pts], rot


def _serial_each(hip, records, pts, sc):
    """one plk_msm_g1_serial_dev per row of pts (m, n, 3) / sc (m, n), all on one stream, each with
    its own record; one synchronisation; the g1 bytes (m, 3)"""
    import torch
    m, n = sc.shape
    dp, ds = _up(pts), _up(sc)
    _arm(hip, records, m)
    st = torch.cuda.current_stream().cuda_stream
    p0, s0, r0, R = dp.data_ptr(), ds.data_ptr(), records.data_ptr(), hip.MSM_RESULT_BYTES
    for i in range(m):
        hip.msm_g1_serial_dev(p0 + 3 * n * i, s0 + n * i, n, r0 + i * R, st)
    return _fields(hip, records, m)[2]


def _assert_bytes(got, want, describe):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, ("%d of %d differ" % (bad.size, len(want)),
                           [(describe(i), bytes(got[i]).hex(), bytes(want[i]).hex()) for i in bad[:6]])


@pytest.mark.parametrize("k", range(4))
def test_near_misses_fold_prefix(hip, oracle, records, k):
    """msm_fold_prefix_kernel (n = 9,000 takes the chunked fold): a canonical input with one
    candidate at index PREFIX_POS[k] -- the first point, either side of 4,096, the last"""
    base = ge.control_and_near_misses()[k::4]
    cands = np.concatenate([base, ge.special_candidates()])
    pts, sc = ge.prefix_cases(cands, np.full(len(cands), ge.PREFIX_POS[k]))
    assert sc.shape[1] >= ge.FOLD_CHUNKED_MIN
    got = _serial_each(hip, records, pts, sc)
    _assert_bytes(got, oracle.msm_many(pts, sc), lambda i: (cands[i].tolist(), ge.PREFIX_POS[k]))
    print("fold-prefix inputs at index %d: %d" % (ge.PREFIX_POS[k], len(cands)))


# ------------------------------------------------------ raw arithmetic, one pair per fold
@pytest.fixture(scope="module")
def mul_family(oracle):
    return ge.pairs_mul(oracle)


def _check_family(hip, records, fam, lo=0, hi=None):
    A, T, c, want = (a[lo:hi] for a in fam)
    pts, sc = ge.pair_folds((A, T, c, want))
    got = _serial_each(hip, records, pts, sc)
    _assert_bytes(got, want, lambda i: (A[i].tolist(), T[i].tolist(), int(c[i])))
    return len(want)


def test_pair_folds_same_x(hip, oracle, records):
    """msm_serial_fold_kernel on [A, 1], [T, 1] with a.x == b.x: 15,463 folds"""
    assert _check_family(hip, records, ge.pairs_same_x(oracle)) == 15463


@pytest.mark.parametrize("which", [0, 1])
def test_pair_folds_chord(hip, oracle, records, which):
    """all 65,536 (a.x, b.x) at one (a.y, b.y): 65,536 folds"""
    assert _check_family(hip, records, ge.pairs_chord(oracle, which)) == 65536


def test_pair_folds_flags(hip, oracle, records):
    """flag bytes {0, 1, 2, 255} on both operands: 1,600 folds"""
    assert _check_family(hip, records, ge.pairs_flags(oracle)) == 1600


@pytest.mark.parametrize("part", range(6))
def test_pair_folds_mul(hip, records, mul_family, part):
    """g1_mul(T, c) alone (n = 1) for the canonical points and the near-misses at every scalar byte:
    340,480 folds in parts of at most 65,536"""
    total = len(mul_family[0])
    assert 5 * MAX_RECORDS < total <= 6 * MAX_RECORDS
    n = _check_family(hip, records, mul_family, part * MAX_RECORDS, min(total, (part + 1) * MAX_RECORDS))
    assert n == min(MAX_RECORDS, total - part * MAX_RECORDS)


# ------------------------------------------------------ raw arithmetic at chunk boundaries
@pytest.fixture(scope="module")
def boundary():
    return ge.boundary_cases()


@pytest.mark.parametrize("part", range(8))
def test_chunk_boundary_states(hip, oracle, records, boundary, part):
    """msm_fold_chunk_kernel / msm_fold_resolve_kernel at n = 8192 (four chunks of 2048): the state S
    crosses into a chunk whose first term is T_j; an eighth of the 1,012 layouts per item (runs of
    identity terms merge no trajectories, so a layout is the chunk kernel's slow case: ~29 ms)"""
    S, T, c = (a[part::8] for a in boundary)
    pts, sc = ge.boundary_layout(S, T, c)
    got = _serial_each(hip, records, pts, sc)
    _assert_bytes(got, oracle.msm_many(pts, sc), lambda i: (S[i].tolist(), T[i].tolist(), c[i].tolist()))
    print("chunk-boundary layouts: %d" % len(S))


def test_chunk_boundary_states_host_msm(hip, oracle, boundary):
    S, T, c = (a[5::32] for a in boundary)
    assert len(S) == 32
    pts, sc = ge.boundary_layout(S, T, c)
    want = oracle.msm_many(pts, sc)
    for i in range(len(S)):
        assert hip.msm_g1(pts[i], sc[i]) == bytes(want[i]), (S[i].tolist(), T[i].tolist(), c[i].tolist())


def test_chunk_boundary_longer_chunks(hip, oracle, records):
    """n = 2048 * 256 + 1: the first size whose chunks are longer than 2048 (3072 terms)"""
    pts, sc = ge.big_layout()
    want = oracle.msm(pts, sc)
    got = _serial_each(hip, records, pts[None], sc[None])
    assert bytes(got[0]) == want
    assert hip.msm_g1(pts, sc) == want
