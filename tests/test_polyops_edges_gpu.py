"""polyops.hip past toy sizes: the batched poly_eval's block geometry, tickets, job-count and
alignment edges; poly_divide by constants and binomials at the one-thread-per-chain / suffix-scan
switch, the scan-block and carry edges, every multiplier, the gated serial re-run and the trim;
matrix_mul / matrix_inv / interpolate above 17 x 17 and matrix_inv's range errors.

Every result is compared byte for byte with the oracle restatement, which
tests/test_polyops_edges_cpu.py pins to the compiled reference at the very same inputs
(tests/polyops_edge_cases.py); the position weights and M M^-1 = I are checked with plain integers."""
import numpy as np
import pytest

import polyops_edge_cases as pe

pytestmark = pytest.mark.gpu


def _oracle_evals(oracle, polys, xs):
    return [oracle.poly_eval(np.zeros(0, np.uint8) if p is None else p, x) for p, x in zip(polys, xs)]


def _eval_dev(hip, polys, xs, tick):
    """the device form on fresh copies of host arrays (None stays a NULL pointer); returns ys and the
    copies (to be kept until the stream is synchronised)"""
    import torch
    ds = [None if p is None else torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in polys]
    ys = torch.full((len(polys),), 0xEE, dtype=torch.uint8, device="cuda")
    hip.poly_eval_batch_dev(ds, [0 if p is None else p.size for p in polys], xs, ys, tick)
    return ys, ds


# --------------------------------------------------------------------------------- poly_eval
@pytest.mark.parametrize("length", pe.EVAL_GEOMETRY_LENS)
def test_eval_block_geometry(hip, oracle, length):
    """1, 2, 3 blocks, the 64-block cap and the grid stride beyond it, at every kind of x"""
    polys, xs = pe.eval_geometry(length)
    assert hip.poly_eval_batch(polys, xs) == _oracle_evals(oracle, polys, xs)


def test_eval_mixed_lengths_in_one_launch(hip, oracle):
    """short jobs beside a 64-block job: their tickets still count all 64 arrivals"""
    for name, polys, xs in pe.eval_mixed():
        assert hip.poly_eval_batch(polys, xs) == _oracle_evals(oracle, polys, xs), name


@pytest.mark.parametrize("indices", [pe.ONE_HOT_SMALL, pe.ONE_HOT_LARGE], ids=["0..40", "multi_block"])
def test_eval_position_weights(hip, indices):
    """one coefficient 1 at index i evaluates to x^i mod 17 (Python integers, not the oracle)"""
    polys, xs, want = pe.eval_one_hot(indices)
    assert hip.poly_eval_batch(polys, xs) == want


@pytest.mark.parametrize("n", pe.EVAL_JOB_COUNTS + (pe.EVAL_MAPPED_MAX_JOBS,))
def test_eval_job_counts_host(hip, oracle, n):
    """one launch exactly, one job into the second, two launches, one job into the third: short jobs
    (the mapped toy-size path up to 63 jobs, a 256-byte slot each; staged beyond) and 3000-byte jobs
    (staged)"""
    for make in (pe.eval_short_jobs, pe.eval_staged_jobs):
        polys, xs = make(n)
        want = _oracle_evals(oracle, polys, xs)
        assert hip.poly_eval_batch(polys, xs) == want, make.__name__
        with hip.options(TINY_CALLS=0):     # every call staged
            assert hip.poly_eval_batch(polys, xs) == want, make.__name__


@pytest.mark.parametrize("n", pe.EVAL_JOB_COUNTS)
def test_eval_job_counts_dev(hip, oracle, n):
    import torch
    polys, xs = pe.eval_dev_jobs(n)
    nbytes = hip.poly_eval_workspace(n)
    assert nbytes == 128 * n
    guard = 256
    tick = torch.zeros(nbytes + guard, dtype=torch.uint8, device="cuda")
    tick[nbytes:] = 0xEE
    for rep in range(2):   # the launches leave the tick words zero
        ys, _ = _eval_dev(hip, polys, xs, tick)
        torch.cuda.synchronize()
        assert ys.cpu().tolist() == _oracle_evals(oracle, polys, xs)
    th = tick.cpu().numpy()
    assert not th[:nbytes].any() and (th[nbytes:] == 0xEE).all()


def test_eval_host_tick_buffer_grows_and_is_reused(hip, oracle):
    """5 jobs, 70, 5 again (the issue's sequence: 70 short jobs are staged), then 63 -- the most the
    mapped path takes, where the library's own tick buffer grows -- and 5 on the grown buffer"""
    for n in (5, 70, 5, pe.EVAL_MAPPED_MAX_JOBS, 5):
        polys, xs = pe.eval_short_jobs(n)
        assert hip.poly_eval_batch(polys, xs) == _oracle_evals(oracle, polys, xs), n


def test_eval_raw_bytes_four_blocks(hip, oracle):
    """bytes 17..239 on the parallel path, 239 / 240 at index 1, 255 at index 0, one block or every
    block flagging the serial loop; all jobs in one 4-block launch"""
    cases = list(pe.eval_raw_four_blocks())
    assert len(cases) <= pe.EVAL_MAX_JOBS and all(p.size == pe.EVAL_RAW_LEN for _, p, _ in cases)
    polys, xs = [p for _, p, _ in cases], [x for _, _, x in cases]
    got = hip.poly_eval_batch(polys, xs)
    want = _oracle_evals(oracle, polys, xs)
    assert got == want, [name for (name, _, _), g, w in zip(cases, got, want) if g != w]


def test_eval_raw_all_255(hip, oracle):
    polys, xs = pe.eval_raw_all_255()
    assert hip.poly_eval_batch(polys, xs) == _oracle_evals(oracle, polys, xs)


def test_eval_dev_unaligned_pointers(hip, oracle):
    """views of one tensor at byte offsets 1 and 15 (the byte path), len mod 16 in {0, 1, 15}; one
    half of the tensor carries a byte >= 240 (the serial loop from an unaligned pointer)"""
    import torch
    base, jobs = pe.eval_unaligned()
    d = torch.from_numpy(base).cuda()
    assert d.data_ptr() % 16 == 0
    views = [d[off:off + ln] for off, ln, _ in jobs]
    assert {v.data_ptr() % 16 for v in views} == set(pe.EVAL_UNALIGNED_OFFSETS)
    xs = [x for _, _, x in jobs]
    ys = torch.full((len(jobs),), 0xEE, dtype=torch.uint8, device="cuda")
    tick = torch.zeros(hip.poly_eval_workspace(len(jobs)), dtype=torch.uint8, device="cuda")
    hip.poly_eval_batch_dev(views, [ln for _, ln, _ in jobs], xs, ys, tick)
    torch.cuda.synchronize()
    assert ys.cpu().tolist() == [oracle.poly_eval(base[off:off + ln], x) for off, ln, x in jobs]


def test_eval_dev_tick_reuse_across_launches(hip, oracle):
    """one tick buffer, three launches in a row with no synchronisation between them: 64 blocks with
    a flagged job, 1 block clean on the same slots, the first again"""
    import torch
    (big, bx), (small, sx) = pe.eval_tick_reuse()
    tick = torch.zeros(hip.poly_eval_workspace(3), dtype=torch.uint8, device="cuda")
    runs = [_eval_dev(hip, p, x, tick) for p, x in ((big, bx), (small, sx), (big, bx))]
    torch.cuda.synchronize()
    want_big, want_small = _oracle_evals(oracle, big, bx), _oracle_evals(oracle, small, sx)
    assert [ys.cpu().tolist() for ys, _ in runs] == [want_big, want_small, want_big]
    assert not tick.cpu().numpy().any()


def test_eval_dev_null_pointer_with_length_zero(hip, oracle):
    import torch
    polys, xs = pe.eval_null_job()
    assert polys[1] is None
    tick = torch.zeros(hip.poly_eval_workspace(3), dtype=torch.uint8, device="cuda")
    ys, _ = _eval_dev(hip, polys, xs, tick)
    torch.cuda.synchronize()
    assert ys.cpu().tolist() == _oracle_evals(oracle, polys, xs)


# ------------------------------------------------------------------------------- poly_divide
@pytest.mark.parametrize("group", pe.DIVIDE_GROUPS)
def test_divide_host(hip, oracle, group):
    """constant (path 1), binomial (path 2) and trivial (path 0) divisions, host form"""
    n = 0
    for name, num, den, path in pe.divide_groups(oracle)[group]():
        assert hip.poly_divide_path(den, num.size) == path, name
        assert hip.poly_divide(num, den) == oracle.poly_divide(num, den), name
        n += 1
    assert n


def test_divide_exact_leaves_no_remainder(hip, oracle):
    for name, num, den, _ in pe.divide_trim(oracle):
        if "exact" in name:
            q, r = hip.poly_divide(num, den)
            assert r == b"\x00" and len(q) == num.size - den.size + 1, name


@pytest.mark.parametrize("shape", ["short", "long", "constant", "long_raw"])
def test_divide_dev_exact_buffers_dirty_workspace(hip, oracle, shape):
    """the device form writes only the documented sizes (quot nl - dl + 1, rem min(dl - 1, nl)) and
    needs no zeroed workspace: the host form hands it a reused arena"""
    import torch
    num, den = {name: (a, b) for name, a, b in pe.divide_device_shapes()}[shape]
    nl, dl = num.size, den.size
    ql, rl, guard = nl - dl + 1, min(dl - 1, nl), 64
    wl = hip.poly_divide_workspace(nl, dl)
    q = torch.full((ql + guard,), 0xEE, dtype=torch.uint8, device="cuda")
    r = torch.full((rl + guard,), 0xEE, dtype=torch.uint8, device="cuda")
    lens = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    work = torch.full((wl + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_num = torch.from_numpy(num).cuda()
    hip.poly_divide_dev(d_num, nl, den, q, r, lens, work)
    torch.cuda.synchronize()
    qh, rh = q.cpu().numpy(), r.cpu().numpy()
    assert (qh[ql:] == 0xEE).all() and (rh[rl:] == 0xEE).all() and (work.cpu().numpy()[wl:] == 0xA5).all()
    assert bytes(d_num.cpu().numpy()) == bytes(num)
    want = oracle.poly_divide(num, den)
    assert hip.poly_divide(num, den) == want
    lq, lr = lens.cpu().tolist()
    assert (lq, lr) == (len(want[0].rstrip(b"\x00")), len(want[1].rstrip(b"\x00")))
    assert bytes(qh[:max(lq, 1)]) == want[0]
    assert bytes(rh[:max(lr, 1)] if rl else b"") == want[1]


# ---------------------------------------------------------------------------------- matrices
@pytest.mark.parametrize("shape", pe.MATRIX_MUL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matrix_mul_shapes(hip, oracle, shape):
    m, k, n = shape
    a, b = pe.matrix_mul_case(m, k, n)
    got = hip.matrix_mul(a, m, k, b, n)
    assert got == oracle.matrix_mul(a, m, k, b, n)
    if k == 0:
        assert got == bytes(m * n)


@pytest.mark.parametrize("n", pe.MATRIX_INV_SIZES)
def test_matrix_inv_sizes(hip, oracle, n):
    """the 2n-column loops stride past 256 threads from n = 129, the row and multiplier loops from
    n = 257; swaps at every step, a skipped lead, and the stop inside the identity half"""
    for variant in pe.MATRIX_INV_VARIANTS:
        mat = pe.matrix_inv_case(n, variant)
        got = hip.matrix_inv(mat, n)
        assert got == oracle.matrix_inv(mat, n), variant
        if variant in ("lu", "permutation"):
            a = mat.reshape(n, n).astype(np.int64)
            inv = np.frombuffer(got, np.uint8).reshape(n, n).astype(np.int64)
            assert inv.max() < 17 and (a @ inv % 17 == np.eye(n, dtype=np.int64)).all(), variant


def test_matrix_inv_range_errors(hip):
    for at in (0, 12, 24):
        for byte in (17, 255):
            mat = np.eye(5, dtype=np.uint8).reshape(-1)
            mat[at] = byte
            with pytest.raises(hip.PlonkHipError) as e:
                hip.matrix_inv(mat, 5)
            assert e.value.code == hip.PLK_ERR_RANGE, (at, byte)
    with pytest.raises(hip.PlonkHipError) as e:
        hip.matrix_inv(np.eye(1025, dtype=np.uint8).reshape(-1), 1025)
    assert e.value.code == hip.PLK_ERR_RANGE
    # the library is usable after both errors
    eye = np.eye(5, dtype=np.uint8).reshape(-1)
    assert hip.matrix_inv(eye * 2, 5) == bytes(eye * 9)     # 2 * 9 = 18 = 1 mod 17


@pytest.mark.parametrize("n,variant", pe.INTERPOLATE_CASES)
def test_interpolate_sizes(hip, oracle, n, variant):
    mat, v = pe.interpolate_case(n, variant)
    want = pe.trimmed(oracle.matrix_mul(mat, n, n, v, 1))
    assert hip.interpolate(mat, v) == want
    if variant == "tail_rows_zero":
        assert len(want) <= n - 40
    if variant == "zero":
        assert want == b"\x00"
