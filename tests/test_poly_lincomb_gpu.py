"""plk_poly_lincomb / plk_poly_lincomb_batch_dev on the GPU.

Expected bytes come from the numpy statement of the specification (tests/poly_lincomb_model.py, pinned to the
reference's recorded outputs by tests/test_poly_lincomb_cpu.py) and from those recorded outputs themselves
(tests/golden/poly_lincomb.json) replayed through the device.  Everything is exact: out and d_nz are compared
for equality, and the guard bytes on both sides of every output must be unchanged."""
import numpy as np
import pytest

import gen
import make_poly_lincomb_golden as mk
import poly_lincomb_model as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

RAW = M.RAW
BLOCK = 4096           # result bytes per block (csrc/lincomb.hip LC_CHUNK)
LAUNCH_JOBS, LAUNCH_TERMS = 24, 48   # csrc/lincomb.hip LC_JOBS, LC_TERMS
GUARD = 48
FILL = 0xA5
LENGTHS = [1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5]
OFFSETS = [0, 1, 15]


def rnd(seed, n, wild=False):
    """n canonical bytes (wild: arbitrary bytes), a pure function of the seed"""
    r = (gen.splitmix64(seed, n) >> np.uint64(11))
    return (r % np.uint64(256 if wild else 17)).astype(np.uint8)


def dev_buf(data, off):
    """(tensor, pointer): the bytes on the device, starting off bytes past a 16-byte boundary"""
    import torch
    data = np.ascontiguousarray(data, np.uint8)
    t = torch.empty(data.size + 32, dtype=torch.uint8, device="cuda")
    start = (-t.data_ptr()) % 16 + off
    t[start:start + data.size] = torch.from_numpy(data.copy()).cuda()
    return t, t.data_ptr() + start


def out_buf(L, off):
    """(tensor, pointer, start): L result bytes off bytes past a 16-byte boundary, guards all round"""
    import torch
    t = torch.full((L + 2 * GUARD + 32,), FILL, dtype=torch.uint8, device="cuda")
    start = (-t.data_ptr()) % 16 + GUARD + off
    return t, t.data_ptr() + start, start


NZ_GUARD = 0x5EADBEEF


def prepare(hip, jobs, in_off=0, out_off=0, want_nz=True):
    """upload the jobs' polynomials -> (call list, output buffers, nz words or None, tensors to keep)"""
    import torch
    keep, call, outs = [], [], []
    for terms, add_hf in jobs:
        dt = []
        for t in terms:
            buf, ptr = dev_buf(t["p"], in_off)
            keep.append(buf)
            dt.append(hip.lc_term(ptr, len=len(t["p"]), shift=t["shift"], sub=t["sub"], scale=t["scale"], neg=t["neg"],
                                  twist=t["twist"]))
        L = M.length(terms)
        ob, optr, start = out_buf(L, out_off)
        outs.append((ob, start, L))
        call.append((dt, add_hf, optr))
    nz = torch.full((len(jobs) + 2,), NZ_GUARD, dtype=torch.int32, device="cuda") if want_nz else None
    return call, outs, nz, keep


def launch(hip, prep, stream=None):
    call, outs, nz, _ = prep
    hip.poly_lincomb_batch_dev(call, None if nz is None else nz.data_ptr() + 4, stream=stream)


def run_dev(hip, jobs, in_off=0, out_off=0, want_nz=True):
    """jobs: [(terms, add_hf)] with numpy / list coefficients -> ([result bytes], [nz words] or None)"""
    prep = prepare(hip, jobs, in_off, out_off, want_nz)
    launch(hip, prep)
    return collect(prep[1], prep[2])


def collect(outs, nz):
    import torch
    torch.cuda.synchronize()
    res = []
    for ob, start, L in outs:
        h = ob.cpu().numpy()
        assert (h[:start] == FILL).all() and (h[start + L:] == FILL).all(), "guard bytes changed"
        res.append(h[start:start + L].copy())
    if nz is None:
        return res, None
    w = nz.cpu().numpy()
    assert w[0] == NZ_GUARD and w[-1] == NZ_GUARD
    return res, [int(v) for v in w[1:-1]]


def check(hip, jobs, **kw):
    outs, nz = run_dev(hip, jobs, **kw)
    for b, (terms, add_hf) in enumerate(jobs):
        want = M.lincomb(terms, add_hf)
        assert np.array_equal(outs[b], want), (b, np.flatnonzero(outs[b] != want)[:8])
        if nz is not None:
            assert nz[b] == M.nz(want), (b, nz[b], M.nz(want))


@pytest.fixture(scope="module")
def golden():
    return mk.expand(load_golden("poly_lincomb.json"))


def test_golden_host_form(hip, golden):
    for g, (terms, add_hf, ref) in enumerate(golden):
        out, n = hip.poly_lincomb(([hip.lc_term(t["p"], shift=t["shift"], sub=t["sub"], scale=t["scale"], neg=t["neg"],
                                                twist=t["twist"]) for t in terms], add_hf))
        assert n == len(ref) and out[:n] == ref and not any(out[n:]), g
        assert len(out) == M.length(terms)


def test_golden_dev_one_batch(hip, golden):
    jobs = [(terms, add_hf) for terms, add_hf, _ in golden]
    assert len(jobs) > LAUNCH_JOBS and sum(len(t) for t, _ in jobs) > LAUNCH_TERMS
    outs, nz = run_dev(hip, jobs, in_off=3, out_off=5)
    for g, (terms, add_hf, ref) in enumerate(golden):
        n = max(nz[g], 1)
        assert bytes(outs[g][:n]) == ref and not outs[g][n:].any(), g
        assert nz[g] == (0 if ref == b"\0" else len(ref)), g


# ---- edge lengths x shifts x term counts x base pointers
def edge_jobs():
    jobs = []
    seed = 1000
    for ln in LENGTHS:
        for shift in (0, 1, 15, 16, 17, 4096, "gap"):
            for k in (1, 2, 16):
                seed += 1
                sh = ln + 37 if shift == "gap" else shift      # gap: past every other term's end
                wild = seed % 2 == 0
                terms = [M.term(rnd(seed, ln, wild), shift=sh if k == 1 else 0)]
                for i in range(1, k):
                    li = ln if i == 1 else 1 + (ln * (i + 3)) // 19 % ln
                    scale = RAW if i % 3 == 1 else (5 * i) % 17
                    terms.append(M.term(rnd(seed * 100 + i, li, wild and i % 2 == 1), shift=sh if i == 1 else (i * 7) % 23,
                                        sub=i % 2, scale=scale, neg=(i // 2) % 2, twist=(3 * i) % 17 if i % 4 == 2 else 0))
                jobs.append((terms, seed % 17 if seed % 3 else None))
    return jobs


@pytest.fixture(scope="module")
def edges():
    jobs = edge_jobs()
    return jobs, [M.lincomb(t, a) for t, a in jobs]


@pytest.mark.parametrize("out_off", OFFSETS)
@pytest.mark.parametrize("in_off", OFFSETS)
def test_edges(hip, edges, in_off, out_off):
    jobs, want = edges
    assert len(jobs) == 8 * 7 * 3
    outs, nz = run_dev(hip, jobs, in_off=in_off, out_off=out_off)
    for b in range(len(jobs)):
        assert np.array_equal(outs[b], want[b]), (b, np.flatnonzero(outs[b] != want[b])[:8])
        assert nz[b] == M.nz(want[b]), b


# ---- raw bytes >= 17 at the edges of a group, a block, the polynomial
@pytest.mark.parametrize("out_off", [0, 1])
def test_noncanonical_positions(hip, out_off):
    L = 3 * BLOCK + 5
    base = [rnd(71, L), rnd(72, L - 9), rnd(73, L)]
    spots = [0, 15, 16, 31, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK, 3 * BLOCK - 1, 3 * BLOCK, L - 1]
    spots += [s - out_off for s in (16, 32, BLOCK, 2 * BLOCK) if out_off]      # the groups are cut on out's address
    jobs = []
    for which, val in ((0, 17), (2, 255), (0, 128), (2, 200)):
        for s in spots:                                 # one group alone takes the slow path
            p = [b.copy() for b in base]
            p[which][s] = val
            jobs.append(([M.term(p[0]), M.term(p[1], shift=9, scale=7, sub=1), M.term(p[2], neg=1)], 4))
    p = [b.copy() for b in base]
    for s in spots:                                     # and all of them at once, in both raw terms
        p[0][s], p[2][s] = 17 + s % 200, 255 - s % 100
    jobs.append(([M.term(p[0]), M.term(p[1], shift=9, scale=7, sub=1), M.term(p[2], neg=1)], None))
    jobs.append(([M.term(rnd(74, L, True)), M.term(rnd(75, L, True), sub=1), M.term(rnd(76, L, True), shift=3)], 0))
    check(hip, jobs, out_off=out_off)


# ---- every scale, twist, flag and add_hf
def test_every_scale_neg_sub(hip):
    a, w = rnd(81, 70), rnd(82, 61, True)
    jobs = []
    for scale in list(range(17)) + [RAW]:
        for neg in (0, 1):
            for sub in (0, 1):
                jobs.append(([M.term(a), M.term(w, shift=4, sub=sub, scale=scale, neg=neg)], None))
                jobs.append(([M.term(w, scale=scale, neg=neg), M.term(a, sub=sub)], 3))
    check(hip, jobs)


def test_every_twist_wraps_the_period(hip):
    a, w = rnd(83, 75), rnd(84, 50, True)
    jobs = []
    for twist in range(17):
        jobs.append(([M.term(w, twist=twist)], None))
        jobs.append(([M.term(a, shift=5), M.term(w, shift=21, twist=twist, scale=RAW if twist % 2 else 3, sub=twist % 2)], None))
        jobs.append(([M.term(a, twist=twist, scale=11, neg=1, shift=twist)], 16))
    check(hip, jobs, in_off=1, out_off=15)


def test_add_hf(hip):
    a, w = rnd(85, 40), rnd(86, 40, True)
    jobs = []
    for add in [None] + list(range(17)):
        jobs.append(([M.term(a)], add))
        jobs.append(([M.term(w), M.term(a, sub=1)], add))          # slow path: hf_add(x, 0) is not x for x >= 17
        jobs.append(([M.term([3]), M.term([3], sub=1, shift=2)], add))
    for c in range(1, 17):                                          # coefficient 0 made zero
        one = np.zeros(20, np.uint8)
        one[0] = c
        jobs.append(([M.term(one)], 17 - c))
        lead = a.copy()
        lead[0] = c
        jobs.append(([M.term(lead)], 17 - c))
    check(hip, jobs)
    outs, nz = run_dev(hip, jobs[-32::2])
    assert nz == [0] * 16 and not any(o.any() for o in outs)


# ---- the d_nz word
def test_nz_cases(hip):
    L = 3 * BLOCK
    a = rnd(91, L)
    z = np.zeros(L, np.uint8)
    first = z.copy()
    first[7] = 9
    last = z.copy()
    last[L - 1] = 1
    top = a.copy()
    top[2 * BLOCK:] = 0
    top[2 * BLOCK] = 6                 # the top coefficient, first byte of the last block ...
    cancel = z.copy()
    cancel[2 * BLOCK] = 11             # ... cancels exactly at the block boundary
    jobs = [
        ([M.term(a), M.term(a, sub=1)], None),                       # all zero
        ([M.term(a, scale=0)], None),
        ([M.term(first)], None),                                     # only the first block of three holds a byte
        ([M.term(last)], None),                                      # the last byte
        ([M.term(top), M.term(cancel)], None),                       # 6 + 11 = 0 at index 2 BLOCK
        ([M.term(top)], None),
        ([M.term(a)], None),
    ]
    want = [M.lincomb(t, ad) for t, ad in jobs]
    assert [M.nz(w) for w in want[:5]] == [0, 0, 8, L, 2 * BLOCK] and want[4][2 * BLOCK - 1] != 0
    check(hip, jobs)
    check(hip, jobs, out_off=15)
    check(hip, jobs, want_nz=False)                                  # d_nz = NULL


def test_nz_array_reused_without_clearing(hip):
    import torch
    L = 2 * BLOCK + 100
    big, small = rnd(92, L), np.zeros(L, np.uint8)
    small[3] = 5
    nz = torch.zeros(2, dtype=torch.int32, device="cuda")
    res = []
    for polys in ((big, small), (small, np.zeros(L, np.uint8))):
        bufs = [dev_buf(p, 0) for p in polys]
        obs = [out_buf(L, 0) for _ in polys]
        hip.poly_lincomb_batch_dev([([hip.lc_term(b[1], len=L)], None, o[1]) for b, o in zip(bufs, obs)], nz)
        res.append(nz.cpu().numpy().tolist())
    assert res == [[L, 4], [4, 0]]


# ---- accumulation in place
def test_in_place(hip):
    import torch
    L = 2 * BLOCK + 77
    a, b, c = rnd(93, L, True), rnd(94, L - 5), rnd(95, L)
    low = rnd(96, L)
    low[BLOCK - 40:] = 0
    high = low.copy()
    high[:BLOCK - 40] = 0                  # low + high - high: only the first block keeps non-zero bytes
    cases = [([a, b, c], 0, [{}, {"sub": 1}, {"scale": 9}], 2),          # out = term 0's p
             ([b, a, c], 1, [{}, {"sub": 1}, {"scale": 9}], 2),          # out = a middle term's p
             ([low + high, high], 0, [{}, {"sub": 1}], None)]       # out = term 0's p, the top blocks cancel
    for srcs, tgt, kws, add_hf in cases:
        terms = [M.term(p, **kw) for p, kw in zip(srcs, kws)]
        want = M.lincomb(terms, add_hf)
        bufs = [dev_buf(p, 1) for p in srcs]
        nz = torch.zeros(1, dtype=torch.int32, device="cuda")
        dt = [hip.lc_term(bufs[i][1], len=len(srcs[i]), **kws[i]) for i in range(len(srcs))]
        assert len(srcs[tgt]) == L
        hip.poly_lincomb_batch_dev([(dt, add_hf, bufs[tgt][1])], nz)
        torch.cuda.synchronize()
        t, ptr = bufs[tgt]
        start = ptr - t.data_ptr()
        got = t.cpu().numpy()[start:start + L]
        assert np.array_equal(got, want), tgt
        assert int(nz.item()) == M.nz(want)
        for i in range(len(srcs)):      # the other inputs are untouched
            if i != tgt:
                ti, pi = bufs[i]
                s = pi - ti.data_ptr()
                assert np.array_equal(ti.cpu().numpy()[s:s + len(srcs[i])], srcs[i])
    assert M.nz(M.lincomb([M.term(low + high), M.term(high, sub=1)])) <= BLOCK - 40


# ---- more jobs and more terms than one launch carries
def test_batch_beyond_one_launch(hip):
    jobs = []
    for b in range(3 * LAUNCH_JOBS + 5):
        if b % 2:
            jobs.append(([M.term([b % 17])], None if b % 4 == 1 else (17 - b) % 17))     # one byte between long ones
        else:
            k = [16, 3, 9, 16, 1][b // 2 % 5]
            ln = BLOCK + 300 + b
            jobs.append(([M.term(rnd(2000 + 20 * b + i, ln - 3 * i, wild=(b % 6 == 0 and i == 2)), shift=i, sub=i % 2,
                                 scale=RAW if i % 2 == 0 else 1 + i, twist=i if i % 5 == 3 else 0) for i in range(k)], b % 17))
    assert sum(len(t) for t, _ in jobs) > 4 * LAUNCH_TERMS
    check(hip, jobs, in_off=15, out_off=1)


def test_two_streams(hip):
    import torch
    L = 64 * BLOCK + 3
    jobs_a = [([M.term(rnd(96, L)), M.term(rnd(97, L), scale=4, shift=1)], 1)]
    jobs_b = [([M.term(rnd(98, L, True)), M.term(rnd(99, L - 1), sub=1), M.term(rnd(100, L), twist=3)], None)]
    pa, pb = prepare(hip, jobs_a), prepare(hip, jobs_b, in_off=1, out_off=15)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()            # the uploads ran on the default stream
    launch(hip, pa, stream=s1)
    launch(hip, pb, stream=s2)
    for jobs, prep in ((jobs_a, pa), (jobs_b, pb)):
        got, words = collect(prep[1], prep[2])
        want = M.lincomb(*jobs[0])
        assert np.array_equal(got[0], want) and words[0] == M.nz(want)
