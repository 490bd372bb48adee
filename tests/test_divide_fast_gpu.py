"""poly_divide by general divisors through the Newton inverse over the exact products
against the oracle restatement of the reference's loop (src/poly.h:124-177; itself pinned to the
compiled reference): bytes and trimmed lengths must be identical.  Every case first asserts that
plk_poly_divide_path reports the Newton path, so nothing here spins the one-thread loop on a large
shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEWTON = 4
B0 = 1024   # polyops.hip INV_B0: the base inverse's size, the first Newton step starts there


def _inputs(seed, nl, dl, lead=None):
    """canonical numerator, general canonical divisor (a non-zero middle term, non-zero lead)"""
    rng = np.random.default_rng(seed)
    num = rng.integers(0, 17, nl).astype(np.uint8)
    den = rng.integers(0, 17, dl).astype(np.uint8)
    den[1] = int(rng.integers(1, 17))
    den[-1] = int(rng.integers(1, 17)) if lead is None else lead
    return num, den


def _fast(hip, num, den):
    assert hip.poly_divide_path(den, len(num)) == NEWTON, (len(num), len(den))
    return hip.poly_divide(num, den)


def _check(hip, oracle, num, den, note=None):
    got = _fast(hip, num, den)
    want = oracle.poly_divide(num, den)
    assert got == want, note if note is not None else (len(num), len(den))
    return got


@pytest.fixture()
def forced(hip):
    with hip.options(DIVIDE_FAST_MIN=1):
        yield hip


@pytest.mark.parametrize("nl,dl", [(3, 3), (4, 3), (5, 3), (7, 4), (40, 17), (100, 3)])
def test_tiny_shapes(forced, oracle, nl, dl):
    for seed in range(4):
        num, den = _inputs(100 * nl + seed, nl, dl)
        _check(forced, oracle, num, den)


@pytest.mark.parametrize("k", [B0 - 1, B0, B0 + 1, 2 * B0 - 1, 2 * B0, 2 * B0 + 1])
@pytest.mark.parametrize("dl", [37, 3000])
def test_base_size_and_first_step_edges(forced, oracle, k, dl):
    num, den = _inputs(k + dl, k + dl - 1, dl)
    q, _ = _check(forced, oracle, num, den)
    assert len(q) == k or num[-1] == 0


@pytest.mark.parametrize("nl,dl", [(5000, 1500), (1500 + 37, 1500), (3001, 1500), (9000, 5)])
def test_k_not_a_power_of_two(forced, oracle, nl, dl):
    """k >> m, k << m, k ~ m"""
    num, den = _inputs(nl ^ dl, nl, dl)
    _check(forced, oracle, num, den)


def test_zero_structure(forced, oracle):
    nl, dl = 2600, 700   # k = 1901: the base inverse and one (clipped) Newton step
    num, den = _inputs(7, nl, dl)
    d = den.copy()
    d[0] = 0
    _check(forced, oracle, num, d, "den[0] = 0")
    d = den.copy()
    d[:20] = 0
    d[300] = 4
    _check(forced, oracle, num, d, "low zeros in the divisor")
    d = den.copy()
    d[-21:-1] = 0
    _check(forced, oracle, num, d, "zeros below the lead")
    n = num.copy()
    n[-30:] = 0
    q, _ = _check(forced, oracle, n, den, "numerator with zero top bytes")
    assert len(q) == nl - dl + 1 - 30 or n[-31] == 0
    z = np.zeros(nl, np.uint8)
    assert _check(forced, oracle, z, den, "zero numerator") == (b"\x00", b"\x00")
    for lead in (1, 16):
        n2, d2 = _inputs(20 + lead, nl, dl, lead=lead)
        _check(forced, oracle, n2, d2, "lead %d" % lead)


def test_exact_division(forced, oracle):
    rng = np.random.default_rng(21)
    q = rng.integers(1, 17, 1901).astype(np.uint8)
    _, den = _inputs(22, 10, 700)
    num = np.frombuffer(oracle.poly_mul(q, den), np.uint8)
    gq, gr = _check(forced, oracle, num, den)
    assert gq == bytes(q) and gr == b"\x00"   # rem_len 1 on the host form


@pytest.mark.parametrize("pos", [0, 20, 39, 300, 599])
def test_non_canonical_numerator(forced, oracle, pos):
    """a numerator byte >= 17 (first, last, a middle one; 20 / 39: the remainder kernel's wide part
    and the reversal's tail -- k = 561 is no multiple of 16 or 64) flags the run and the finish
    kernel re-runs the reference's loop: raw-byte results equal the oracle's"""
    nl, dl = 600, 40
    num, den = _inputs(31, nl, dl)
    for byte in (17, 200):
        n = num.copy()
        n[pos] = byte
        _check(forced, oracle, n, den, (pos, byte))


def _device_divide(hip, num, den, guard=64):
    import torch
    nl, dl = len(num), len(den)
    ql, rl = nl - dl + 1, dl - 1
    d_num = torch.zeros(nl + 1, dtype=torch.uint8, device="cuda")
    d_num[1:] = torch.from_numpy(np.ascontiguousarray(num)).cuda()
    d_num = d_num[1:]                                    # an odd device address
    assert d_num.data_ptr() % 2 == 1
    q = torch.full((ql + guard,), 0xEE, dtype=torch.uint8, device="cuda")
    r = torch.full((rl + guard,), 0xEE, dtype=torch.uint8, device="cuda")
    lens = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    ws = hip.poly_divide_workspace(nl, dl)
    work = torch.full((ws + guard,), 0xEE, dtype=torch.uint8, device="cuda")
    assert hip.poly_divide_path(den, nl) == NEWTON
    hip.poly_divide_dev(d_num, nl, den, q, r, lens, work)
    torch.cuda.synchronize()
    qh, rh, wh = q.cpu().numpy(), r.cpu().numpy(), work.cpu().numpy()
    assert (qh[ql:] == 0xEE).all() and (rh[rl:] == 0xEE).all() and (wh[ws:] == 0xEE).all()
    return qh[:ql], rh[:rl], lens.cpu().tolist()


@pytest.mark.parametrize("nl,dl", [(7, 4), (2600, 700), (5000, 1500), (1537, 1500)])
def test_device_form_exact_buffers(forced, oracle, nl, dl):
    num, den = _inputs(nl + dl, nl, dl)
    q, r, (lq, lr) = _device_divide(forced, num, den)
    wq, wr = oracle.poly_divide(num, den)
    assert bytes(q[:max(lq, 1)]) == wq and bytes(r[:max(lr, 1)]) == wr
    assert lq == len(wq.rstrip(b"\x00")) and lr == len(wr.rstrip(b"\x00"))
    assert not q[lq:].any() and not r[lr:].any()


def test_device_form_exact_division_and_raw_numerator(forced, oracle):
    rng = np.random.default_rng(41)
    qq = rng.integers(1, 17, 561).astype(np.uint8)
    _, den = _inputs(42, 10, 40)
    num = np.frombuffer(oracle.poly_mul(qq, den), np.uint8).copy()
    q, r, lens = _device_divide(forced, num, den)
    assert bytes(q) == bytes(qq) and lens == [561, 0] and not r.any()
    num[77] = 130                                        # the gated loop writes the same exact sizes
    q, r, (lq, lr) = _device_divide(forced, num, den)
    wq, wr = oracle.poly_divide(num, den)
    assert bytes(q[:max(lq, 1)]) == wq and bytes(r[:max(lr, 1)]) == wr


def test_default_threshold_vs_oracle(hip, oracle):
    nl, dl = (1 << 15) + 77, (1 << 14) + 5
    num, den = _inputs(51, nl, dl)
    _check(hip, oracle, num, den)


def test_default_threshold_large_by_construction(hip):
    """num = q den + r with deg r < deg den: Euclidean division is unique, so the result must be
    exactly (trim(q), trim(r)); the product is the library's poly_mul (pinned to reference digests
    in test_polymul_gpu.py), not the code under test"""
    rng = np.random.default_rng(61)
    ql, dl = (1 << 18) + 3, (1 << 18) - 1
    q = rng.integers(0, 17, ql).astype(np.uint8)
    q[-1] = 3
    _, den = _inputs(62, 10, dl)
    r = rng.integers(0, 17, dl - 1).astype(np.uint8)
    prod = np.frombuffer(hip.poly_mul(q, den), np.uint8)
    assert prod.size == ql + dl - 1
    num = prod.copy()
    num[:dl - 1] = (num[:dl - 1].astype(np.uint16) + r) % 17
    gq, gr = _fast(hip, num, den)
    assert gq == bytes(q)
    assert gr == (bytes(r).rstrip(b"\x00") or b"\x00")


def test_same_bytes_under_the_product_options(forced, oracle):
    nl, dl = 20000, 7000
    num, den = _inputs(71, nl, dl)
    want = _check(forced, oracle, num, den)
    with forced.options(NTT_F29=0):
        assert _fast(forced, num, den) == want
    with forced.options(POLY_BLOCK_L=4096, POLY_BLOCK_S=513):
        assert _fast(forced, num, den) == want


def test_parity_with_the_serial_loop(hip):
    nl, dl = 3000, 1000
    num, den = _inputs(81, nl, dl)
    with hip.options(DIVIDE_FAST_MIN=0):
        assert hip.poly_divide_path(den, nl) == 3
        serial = hip.poly_divide(num, den)
    with hip.options(DIVIDE_FAST_MIN=1):
        assert _fast(hip, num, den) == serial
