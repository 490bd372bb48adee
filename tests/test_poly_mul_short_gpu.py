"""plk_poly_mul_short_batch(_dev) on the GPU against the reference's recorded products, the model
(tests/poly_mul_short_model.py: numpy.convolve over the operands mod 17) and plk_poly_mul_dev on the same
device buffers: bytes and the trimmed-length word must be identical.  Every buffer is placed by
tests/devbuf.py: outputs between 0xEE guards, inputs between poison, the input backing unchanged afterwards.
The shapes come from plk_poly_mul_short_plan, so they follow the kernel's geometry."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import poly_mul_short_model as M  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu


def _u8(a):
    return np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a, np.uint8)


class Spec:
    """one run: A and B hold every operand of the run (product i at A[i sa : i sa + la], B[i sb : i sb + lb]);
    so = 0: the tight out_stride la + lb - 1; res: the residues mod 16 of a, b and out"""

    def __init__(self, A, B, la=None, lb=None, count=1, sa=0, sb=0, so=0, res=(0, 0, 0), poison="canon"):
        self.A, self.B = _u8(A), _u8(B)
        self.la, self.lb = len(self.A) if la is None else la, len(self.B) if lb is None else lb
        self.count, self.sa, self.sb, self.res, self.poison = count, sa, sb, res, poison
        self.lo = self.la + self.lb - 1
        self.so = so or self.lo
        assert (count - 1) * sa + self.la <= len(self.A) and (count - 1) * sb + self.lb <= len(self.B)

    def a(self, i):
        return self.A[i * self.sa:i * self.sa + self.la]

    def b(self, i):
        return self.B[i * self.sb:i * self.sb + self.lb]


class Call:
    """one _dev call over Specs, the words pre-filled with 0xEE bytes"""

    def __init__(self, hip, specs, want_nz=True):
        import torch

        import devbuf
        self.hip, self.specs = hip, specs
        self.ins, self.snaps, self.outs, runs = [], [], [], []
        for r, s in enumerate(specs):
            a = devbuf.place(s.A, s.res[0], poison=s.poison, seed=2 * r)
            b = devbuf.place(s.B, s.res[1], poison=s.poison, seed=2 * r + 1)
            o = devbuf.place_out((s.count - 1) * s.so + s.lo, s.res[2])
            self.ins.append((a, b))
            self.snaps.append((devbuf.snapshot(a[0]), devbuf.snapshot(b[0])))
            self.outs.append(o)
            runs.append((a[1], s.la, s.sa, b[1], s.lb, s.sb, o[1], s.so, s.count))
        self.first = np.cumsum([0] + [s.count for s in specs])
        total = int(self.first[-1])
        self.nz = torch.full((4 * total + 8,), 0xEE, dtype=torch.uint8, device="cuda") if want_nz else None
        hip.poly_mul_short_batch_dev(runs, None if self.nz is None else self.nz[4:])
        torch.cuda.synchronize()
        self.bytes = [o[1].cpu().numpy() for o in self.outs]
        if want_nz:
            w = self.nz.cpu().numpy().view(np.uint32)
            assert w[0] == 0xEEEEEEEE and w[-1] == 0xEEEEEEEE     # the words beside the call's own
            self.words = w[1:-1]

    def product(self, r, i):
        s = self.specs[r]
        return self.bytes[r][i * s.so:i * s.so + s.lo].tobytes()

    def word(self, r, i):
        return int(self.words[self.first[r] + i])

    def check_guards(self):
        import devbuf
        for r, s in enumerate(self.specs):
            assert devbuf.guards_intact(*self.outs[r]), r
            assert devbuf.unchanged(self.ins[r][0][0], self.snaps[r][0]), r
            assert devbuf.unchanged(self.ins[r][1][0], self.snaps[r][1]), r
            if s.so > s.lo:        # the bytes between consecutive outputs keep their fill
                gaps = np.concatenate([self.bytes[r][i * s.so + s.lo:(i + 1) * s.so] for i in range(s.count - 1)] or
                                      [np.zeros(0, np.uint8)])
                assert (gaps == devbuf.OUT_GUARD).all(), r

    def check_model(self, want_words=True):
        for r, s in enumerate(self.specs):
            for i in range(s.count):
                want = M.product(s.a(i), s.b(i))
                got = self.product(r, i)
                assert got == want, (r, i, s.la, s.lb, s.res, _first_diff(got, want))
                if want_words and self.nz is not None:
                    assert self.word(r, i) == M.trim(want), (r, i, s.la, s.lb)

    def check_against_mul_dev(self):
        """plk_poly_mul_dev on the same operand buffers: bytes and the trimmed-length word, one synchronisation"""
        import torch
        hip, got = self.hip, []
        for r, s in enumerate(self.specs):
            work = torch.empty(max(hip.poly_mul_workspace(s.la, s.lb), 16), dtype=torch.uint8, device="cuda")
            av, bv = self.ins[r][0][1], self.ins[r][1][1]
            for i in range(s.count):
                out = torch.full((s.lo,), 0xEE, dtype=torch.uint8, device="cuda")
                nz = torch.full((1,), 0x6EEEEEEE, dtype=torch.int32, device="cuda")
                hip.poly_mul_dev(av[i * s.sa:i * s.sa + s.la], s.la, bv[i * s.sb:i * s.sb + s.lb], s.lb, out, nz, work)
                got.append((r, i, out, nz))
        torch.cuda.synchronize()
        for r, i, out, nz in got:
            assert out.cpu().numpy().tobytes() == self.product(r, i), (r, i, self.specs[r].la, self.specs[r].lb)
            if self.nz is not None:
                assert int(nz.cpu().numpy().view(np.uint32)[0]) == self.word(r, i), (r, i)

    def check_all(self):
        self.check_guards()
        self.check_model()
        self.check_against_mul_dev()


def _first_diff(got, want):
    g, w = _u8(got), _u8(want)
    d = np.flatnonzero(g != w)
    return "first difference at %d of %d (%d differ)" % (int(d[0]), len(w), len(d)) if len(d) else ""


def _poly(rng, n, hi=17):
    p = rng.integers(0, hi, n).astype(np.uint8)
    p[-1] = int(rng.integers(1, 17))
    return p


@pytest.fixture(scope="module")
def golden():
    return [(c["tag"],) + tuple(bytes.fromhex(c[k]) for k in ("a", "b", "out"))
            for c in load_golden("poly_mul_short.json")["cases"]]


@pytest.fixture(scope="module")
def U(hip):
    return hip.poly_mul_short_plan(1, 1)["per_unit"]


def test_goldens_dev_form(hip, golden):
    assert len(golden) > 2 * hip.PLK_MUL_SHORT_LAUNCH_RUNS       # one ragged call across launch boundaries
    call = Call(hip, [Spec(a, b, res=(g % 16, (3 * g + 1) % 16, (7 * g + 2) % 16),
                           poison="raw" if tag == "raw" else "canon") for g, (tag, a, b, _) in enumerate(golden)])
    call.check_all()
    for g, (tag, a, b, out) in enumerate(golden):
        got = call.product(g, 0)
        assert M.trimmed(got) == out and max(call.word(g, 0), 1) == len(out), (g, tag)


def _edge_specs(U, seed, short_is_a):
    rng = np.random.default_rng(seed)
    specs = []
    for lo in (U - 1, U, U + 1, 2 * U, 2 * U + 1):
        for ls in (1, 2, 3, 4, 5, 1023, 1024):
            ll = lo + 1 - ls
            if ll < 1:
                continue
            s, l = _poly(rng, ls), _poly(rng, ll)
            k = len(specs)
            res = ((5 * k) % 16, (3 * k + 1) % 16, (11 * k + 7) % 16)
            specs.append(Spec(s, l, res=res) if short_is_a else Spec(l, s, res=res))
    return specs


@pytest.mark.parametrize("short_is_a", [True, False])
def test_tile_edges(hip, U, short_is_a):
    specs = _edge_specs(U, 11 + short_is_a, short_is_a)
    assert len(specs) == 34 and {s.lo for s in specs} == {U - 1, U, U + 1, 2 * U, 2 * U + 1}
    for s in specs:
        assert hip.poly_mul_short_plan(s.la, s.lb)["units_per_product"] == -(-s.lo // U)
    Call(hip, specs).check_all()


@pytest.mark.parametrize("gap", [0, 1, 37])
def test_wave_and_block_remainders(hip, gap):
    per_block = hip.poly_mul_short_plan(48, 48)["units_per_block"]
    assert per_block == 4                                 # the counts below sit around a block of four units
    rng = np.random.default_rng(48 + gap)
    specs = []
    for k, count in enumerate((1, 3, 4, 5, 257)):
        A, B = rng.integers(0, 17, 48 * count).astype(np.uint8), rng.integers(0, 17, 48 * count).astype(np.uint8)
        specs.append(Spec(A, B, 48, 48, count, 48, 48, 95 + gap, res=((3 * k) % 16, (5 * k + 1) % 16, (7 * k + gap) % 16)))
        assert hip.poly_mul_short_plan(48, 48, count)["blocks"] == -(-count // per_block)
    Call(hip, specs).check_all()


def test_strides_shared_and_overlapping(hip, U):
    rng = np.random.default_rng(5)
    count = 70
    A = rng.integers(0, 17, 48 * count).astype(np.uint8)
    specs = [
        Spec(A, _poly(rng, 31), 48, 31, count, 48, 0, 80, res=(1, 2, 3)),                   # one multiplier for the run
        Spec(rng.integers(0, 17, 200 + count).astype(np.uint8), _poly(rng, 9), 200, 9, count, 1, 0, res=(4, 9, 15)),
        Spec(rng.integers(0, 17, U + 300 + count).astype(np.uint8), rng.integers(1, 17, 5 + count).astype(np.uint8),
             U + 300, 5, count, 1, 1, U + 320, res=(7, 3, 5)),                               # both overlap, two tiles
        Spec(_poly(rng, 1024), rng.integers(0, 17, 3000 + 2 * count).astype(np.uint8), 1024, 3000, count, 0, 2,
             res=(15, 1, 9)),                                                                # a shared, b overlapping
    ]
    call = Call(hip, specs)
    call.check_guards()
    call.check_model()
    Call(hip, specs[:3]).check_against_mul_dev()


_SWEEP = [(r, 0, 0) for r in range(16)] + [(0, r, 0) for r in range(16)] + [(0, 0, r) for r in range(16)] + \
         [(r, 5, 11) for r in range(16)] + [(3, r, 7) for r in range(16)] + [(9, 13, r) for r in range(16)]


@pytest.mark.parametrize("shape", ["short", "two tiles"])
def test_every_alignment(hip, U, shape):
    rng = np.random.default_rng(16)
    la, lb = (48, 33) if shape == "short" else (U + 41, 100)
    assert hip.poly_mul_short_plan(la, lb)["units_per_product"] == (1 if shape == "short" else 2)
    a, b = _poly(rng, la), _poly(rng, lb)
    call = Call(hip, [Spec(a, b, res=res, poison="raw" if k % 3 == 0 else "canon") for k, res in enumerate(_SWEEP)])
    call.check_all()
    assert len({call.product(r, 0) for r in range(len(_SWEEP))}) == 1


def test_raw_bytes(hip, U):
    rng = np.random.default_rng(255)
    specs = [Spec(rng.integers(0, 256, la).astype(np.uint8), rng.integers(0, 256, lb).astype(np.uint8),
                  res=(la % 16, lb % 16, (la + lb) % 16), poison="raw")
             for la, lb in ((1, 1), (5, 7), (48, 48), (64, 33), (1024, 1024), (1023, 2 * U + 5), (3000, 1024), (2, U))]
    specs += [Spec(np.full(la, 0xFF, np.uint8), np.full(lb, 0xFF, np.uint8), poison="raw")
              for la, lb in ((1024, 1024), (64, 64), (1024, 5000))]
    specs += [Spec(np.full(1024, 0xF0, np.uint8), np.full(1500, 0xFE, np.uint8), poison="raw")]   # 2 and 16 mod 17
    Call(hip, specs).check_all()


def test_trimmed_length(hip, U):
    rng = np.random.default_rng(3)

    def unit(n, at, v):
        p = np.zeros(n, np.uint8)
        p[at] = v
        return p

    top_zero = rng.integers(0, 17, 2 * U).astype(np.uint8)
    top_zero[500:] = 0
    top_zero[499] = 3
    specs = [
        Spec(np.zeros(40, np.uint8), _poly(rng, 50)),                   # all zero: word 0
        Spec(_poly(rng, 3 * U), np.zeros(7, np.uint8)),
        Spec(np.full(33, 17, np.uint8), np.full(2 * U, 0xEE, np.uint8), poison="raw"),   # zero mod 17 everywhere
        Spec(unit(48, 0, 5), unit(48, 0, 7)),                           # only the first byte
        Spec(unit(U + 9, 0, 2), unit(1024, 0, 9)),
        Spec(unit(48, 47, 5), unit(48, 47, 7)),                         # only the last byte
        Spec(unit(2 * U + 1, 2 * U, 2), unit(1024, 1023, 9)),
        Spec(top_zero, _poly(rng, 100)),                                # three tiles, the upper two all zero
        Spec(_poly(rng, U), unit(2, 0, 1)),                             # the top byte zero, the one below it not
    ]
    want = [0, 0, 0, 1, 1, 95, 2 * U + 1024, 599, U]
    call = Call(hip, specs)
    call.check_all()
    assert [call.word(r, 0) for r in range(len(specs))] == want
    assert hip.poly_mul_short_plan(2 * U, 100)["units_per_product"] == 3
    # d_nz = NULL is accepted and changes nothing else
    quiet = Call(hip, specs, want_nz=False)
    quiet.check_guards()
    quiet.check_model()
    assert [quiet.product(r, 0) for r in range(len(specs))] == [call.product(r, 0) for r in range(len(specs))]


def test_many_mixed_runs(hip, U):
    n = 2 * hip.PLK_MUL_SHORT_LAUNCH_RUNS + 3
    rng = np.random.default_rng(n)
    specs = []
    for k in range(n):
        ls = (1, 4, 17, 48, 64, 300, 1024)[k % 7]
        ll = (1, 30, 64, U - 5, U + 7, 2 * U + 100, 5000)[(3 * k + k // 7) % 7]
        count = (1, 1, 2, 5, 1, 9)[k % 6]
        so = ls + ll - 1 + (0, 3, 16)[k % 3] if count > 1 else 0
        S = rng.integers(0, 17, (ls + 1) * count).astype(np.uint8)
        Lg = rng.integers(0, 17, ll + 3 * count).astype(np.uint8)
        res = ((7 * k) % 16, (5 * k + 3) % 16, (13 * k + 1) % 16)
        if k % 2:
            specs.append(Spec(S, Lg, ls, ll, count, ls + 1, 3, so, res=res))
        else:
            specs.append(Spec(Lg, S, ll, ls, count, 3, ls + 1, so, res=res))
    Call(hip, specs).check_all()


def test_large_shapes_against_the_model(hip, U):
    """one 2^20 x 1024 product and one run of 2^16 products of 48 x 48"""
    import devbuf
    rng = np.random.default_rng(20)
    a, b = rng.integers(0, 17, 1 << 20).astype(np.uint8), rng.integers(0, 17, 1024).astype(np.uint8)
    call = Call(hip, [Spec(a, b, res=(3, 9, 5))])
    call.check_guards()
    call.check_model()
    count = 1 << 16
    A, B = rng.integers(0, 17, (count, 48)).astype(np.uint8), rng.integers(0, 17, (count, 48)).astype(np.uint8)
    A[::5, 40:] = 0                                             # a zero top here and there
    call = Call(hip, [Spec(A.reshape(-1), B.reshape(-1), 48, 48, count, 48, 48, 96, res=(1, 2, 3))])
    call.check_guards()
    want = M.product_rows(A, B)
    got = np.append(call.bytes[0], devbuf.OUT_GUARD).reshape(count, 96)
    assert (got[:, :95] == want).all() and (got[:, 95] == devbuf.OUT_GUARD).all()
    nzw = np.where(want.any(axis=1), 95 - np.argmax(want[:, ::-1] != 0, axis=1), 0)
    assert (call.words == nzw).all()


def test_host_form(hip, golden):
    want = [M.product(a, b) for _, a, b, _ in golden]
    got = hip.poly_mul_short_batch([(a, b) for _, a, b, _ in golden])
    assert got == [out for _, _, _, out in golden] == [M.trimmed(w) for w in want]
    # the same ragged set through the C call: out_lens against the model's trimmed lengths, then NULL
    n = len(golden)
    ops = [(_u8(a).copy(), _u8(b).copy(), np.full(len(a) + len(b) - 1, 0xEE, np.uint8)) for _, a, b, _ in golden]
    arr = (hip.MulShortRun * n)(*[hip.MulShortRun(a.ctypes.data, len(a), 0, b.ctypes.data, len(b), 0, o.ctypes.data, 0, 1)
                                  for a, b, o in ops])
    lens = (C.c_size_t * n)()
    assert hip.lib().plk_poly_mul_short_batch(arr, n, lens) == hip.PLK_OK
    assert [o.tobytes() for _, _, o in ops] == want and list(lens) == [max(M.trim(w), 1) for w in want]
    for _, _, o in ops:
        o[:] = 0xEE
    assert hip.lib().plk_poly_mul_short_batch(arr, n, None) == hip.PLK_OK
    assert [o.tobytes() for _, _, o in ops] == want
    # strided runs, the bytes between the outputs untouched, out_lens given and NULL
    rng = np.random.default_rng(9)
    count, la, lb, so = 37, 48, 1024, 48 + 1024 - 1 + 5
    A = rng.integers(0, 256, la * count).astype(np.uint8)
    b = rng.integers(0, 17, lb).astype(np.uint8)
    A[la:2 * la] = 0
    got = hip.poly_mul_short_batch([(A, la, la, b, lb, 0, count), (b, A[:5])])
    assert got[:count] == [M.trimmed(M.product(A[i * la:(i + 1) * la], b)) for i in range(count)] and got[1] == b"\0"
    assert got[count] == M.trimmed(M.product(b, A[:5]))
    for lens in ((C.c_size_t * count)(), None):
        out = np.full(count * so, 0xEE, np.uint8)
        run = hip.MulShortRun(A.ctypes.data, la, la, b.ctypes.data, lb, 0, out.ctypes.data, so, count)
        assert hip.lib().plk_poly_mul_short_batch(C.byref(run), 1, lens) == hip.PLK_OK
        rows = out.reshape(count, so)
        for i in range(count):
            p = M.product(A[i * la:(i + 1) * la], b)
            assert rows[i, :la + lb - 1].tobytes() == p, i
            assert lens is None or lens[i] == max(M.trim(p), 1), i
        assert (rows[:, la + lb - 1:] == 0xEE).all()
