"""plk_poly_divide_short_batch(_dev) on the GPU against the reference's recorded outputs, the oracle's
long division (src/poly.h:124-177 restated, itself pinned to the compiled reference) and
plk_poly_divide_dev on the same device buffers: bytes, trimmed lengths and status words must be identical.
The shapes come from plk_poly_divide_short_plan, so they follow the kernels' geometry."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import divide_short_model as M  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu


def _u8(a):
    return np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a, np.uint8)


def _sizes(nl, dl):
    return max(nl - dl + 1, 1), min(dl - 1, nl)


class Run:
    """one _dev call over (num, den) pairs, every buffer placed by tests/devbuf.py at its residue mod 16"""

    def __init__(self, hip, pairs, residues=None):
        import torch

        import devbuf
        self.hip, self.pairs = hip, [(_u8(n), _u8(d)) for n, d in pairs]
        n = len(self.pairs)
        residues = residues or [(0, 0, 0)] * n
        self.nums = [devbuf.place(a, r[0], seed=i) for i, ((a, _), r) in enumerate(zip(self.pairs, residues))]
        self.snaps = [devbuf.snapshot(b) for b, _ in self.nums]
        self.quots = [devbuf.place_out(_sizes(len(a), len(d))[0], r[1]) for (a, d), r in zip(self.pairs, residues)]
        self.rems = [devbuf.place_out(_sizes(len(a), len(d))[1], r[2]) for (a, d), r in zip(self.pairs, residues)]
        ws = hip.poly_divide_short_workspace([(len(a), len(d)) for a, d in self.pairs])
        assert ws > 0
        self.work = torch.full((ws,), 0xEE, dtype=torch.uint8, device="cuda")
        self.lens = torch.full((12 * n,), 0xEE, dtype=torch.uint8, device="cuda")
        self.jobs = [(nv, len(a), d, qv, rv) for (a, d), (_, nv), (_, qv), (_, rv) in
                     zip(self.pairs, self.nums, self.quots, self.rems)]
        self.call()

    def call(self):
        import torch
        self.hip.poly_divide_short_batch_dev(self.jobs, self.lens, self.work)
        torch.cuda.synchronize()
        self.words = self.lens.cpu().numpy().view(np.uint32).reshape(-1, 3)
        self.q = [qv.cpu().numpy().tobytes() for _, qv in self.quots]
        self.r = [rv.cpu().numpy().tobytes() for _, rv in self.rems]

    def check_guards(self):
        import devbuf
        for i in range(len(self.pairs)):
            assert devbuf.guards_intact(*self.quots[i]) and devbuf.guards_intact(*self.rems[i]), i
            assert devbuf.unchanged(self.nums[i][0], self.snaps[i]), i

    def check_exact(self, i, want, note=None):
        """job i against trimmed (quot, rem): untrimmed bytes, both length words, status 0"""
        wq, wr = want
        note = (i, len(self.pairs[i][0]), len(self.pairs[i][1])) if note is None else note
        lq, lr, st = (int(v) for v in self.words[i])
        assert st == 0, note
        assert (lq, lr) == (M.trim(wq), M.trim(wr)), note
        assert self.q[i] == wq[:lq] + bytes(len(self.q[i]) - lq), note
        assert self.r[i] == wr[:lr] + bytes(len(self.r[i]) - lr), note

    def check_against_divide_dev(self, i):
        """plk_poly_divide_dev on the same numerator buffer: bytes and both length words"""
        import torch
        hip = self.hip
        a, d = self.pairs[i]
        ql, rl = _sizes(len(a), len(d))
        q = torch.full((ql,), 0xEE, dtype=torch.uint8, device="cuda")
        r = torch.full((max(rl, 1),), 0xEE, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(2, dtype=torch.int32, device="cuda")
        work = torch.empty(max(hip.poly_divide_workspace(len(a), len(d)), 16), dtype=torch.uint8, device="cuda")
        hip.poly_divide_dev(self.nums[i][1], len(a), d, q, r, lens, work)
        torch.cuda.synchronize()
        assert q.cpu().numpy().tobytes() == self.q[i], (i, len(a), len(d))
        assert r[:rl].cpu().numpy().tobytes() == self.r[i], (i, len(a), len(d))
        assert lens.cpu().numpy().view(np.uint32).tolist() == self.words[i][:2].tolist(), (i, len(a), len(d))


@pytest.fixture(scope="module")
def golden():
    return [(c["tag"],) + tuple(bytes.fromhex(c[k]) for k in ("num", "den", "quot", "rem"))
            for c in load_golden("divide_short.json")["cases"]]


def test_goldens_dev_form(hip, golden):
    run = Run(hip, [(n, d) for _, n, d, _, _ in golden], [(g % 16, (3 * g) % 16, (7 * g) % 16) for g in range(len(golden))])
    run.check_guards()
    for g, (tag, _, _, q, r) in enumerate(golden):
        if tag == "raw":
            assert int(run.words[g][2]) == 1, g
        else:
            run.check_exact(g, (q, r), (g, tag))


def test_goldens_host_form(hip, golden):
    got = hip.poly_divide_short_batch([n for _, n, _, _, _ in golden], [d for _, _, d, _, _ in golden])
    for g, (tag, _, _, q, r) in enumerate(golden):
        assert got[g] == (q, r), (g, tag)


def test_host_form_non_canonical_equals_poly_divide(hip):
    rng = np.random.default_rng(77)
    nums, dens = [], []
    for i in range(24):
        dl = 2 + i % 16
        nl = int(rng.integers(1, 300)) if i % 3 else int(rng.integers(9000, 20000))
        n = rng.integers(0, 256 if i % 2 == 0 else 17, nl).astype(np.uint8)
        if i % 4 == 0:
            n[int(rng.integers(0, nl))] = (0xFF, 0xEE, 17, 0x80)[i // 4 % 4]
        d = rng.integers(0, 17, dl).astype(np.uint8)
        d[-1] = int(rng.integers(1, 17))
        nums.append(n)
        dens.append(d)
    got = hip.poly_divide_short_batch(nums, dens)
    for i, (n, d) in enumerate(zip(nums, dens)):
        assert got[i] == hip.poly_divide(n, d), (i, len(n), len(d))


def _boundary_lengths(hip, dl):
    p = hip.poly_divide_short_plan(1, dl)
    e, b, lim = p["per_thread"], p["per_block"], p["one_kernel_max"]
    t = dl - 1
    out = set()
    for base in (e, 64 * e, b, lim, 2 * b):
        out |= {base - t, base - 1, base, base + 1, base + t}
    out.add(lim + 65 * b - b + 1)     # the carries phase scans 65 block aggregates: more than one wave
    out.add(lim + 257 * b - b + 1)    # ... 257: more than one block's threads, a second round
    assert hip.poly_divide_short_plan(lim, dl)["kernels"] == 1 and hip.poly_divide_short_plan(lim + 1, dl)["kernels"] == 3
    return sorted(v for v in out if v >= 1)


@pytest.mark.parametrize("dl", [2, 3, 4, 9, 16, 17])
def test_boundaries(hip, oracle, dl):
    rng = np.random.default_rng(1000 + dl)
    pairs = []
    for nl in _boundary_lengths(hip, dl):
        d = rng.integers(0, 17, dl).astype(np.uint8)
        d[-1] = int(rng.integers(1, 17))
        pairs.append((rng.integers(0, 17, nl).astype(np.uint8), d))
        pairs.append((np.full(nl, 16, np.uint8), d))
    run = Run(hip, pairs, [(i % 16, (5 * i + 1) % 16, (3 * i + 2) % 16) for i in range(len(pairs))])
    run.check_guards()
    for i, (n, d) in enumerate(pairs):
        run.check_exact(i, oracle.poly_divide(n, d))
        run.check_against_divide_dev(i)


@pytest.mark.parametrize("dl", [17, 3])
def test_one_large_shape(hip, oracle, dl):
    import torch
    nl, t = (1 << 22) + 5, dl - 1
    rng = np.random.default_rng(dl)
    pts = rng.permutation(17)[:t].astype(np.uint8)
    d = _u8(hip.poly_from_roots(pts))
    assert len(d) == dl
    n = rng.integers(0, 17, nl).astype(np.uint8)
    run = Run(hip, [(n, d)], [(3, 9, 5)])
    run.check_guards()
    run.check_exact(0, oracle.poly_divide(n, d))
    # num = q Z_S + r: r agrees with num on S
    num_dev = run.nums[0][1]
    ys = torch.zeros(t, dtype=torch.uint8, device="cuda")
    tick = torch.zeros(hip.poly_eval_workspace(t), dtype=torch.uint8, device="cuda")
    hip.poly_eval_batch_dev([num_dev] * t, [nl] * t, pts, ys, tick)
    torch.cuda.synchronize()
    r = [int(v) for v in run.r[0]]
    want = [sum(c * pow(int(z), k, 17) for k, c in enumerate(r)) % 17 for z in pts]
    assert ys.cpu().tolist() == want


def test_ragged_batch(hip, oracle):
    assert 70 > hip.PLK_DIV_SHORT_LAUNCH_JOBS      # more jobs than a group of launches carries
    rng = np.random.default_rng(70)
    b = hip.poly_divide_short_plan(1, 2)["per_block"]
    pairs = []
    for i in range(70):
        dl = (2, 3)[i % 2] if i < 40 else 2 + int(rng.integers(0, 16))    # 40 jobs of one class: two groups of it
        nl = (1, dl - 1, dl, int(rng.integers(1, 200)), int(rng.integers(b - 40, b + 40)),
              int(rng.integers(2 * b, 5 * b)), int(rng.integers(200, b)))[i % 7]
        d = rng.integers(0, 17, dl).astype(np.uint8)
        d[-1] = int(rng.integers(1, 17))
        pairs.append((rng.integers(0, 17, max(nl, 1)).astype(np.uint8), d))
    bad = 33
    assert len(pairs[bad][0]) > 2 * b
    pairs[bad][0][b + 5] = 0x80
    run = Run(hip, pairs, [((11 * i) % 16, (5 * i) % 16, (9 * i) % 16) for i in range(70)])
    run.check_guards()
    for i, (n, d) in enumerate(pairs):
        if i == bad:
            assert int(run.words[i][2]) == 1
        else:
            run.check_exact(i, oracle.poly_divide(n, d))


def test_placement(hip, oracle):
    rng = np.random.default_rng(16)
    b = hip.poly_divide_short_plan(1, 5)["per_block"]
    shapes = [(2 * b + 100, 5), (300, 17)]
    pairs, residues, want = [], [], []
    base = {}
    for nl, dl in shapes:
        d = rng.integers(0, 17, dl).astype(np.uint8)
        d[-1] = int(rng.integers(1, 17))
        n = rng.integers(0, 17, nl).astype(np.uint8)
        base[(nl, dl)] = oracle.poly_divide(n, d)
        for rn in (0, 1, 7, 15):
            for rq in (0, 1, 7, 15):
                for rr in (0, 1, 7, 15):
                    pairs.append((n, d))
                    residues.append((rn, rq, rr))
                    want.append(base[(nl, dl)])
    run = Run(hip, pairs, residues)
    run.check_guards()
    for i in range(len(pairs)):
        run.check_exact(i, want[i], (i, residues[i]))
    first = (run.q, run.r, run.words.copy())
    run.call()                                     # the same workspace and length words, as the first call left them
    run.check_guards()
    assert (run.q, run.r) == first[:2] and (run.words == first[2]).all()
