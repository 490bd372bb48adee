"""plk_poly_mul_dev and plk_poly_mul_batch_dev from exactly sized, guarded buffers at every alignment.

The products feed every round of the prover, and the wrapped ones read operand bytes again in
their last inverse pass and patch both ends of the output.  Here a, b and out sit at chosen
address residues mod 16 (tests/devbuf.py): the inputs between 64 bytes of poison that is non-zero
mod 17, `out` exactly la + lb - 1 bytes between 0xEE guards, the workspace exactly
plk_poly_mul_workspace() bytes before a 0xEE guard, the trimmed length in word 1 of four words of
0x7FFFFFFF.  Checked: the product bytes and the trimmed length against the oracle, every guard,
both input allocations unchanged, the three neighbour words of d_out_nz.

The shapes are the smallest of each dispatch class of plk_poly_mul_launch (ntt.hip), restated by
_plan below and asserted, so a moved threshold shows as a test that no longer covers its class.
"""
import numpy as np
import pytest
import torch

import devbuf
import gen
from prove_large_cases import DIRECT_MAX, SMALL_LOG, T13_MIN_K, WRAP_MAX, product_plan

pytestmark = pytest.mark.gpu

RES = (0, 1, 4, 8, 15)
ALL_TRIPLES = [(ra, rb, ro) for ra in RES for rb in RES for ro in RES]
FEW_TRIPLES = [(0, 0, 0), (1, 15, 4), (15, 1, 8)]
STALE = 0x7FFFFFFF

# (la, lb): (class, log2 of the transform, wrapped top coefficients)
SHAPES = {
    (1, 1): ("direct", 0, 0), (3, 100): ("direct", 7, 0), (32, 5000): ("direct", 13, 0),
    (33, 33): ("one workgroup", 7, 0), (2048, 2049): ("one workgroup", 12, 0),
    (3000, 5000): ("passes", 13, 0),
    (4097, 4100): ("passes", 13, 4),
    (8200, 8201): ("passes", 14, 16),                 # the widest wrap
    (8200, 8202): ("passes", 15, 0),                  # 2^14 + 17 coefficients: one too many to wrap
    ((1 << 16) + 2, 1 << 16): ("passes", 17, 1),
    (1 << 20, 1 << 20): ("passes", 21, 0),            # 2^13 tiles
    ((1 << 22) + 3, (1 << 22) + 5): ("passes", 23, 7),   # the three-pass plan, wrapped
}
for _e in (1, 8, 16):                                # 8193 + e coefficients, both operand orders
    _w = (13, _e + 1) if _e + 1 <= WRAP_MAX else (14, 0)
    SHAPES[8193 - 32 + _e, 33] = SHAPES[33, 8193 - 32 + _e] = ("passes",) + _w
SMALL = [s for s in SHAPES if s[0] + s[1] - 1 <= (1 << 14) + 17]
LARGE = [s for s in SHAPES if s not in SMALL]
WRAPPED = [s for s, c in SHAPES.items() if c[2]]


def _plan(la, lb):
    if min(la, lb) <= DIRECT_MAX:
        return ("direct", (la + lb - 2).bit_length(), 0)
    k, e = product_plan(la, lb)
    return ("one workgroup" if k <= SMALL_LOG else "passes", k, e)


def test_shapes_cover_their_classes():
    for (la, lb), want in SHAPES.items():
        assert _plan(la, lb) == want, (la, lb, _plan(la, lb))
    assert len(SMALL) == 15 and len(LARGE) == 3 and len(WRAPPED) == 8
    assert {c[2] for c in SHAPES.values()} >= {0, 1, 2, 4, 7, 9, 16}
    assert max(c[1] for c in SHAPES.values()) >= 23 and SHAPES[1 << 20, 1 << 20][1] >= T13_MIN_K


_REF = {}


def _operands(la, lb, ta=None, tb=None):
    a, b = gen.poly_inputs(la * 31 + lb, la, lb)
    a, b = a.copy(), b.copy()
    if ta is not None:               # a leading byte that is 0 mod 17; the next coefficients vanish too
        a[-1] = ta
        if la >= 3:
            a[-3:-1] = [0, 17]
    if tb is not None:
        b[-1] = tb
    return a, b


def _ref(oracle, la, lb, ta=None, tb=None):
    """(a, b, the oracle's trimmed product), once per module"""
    key = (la, lb, ta, tb)
    if key not in _REF:
        a, b = _operands(la, lb, ta, tb)
        want = oracle.poly_mul(a, b) if la * lb <= (1 << 24) else oracle.poly_mul_ntt(a, b)
        _REF[key] = (a, b, want)
    return _REF[key]


def _full(want, rl):
    return torch.from_numpy(np.pad(np.frombuffer(want, np.uint8), (0, rl - len(want)))).to("cuda")


def _work(ws):
    """exactly ws workspace bytes, 16-byte aligned, between 0xEE guards"""
    return devbuf.place_out(ws, 0)


def _single(hip, a, b, want, triples, poison):
    """'' or what went wrong, over every (a, b, out) residue triple"""
    la, lb, rl = len(a), len(b), len(a) + len(b) - 1
    ws = hip.poly_mul_workspace(la, lb)
    ins = {}
    for r in sorted({t[0] for t in triples}):
        ins["a", r] = devbuf.place(a, r, poison=poison, seed=1)
    for r in sorted({t[1] for t in triples}):
        ins["b", r] = devbuf.place(b, r, poison=poison, seed=2)
    snaps = {k: devbuf.snapshot(v[0]) for k, v in ins.items()}
    outs = {r: devbuf.place_out(rl, r) for r in sorted({t[2] for t in triples})}
    wback, work = _work(ws)
    nz = torch.full((4,), STALE, dtype=torch.int32, device="cuda")
    full = _full(want, rl)
    st = torch.cuda.current_stream()
    bad = []
    for ra, rb, ro in triples:
        oback, out = outs[ro]
        oback.fill_(devbuf.OUT_GUARD)
        nz.fill_(STALE)
        hip.poly_mul_dev(ins["a", ra][1], la, ins["b", rb][1], lb, out, nz[1:], work, st)
        torch.cuda.synchronize()
        words = nz.tolist()
        if (words[1] or 1) != len(want):
            bad.append(((ra, rb, ro), "trimmed length %d, oracle %d" % (words[1], len(want))))
        if words[0] != STALE or words[2:] != [STALE, STALE]:
            bad.append(((ra, rb, ro), "words beside d_out_nz: %s" % words))
        if not torch.equal(out, full):
            bad.append(((ra, rb, ro), "product differs at %d" % int(torch.nonzero(out != full)[0])))
        if not devbuf.guards_intact(oback, out):
            bad.append(((ra, rb, ro), "output guard"))
        if not devbuf.guards_intact(wback, work):
            bad.append(((ra, rb, ro), "workspace guard (%d bytes)" % ws))
    for k, (back, _) in ins.items():
        if not devbuf.unchanged(back, snaps[k]):
            bad.append((k, "input changed"))
    return bad[:12]


@pytest.mark.parametrize("la,lb", SMALL)
def test_every_residue_triple(hip, oracle, la, lb):
    """all 125 (a, b, out) residue triples from {0, 1, 4, 8, 15}^3, "canon" poison; three of them
    again with "raw" poison"""
    a, b, want = _ref(oracle, la, lb)
    assert _single(hip, a, b, want, ALL_TRIPLES, "canon") == []
    assert _single(hip, a, b, want, FEW_TRIPLES, "raw") == []


@pytest.mark.parametrize("la,lb", LARGE)
def test_large_shapes(hip, oracle, la, lb):
    a, b, want = _ref(oracle, la, lb)
    assert _single(hip, a, b, want, FEW_TRIPLES, "canon") == []
    assert _single(hip, a, b, want, FEW_TRIPLES[1:], "raw") == []


@pytest.mark.parametrize("la,lb", WRAPPED)
def test_wrapped_trimmed_length(hip, oracle, la, lb):
    """leading bytes 17 and 34 (0 mod 17) on the wrapped shapes: the trimmed length comes from a
    block maximum per tile and from the fix-up of both ends, not from the top coefficient (the
    2^23-point shape with both at once only: its oracle product costs seconds)"""
    for ta, tb in ((17, None), (None, 34), (17, 34)) if la < (1 << 22) else ((17, 34),):
        a, b, want = _ref(oracle, la, lb, ta, tb)
        assert len(want) < la + lb - 1
        assert _single(hip, a, b, want, FEW_TRIPLES, "canon") == [], (ta, tb)


# ------------------------------------------------------------------ batch
def _batch(hip, jobs_host, residues, poison="canon", pool=None):
    """jobs_host: (a, b, acc) arrays (`pool`: id(array) -> one shared placement).  Runs ONE
    plk_poly_mul_batch_dev from placed buffers with the workspace exactly
    plk_poly_mul_batch_workspace() bytes.  Returns (outs as bytes, problems)."""
    placed, snaps, jobs, outs = {}, {}, [], []

    def put(x, r, seed):
        key = id(x) if pool is not None and id(x) in pool else len(placed)
        if key not in placed:
            placed[key] = devbuf.place(x, r, poison=poison, seed=seed)
            snaps[key] = devbuf.snapshot(placed[key][0])
        return placed[key][1]

    for i, ((a, b, acc), (ra, rb, ro)) in enumerate(zip(jobs_host, residues)):
        va, vb = put(a, ra, 2 * i), put(b, rb, 2 * i + 1)
        ob, ov = devbuf.place_out(len(a) + len(b) - 1, ro)
        outs.append((ob, ov, devbuf.snapshot(ob)))
        jobs.append((va, len(a), vb, len(b), ov, acc))
    ws = hip.poly_mul_batch_workspace(jobs)
    wback, work = _work(ws)
    hip.poly_mul_batch_dev(jobs, work, ws, torch.cuda.current_stream())
    torch.cuda.synchronize()
    bad = []
    if not devbuf.guards_intact(wback, work):
        bad.append("workspace guard (%d bytes)" % ws)
    for i, (ob, ov, snap) in enumerate(outs):
        if jobs_host[i][2]:
            if not devbuf.unchanged(ob, snap):
                bad.append("member %d's out was written" % i)
        elif not devbuf.guards_intact(ob, ov):
            bad.append("job %d output guard" % i)
    for key, (back, _) in placed.items():
        if not devbuf.unchanged(back, snaps[key]):
            bad.append("input %s changed" % (key,))
    return [bytes(ov.cpu().numpy()) for _, ov, _ in outs], bad


def _padded(want, rl):
    return want + bytes(rl - len(want))


@pytest.mark.parametrize("shift,poison", [(0, "canon"), (1, "canon"), (2, "raw")])
def test_batch_same_shapes(hip, oracle, shift, poison):
    """every shape above as one batched call, the residue triples rotated over the jobs"""
    shapes = list(SHAPES)
    refs = [_ref(oracle, la, lb) for la, lb in shapes]
    residues = [ALL_TRIPLES[(37 * i + 41 * shift + 5) % 125] for i in range(len(shapes))]
    assert len({r[0] for r in residues}) == 5 and len({r[2] for r in residues}) == 5
    outs, bad = _batch(hip, [(a, b, 0) for a, b, _ in refs], residues, poison)
    assert bad == []
    wrong = [s for s, (a, b, w), o in zip(shapes, refs, outs) if o != _padded(w, len(a) + len(b) - 1)]
    assert wrong == []


_GROUP = [(4097, 4100), (4096, 4000), (4097, 4099)]      # 2^13: wrapped by 4, not wrapped, wrapped by 3


@pytest.mark.parametrize("csum", [0, 1])
def test_batch_sum_group_members_not_written(hip, oracle, csum):
    """a leader and two members (one transform size, shorter members): the leader's out is the
    sum, each member's out -- a fully poisoned buffer -- comes back unchanged (include/plonkhip.h:
    "the members' out is not written"), with the members merged into the leader's centre item
    (PLK_OPT_NTT_CENTER_SUM = 1) or added in the inverse pass (0)"""
    assert all(_plan(la, lb)[:2] == ("passes", 13) for la, lb in _GROUP)
    refs = [_ref(oracle, la, lb) for la, lb in _GROUP]
    rl = sum(_GROUP[0]) - 1
    want = np.zeros(rl, np.int64)
    for a, b, w in refs:
        want[:len(w)] += np.frombuffer(w, np.uint8)
    want = (want % 17).astype(np.uint8).tobytes()
    lone = _ref(oracle, 3000, 5000)                    # a bystander of the same transform size
    hosts = [(lone[0], lone[1], 0)] + [(a, b, int(i > 0)) for i, (a, b, _) in enumerate(refs)]
    for residues in ([(0, 0, 0)] * 4, [(1, 15, 4), (15, 1, 8), (4, 8, 1), (8, 4, 15)],
                     [(15, 15, 15), (1, 1, 1), (15, 4, 0), (0, 1, 8)]):
        with hip.options(NTT_CENTER_SUM=csum):
            outs, bad = _batch(hip, hosts, residues)
        assert bad == [], residues
        assert outs[1] == want, residues
        assert outs[0] == _padded(lone[2], 7999), residues


def test_batch_shared_operand_transformed_once(hip, oracle):
    """three products with one operand given by the same pointer and length, at residue 1: the
    forward pass transforms 4 distinct arrays (PLK_OPT_NTT_SHARE = 1), 6 without sharing"""
    s, b0, _ = _ref(oracle, 4097, 4100)
    others = [b0, _ref(oracle, 4096, 4000)[1], _ref(oracle, 4097, 4099)[1]]
    wants = [oracle.poly_mul(s, b) for b in others]
    for share, arrays in ((1, 4), (0, 6)):
        hip.ntt_launch_log()
        with hip.options(NTT_SHARE=share, NTT_LAUNCH_LOG=1):
            try:
                outs, bad = _batch(hip, [(s, b, 0) for b in others], [(1, 4, 15), (1, 15, 0), (1, 0, 1)],
                                   pool={id(s)})
            finally:
                log = hip.ntt_launch_log()
        assert bad == []
        fwd = [r["n"] for r in log if r["kind"] == 0]
        assert fwd and all(n == arrays for n in fwd), (share, log)
        assert [r["n"] for r in log if r["kind"] == 2] == [3], log
        for b, w, o in zip(others, wants, outs):
            assert o == _padded(w, len(s) + len(b) - 1), (share, len(b))


# ------------------------------------------------------------------ forced blocked path
@pytest.mark.parametrize("la,lb", [(20000, 15000), (12345, 999)])
def test_blocked_forced_guarded(hip, oracle, la, lb):
    """POLY_BLOCK_L = 4000, POLY_BLOCK_S = 3000: piece products accumulated into the zeroed output
    at the pieces' offsets, with out at residues 0, 1 and 15"""
    a, b, want = _ref(oracle, la, lb)
    with hip.options(POLY_BLOCK_L=4000, POLY_BLOCK_S=3000):
        assert hip.poly_mul_workspace(la, lb) >= 4000 + min(lb, 3000) - 1
        assert _single(hip, a, b, want, [(1, 15, 0), (15, 1, 1), (4, 8, 15), (0, 0, 0)], "canon") == []
        assert _single(hip, a, b, want, [(1, 15, 15)], "raw") == []
