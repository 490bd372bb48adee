"""Batched small-circuit prover: plk_prover_prove_batch / plk_prover_rounds_batch (one wave per proof,
prove_batch.hip) against the single calls, the reference's recorded proofs and the restatement
oracle/prove_ref.py -- proofs byte for byte, exits by code and message, neighbours untouched."""
import numpy as np
import pytest
import torch

import gen
from conftest import load_golden
from prove_ref import Prover as RefProver, ProveError

pytestmark = pytest.mark.gpu

SRS_MSG = "SRS length is less than polynomial length"
SLICE_MSG = "Invalid slice indices in poly_slice"
REM_MSG = "Non-zero remainder in t(x) division"
COPY_MSG = "Invalid copy_of type"
FA, FB, FC, QO, QM, QL, QR, QC, S1, S2, S3, ACC, L1 = range(13)
NAMES = ("f_a", "f_b", "f_c", "q_o", "q_m", "q_l", "q_r", "q_c", "s1", "s2", "s3", "acc_x", "l_1")
X_GATE, X_COPY, X_SRS, X_ACC, X_REM_T, X_SLICE, X_REM_W1, X_REM_W2, X_INPUT = range(1, 10)


def _code(hip, msg):
    """the error code of each kind of reference exit (check_status in prove.hip)"""
    return hip.PLK_ERR_RANGE if msg in (SRS_MSG, SLICE_MSG) else hip.PLK_ERR_ARG


def _split(proofs, status):
    assert len(proofs) == 34 * len(status)
    return [proofs[34 * i:34 * i + 34] for i in range(len(status))]


def _diff(hip, proofs, status, want):
    """want: per entry (proof bytes, None) or (None, message[, code]); what differs, by entry"""
    bad = {}
    got = _split(proofs, status)
    assert len(got) == len(want)
    for i, (w, g, st) in enumerate(zip(want, got, status)):
        st = int(st)
        if w[1] is None:
            if st != 0 or g != w[0]:
                bad[i] = "status 0x%x proof %s, want proof %s" % (st, g.hex(), w[0].hex())
            continue
        code = w[2] if len(w) > 2 else _code(hip, w[1])
        if st == 0 or (st & 0xFF) != code or hip.prove_exit_message(st) != w[1] or g != bytes(34):
            bad[i] = "status 0x%x (%r) proof %s, want exit %r code %d" % (st, hip.prove_exit_message(st) if st else "",
                                                                        g.hex(), w[1], code)
    return bad


# ------------------------------------------------------------------ circuits (n = 4 fixtures)
def _cir_bytes(c):
    """q_m q_l q_r q_o q_c | copy_a copy_b copy_c | a b c: the 14 n bytes of one batch entry"""
    assert len(c["gates"]) == 20 and len(c["copies"]) == 24 and len(c["wires"]) == 12
    return bytes(c["gates"]) + bytes(c["copies"]) + bytes(c["wires"])


def _circuit_kw(cir):
    n = len(cir) // 14
    b = list(cir)
    return dict(q_m=b[0:n], q_l=b[n:2 * n], q_r=b[2 * n:3 * n], q_o=b[3 * n:4 * n], q_c=b[4 * n:5 * n],
                copy_a=b[5 * n:7 * n], copy_b=b[7 * n:9 * n], copy_c=b[9 * n:11 * n], a=b[11 * n:12 * n],
                b=b[12 * n:13 * n], c=b[13 * n:14 * n])


def _single(hip, pr, cir, chal, rnd):
    """the single call's answer for one entry: (proof, None) or (None, message, code)"""
    try:
        return pr.prove(**_circuit_kw(cir), chal=chal, rand=rnd), None
    except hip.PlonkHipError as e:
        if e.code not in (hip.PLK_ERR_ARG, hip.PLK_ERR_RANGE):
            raise
        return None, str(e).split("): ", 1)[1], e.code


def _prover4(hip, s):
    return hip.Prover(4, s["z_h"], s["g1s"], s["h"], s["k1_h"], s["k2_h"], s["h_pows_inv"])


def _interleave(a, b):
    out = []
    for i in range(max(len(a), len(b))):
        out += a[i:i + 1] + b[i:i + 1]
    return out


def _entries(cases):
    cir = b"".join(_cir_bytes(c) for c in cases)
    ch = np.array([c["chal"] for c in cases], np.uint8)
    rd = np.array([c["rand"] for c in cases], np.uint8)
    return cir, ch, rd


def _run_recorded(hip, pr, cases):
    """one prove_batch call over the cases: recorded proofs byte for byte, recorded None = the single
    call's own exit (code and message)"""
    assert pr.batch_path() == 1
    proofs, status = pr.prove_batch(*_entries(cases))
    want = []
    for c in cases:
        if c["proof"] is not None:
            want.append((bytes.fromhex(c["proof"]), None))
        else:
            w = _single(hip, pr, _cir_bytes(c), c["chal"], c["rand"])
            assert w[0] is None, "the single call accepts what the reference rejected"
            want.append(w)
    return _diff(hip, proofs, status, want), status


def test_recorded_edge_fixtures(hip):
    """every setup of prove_edges.json as ONE call, its proofs and rejections interleaved (the file
    records cases for 8 of its 10 setups: 64 each at srs_mode 0, 49, 43 and 1 at srs_mode 1)"""
    g = load_golden("prove_edges.json")
    assert len(g["setups"]) == 10
    sizes, mixed = [], 0
    for key, setup in g["setups"].items():
        sel = lambda lst: [dict(g["circuits"][c["circuit"]], **c) for c in lst
                           if "%d/%d" % (c["srs_n"], c["srs_mode"]) == key]
        cases = _interleave(sel(g["proofs"]), sel(g["failures"]))
        if not cases:
            continue
        pr = _prover4(hip, {k: bytes.fromhex(v) for k, v in setup.items()})
        bad, status = _run_recorded(hip, pr, cases)
        assert not bad, (key, bad)
        sizes.append(len(cases))
        mixed += bool(np.any(status == 0) and np.any(status != 0))
        pr.close()
    assert sum(sizes) == len(g["proofs"]) + len(g["failures"]) and max(sizes) == 64 and mixed >= 3


def test_recorded_prove_fixtures_and_constructed_rejections(hip, oracle):
    """prove.json's 26 proofs and 8 rejections, and two rejections of our own checked against the
    restatement's plonk_prove: a wire changed (GATE with its index), a copy type of 3 (COPY)"""
    g = load_golden("prove.json")
    assert len(g["proofs"]) == 26 and len(g["failures"]) == 8
    key = lambda c: "short" if c["srs_n"] == 4 else str(c["srs_mode"])
    for k, setup in g["setups"].items():
        cases = _interleave([c for c in g["proofs"] if key(c) == k], [c for c in g["failures"] if key(c) == k])
        s = {a: bytes.fromhex(v) for a, v in setup.items()}
        pr = _prover4(hip, s)
        bad, status = _run_recorded(hip, pr, cases)
        assert not bad, (k, bad)
        if k != "0":
            continue
        # the recorded "unsatisfied gate 0" is the GATE exit in the batch and in the single call alike
        gate0 = [i for i, c in enumerate(cases) if c.get("note", "").startswith("unsatisfied gate 0")]
        assert len(gate0) == 1 and int(status[gate0[0]]) == hip.PLK_ERR_ARG | (X_GATE << 8)
        base = g["proofs"][0]
        wire = dict(base, wires=list(base["wires"]))
        wire["wires"][4 + 2] = (wire["wires"][4 + 2] + 1) % 17          # b[2]: gate 2 fails first
        copy = dict(base, copies=list(base["copies"]))
        copy["copies"][8 + 2 * 1] = 3                                   # copy_b[1].type
        ref = RefProver(oracle, s["g1s"], 4, s["h"], s["k1_h"], s["k2_h"], s["h_pows_inv"], s["z_h"])
        want = []
        for c in (base, wire, base, copy, base):
            kw = _circuit_kw(_cir_bytes(c))
            cps = [list(zip(kw[x][0::2], kw[x][1::2])) for x in ("copy_a", "copy_b", "copy_c")]
            try:
                want.append((ref.prove(kw["q_m"], kw["q_l"], kw["q_r"], kw["q_o"], kw["q_c"], cps, kw["a"], kw["b"],
                                       kw["c"], c["chal"], c["rand"]), None))
            except ProveError as e:
                want.append((None, str(e)))
        assert [w[1] for w in want] == [None, "Constraint 2 not satisfied.", None, COPY_MSG, None]
        proofs, status = pr.prove_batch(*_entries([base, wire, base, copy, base]))
        assert not _diff(hip, proofs, status, want)
        assert int(status[1]) == hip.PLK_ERR_ARG | (X_GATE << 8) | (2 << 16)
        assert int(status[3]) == hip.PLK_ERR_ARG | (X_COPY << 8)


# ------------------------------------------------------------------ batch geometry
_GEO = {}


def _geometry(hip):
    """the 64 cases of prove_edges.json's setup 6/0 with their single-call answers (once per module)"""
    if not _GEO:
        g = load_golden("prove_edges.json")
        cases = [dict(g["circuits"][c["circuit"]], **c) for c in g["proofs"] + g["failures"]
                 if (c["srs_n"], c["srs_mode"]) == (6, 0)]
        pr = _prover4(hip, {k: bytes.fromhex(v) for k, v in g["setups"]["6/0"].items()})
        ans = [_single(hip, pr, _cir_bytes(c), c["chal"], c["rand"]) for c in cases]
        rej = [i for i, a in enumerate(ans) if a[0] is None]
        assert len(cases) == 64 and 10 <= len(rej) <= 54
        _GEO.update(pr=pr, cases=cases, ans=ans, rej=rej)
    return _GEO


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 63, 64, 65, 257, 4099])
def test_batch_geometry(hip, batch):
    """sizes around the 4-proof block and the grid stride, a rejecting case at position 0, at the last
    position, at every multiple of 4 and before every other one: each entry is its single-call answer,
    a second run gives the same bytes, a permuted batch the permuted outputs"""
    G = _geometry(hip)
    pick = []
    for p in range(batch):
        if p == 0 or p == batch - 1 or p % 4 == 0 or p % 8 == 3:
            pick.append(G["rej"][p % len(G["rej"])])
        else:
            pick.append(p % 64)
    assert batch < 8 or any(G["ans"][i][0] is not None for i in pick)

    def run(order):
        proofs, status = G["pr"].prove_batch(*_entries([G["cases"][i] for i in order]))
        return proofs, status

    proofs, status = run(pick)
    assert not _diff(hip, proofs, status, [G["ans"][i] for i in pick])
    again, status2 = run(pick)
    assert again == proofs and np.array_equal(status, status2)
    perm = np.random.default_rng(batch).permutation(batch)
    pp, ps = run([pick[i] for i in perm])
    got = _split(proofs, status)
    assert _split(pp, ps) == [got[i] for i in perm] and np.array_equal(ps, status[perm])


# ------------------------------------------------------------------ rounds_batch against the oracle
def _ref(oracle, pts, n, zh, cls=RefProver):
    return cls(oracle, np.ascontiguousarray(pts).tobytes(), n, z_h=np.asarray(zh, np.uint8).tobytes())


def _answer(ref, polys, chal, rnd, strict=False):
    try:
        return ref.rounds(polys, chal, rnd, strict=strict), None
    except ProveError as e:
        return None, str(e)


def _pack(items):
    """[(polys, chal, rnd)] -> the three arrays of a rounds_batch call"""
    return (np.concatenate([np.concatenate(p) for p, _, _ in items]).astype(np.uint8),
            np.array([c for _, c, _ in items], np.uint8), np.array([r for _, _, r in items], np.uint8))


_SEEDS = {}


def _seeded(oracle, n):
    """gen.prove_instance(n, seed, 2n + 8) for seeds 1..40 over seed 1's SRS, with the oracle's answers"""
    if n not in _SEEDS:
        insts = [gen.prove_instance(n, seed, 2 * n + 8) for seed in range(1, 41)]
        zh, pts = insts[0][3], insts[0][4]
        items = [(p, c, r) for p, c, r, _, _ in insts]
        ref = _ref(oracle, pts, n, zh)
        _SEEDS[n] = dict(n=n, zh=zh, pts=pts, items=items, want=[_answer(ref, *it) for it in items])
    return _SEEDS[n]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 13, 14, 15, 16])
def test_rounds_batch_vs_oracle(hip, oracle, n):
    """40 instances per n as one call, non-strict; n = 14, 15, 16 straddle the 64-coefficient edge of
    the t(x) numerator (62, 66, 70 coefficients)"""
    I = _seeded(oracle, n)
    assert sum(w[1] is None for w in I["want"]) >= 35
    assert all(w[1] in (None, SLICE_MSG) for w in I["want"])
    pr = hip.Prover(n, I["zh"], I["pts"])
    assert pr.batch_path(circuit=False) == 1
    proofs, status = pr.rounds_batch(*_pack(I["items"]))
    assert not _diff(hip, proofs, status, I["want"])


class _Recording(RefProver):
    """remembers the remainder of its first division (t(x)'s) and the longest committed length"""
    rem = None
    longest = 0

    def divide(self, num, den):
        q, r = super().divide(num, den)
        if self.rem is None:
            self.rem = r
        return q, r

    def commit(self, p):
        self.longest = max(self.longest, len(p))
        return super().commit(p)


def test_srs_boundary_inside_a_batch(hip, oracle):
    """n = 16: 33 points change nothing; with 32 exactly the entries whose longest commitment is 33
    (w_z's quotient, 2n + 1) take the SRS exit and the rest keep their proofs"""
    n = 16
    I = _seeded(oracle, n)
    longest = []
    for it in I["items"]:
        rec = _ref(oracle, I["pts"], n, I["zh"], _Recording)
        _answer(rec, *it)
        longest.append(rec.longest)
    data = _pack(I["items"])
    for ln in (33, 32):
        pts = np.ascontiguousarray(I["pts"][:ln])
        ref = _ref(oracle, pts, n, I["zh"])
        want = [_answer(ref, *it) for it in I["items"]]
        pr = hip.Prover(n, I["zh"], pts)
        assert pr.batch_path(circuit=False) == 1
        proofs, status = pr.rounds_batch(*data)
        assert not _diff(hip, proofs, status, want), ln
        if ln == 33:
            assert want == I["want"]
        else:
            srs = {i for i, w in enumerate(want) if w[1] == SRS_MSG}
            assert srs == {i for i, w in enumerate(I["want"]) if w[1] is None and longest[i] == 33}
            assert 1 <= len(srs) < 40 and any(w[1] is None for w in want)
            assert all(int(status[i]) == hip.PLK_ERR_RANGE | (X_SRS << 8) for i in srs)
        pr.close()


def _strict_case(oracle, n, seed):
    """a strictly valid synthetic instance: q_c = -(the t(x) remainder at q_c = 0), Z_H = x^n - 1 having
    one more coefficient than q_c (the construction of tests/test_prove_edges_gpu.py)"""
    polys, chal, rnd, zh, pts = gen.prove_instance(n, seed, 2 * n + 8)
    polys = [p.copy() for p in polys]
    polys[QC] = np.zeros(n, np.uint8)
    rec = _ref(oracle, pts, n, zh, _Recording)
    loose = rec.rounds(polys, chal, rnd, strict=False)
    r = np.zeros(n, np.int64)
    r[:len(rec.rem)] = rec.rem
    assert np.any(r) and len(rec.rem) <= n
    polys[QC] = ((17 - r) % 17).astype(np.uint8)
    want = _ref(oracle, pts, n, zh).rounds(polys, chal, rnd, strict=True)
    assert want == loose
    return dict(polys=polys, chal=chal, rnd=rnd, zh=zh, pts=pts, want=want)


@pytest.mark.parametrize("n,seed", [(5, 3), (16, 6)])
def test_strict_accept_and_one_changed_coefficient(hip, oracle, n, seed):
    c = _strict_case(oracle, n, seed)
    pr = hip.Prover(n, c["zh"], c["pts"])
    assert pr.batch_path(circuit=False) == 1
    good = (c["polys"], c["chal"], c["rnd"])
    for k in sorted({0, 1, n // 2, n - 1}):
        qc = c["polys"][QC].copy()
        qc[k] = (qc[k] + 1) % 17
        broken = list(c["polys"])
        broken[QC] = qc
        items = [good, good, (broken, c["chal"], c["rnd"]), good, good]
        proofs, status = pr.rounds_batch(*_pack(items), strict=True)
        want = [(c["want"], None)] * 2 + [(None, REM_MSG)] + [(c["want"], None)] * 2
        assert not _diff(hip, proofs, status, want), k
        assert int(status[2]) == hip.PLK_ERR_ARG | (X_REM_T << 8)
        proofs, status = pr.rounds_batch(*_pack(items), strict=False)      # q_c only moves the remainder
        assert not _diff(hip, proofs, status, [(c["want"], None)] * 5), k


def _edge_cases(n, polys, chal, rnd):
    """name -> (polys, chal, rnd): the 36 degenerate variants of one dense instance
    (tests/test_prove_edges_gpu.py's set)"""
    zero = np.zeros(n, np.uint8)

    def P(**kw):
        out = [p.copy() for p in polys]
        for i, v in kw.items():
            out[int(i[1:])] = v
        return out

    def Z(*idx):
        return P(**{"p%d" % i: zero.copy() for i in idx})

    def C(**kw):
        c = list(chal)
        for k, v in kw.items():
            c[("alpha", "beta", "gamma", "z", "v").index(k)] = v
        return c

    def R(*zeroed):
        return [0 if i + 1 in zeroed else x for i, x in enumerate(rnd)]

    upper = [p.copy() for p in polys]
    const = [p.copy() for p in polys]
    for p in upper:
        p[n // 2:] = 0
    for p in const:
        p[1:] = 0
    cases = {
        "plain": (P(), C(), R()),
        "zero blinding": (P(), C(), R(*range(1, 10))),
        "b1=0": (P(), C(), R(1)),
        "b7=0": (P(), C(), R(7)),
        "b7=b8=0": (P(), C(), R(7, 8)),
        "beta=0": (P(), C(beta=0), R()),
        "gamma=0": (P(), C(gamma=0), R()),
        "beta=gamma=0": (P(), C(beta=0, gamma=0), R()),
        "v=0": (P(), C(v=0), R()),
        "z=0": (P(), C(z=0), R()),
        "z=1": (P(), C(z=1), R()),
        "z=16": (P(), C(z=16), R()),
        "alpha=0": (P(), C(alpha=0), R()),
        "challenges zero": (P(), [0] * 5, R()),
        "upper half zero": (upper, C(), R()),
        "constants": (const, C(), R()),
        "selectors zero": (Z(QO, QM, QL, QR, QC), C(), R()),
        "f_a=0 unblinded": (Z(FA), C(), R(1, 2)),
        "acc_x=0": (Z(ACC), C(), R()),
        "all zero": (Z(*range(13)), C(), R()),
        "all zero, zero blinding": (Z(*range(13)), C(), R(*range(1, 10))),
        "sigmas zero": (Z(S1, S2, S3), C(), R()),
        "l_1=0": (Z(L1), C(), R()),
    }
    for i in range(13):
        cases["only %s=0" % NAMES[i]] = (Z(i), C(), R())
    assert len(cases) == 36
    return cases


def test_degenerate_variants_in_one_batch(hip, oracle):
    n = 16
    polys, chal, rnd, zh, pts = gen.prove_instance(n, 7, 2 * n + 8)
    cases = _edge_cases(n, polys, chal, rnd)
    ref = _ref(oracle, pts, n, zh)
    names = list(cases)
    want = [_answer(ref, *cases[k]) for k in names]
    assert sum(w[1] is None for w in want) >= 25
    assert want[names.index("f_a=0 unblinded")][0][:3] == bytes([0, 0, 1])
    pr = hip.Prover(n, zh, pts)
    assert pr.batch_path(circuit=False) == 1
    proofs, status = pr.rounds_batch(*_pack([cases[k] for k in names]))
    bad = _diff(hip, proofs, status, want)
    assert not bad, {names[i]: v for i, v in bad.items()}
    assert _split(proofs, status)[names.index("f_a=0 unblinded")][:3] == bytes([0, 0, 1])


@pytest.mark.parametrize("zl,path", [(9, 1), (3, 1), (10, 0)])
def test_zh_shapes(hip, oracle, zl, path):
    """n = 8 with a dense canonical Z_H (lead 5): length n + 1 and 3 run the fused kernel, n + 2 the
    composition; all three against the oracle"""
    n = 8
    insts = [gen.prove_instance(n, seed, 2 * n + 12) for seed in range(1, 9)]
    zh = (np.arange(zl) * 7 + 3) % 17
    zh[-1] = 5
    zh = zh.astype(np.uint8)
    pts = insts[0][4]
    items = [(p, c, r) for p, c, r, _, _ in insts]
    ref = _ref(oracle, pts, n, zh)
    want = [_answer(ref, *it) for it in items]
    assert sum(w[1] is None for w in want) >= 6
    pr = hip.Prover(n, zh, pts)
    assert pr.batch_path(circuit=False) == path
    proofs, status = pr.rounds_batch(*_pack(items))
    assert not _diff(hip, proofs, status, want)


def _rounds_single(hip, pr, item, strict=False):
    polys, chal, rnd = item
    d = [torch.from_numpy(np.ascontiguousarray(p)).to("cuda") for p in polys]
    try:
        return pr.rounds_dev(d, chal, rnd, strict=strict), None
    except hip.PlonkHipError as e:
        if e.code not in (hip.PLK_ERR_ARG, hip.PLK_ERR_RANGE):
            raise
        return None, str(e).split("): ", 1)[1], e.code


def _dev_call(pr, data, batch, stream=None, strict=False):
    d = [torch.from_numpy(x.reshape(-1)).to("cuda") for x in data]
    proofs = torch.full((34 * batch,), 0xEE, dtype=torch.uint8, device="cuda")
    status = torch.full((batch,), -1, dtype=torch.int32, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())     # the fills above
    pr.rounds_batch_dev(d[0], d[1], d[2], batch, proofs, status, strict=strict, stream=stream)
    return d, proofs, status


def test_composition_fallbacks(hip, oracle):
    """an irregular SRS (pts[5] off the curve) and n = 17 take path 0: the host form is the single calls
    entry by entry, the _dev form PLK_ERR_RANGE"""
    n = 8
    I = _seeded(oracle, n)
    pts = I["pts"].copy()
    pts[5] = [7, 7, 0]
    items = I["items"][:6]
    pr = hip.Prover(n, I["zh"], pts)
    assert pr.batch_path(circuit=False) == 0
    proofs, status = pr.rounds_batch(*_pack(items))
    want = [_rounds_single(hip, pr, it) for it in items]
    assert not _diff(hip, proofs, status, want)
    assert want != I["want"][:6]
    with pytest.raises(hip.PlonkHipError) as e:
        _dev_call(pr, _pack(items), len(items))
    assert e.value.code == hip.PLK_ERR_RANGE and "not eligible" in str(e.value)
    torch.cuda.synchronize()
    n = 17
    insts = [gen.prove_instance(n, seed, 2 * n + 8) for seed in range(1, 4)]
    items = [(p, c, r) for p, c, r, _, _ in insts]
    pr = hip.Prover(n, insts[0][3], insts[0][4])
    assert pr.batch_path(circuit=False) == 0
    ref = _ref(oracle, insts[0][4], n, insts[0][3])
    proofs, status = pr.rounds_batch(*_pack(items))
    assert not _diff(hip, proofs, status, [_answer(ref, *it) for it in items])


def test_dev_forms_on_two_streams(hip, oracle):
    """two provers on two torch streams, then synchronized: the bytes and statuses of the host form; a
    byte 17 in one entry is the INPUT exit and its neighbours are exact"""
    out = []
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    keep = []
    for n, st in zip((16, 5), streams):
        I = _seeded(oracle, n) if n == 16 else None
        if I is None:
            insts = [gen.prove_instance(n, seed, 2 * n + 8) for seed in range(1, 41)]
            I = dict(zh=insts[0][3], pts=insts[0][4], items=[(p, c, r) for p, c, r, _, _ in insts])
        data = [x.copy() for x in _pack(I["items"])]
        data[0][13 * n * 3 + 5] = 17                    # entry 3: one polynomial byte out of range
        pr = hip.Prover(n, I["zh"], I["pts"])
        keep.append((pr, data, _dev_call(pr, data, 40, stream=st)))
    torch.cuda.synchronize()
    for pr, data, (_, proofs, status) in keep:
        hp, hs = pr.rounds_batch(*data)
        assert proofs.cpu().numpy().tobytes() == hp
        assert np.array_equal(status.cpu().numpy().astype(np.uint32), hs)
        assert int(hs[3]) == hip.PLK_ERR_ARG | (X_INPUT << 8) and hp[34 * 3:34 * 4] == bytes(34)
        assert hip.prove_exit_message(int(hs[3])) != ""
        out.append((hp, hs))
    # entry 3's neighbours: the oracle's answers of the unmodified batch (n = 16)
    I = _seeded(oracle, 16)
    want = list(I["want"])
    got = _split(*out[0])
    assert all(got[i] == (want[i][0] or bytes(34)) for i in range(40) if i != 3)
    assert sum(int(s) == 0 for s in out[0][1]) >= 34


def test_prove_batch_dev_matches_host_form(hip):
    G = _geometry(hip)
    cir, ch, rd = _entries(G["cases"])
    d = [torch.from_numpy(np.frombuffer(cir, np.uint8).copy()).to("cuda"), torch.from_numpy(ch.reshape(-1)).to("cuda"),
         torch.from_numpy(rd.reshape(-1)).to("cuda")]
    proofs = torch.full((34 * 64,), 0xEE, dtype=torch.uint8, device="cuda")
    status = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    G["pr"].prove_batch_dev(d[0], d[1], d[2], 64, proofs, status, stream=st)
    st.synchronize()
    hp, hs = G["pr"].prove_batch(cir, ch, rd)
    assert proofs.cpu().numpy().tobytes() == hp and np.array_equal(status.cpu().numpy().astype(np.uint32), hs)
    assert not _diff(hip, hp, hs, G["ans"])
