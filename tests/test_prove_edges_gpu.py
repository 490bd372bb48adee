"""Device prover on the inputs that dense random instances never produce.

prove.hip carries every polynomial at its upper-bound length and recomputes the reference's
trimmed lengths on the device, to decide the reference's exits (check_status) and to clamp each
commitment row (msm_row_lens).  Dense inputs have trimmed length == upper bound, so here the
inputs are degenerate on purpose:

* n = 4: every proof and every rejection the compiled reference recorded for four circuits (one
  with q_c != 0) under zeroed challenges / blinding and SRS lengths around the commitment lengths
  (tests/golden/prove_edges.json; the CPU restatement is pinned to the same file by
  tests/test_prove_cpu.py).
* rounds 1-5 at n = 64, 1000 (and zero tails of 20000+ coefficients at n = 40000) with scalars
  and polynomials zeroed, against the restatement oracle/prove_ref.py -- proofs byte for byte,
  exits with the reference's message and the error code of its kind.
* the SRS length check from both sides: the shortest SRS the oracle accepts (L*) gives the
  proof, one point fewer the reference's exit, in every commitment form.
* strict mode accepted above n = 4: q_c only moves the remainder of the t(x) division, so
  q_c = -(remainder at q_c = 0) makes a synthetic instance strictly valid, and one changed
  coefficient of q_c brings the exit back.
"""
import numpy as np
import pytest
import torch

import gen
from conftest import load_golden
from prove_ref import Prover as RefProver, ProveError
from prove_strict_case import strict_case as _strict_case

pytestmark = pytest.mark.gpu

SRS_MSG = "SRS length is less than polynomial length"
SLICE_MSG = "Invalid slice indices in poly_slice"
REM_MSG = "Non-zero remainder in t(x) division"
FA, FB, FC, QO, QM, QL, QR, QC, S1, S2, S3, ACC, L1 = range(13)
NAMES = ("f_a", "f_b", "f_c", "q_o", "q_m", "q_l", "q_r", "q_c", "s1", "s2", "s3", "acc_x", "l_1")


def _code(hip, msg):
    """the error code of each kind of reference exit (check_status in prove.hip)"""
    if msg in (SRS_MSG, SLICE_MSG):
        return hip.PLK_ERR_RANGE
    assert "remainder" in msg or "poly_is_zero" in msg, msg
    return hip.PLK_ERR_ARG


def _dev(polys):
    return [torch.from_numpy(np.ascontiguousarray(p)).to("cuda") for p in polys]


def _ref(oracle, pts, n, zh, cls=RefProver):
    return cls(oracle, np.ascontiguousarray(pts).tobytes(), n, z_h=zh.tobytes())


def _answer(ref, polys, chal, rnd, strict=False):
    """(proof, None) or (None, the exit's message)"""
    try:
        return ref.rounds(polys, chal, rnd, strict=strict), None
    except ProveError as e:
        return None, str(e)


def _same(hip, call, want, msg):
    """'' if the device call gives the oracle's proof / takes the oracle's exit, else what differs"""
    try:
        got = call()
    except hip.PlonkHipError as e:
        if e.code not in (hip.PLK_ERR_ARG, hip.PLK_ERR_RANGE):
            raise                     # not a reference exit: a runtime failure ends the test
        if msg is None:
            return "device raised %s, oracle proof %s" % (e, want.hex())
        if msg not in str(e) or e.code != _code(hip, msg):
            return "device raised %s (code %d), oracle exit %r" % (e, e.code, msg)
        return ""
    if msg is not None:
        return "device proof %s, oracle exit %r" % (got.hex(), msg)
    return "" if got == want else "device %s != oracle %s" % (got.hex(), want.hex())


# ------------------------------------------------------------------ n = 4: reference-recorded edges
def _expand(g, case):
    return dict(g["circuits"][case["circuit"]], **case)


def _circuit(case):
    gt, cp, w = case["gates"], case["copies"], case["wires"]
    return dict(q_m=gt[0:4], q_l=gt[4:8], q_r=gt[8:12], q_o=gt[12:16], q_c=gt[16:20],
                copy_a=cp[0:8], copy_b=cp[8:16], copy_c=cp[16:24], a=w[0:4], b=w[4:8], c=w[8:12])


@pytest.mark.parametrize("logs", [1, 0])
def test_prove_edge_fixtures(hip, logs):
    """plk_prover_prove against tests/golden/prove_edges.json, with the commitments from the SRS in
    log form (the default) and in G1 form"""
    g = load_golden("prove_edges.json")
    assert len(g["proofs"]) >= 100 and len(g["failures"]) >= 100
    provers, bad = {}, []
    with hip.options(PROVE_SRS_LOGS=logs):
        for case in g["proofs"] + g["failures"]:
            key = "%d/%d" % (case["srs_n"], case["srs_mode"])
            if key not in provers:
                s = {k: bytes.fromhex(v) for k, v in g["setups"][key].items()}
                provers[key] = hip.Prover(4, s["z_h"], s["g1s"], s["h"], s["k1_h"], s["k2_h"], s["h_pows_inv"])
            c = _expand(g, case)
            try:
                got = provers[key].prove(**_circuit(c), chal=c["chal"], rand=c["rand"]).hex()
            except hip.PlonkHipError as e:
                if e.code not in (hip.PLK_ERR_ARG, hip.PLK_ERR_RANGE):
                    raise
                got = None
            if got != case["proof"]:
                bad.append((case["circuit"], case["variant"], key, got, case["proof"]))
    assert not bad, bad


# ------------------------------------------------------------------ degenerate synthetic inputs
def _edge_cases(n, polys, chal, rnd):
    """name -> (polys, chal, rnd): the 36 degenerate variants of one dense instance"""
    zero = np.zeros(n, np.uint8)

    def P(**kw):                      # polynomials replaced by index
        out = [p.copy() for p in polys]
        for i, v in kw.items():
            out[int(i[1:])] = v
        return out

    def Z(*idx):
        return P(**{"p%d" % i: zero.copy() for i in idx})

    def C(**kw):                      # alpha beta gamma z v
        c = list(chal)
        for k, v in kw.items():
            c[("alpha", "beta", "gamma", "z", "v").index(k)] = v
        return c

    def R(*zeroed):                   # b1..b9 zeroed by number
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
    assert len(cases) == 23
    for i in range(13):               # each polynomial zeroed alone (acc_x and l_1 a second time)
        cases["only %s=0" % NAMES[i]] = (Z(i), C(), R())
    assert len(cases) == 36
    return cases


SIZES = [(64, 7), (1000, 4)]
EXITS = ("alpha=0", "challenges zero", "all zero, zero blinding")   # the oracle's three exits, at both sizes
_INST = {}


def _instance(oracle, n, seed):
    """one dense instance, its 36 degenerate variants and the oracle's answers (once per module)"""
    if (n, seed) not in _INST:
        polys, chal, rnd, zh, pts = gen.prove_instance(n, seed, 2 * n + 8)
        ref = _ref(oracle, pts, n, zh)
        cases = _edge_cases(n, polys, chal, rnd)
        want = {k: _answer(ref, *c) for k, c in cases.items()}
        _INST[n, seed] = dict(n=n, zh=zh, pts=pts, cases=cases, want=want)
    return _INST[n, seed]


@pytest.mark.parametrize("n,seed", SIZES)
def test_rounds_degenerate_vs_oracle(hip, oracle, n, seed):
    """The 36 variants through rounds_dev (non-strict): the oracle's 34 bytes, or the oracle's exit.
    33 of the 36 are proofs (asserted: at least 30), so an exit cannot stand in for a wrong proof;
    f_a = 0 unblinded commits to the zero polynomial, the identity 00 00 01."""
    I = _instance(oracle, n, seed)
    exits = {k: m for k, (_, m) in I["want"].items() if m is not None}
    assert len(I["want"]) == 36 and len(exits) <= 6
    assert exits == {k: SLICE_MSG for k in EXITS}, exits
    assert I["want"]["f_a=0 unblinded"][0][:3] == bytes([0, 0, 1])
    pr = hip.Prover(n, I["zh"], I["pts"])
    bad = {}
    for name, (polys, chal, rnd) in I["cases"].items():
        d = _dev(polys)
        diff = _same(hip, lambda: pr.rounds_dev(d, chal, rnd, strict=False), *I["want"][name])
        if diff:
            bad[name] = diff
    assert not bad, bad


_TAILS = {}


@pytest.mark.parametrize("name", ["zero blinding", "upper half zero", "f_a=0 unblinded"])
def test_rounds_long_zero_tails(hip, oracle, name):
    """n = 40000: zero tails of 20000+ coefficients (more than 16 KiB) in front of the trim scans"""
    n, seed = 40000, 9
    if not _TAILS:
        polys, chal, rnd, zh, pts = gen.prove_instance(n, seed, 2 * n + 8)
        _TAILS.update(zh=zh, pts=pts, cases=_edge_cases(n, polys, chal, rnd))
    polys, chal, rnd = _TAILS["cases"][name]
    want, msg = _answer(_ref(oracle, _TAILS["pts"], n, _TAILS["zh"]), polys, chal, rnd)
    assert msg is None
    pr = hip.Prover(n, _TAILS["zh"], _TAILS["pts"])
    assert pr.rounds_dev(_dev(polys), chal, rnd, strict=False).hex() == want.hex()


# ------------------------------------------------------------------ SRS boundary
def _lstar(oracle, I, name):
    """the smallest SRS length at which the oracle accepts the case (the accept set is monotone
    in the length: srs_eval_at_s only compares lengths), by bisection; cached"""
    memo = I.setdefault("lstar", {})
    if name not in memo:
        polys, chal, rnd = I["cases"][name]
        n, pts = I["n"], I["pts"]
        lo, hi = 0, len(pts)           # lo rejects (nothing fits in no points), hi accepts
        while hi - lo > 1:
            mid = (lo + hi) // 2
            want, msg = _answer(_ref(oracle, pts[:mid], n, I["zh"]), polys, chal, rnd)
            assert msg in (None, SRS_MSG), (name, mid, msg)
            lo, hi = (lo, mid) if msg is None else (mid, hi)
        want, msg = _answer(_ref(oracle, pts[:hi], n, I["zh"]), polys, chal, rnd)
        assert msg is None and want == I["want"][name][0]   # the points past a commitment's length are not read
        memo[name] = hi
    return memo[name]


LSTAR = {"plain": (129, 2001), "zero blinding": (125, 1998), "b7=0": (128, 2000), "b7=b8=0": (127, 1998),
         "beta=0": (67, 1003), "v=0": (67, 1003), "upper half zero": (97, 1003)}


def _boundary(hip, I, name, L, pre=False, irregular=None):
    """'' if a prover over pts[:L] gives the oracle's proof and one over pts[:L - 1] the SRS exit"""
    polys, chal, rnd = I["cases"][name]
    d = _dev(polys)
    out = []
    for ln, (want, msg) in ((L, I["want"][name]), (L - 1, (None, SRS_MSG))):
        pr = hip.Prover(I["n"], I["zh"], np.ascontiguousarray(I["pts"][:ln]))
        if pre:
            pr.preprocess(d)
        diff = _same(hip, lambda: pr.rounds_dev(d, chal, rnd, strict=False, preprocessed=pre), want, msg)
        if diff:
            out.append("SRS %d: %s" % (ln, diff))
        pr.close()
    return "; ".join(out)


@pytest.mark.parametrize("n,seed", SIZES)
def test_srs_boundary_every_case(hip, oracle, n, seed):
    """L* and L* - 1 for every accepted case at n = 64 and for the tabulated seven at n = 1000.
    Where L* = n + 3 (beta = 0, v = 0, and at n = 1000 the half-zero inputs) the SRS is about half
    the upper-bound commitment length: those rows run with msm_row_lens clamped to the SRS."""
    I = _instance(oracle, n, seed)
    names = [k for k, (_, m) in I["want"].items() if m is None] if n == 64 else list(LSTAR)
    assert len(names) >= (30 if n == 64 else 7)
    bad = {}
    for name in names:
        L = _lstar(oracle, I, name)
        if name in LSTAR:
            assert L == LSTAR[name][SIZES.index((n, seed))], (name, L)
        assert n + 3 <= L <= 2 * n + 1
        diff = _boundary(hip, I, name, L)
        if diff:
            bad[name] = diff
    assert not bad, bad


FORMS = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]   # (SRS_LOGS, PACK_FUSE, EARLY_COMMITS)


@pytest.mark.parametrize("n,seed", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_srs_boundary_commitment_forms(hip, oracle, n, seed, form):
    """The same pair under each commitment form -- log form fused (early commitments in round 5's
    division launch, or in none), log form unfused, G1 form -- plain and preprocessed"""
    I = _instance(oracle, n, seed)
    bad = {}
    with hip.options(PROVE_SRS_LOGS=form[0], PROVE_PACK_FUSE=form[1], PROVE_EARLY_COMMITS=form[2]):
        for name in ("plain", "beta=0", "zero blinding"):
            for pre in (False, True):
                diff = _boundary(hip, I, name, _lstar(oracle, I, name), pre=pre)
                if diff:
                    bad[name, pre] = diff
    assert not bad, bad


@pytest.mark.parametrize("n,seed", SIZES)
def test_srs_boundary_irregular_srs(hip, oracle, n, seed):
    """beta = 0 at L* = n + 3 over an SRS with an off-curve point below L*: the serial-fold
    commitments (whatever PROVE_SRS_LOGS says) with their lengths clamped to the SRS"""
    I = _instance(oracle, n, seed)
    polys, chal, rnd = I["cases"]["beta=0"]
    L = _lstar(oracle, I, "beta=0")
    assert L == n + 3
    pts = np.ascontiguousarray(I["pts"][:L]).copy()
    pts[5] = [7, 7, 0]                      # off the curve y^2 = x^3 + 3
    want, msg = _answer(_ref(oracle, pts, n, I["zh"]), polys, chal, rnd)
    assert msg is None and want != I["want"]["beta=0"][0]
    d = _dev(polys)
    for logs in (1, 0):
        with hip.options(PROVE_SRS_LOGS=logs):
            pr = hip.Prover(n, I["zh"], pts)
            assert pr.rounds_dev(d, chal, rnd, strict=False).hex() == want.hex(), logs
            short = hip.Prover(n, I["zh"], np.ascontiguousarray(pts[:L - 1]))
            assert _same(hip, lambda: short.rounds_dev(d, chal, rnd, strict=False), None, SRS_MSG) == ""


# ------------------------------------------------------------------ strict acceptance
STRICT_SIZES = [(37, 2), (1000, 4), (5000, 7), (65536, 41)]


@pytest.mark.parametrize("n,seed", STRICT_SIZES)
def test_strict_accept_and_single_coefficient(hip, oracle, n, seed):
    """rounds_dev(strict) accepts with the oracle's strict proof -- the first strict accept above
    n = 4, and the first test in which q_c matters: one coefficient of q_c changed, at the first /
    last byte, around 16-byte and 256-thread edges and mid-array, and strict takes the remainder
    exit while the non-strict bytes stay (a remainder flag that misses a block, or q_c read at a
    wrong offset or scale, fails here)."""
    c = _strict_case(oracle, n, seed)
    pr = hip.Prover(n, c["zh"], c["pts"])
    d = _dev(c["polys"])
    assert pr.rounds_dev(d, c["chal"], c["rnd"], strict=True).hex() == c["want"].hex()
    assert pr.rounds_dev(d, c["chal"], c["rnd"], strict=False).hex() == c["want"].hex()
    bad = {}
    for k in sorted({k for k in (0, 1, 15, 16, 255, 256, n // 2, n - 1) if k < n}):
        qc = c["polys"][QC].copy()
        qc[k] = (qc[k] + 1) % 17
        e = list(d)
        e[QC] = torch.from_numpy(qc).to("cuda")
        diff = _same(hip, lambda: pr.rounds_dev(e, c["chal"], c["rnd"], strict=True), None, REM_MSG)
        diff += _same(hip, lambda: pr.rounds_dev(e, c["chal"], c["rnd"], strict=False), c["want"], None)
        if diff:
            bad[k] = diff
    assert not bad, bad
    # the instance's own dense q_c: the remainder exit again, the same non-strict bytes
    e = list(d)
    e[QC] = torch.from_numpy(c["dense_qc"]).to("cuda")
    assert _same(hip, lambda: pr.rounds_dev(e, c["chal"], c["rnd"], strict=True), None, REM_MSG) == ""
    assert pr.rounds_dev(e, c["chal"], c["rnd"], strict=False).hex() == c["want"].hex()


@pytest.mark.parametrize("n,seed", STRICT_SIZES)
def test_strict_accept_every_division_form(hip, oracle, n, seed):
    """The strict accept where the round-5 remainder words come from other kernels: the generic
    two-launch division (q_m at an odd address, twice), a preprocessed circuit, and the split proof
    (chains_dev + rounds_ext_dev, both chains)"""
    c = _strict_case(oracle, n, seed)
    pr = hip.Prover(n, c["zh"], c["pts"])
    d = _dev(c["polys"])
    chal, rnd, want = c["chal"], c["rnd"], c["want"].hex()
    # q_m at an odd address: round 5's numerators by lincomb_batch, then the two-launch scan
    backing = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    backing[3:3 + n] = d[QM]
    odd = list(d)
    odd[QM] = backing[3:3 + n]
    assert odd[QM].data_ptr() % 16 == 3
    for _ in range(2):
        assert pr.rounds_dev(odd, chal, rnd, strict=True).hex() == want, "q_m at an odd address"
    pr.preprocess(d)
    assert pr.rounds_dev(d, chal, rnd, strict=True, preprocessed=True).hex() == want
    pr.preprocess(None)
    # q_c at an odd address: the numerator and its division by Z_H in separate launches
    backing = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    backing[3:3 + n] = d[QC]
    odd = list(d)
    odd[QC] = backing[3:3 + n]
    assert odd[QC].data_ptr() % 4 == 3
    assert pr.rounds_dev(odd, chal, rnd, strict=True).hex() == want
    backing[3 + n - 1] = (backing[3 + n - 1] + 1) % 17        # one coefficient changed in place
    assert _same(hip, lambda: pr.rounds_dev(odd, chal, rnd, strict=True), None, REM_MSG) == ""
    helper =hip.Prover(n, c["zh"], c["pts"])
    t2 = torch.zeros(pr.chain_bytes(hip.PLK_CHAIN_T2), dtype=torch.uint8, device="cuda")
    t3 = torch.zeros(pr.chain_bytes(hip.PLK_CHAIN_T3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    helper.chains_dev(d, chal, rnd, 3, t2, t3, done=st)
    assert pr.rounds_ext_dev(d, chal, rnd, 3, t2, t3, ready=st, strict=True).hex() == want
    torch.cuda.synchronize()
    helper.close()


@pytest.mark.parametrize("n,seed", STRICT_SIZES)
def test_strict_srs_exit_comes_first(hip, oracle, n, seed):
    """Strict, the fixed q_c: an SRS of n + 1 points is the SRS exit (the `a` commitment comes
    before the division), and so is L* - 1 (only the last commitments do not fit: after every
    remainder check passed); L* itself accepts.  With the instance's dense q_c (a non-zero
    remainder) both exits are due: n + 1 points is still the SRS exit, L* - 1 the remainder exit
    (the division comes before the commitments that do not fit).  The oracle's messages,
    check_status's order."""
    c = _strict_case(oracle, n, seed)
    L = c["lstar"]
    assert n + 3 < L <= 2 * n + 1
    d = _dev(c["polys"])
    dense = list(c["polys"])
    dense[QC] = c["dense_qc"]
    e = list(d)
    e[QC] = torch.from_numpy(c["dense_qc"]).to("cuda")
    for ln in (n + 1, L - 1, L):
        pts = np.ascontiguousarray(c["pts"][:ln])
        pr = hip.Prover(n, c["zh"], pts)
        want, msg = c["want"], None       # (L* is the longest length commit() saw: nothing past it is read)
        if ln < L:
            want, msg = _answer(_ref(oracle, pts, n, c["zh"]), c["polys"], c["chal"], c["rnd"], strict=True)
            assert msg == SRS_MSG
            _, both = _answer(_ref(oracle, pts, n, c["zh"]), dense, c["chal"], c["rnd"], strict=True)
            assert both == (SRS_MSG if ln == n + 1 else REM_MSG)
            assert _same(hip, lambda: pr.rounds_dev(e, c["chal"], c["rnd"], strict=True), None, both) == "", ln
        assert _same(hip, lambda: pr.rounds_dev(d, c["chal"], c["rnd"], strict=True), want, msg) == "", ln
        pr.close()
