"""Device prover from caller buffers at every alignment, surrounded by bytes that would change the
proof if read.

rounds() (plonk.c_amd/csrc/prove.hip) chooses its kernels from the address of each caller
polynomial mod 16 and mod 4, n % 4 and n % 16 (tests/prove_variant_cases.py restates the rules);
every choice must give the oracle's 34 bytes.  Each polynomial sits in its own allocation at a
chosen residue with 64 bytes of poison that is non-zero mod 17 on both sides (tests/devbuf.py), so
a 16-byte or 4-byte load that reads past n, an unmasked tail or a wrong buffer limit changes the
proof instead of meeting the zeros of a fresh allocation.  The oracle's proof is computed once per
size; every placement is compared with those bytes, never with another device run, the backing
buffers must come back unchanged, and the counted kernel launches must differ from the aligned
placement's by the derived launch_delta.
"""
import pytest
import torch

import devbuf
import gen
import prove_variant_cases as V
from prove_ref import Prover as RefProver
from prove_strict_case import strict_case

pytestmark = pytest.mark.gpu

REM_MSG = "Non-zero remainder in t(x) division"
FIXED = (3, 4, 5, 6, 10, 12)          # q_o q_m q_l q_r s_sigma_3 l_1_x: what preprocess() transforms
_CASE = {}


def _case(oracle, n):
    """the size's instance and the oracle's proof (once per module)"""
    if n not in _CASE:
        polys, chal, rnd, zh, pts = gen.prove_instance(n, V.SIZES[n], 2 * n + 8)
        want = RefProver(oracle, pts.tobytes(), n, z_h=zh.tobytes()).rounds(polys, chal, rnd, strict=False)
        _CASE[n] = dict(n=n, polys=polys, chal=chal, rnd=rnd, zh=zh, pts=pts, want=want)
    return _CASE[n]


class Placed:
    """the 13 polynomials, each in its own poisoned allocation at its residue"""

    def __init__(self, polys, residues, poison="canon"):
        assert len(polys) == len(residues) == 13
        pairs = [devbuf.place(p, r, poison=poison, seed=i) for i, (p, r) in enumerate(zip(polys, residues))]
        self.backing = [b for b, _ in pairs]
        self.views = [v for _, v in pairs]
        assert [v.data_ptr() % 16 for v in self.views] == list(residues)
        self.snap = [devbuf.snapshot(b) for b in self.backing]
        torch.cuda.synchronize()      # (the prover runs on its own stream)

    def changed(self):
        """names of the polynomials whose backing buffer no longer holds what was placed"""
        torch.cuda.synchronize()
        return [V.NAMES[i] for i, (b, s) in enumerate(zip(self.backing, self.snap)) if not devbuf.unchanged(b, s)]


def _answer(hip, call):
    """the proof's hex, or the reference exit's message"""
    try:
        return call().hex()
    except hip.PlonkHipError as e:
        if e.code not in (hip.PLK_ERR_ARG, hip.PLK_ERR_RANGE):
            raise                     # not a reference exit: a runtime failure ends the test
        return "exit: %s" % e


# ------------------------------------------------------------------ single polynomial and mixes
@pytest.mark.parametrize("poison", ["canon", "raw"])
@pytest.mark.parametrize("n", sorted(V.SIZES))
def test_placements_vs_oracle(hip, oracle, n, poison):
    """Lists (a) (at 1008, 1000, 1001), (b) and (c) with "canon" poison, (b) and (c) again with
    "raw": the oracle's bytes, every backing buffer unchanged, and the counted launches minus the
    aligned placement's equal to launch_delta.  The aligned placement is itself a poisoned one
    (at n % 16 != 0 its 16-byte tail loads must be masked: vec == 1)."""
    c = _case(oracle, n)
    pr = hip.Prover(n, c["zh"], c["pts"])
    want = c["want"].hex()
    base = Placed(c["polys"], V.ALIGNED, poison)
    assert _answer(hip, lambda: pr.rounds_dev(base.views, c["chal"], c["rnd"], strict=False)) == want
    assert base.changed() == []
    k0, other0 = pr.launches(base.views, c["chal"], c["rnd"])
    cases = V.placements(n) if poison == "canon" else V.TOGETHER + V.MIXES
    bad, measured = {}, {}
    for name, res in cases:
        p = Placed(c["polys"], res, poison)
        got = _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"], strict=False))
        if got != want:
            bad[name] = "proof %s, oracle %s" % (got, want)
        if p.changed():
            bad[name, "inputs"] = p.changed()
        k, _ = pr.launches(p.views, c["chal"], c["rnd"])
        measured[name] = k - k0
        if k - k0 != V.launch_delta(n, res):
            bad[name, "launches"] = "measured %+d, derived %+d (%s)" % (k - k0, V.launch_delta(n, res),
                                                                        V.variants(n, res))
    print("n = %d (%s): aligned %d kernels + %d other nodes; launch deltas %s" % (n, poison, k0, other0, measured))
    pr.close()
    assert not bad, bad


# ------------------------------------------------------------------ strict
@pytest.mark.parametrize("n", sorted(V.STRICT))
def test_strict_accepts_at_every_placement(hip, oracle, n):
    """The strictly valid instances: rounds_dev(strict) accepts with the oracle's strict bytes at
    every placement of lists (a) and (b) -- q_c enters through numdiv_kernel's dword loads or the
    lincomb + division launches, and a misread coefficient is a remainder exit."""
    c = strict_case(oracle, n, V.STRICT[n])
    pr = hip.Prover(n, c["zh"], c["pts"])
    want = c["want"].hex()
    bad = {}
    for name, res in [("aligned", V.ALIGNED)] + V.SINGLE + V.TOGETHER:
        p = Placed(c["polys"], res)
        got = _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"], strict=True))
        if got != want:
            bad[name] = "%s, oracle %s" % (got, want)
        if p.changed():
            bad[name, "inputs"] = p.changed()
    pr.close()
    assert not bad, bad


@pytest.mark.parametrize("n", sorted(V.STRICT))
def test_strict_q_c_in_place(hip, oracle, n):
    """q_c at each of its residues, the other twelve aligned.  The first poison byte after q_c
    changed in place: the proof and its acceptance stay (that byte is not q_c's).  One coefficient
    of q_c changed in place (the last, beside the poison; then the first): the remainder exit,
    while the non-strict bytes stay."""
    c = strict_case(oracle, n, V.STRICT[n])
    pr = hip.Prover(n, c["zh"], c["pts"])
    want = c["want"].hex()
    bad = {}
    for r in (0, 1, 2, 4, 8, 12, 15):
        p = Placed(c["polys"], V.only(V.QC, r=r))
        back, qc = p.backing[V.QC], p.views[V.QC]
        off = qc.data_ptr() - back.data_ptr()
        strict = lambda: _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"], strict=True))
        loose = lambda: _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"], strict=False))
        if strict() != want:
            bad[r, "accept"] = strict()
        for step in (1, 2, 7):                       # (stays non-zero mod 17 for poison in 1..16)
            back[off + n] = (int(back[off + n].item()) + step) % 17 or 5
            torch.cuda.synchronize()
            if strict() != want:
                bad[r, "poison after q_c +%d" % step] = strict()
        back[off - 1] = (int(back[off - 1].item()) + 3) % 17 or 5
        torch.cuda.synchronize()
        if strict() != want:
            bad[r, "poison before q_c"] = strict()
        for k in (n - 1, 0):
            old = int(qc[k].item())
            qc[k] = (old + 1) % 17
            torch.cuda.synchronize()
            if REM_MSG not in strict():
                bad[r, "coefficient %d" % k] = strict()
            if loose() != want:
                bad[r, "coefficient %d, non-strict" % k] = loose()
            qc[k] = old
            torch.cuda.synchronize()
        if strict() != want:
            bad[r, "restored"] = strict()
    pr.close()
    assert not bad, bad


# ------------------------------------------------------------------ options
@pytest.mark.parametrize("n", V.OPTION_SIZES)
def test_options_at_placements(hip, oracle, n):
    """List (b) and the q_c-only, q_m-only and s_sigma_1-only placements under the option
    values of test_round5_divisions_vs_oracle (PROVE_EARLY_COMMITS), the combinations of
    test_commitments_srs_log_form (PROVE_SRS_LOGS / PROVE_PACK_FUSE /
    PROVE_EARLY_COMMITS) and test_derive_t2a_modes_vs_oracle: the oracle's bytes, and the launch
    difference from the aligned placement under the same options."""
    c = _case(oracle, n)
    pr = hip.Prover(n, c["zh"], c["pts"])
    want = c["want"].hex()
    base = Placed(c["polys"], V.ALIGNED)
    placed = [(name, res, Placed(c["polys"], res)) for name, res in V.OPTION_PLACEMENTS]
    bad = {}
    for opt in V.OPTION_SETS:
        key = ",".join("%s=%d" % (k[6:], v) for k, v in opt.items())
        with hip.options(**opt):
            if _answer(hip, lambda: pr.rounds_dev(base.views, c["chal"], c["rnd"], strict=False)) != want:
                bad["aligned", key] = "differs from the oracle"
            k0, _ = pr.launches(base.views, c["chal"], c["rnd"])
            for name, res, p in placed:
                got = _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"], strict=False))
                if got != want:
                    bad[name, key] = "proof %s, oracle %s" % (got, want)
                k, _ = pr.launches(p.views, c["chal"], c["rnd"])
                if k - k0 != V.launch_delta(n, res, opt):
                    bad[name, key, "launches"] = "measured %+d, derived %+d" % (k - k0, V.launch_delta(n, res, opt))
    for name, _, p in placed + [("aligned", None, base)]:
        if p.changed():
            bad[name, "inputs"] = p.changed()
    pr.close()
    assert not bad, bad


# ------------------------------------------------------------------ preprocessed
@pytest.mark.parametrize("n", V.PREPROCESSED_SIZES)
def test_preprocessed_from_misaligned_inputs(hip, oracle, n):
    """preprocess() with the six fixed polynomials at residues 1, 4 and 15 in poisoned buffers (the
    other seven aligned), then rounds_dev(preprocessed): the oracle's bytes, repeatedly, inputs
    unchanged.  Then one byte of q_l changed in place: the transforms held by the prover are stale
    (include/plonkhip.h: call preprocess again after a change) -- the plain call reads the new
    bytes whatever is held, and after preprocess() the preprocessed call does too; both against
    the oracle's proof of the new bytes."""
    c = _case(oracle, n)
    pr = hip.Prover(n, c["zh"], c["pts"])
    want = c["want"].hex()
    new = [p.copy() for p in c["polys"]]
    new[V.QL][n - 1] = (new[V.QL][n - 1] + 1) % 17
    want2 = RefProver(oracle, c["pts"].tobytes(), n, z_h=c["zh"].tobytes()).rounds(new, c["chal"], c["rnd"],
                                                                                   strict=False).hex()
    assert want2 != want
    for r in (1, 4, 15):
        p = Placed(c["polys"], V.only(*FIXED, r=r))
        pr.preprocess(p.views)
        for _ in range(2):
            assert _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"], preprocessed=True)) == want, r
        assert _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"])) == want, r
        assert p.changed() == [], r
        p.views[V.QL][n - 1] = int(new[V.QL][n - 1])
        torch.cuda.synchronize()
        assert _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"])) == want2, r
        pr.preprocess(p.views)
        assert _answer(hip, lambda: pr.rounds_dev(p.views, c["chal"], c["rnd"], preprocessed=True)) == want2, r
        assert p.changed() == [V.NAMES[V.QL]], r
        pr.preprocess(None)
    pr.close()


# ------------------------------------------------------------------ split proof
@pytest.mark.parametrize("n", V.SPLIT_SIZES)
def test_split_proof_from_misaligned_inputs(hip, oracle, n):
    """chains_dev with both chains on a second prover, then rounds_ext_dev, from the inputs of list
    (b); the chain buffers stay 16-byte aligned, as the API requires."""
    c = _case(oracle, n)
    pr = hip.Prover(n, c["zh"], c["pts"])
    helper = hip.Prover(n, c["zh"], c["pts"])
    both = hip.PLK_CHAIN_T2 | hip.PLK_CHAIN_T3
    st = torch.cuda.Stream()
    bad = {}
    for name, res in V.TOGETHER:
        p = Placed(c["polys"], res)
        t2 = torch.full((pr.chain_bytes(hip.PLK_CHAIN_T2),), 0xEE, dtype=torch.uint8, device="cuda")
        t3 = torch.full((pr.chain_bytes(hip.PLK_CHAIN_T3),), 0xEE, dtype=torch.uint8, device="cuda")
        assert t2.data_ptr() % 16 == 0 and t3.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        helper.chains_dev(p.views, c["chal"], c["rnd"], both, t2, t3, done=st)
        got = _answer(hip, lambda: pr.rounds_ext_dev(p.views, c["chal"], c["rnd"], both, t2, t3, ready=st))
        torch.cuda.synchronize()
        if got != c["want"].hex():
            bad[name] = "proof %s, oracle %s" % (got, c["want"].hex())
        if p.changed():
            bad[name, "inputs"] = p.changed()
    helper.close()
    pr.close()
    assert not bad, bad
