"""The public device API is closed under the operations of a PLONK proof: plk_prover_rounds_dev's 34 bytes
against a proof assembled ONLY from public _dev calls -- plk_poly_lincomb_batch_dev, plk_poly_mul_dev,
plk_poly_divide_dev, plk_poly_eval_batch_dev, plk_kzg_commit_batch_dev and plk_kzg_open_batch_dev --
following oracle/prove_ref.py (src/plonk.h:277-655) step by step, the product of two committed polynomials
in r(x) included.  Polynomial data never returns to the host: only trimmed lengths (the d_nz words) and
evaluations are read back, as a caller driving the protocol would read them.  Both sides must equal each
other and the reference's recorded proof bytes (tests/golden/prove.json, tests/golden/prove_circuits.json)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from prove_circuit_cases import expand, is_proof, long_key
from prove_ref import K1, K2, OMEGA, Prover as RefProver, hpow

pytestmark = pytest.mark.gpu

P = 17
REC = 2176


class Capture(RefProver):
    """the restatement, keeping the 13 interpolated polynomials it hands to rounds()"""

    def rounds(self, polys, chal, rnd, strict=True):
        self.polys = [np.asarray(p, np.uint8).copy() for p in polys]
        return super().rounds(polys, chal, rnd, strict)


class DP:
    """a device polynomial: tensor, offset, trimmed length"""

    def __init__(self, t, n, off=0):
        self.t, self.n, self.off = t, int(n), int(off)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.off


def dev_const(vals):
    a = np.asarray(vals, np.uint8)
    nz = np.flatnonzero(a)
    n = int(nz[-1]) + 1 if nz.size else 1
    return DP(torch.from_numpy(a.copy()).cuda(), n)


class PublicProver:
    def __init__(self, hip, srs_g1, n, z_h):
        self.hip, self.n = hip, n
        self.srs = hip.Srs(srs_g1)
        assert not self.srs.irregular
        self.zh_host = np.frombuffer(bytes(z_h), np.uint8)
        self.zh = dev_const(self.zh_host)
        self.zh_host = self.zh_host[:self.zh.n]
        self.calls = {"lincomb": 0, "mul": 0, "divide": 0, "eval": 0, "commit": 0, "open": 0}

    def close(self):
        self.srs.close()

    # -- the public calls
    def lc(self, jobs):
        """jobs: [([(DP, {shift, sub, scale, neg, twist})...], add_hf)] -> [DP] with trimmed lengths"""
        hip = self.hip
        call, outs = [], []
        for terms, add_hf in jobs:
            L = max(p.n + kw.get("shift", 0) for p, kw in terms)
            out = torch.empty(L, dtype=torch.uint8, device="cuda")
            outs.append(out)
            call.append(([hip.lc_term(p.ptr, len=p.n, **kw) for p, kw in terms], add_hf, out))
        nz = torch.empty(len(jobs), dtype=torch.int32, device="cuda")
        hip.poly_lincomb_batch_dev(call, nz)
        self.calls["lincomb"] += 1
        return [DP(o, max(int(v), 1)) for o, v in zip(outs, nz.cpu().tolist())]

    def mul(self, a, b):
        hip = self.hip
        out = torch.empty(a.n + b.n - 1, dtype=torch.uint8, device="cuda")
        nz = torch.empty(1, dtype=torch.int32, device="cuda")
        work = torch.empty(max(hip.poly_mul_workspace(a.n, b.n), 16), dtype=torch.uint8, device="cuda")
        hip.poly_mul_dev(a.ptr, a.n, b.ptr, b.n, out, nz, work)
        self.calls["mul"] += 1
        return DP(out, max(int(nz.item()), 1))

    def divide(self, num, den_host):
        hip = self.hip
        nl, dl = num.n, len(den_host)
        assert nl >= dl
        quot = torch.empty(nl - dl + 1, dtype=torch.uint8, device="cuda")
        rem = torch.empty(max(dl - 1, 1), dtype=torch.uint8, device="cuda")
        lens = torch.empty(2, dtype=torch.int32, device="cuda")
        work = torch.empty(max(hip.poly_divide_workspace(nl, dl), 16), dtype=torch.uint8, device="cuda")
        hip.poly_divide_dev(num.ptr, nl, den_host, quot, rem, lens, work)
        self.calls["divide"] += 1
        ql, rl = lens.cpu().tolist()
        return DP(quot, max(ql, 1)), rl

    def evals(self, polys, xs):
        hip = self.hip
        ys = torch.empty(len(polys), dtype=torch.uint8, device="cuda")
        tick = torch.zeros(max(hip.poly_eval_workspace(len(polys)), 16), dtype=torch.uint8, device="cuda")
        hip.poly_eval_batch_dev([p.ptr for p in polys], [p.n for p in polys], xs, ys, tick)
        self.calls["eval"] += 1
        return [int(v) for v in ys.cpu().tolist()]

    def records(self, res, k):
        out = []
        for r in res.cpu().numpy().reshape(k, REC):
            d = self.hip.parse_result(r.tobytes())
            assert d["irregular"] == 0
            out.append(d["g1"])
        return out

    def commit(self, polys):
        hip = self.hip
        res = torch.zeros(len(polys) * REC, dtype=torch.uint8, device="cuda")
        hip.kzg_commit_dev(self.srs, [p.ptr for p in polys], [p.n for p in polys], res)
        self.calls["commit"] += 1
        return self.records(res, len(polys))

    def open(self, polys, zs):
        """-> the proofs: commitments of (p - p(z)) / (x - z)"""
        hip = self.hip
        k = len(polys)
        res = torch.zeros(k * REC, dtype=torch.uint8, device="cuda")
        ys = torch.empty(k, dtype=torch.uint8, device="cuda")
        lens = [p.n for p in polys]
        work = torch.empty(max(hip.kzg_workspace(lens), 16), dtype=torch.uint8, device="cuda")
        hip.kzg_open_dev(self.srs, [p.ptr for p in polys], lens, zs, ys, res, None, work)
        self.calls["open"] += 1
        return self.records(res, k)

    # -- src/plonk.h:277-655 as oracle/prove_ref.py restates it
    def rounds(self, dev_polys, chal, rnd):
        n, lc, mul = self.n, self.lc, self.mul
        al, be, ga, z, v = (x % P for x in chal)
        b1, b2, b3, b4, b5, b6, b7, b8, b9 = (x % P for x in rnd)
        zh = self.zh
        # the inputs as polynomials: their trimmed lengths (a copy pass that also gives d_nz)
        fa, fb, fc, q_o, q_m, q_l, q_r, q_c, s1, s2, s3, acc_x, l_1 = lc([([(DP(t, n), {})], None) for t in dev_polys])
        # round 1
        ba, bb, bc = mul(dev_const([b2, b1]), zh), mul(dev_const([b4, b3]), zh), mul(dev_const([b6, b5]), zh)
        a_x, b_x, c_x = lc([([(ba, {}), (fa, {})], None), ([(bb, {}), (fb, {})], None), ([(bc, {}), (fc, {})], None)])
        a_s, b_s, c_s = self.commit([a_x, b_x, c_x])
        # round 2
        z_x, = lc([([(mul(dev_const([b9, b8, b7]), zh), {}), (acc_x, {})], None)])
        z_s, = self.commit([z_x])
        # round 3
        ab_qm, a_ql, b_qr, c_qo = mul(mul(a_x, b_x), q_m), mul(a_x, q_l), mul(b_x, q_r), mul(c_x, q_o)
        g_b, g_bk1, g_bk2 = dev_const([ga, be]), dev_const([ga, be * K1 % P]), dev_const([ga, be * K2 % P])
        al2 = hpow(al, 2)
        t1, A2, B2, C2, A3, B3, C3, zw, zm1 = lc([
            ([(ab_qm, {}), (a_ql, {}), (b_qr, {}), (c_qo, {}), (dev_const([0]), {}), (q_c, {})], None),
            ([(a_x, {"scale": al}), (g_b, {"scale": al})], None),                 # poly_scale(a_x + (ga + be x), al)
            ([(b_x, {}), (g_bk1, {})], None),
            ([(c_x, {}), (g_bk2, {})], None),
            ([(a_x, {"scale": al}), (s1, {"scale": al * be % P})], al * ga % P),   # poly_scale(a_x + be s1 + ga, al)
            ([(b_x, {}), (s2, {"scale": be})], ga),
            ([(c_x, {}), (s3, {"scale": be})], ga),
            ([(z_x, {"twist": OMEGA})], None),                                    # z_x(omega x), src/plonk.h:466-470
            ([(z_x, {"scale": al2})], al2 * (P - 1) % P),                         # poly_scale(z_x - 1, al^2)
        ])
        t2 = mul(mul(mul(A2, B2), C2), z_x)
        t3 = mul(mul(mul(A3, B3), C3), zw)
        t4 = mul(zm1, l_1)
        num, = lc([([(t1, {}), (t2, {}), (t3, {"sub": 1}), (t4, {})], None)])
        t_x, rem_len = self.divide(num, self.zh_host)
        part = n + 2
        assert t_x.n > 2 * part, "Invalid slice indices in poly_slice"
        t_lo, t_mid, t_hi = lc([([(DP(t_x.t, part), {})], None), ([(DP(t_x.t, part, part), {})], None),
                                ([(DP(t_x.t, t_x.n - 2 * part, 2 * part), {})], None)])      # poly_slice: p + start
        t_lo_s, t_mid_s, t_hi_s = self.commit([t_lo, t_mid, t_hi])
        # round 4
        a_z, b_z, c_z, s1_z, s2_z, t_z, zw_z, l1_z = self.evals([a_x, b_x, c_x, s1, s2, t_x, zw, l_1], [z] * 8)
        s3s, = lc([([(s3, {"scale": be * zw_z % P})], None)])
        x1 = (a_z + be * z + ga) % P
        x2 = (b_z + be * K1 % P * z + ga) % P
        x3 = (c_z + be * K2 % P * z + ga) % P
        y1 = (a_z + be * s1_z + ga) % P
        y2 = (b_z + be * s2_z + ga) % P
        r_x, = lc([([(q_m, {"scale": a_z * b_z % P}), (q_l, {"scale": a_z}), (q_r, {"scale": b_z}), (q_o, {"scale": c_z}),
                     (z_x, {"scale": x1 * x2 % P * x3 % P * al % P}),
                     (mul(z_x, s3s), {"scale": y1 * y2 % P * al % P}),           # a product of two committed polynomials
                     (z_x, {"scale": l1_z * al2 % P})], None)])
        r_z, = self.evals([r_x], [z])
        # round 5: sum_i w_i (p_i - p_i(z)), then its opening at z; z_x's at z omega
        vp = [hpow(v, k) for k in range(7)]
        const = (t_z + v * r_z + vp[2] * a_z + vp[3] * b_z + vp[4] * c_z + vp[5] * s1_z + vp[6] * s2_z) % P
        w, = lc([([(t_lo, {}), (t_mid, {"scale": hpow(z, n + 2)}), (t_hi, {"scale": hpow(z, 2 * n + 4)}),
                   (r_x, {"scale": v}), (a_x, {"scale": vp[2]}), (b_x, {"scale": vp[3]}), (c_x, {"scale": vp[4]}),
                   (s1, {"scale": vp[5]}), (s2, {"scale": vp[6]})], (P - const) % P)])
        w_s, = self.open([w], [z])
        wo_s, = self.open([z_x], [z * OMEGA % P])
        return b"".join([a_s, b_s, c_s, z_s, t_lo_s, t_mid_s, t_hi_s, w_s, wo_s]) + \
            bytes([a_z, b_z, c_z, s1_z, s2_z, r_z, zw_z])


def both_sides(hip, oracle, n, s, circuit, chal, rnd):
    """(public-API proof, plk_prover_rounds_dev's proof, the restatement's proof) for one circuit"""
    gt, cp, w = circuit
    ref = Capture(oracle, s["g1s"], n, s["h"], s["k1_h"], s["k2_h"], s["h_pows_inv"], s["z_h"])
    copies = [list(zip(cp[2 * n * k:2 * n * (k + 1):2], cp[2 * n * k + 1:2 * n * (k + 1):2])) for k in range(3)]
    want = ref.prove(*(gt[n * k:n * (k + 1)] for k in range(5)), copies, w[0:n], w[n:2 * n], w[2 * n:3 * n], chal, rnd)
    dev = []
    for p in ref.polys:                       # as tests/test_prove_gpu.py: each zero padded to n bytes
        full = np.zeros(n, np.uint8)
        full[:len(p)] = p
        dev.append(torch.from_numpy(full).to("cuda"))
    pr = hip.Prover(n, s["z_h"], s["g1s"])
    fused = pr.rounds_dev(dev, chal, rnd, strict=True)
    pr.close()
    pub = PublicProver(hip, s["g1s"], n, s["z_h"])
    try:
        got = pub.rounds(dev, chal, rnd)
    finally:
        pub.close()
    assert pub.calls["lincomb"] >= 8 and pub.calls["mul"] >= 17
    return got, fused, want


def test_n4_reference_proofs_from_public_calls(hip, oracle):
    g = load_golden("prove.json")
    assert len(g["proofs"]) >= 26
    for case in g["proofs"]:
        s = {k: bytes.fromhex(v) for k, v in g["setups"][str(case["srs_mode"])].items()}
        assert case["srs_n"] == 6
        got, fused, want = both_sides(hip, oracle, 4, s, (case["gates"], case["copies"], case["wires"]), case["chal"],
                                      case["rand"])
        assert got.hex() == fused.hex() == case["proof"] == want.hex(), (case["chal"], case["rand"], case["srs_mode"])


def test_n16_reference_proof_from_public_calls(hip, oracle):
    sets = expand(load_golden("prove_circuits.json"))
    n, s, cases = sets[long_key(16)]
    # (n = 16 has proofs only for the kinds with zero selectors; "mixed" has non-trivial copies and wires)
    c = [c for c in cases if is_proof(c["outcome"]) and c["kind"] == "mixed"][0]
    got, fused, want = both_sides(hip, oracle, 16, s, (c["gates"], c["copies"], c["wires"]), c["chal"], c["rand"])
    assert got.hex() == fused.hex() == c["outcome"] == want.hex(), (c["kind"], c["seed"])
