#!/usr/bin/env python3
"""The folded KZG opening and its verification against what a user composes from the older entry
points (DESIGN, "KZG folded openings"), in one process on the same inputs.

Opening, one group of k polynomials of n coefficients at one z, k in 2, 9, 16, n in 2^20, 2^22:
  fold      plk_kzg_open_fold_batch_dev: F in registers, 1-2 launches
  compose   (a) plk_poly_eval_batch_dev for the ys, an elementwise torch fold of the k device
            polynomials mod 17 (F through HBM), plk_kzg_open_batch_dev on F
  separate  (b) plk_kzg_open_batch_dev on the k polynomials: k proofs
Verification, n jobs of k commitments, n in 2^20, 2^24, k in 2, 9, 16:
  fold      plk_kzg_verify_fold_batch_dev: n jobs
  separate  (b) plk_kzg_verify_batch_dev on n k single openings
Both baselines run this commit's older entry points only.  Each time is a pair of device events
around one variant on the stream, after warm-up; the variants alternate and the median of the repeats
is kept.  The inputs rotate through enough distinct buffer sets (twice the 256 MB last-level cache)
that a call never finds its input cached (the SRS is resident by design and stays warm).  fold and
compose are compared byte for byte at every opening shape.  The fraction of the 8 TB/s HBM peak
counts the folded opening's algorithmic bytes: every polynomial twice and the logs once, (2 k + 1) n.

  python tools/kzg_fold_bench.py [--out profiles/kzg_fold_bench.json] [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk.c_amd"))

import torch  # noqa: E402

import plonkhip as h  # noqa: E402

HBM_PEAK = 8e12
LLC_BYTES = 256 << 20
REC = h.MSM_RESULT_BYTES
OPEN_KS, OPEN_LENGTHS = (2, 9, 16), (1 << 20, 1 << 22)
VERIFY_KS, VERIFY_SIZES = (2, 9, 16), (1 << 20, 1 << 24)
KG = [(0, 0, 1), (1, 2, 0), (68, 74, 0), (26, 45, 0), (65, 98, 0), (12, 32, 0), (32, 42, 0), (91, 35, 0), (18, 49, 0),
      (18, 52, 0), (91, 66, 0), (32, 59, 0), (12, 69, 0), (65, 3, 0), (26, 56, 0), (68, 27, 0), (1, 99, 0)]


def srs_points(n):
    """n points uniform over all 102 group elements (seeded)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen
    pts, _ = gen.msm_inputs(0x5125, n, "full")
    return pts


def timed(fns, reps, warm=3):
    for k in range(warm):
        for f in fns.values():
            f(k)
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for k in range(reps):
        for name, f in fns.items():   # alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(k)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}


class OpenCase:
    def __init__(self, srs, n, k):
        self.srs, self.n, self.k = srs, n, k
        self.sets = -(-2 * LLC_BYTES // (n * k))
        g = torch.Generator(device="cuda")
        g.manual_seed(n + k)
        self.stride = (n + 15) & ~15
        self.polys = [torch.randint(0, 17, (k, self.stride), dtype=torch.uint8, device="cuda", generator=g)
                      for _ in range(self.sets)]
        for p in self.polys:
            p[:, n - 1] = 1 + p[:, n - 1] % 16
        self.lens = [n] * k
        self.z = 5
        self.weights = [(1 + 3 * i) % 17 for i in range(k)]           # 1, 4, 7, ...: the first is 1 as in round 5
        self.d_w = torch.tensor(self.weights, dtype=torch.int32, device="cuda").view(-1, 1)
        self.ys = [torch.zeros(k, dtype=torch.uint8, device="cuda") for _ in range(3)]
        self.res = [torch.zeros(k * REC, dtype=torch.uint8, device="cuda") for _ in range(3)]
        self.fwork = torch.empty(h.kzg_fold_workspace(self.lens, [0, k]), dtype=torch.uint8, device="cuda")
        self.work1 = torch.empty(h.kzg_workspace([n]), dtype=torch.uint8, device="cuda")
        self.workk = torch.empty(h.kzg_workspace(self.lens), dtype=torch.uint8, device="cuda")
        self.tick = torch.zeros(h.poly_eval_workspace(k), dtype=torch.uint8, device="cuda")
        self.yF = torch.zeros(1, dtype=torch.uint8, device="cuda")

    def rows(self, i):
        p = self.polys[i % self.sets]
        return p, [p[b] for b in range(self.k)]

    def fold(self, i):
        _, rows = self.rows(i)
        h.kzg_open_fold_dev(self.srs, rows, self.lens, self.weights, [0, self.k], [self.z], self.ys[0], self.res[0],
                            work=self.fwork)

    def compose(self, i):
        p, rows = self.rows(i)
        h.poly_eval_batch_dev(rows, self.lens, [self.z] * self.k, self.ys[1], self.tick)
        F = torch.remainder((p.to(torch.int32) * self.d_w).sum(0), 17).to(torch.uint8)
        h.kzg_open_dev(self.srs, [F], [self.n], [self.z], self.yF, self.res[1], work=self.work1)

    def separate(self, i):
        _, rows = self.rows(i)
        h.kzg_open_dev(self.srs, rows, self.lens, [self.z] * self.k, self.ys[2], self.res[2], work=self.workk)

    def proof(self, which):
        x = h.parse_result(self.res[which][:REC].cpu().numpy())
        return x["g1"], x["irregular"]

    def measure(self, reps):
        self.fold(0)
        self.compose(0)
        self.separate(0)
        torch.cuda.synchronize()
        assert self.proof(0) == self.proof(1) and self.proof(0)[1] == 0, "fold and compose disagree"
        assert self.ys[0].cpu().tolist() == self.ys[1].cpu().tolist() == self.ys[2].cpu().tolist()
        return timed({"fold": self.fold, "compose": self.compose, "separate": self.separate}, reps)


class VerifyCase:
    def __init__(self, n, k):
        self.n, self.k = n, k
        e = n * k
        self.sets = max(2, -(-2 * LLC_BYTES // (5 * e + 4 * n)))
        g = torch.Generator(device="cuda")
        g.manual_seed(n * 31 + k)
        kg = torch.tensor(KG, dtype=torch.uint8, device="cuda")

        def pts(m):
            return kg[torch.randint(0, 17, (m,), device="cuda", generator=g)].reshape(-1).contiguous()

        def hf(m):
            return torch.randint(0, 17, (m,), dtype=torch.uint8, device="cuda", generator=g)

        # per set: commits e x 3, weights e, ys e, zs n, proofs n x 3
        self.sets_in = [(pts(e), hf(e), hf(e), hf(n), pts(n)) for _ in range(self.sets)]
        # the separate openings need a z and a proof per commitment: one shared set (e x 4 more bytes)
        self.zs_e, self.proofs_e = hf(e), pts(e)
        self.ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.ok_e = torch.zeros(e, dtype=torch.uint8, device="cuda")
        self.vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))

    def fold(self, i):
        c, w, y, z, p = self.sets_in[i % self.sets]
        h.kzg_verify_fold_dev(self.vk, self.k, c, w, y, z, p, self.n, self.ok)

    def separate(self, i):
        c, _, y, _, _ = self.sets_in[i % self.sets]
        h.kzg_verify_dev(self.vk, c, self.zs_e, y, self.proofs_e, self.n * self.k, self.ok_e)

    def measure(self, reps):
        return timed({"fold": self.fold, "separate": self.separate}, reps)


def write_record(path, res):
    """one measured row per line"""
    head = {k: v for k, v in res.items() if k not in ("open", "verify")}
    with open(path, "w") as f:
        f.write(json.dumps(head, indent=1)[:-2])
        for key in ("open", "verify"):
            f.write(',\n "%s": [\n  %s\n ]' % (key, ",\n  ".join(json.dumps(r) for r in res[key])))
        f.write("\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_fold_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    h.init(0)
    srs = h.Srs(srs_points(max(OPEN_LENGTHS)))
    assert not srs.irregular
    opens, verifies = [], []
    for n in OPEN_LENGTHS:
        for k in OPEN_KS:
            c = OpenCase(srs, n, k)
            med, mn = c.measure(a.reps)
            alg = (2 * k + 1) * n
            row = {"len": n, "k": k, "buffer_sets": c.sets, "fold_us": med["fold"], "compose_us": med["compose"],
                   "separate_us": med["separate"], "fold_min_us": mn["fold"], "compose_min_us": mn["compose"],
                   "separate_min_us": mn["separate"], "compose_over_fold": med["compose"] / med["fold"],
                   "separate_over_fold": med["separate"] / med["fold"], "fold_alg_bytes": alg,
                   "fold_fraction_of_hbm_peak": alg / (med["fold"] * 1e-6) / HBM_PEAK}
            opens.append(row)
            print("open  len 2^%d k %2d: fold %9.1f us  compose %9.1f us (x%.2f)  separate %9.1f us (x%.2f)  %.3f of 8 TB/s"
                  % (n.bit_length() - 1, k, med["fold"], med["compose"], row["compose_over_fold"], med["separate"],
                     row["separate_over_fold"], row["fold_fraction_of_hbm_peak"]), flush=True)
            del c
            torch.cuda.empty_cache()
    srs.close()
    for n in VERIFY_SIZES:
        for k in VERIFY_KS:
            c = VerifyCase(n, k)
            med, mn = c.measure(a.reps if n < 1 << 24 else max(5, a.reps // 3))
            row = {"n": n, "k": k, "buffer_sets": c.sets, "fold_us": med["fold"], "separate_us": med["separate"],
                   "fold_min_us": mn["fold"], "separate_min_us": mn["separate"],
                   "separate_over_fold": med["separate"] / med["fold"], "fold_jobs_per_s": n / (med["fold"] * 1e-6),
                   "fold_commitments_per_s": n * k / (med["fold"] * 1e-6),
                   "separate_openings_per_s": n * k / (med["separate"] * 1e-6)}
            verifies.append(row)
            print("verify n 2^%d k %2d: fold %10.1f us  separate (n k openings) %10.1f us  x%.2f" %
                  (n.bit_length() - 1, k, med["fold"], med["separate"], row["separate_over_fold"]), flush=True)
            del c
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around one variant, variants alternating, median of the repeats after warm-up",
           "baselines": {"compose": "plk_poly_eval_batch_dev + torch fold mod 17 + plk_kzg_open_batch_dev on F",
                         "separate": "k single openings (plk_kzg_open_batch_dev) / n k single verifications "
                                     "(plk_kzg_verify_batch_dev)"},
           "open": opens, "verify": verifies}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write_record(a.out, res)


if __name__ == "__main__":
    main()
