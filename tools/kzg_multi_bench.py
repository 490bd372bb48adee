#!/usr/bin/env python3
"""The multi-point KZG opening against what a user composes from the older entry points (DESIGN section
19), in one process on the same inputs.

One group per shape: polynomials p_i, each opened at its own point set, one challenge u.
  fused     plk_kzg_open_multi_batch_dev: ys, h and W in one fused launch (an aggregates launch in front of
            it past 4096 coefficients), then the folded opening's launches for W'
  compose   plk_poly_divide_short_batch_dev (every q_i through HBM), plk_poly_lincomb_batch_dev (h),
            plk_kzg_commit_batch_dev (W), plk_kzg_open_fold_batch_dev on (p_i, h) (W'); the evaluations, which
            the fused call also returns, are left out of it
Both run this commit's public _dev calls.  Each time is a pair of device events around one variant on the
stream, after warm-up; the variants alternate -- the composition twice per round, as compose and compose_b --
and the median of the repeats is kept.  The spread of the composition is the larger of the gap between its two
interleaved medians and its own 10th-to-90th percentile width, over its median; the fused call is held to be
faster only when it wins by more than that.  The inputs rotate through enough distinct buffer sets (twice the
256 MB last-level cache) that a call never finds its polynomials cached (the SRS is resident by design and
stays warm).  The records of fused and compose are compared byte for byte at every shape.  The fraction of the
8 TB/s HBM peak counts the fused path's algorithmic bytes: every polynomial four times, h written once and read
twice, the logs twice -- (4 k + 5) N for k polynomials of N coefficients.

  python tools/kzg_multi_bench.py [--out profiles/kzg_multi_bench.json] [--reps 30]
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
Z, ZW = 3, 12          # a point and its image under omega = 4
PAIR = 1 << Z | 1 << ZW


def shapes():
    """(name, lengths, sets as masks)"""
    n = 1 << 22
    return [
        ("plonk 8 at {z}, 1 at {z, z w}, 2^22", [n] * 9, [1 << Z] * 8 + [PAIR]),
        ("plonk 8 at {z}, 1 at {z, z w}, 2^20", [1 << 20] * 9, [1 << Z] * 8 + [PAIR]),
        ("9 at the same 2 points, 2^22", [n] * 9, [PAIR] * 9),
        ("9 at 2 points each, 9 different pairs, 2^22", [n] * 9, [1 << a | 1 << (a + 8) for a in range(9)]),
        ("1 at 16 points, 2^22", [n], [0xFFFF]),
        ("9 of 4096 (one chunk), plonk sets", [4096] * 9, [1 << Z] * 8 + [PAIR]),
        ("ragged, 9 polynomials up to 2^22, mixed sets",
         [n, (1 << 21) + 5, 1 << 20, 3 * (1 << 20) + 17, 4097, n - 3, 17, 1 << 19, 12345],
         [1 << Z, PAIR, 0b1110, 1, PAIR, 1 << Z | 1, 0xFFFF, 1 << 16, PAIR]),
    ]


def srs_points(n):
    """n points uniform over all 102 group elements (seeded)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen
    pts, _ = gen.msm_inputs(0x5125, n, "full")
    return pts


def points(mask):
    return [a for a in range(17) if (mask >> a) & 1]


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
    return times


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


class Case:
    def __init__(self, srs, lens, sets):
        self.srs, self.lens, self.masks, self.k = srs, lens, sets, len(lens)
        k = self.k
        total = sum(lens)
        self.nsets = max(2, min(64, -(-2 * LLC_BYTES // total)))
        g = torch.Generator(device="cuda")
        g.manual_seed(total + k)
        self.polys = []
        for _ in range(self.nsets):
            row = [torch.randint(0, 17, ((n + 15) & ~15,), dtype=torch.uint8, device="cuda", generator=g) for n in lens]
            for p, n in zip(row, lens):
                p[n - 1] = 1 + p[n - 1] % 16
            self.polys.append(row)
        self.u = 7
        self.weights = [(1 + 3 * i) % 17 or 1 for i in range(k)]
        self.ts = [len(points(m)) for m in sets]
        self.lh = max(max(n - t, 1) for n, t in zip(lens, self.ts))
        # fused
        self.ys = torch.zeros(17 * k, dtype=torch.uint8, device="cuda")
        self.res = torch.zeros(2 * REC, dtype=torch.uint8, device="cuda")
        self.work = torch.empty(h.kzg_multi_workspace(lens, sets, [0, k]), dtype=torch.uint8, device="cuda")
        # compose
        self.dens = [h.poly_from_roots(points(m)) for m in sets]
        self.qlens = [max(n - t, 1) for n, t in zip(lens, self.ts)]
        self.quots = [torch.empty((q + 15) & ~15, dtype=torch.uint8, device="cuda") for q in self.qlens]
        self.rems = [torch.empty(16, dtype=torch.uint8, device="cuda") for _ in lens]
        self.dlens = torch.zeros(3 * k, dtype=torch.int32, device="cuda")
        self.dwork = torch.empty(max(256, h.poly_divide_short_workspace([(n, t + 1) for n, t in zip(lens, self.ts)])),
                                 dtype=torch.uint8, device="cuda")
        self.hbuf = torch.empty((self.lh + 15) & ~15, dtype=torch.uint8, device="cuda")
        self.cres = torch.zeros(2 * REC, dtype=torch.uint8, device="cuda")
        self.c = h.kzg_multi_coeffs(sets, self.weights, self.u)
        self.fys = torch.zeros(k + 1, dtype=torch.uint8, device="cuda")
        self.fwork = torch.empty(h.kzg_fold_workspace(lens + [self.lh], [0, k + 1]), dtype=torch.uint8, device="cuda")

    def fused(self, i):
        h.kzg_open_multi_dev(self.srs, self.polys[i % self.nsets], self.lens, self.masks, self.weights, [0, self.k], [self.u],
                             self.ys, self.res, work=self.work)

    def compose(self, i):
        row = self.polys[i % self.nsets]
        h.poly_divide_short_batch_dev([(p, n, d, q, r) for p, n, d, q, r in zip(row, self.lens, self.dens, self.quots, self.rems)],
                                      self.dlens, self.dwork)
        h.poly_lincomb_batch_dev([([h.lc_term(q, len=ql, scale=w) for q, ql, w in zip(self.quots, self.qlens, self.weights)],
                                   None, self.hbuf)])
        h.kzg_commit_dev(self.srs, [self.hbuf], [self.lh], self.cres[:REC])
        h.kzg_open_fold_dev(self.srs, row + [self.hbuf], self.lens + [self.lh], self.c, [0, self.k + 1], [self.u], self.fys,
                            self.cres[REC:], work=self.fwork)

    def records(self, res):
        b = res.cpu().numpy()
        return [(x["g1"], x["irregular"]) for x in (h.parse_result(b[:REC]), h.parse_result(b[REC:]))]

    def measure(self, reps):
        self.fused(0)
        self.compose(0)
        torch.cuda.synchronize()
        a, b = self.records(self.res), self.records(self.cres)
        assert a == b and a[0][1] == 0 and a[1][1] == 0, ("fused and compose disagree", a, b)
        return timed({"fused": self.fused, "compose": self.compose, "compose_b": self.compose}, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_multi_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    h.init(0)
    srs = h.Srs(srs_points(1 << 22))
    assert not srs.irregular
    rows = []
    for name, lens, sets in shapes():
        c = Case(srs, lens, sets)
        t = c.measure(a.reps)
        med = {k: statistics.median(v) for k, v in t.items()}
        both = t["compose"] + t["compose_b"]
        cmed = statistics.median(both)
        spread = max(abs(med["compose"] - med["compose_b"]), pct(both, 0.9) - pct(both, 0.1)) / cmed
        alg = sum(4 * n for n in lens) + 5 * c.lh
        row = {"shape": name, "k": c.k, "coefficients": sum(lens), "pairs": sum(c.ts), "buffer_sets": c.nsets,
               "fused_us": med["fused"], "compose_us": cmed, "compose_a_us": med["compose"], "compose_b_us": med["compose_b"],
               "fused_min_us": min(t["fused"]), "compose_min_us": min(both), "compose_spread": spread,
               "compose_over_fused": cmed / med["fused"],
               "fused_wins_by_more_than_spread": bool(med["fused"] < cmed * (1 - spread)),
               "fused_alg_bytes": alg, "fused_fraction_of_hbm_peak": alg / (med["fused"] * 1e-6) / HBM_PEAK}
        rows.append(row)
        print("%-52s fused %9.1f us  compose %9.1f us (x%.2f, spread %.3f)  %.3f of 8 TB/s"
              % (name, med["fused"], cmed, row["compose_over_fused"], spread, row["fused_fraction_of_hbm_peak"]), flush=True)
        del c
        torch.cuda.empty_cache()
    srs.close()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around one variant, variants alternating (the composition twice a round), median of "
                     "the repeats after warm-up; spread = max(gap of the composition's two medians, its p90 - p10) / median",
           "baseline": "plk_poly_divide_short_batch_dev + plk_poly_lincomb_batch_dev + plk_kzg_commit_batch_dev + "
                       "plk_kzg_open_fold_batch_dev (the evaluations left out)",
           "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1)[:-2])
        f.write(',\n "shapes": [\n  %s\n ]\n}\n' % ",\n  ".join(json.dumps(r) for r in rows))


if __name__ == "__main__":
    main()
