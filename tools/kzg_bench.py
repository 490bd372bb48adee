#!/usr/bin/env python3
"""The fused KZG opening against its composition from the older public calls (DESIGN, "KZG over a
resident SRS"), in one process on the same inputs.

  fused:    plk_kzg_open_batch_dev over an Srs handle (log form): 1-2 launches per batch
  composed: plk_poly_eval_batch_dev, one plk_poly_divide_dev by x - z per job, and one
            plk_msm_g1_batch_dev over the quotients with the SRS in G1 form -- code this tool's
            subject leaves untouched

for lengths 2^12, 2^16, 2^20, 2^22 and batches 1 and 9.  Each time is a pair of device events around
one call on the stream, after warm-up; the two variants alternate, the median of the repeats is
kept.  The polynomials rotate through enough distinct buffer sets that a call never finds its
input in the 256 MB last-level cache (the SRS is resident by design and stays warm).  Outputs of the
two variants are compared at every size.  The fraction of the 8 TB/s HBM peak counts the fused
path's algorithmic bytes: 3 per coefficient (p twice, the logs once) -- 2 where one chunk holds the
polynomial.

  python tools/kzg_bench.py [--out profiles/kzg_open_bench.json] [--reps 40] [--only 22 9]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk.c_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import plonkhip as h  # noqa: E402

HBM_PEAK = 8e12
LLC_BYTES = 256 << 20
REC = h.MSM_RESULT_BYTES
LENGTHS = (1 << 12, 1 << 16, 1 << 20, 1 << 22)
BATCHES = (1, 9)


def srs_points(n):
    """n points uniform over all 102 group elements (seeded)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen
    pts, _ = gen.msm_inputs(0x5125, n, "full")
    return pts


class Case:
    def __init__(self, srs, d_g1, n, batch):
        self.srs, self.d_g1, self.n, self.batch = srs, d_g1, n, batch
        # large sizes: twice the last-level cache in distinct inputs; small ones are launch-bound
        self.sets = -(-2 * LLC_BYTES // (n * batch)) if n >= 1 << 20 else 4
        g = torch.Generator(device="cuda")
        g.manual_seed(n + batch)
        self.stride = (n + 15) & ~15
        self.polys = [torch.randint(0, 17, (batch, self.stride), dtype=torch.uint8, device="cuda", generator=g)
                      for _ in range(self.sets)]
        for p in self.polys:
            p[:, n - 1] = 1 + p[:, n - 1] % 16
        self.lens = [n] * batch
        self.zs = [(3 + 5 * b) % 16 + 1 for b in range(batch)]
        self.ys = [torch.zeros(batch, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.res = [torch.zeros(batch * REC, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.work = torch.empty(h.kzg_workspace(self.lens), dtype=torch.uint8, device="cuda")
        # the composition's buffers
        self.tick = torch.zeros(h.poly_eval_workspace(batch), dtype=torch.uint8, device="cuda")
        self.quot = torch.zeros((batch, self.stride), dtype=torch.uint8, device="cuda")
        self.rem = torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.dlens = torch.zeros(2 * batch, dtype=torch.int32, device="cuda")
        self.dwork = torch.zeros(max(h.poly_divide_workspace(n, 2), 16), dtype=torch.uint8, device="cuda")
        self.dens = [np.array([(17 - z) % 17, 1], np.uint8) for z in self.zs]

    def fused(self, k):
        p = self.polys[k % self.sets]
        h.kzg_open_dev(self.srs, [p[b] for b in range(self.batch)], self.lens, self.zs, self.ys[0], self.res[0],
                       work=self.work)

    def composed(self, k):
        p = self.polys[k % self.sets]
        rows = [p[b] for b in range(self.batch)]
        h.poly_eval_batch_dev(rows, self.lens, self.zs, self.ys[1], self.tick)
        for b in range(self.batch):
            h.poly_divide_dev(rows[b], self.n, self.dens[b], self.quot[b], self.rem, self.dlens[2 * b:], self.dwork)
        h.msm_g1_batch_dev(self.d_g1, 0, self.quot, self.stride, self.n - 1, self.batch, self.res[1])

    def outputs(self, which):
        r = self.res[which].cpu().numpy()
        recs = [h.parse_result(r[i * REC:(i + 1) * REC]) for i in range(self.batch)]
        return self.ys[which].cpu().tolist(), [(x["g1"], x["irregular"]) for x in recs]

    def measure(self, reps, warm=5):
        fns = {"fused": self.fused, "composed": self.composed}
        for k in range(warm):
            for f in fns.values():
                f(k)
        torch.cuda.synchronize()
        # same buffer set for both variants: the outputs must agree
        self.fused(0)
        self.composed(0)
        assert self.outputs(0) == self.outputs(1), "fused and composed disagree at n %d batch %d" % (self.n, self.batch)
        times = {"fused": [], "composed": []}
        for k in range(reps):
            for name, f in fns.items():   # alternate
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f(k)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        return {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_open_bench.json"))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--only", type=int, nargs=2, default=None, metavar=("LOG2_LEN", "BATCH"),
                    help="run just this case and write no record (for a kernel trace)")
    a = ap.parse_args()
    h.init(0)
    nmax = max(LENGTHS)
    pts = srs_points(nmax)
    srs = h.Srs(pts)
    assert not srs.irregular
    d_g1 = torch.from_numpy(pts.reshape(-1)).cuda()
    if a.only:
        c = Case(srs, d_g1, 1 << a.only[0], a.only[1])
        print(c.measure(a.reps))
        return
    rows = []
    for n in LENGTHS:
        for batch in BATCHES:
            c = Case(srs, d_g1, n, batch)
            med, mn = c.measure(a.reps if n >= 1 << 20 else 3 * a.reps)
            fused_bytes = (3 if n > 4096 else 2) * n * batch
            row = {"len": n, "batch": batch, "buffer_sets": c.sets, "fused_us": med["fused"],
                   "composed_us": med["composed"], "fused_min_us": mn["fused"], "composed_min_us": mn["composed"],
                   "speedup": med["composed"] / med["fused"], "fused_alg_bytes": fused_bytes,
                   "fused_fraction_of_hbm_peak": fused_bytes / (med["fused"] * 1e-6) / HBM_PEAK}
            rows.append(row)
            print("len 2^%d batch %d: fused %9.1f us  composed %9.1f us  x%.2f  (%.3f of 8 TB/s)" %
                  (n.bit_length() - 1, batch, med["fused"], med["composed"], row["speedup"],
                   row["fused_fraction_of_hbm_peak"]), flush=True)
            del c
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around one call, variants alternating, median of the repeats", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    srs.close()


if __name__ == "__main__":
    main()
