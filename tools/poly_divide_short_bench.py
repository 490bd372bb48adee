#!/usr/bin/env python3
"""plk_poly_divide_short_batch_dev against plk_poly_divide_dev called once per job and against a
device-to-device copy of the same traffic, in one process on the same inputs.

Shapes: numerators of nl in 2^16, 2^20, 2^24 canonical coefficients, divisors of dl in 2, 3, 5, 17
coefficients (dense, non-zero lead), batches of 1 and 9 jobs.  Variants, alternating:
  short    one plk_poly_divide_short_batch_dev call for the whole batch
  divide   plk_poly_divide_dev once per job: the binomial chain scans at dl = 2, the Newton inverse above
           (plk_poly_divide_path is recorded per row)
  copy     one device-to-device copy whose read + write traffic equals the scan's algorithmic bytes, two
           reads and one write of every numerator = 3 nl per job (a copy of 1.5 nl batch bytes): the floor
Each time is a pair of device events around one variant, after warm-up; the median of the repeats is
kept.  From 2^20 coefficients up the numerators rotate through distinct buffer sets of at least twice the
256 MB last-level cache in all, and consecutive calls -- the variants included -- take different sets, so a
call never finds its input cached; at 2^16 the working set is cache resident and the row says so.  short
and divide are compared byte for byte (quotient, remainder, both length words) at every shape.

  python tools/poly_divide_short_bench.py [--out profiles/poly_divide_short_bench.json] [--reps 20]
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
LENGTHS, DLS, BATCHES = (1 << 16, 1 << 20, 1 << 24), (2, 3, 5, 17), (1, 9)


def timed(fns, reps, warm=3):
    for i in range(warm):
        for f in fns.values():
            f(i)
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for i in range(reps):
        for name, f in fns.items():   # alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}


class Case:
    def __init__(self, nl, dl, batch):
        self.nl, self.dl, self.batch = nl, dl, batch
        rng = np.random.default_rng(nl + 31 * dl + batch)
        self.den = rng.integers(1, 17, dl).astype(np.uint8)     # dense: no zero coefficient
        self.sets = max(3, -(-2 * LLC_BYTES // (nl * batch))) if nl >= 1 << 20 else 3
        g = torch.Generator(device="cuda")
        g.manual_seed(nl + dl + batch)
        self.stride = (nl + 15) & ~15
        self.nums = torch.randint(0, 17, (self.sets, batch, self.stride), dtype=torch.uint8, device="cuda", generator=g)
        self.nums[:, :, nl - 1] = 1
        ql, rl = nl - dl + 1, dl - 1
        self.q = torch.empty((2, batch, self.stride), dtype=torch.uint8, device="cuda")   # [0] short, [1] divide
        self.r = torch.empty((2, batch, 16), dtype=torch.uint8, device="cuda")
        self.lens = torch.zeros((2, batch, 3), dtype=torch.int32, device="cuda")
        self.work = torch.empty(h.poly_divide_short_workspace([(nl, dl)] * batch), dtype=torch.uint8, device="cuda")
        self.dwork = torch.empty(max(h.poly_divide_workspace(nl, dl), 16), dtype=torch.uint8, device="cuda")
        self.alg = 3 * nl * batch
        half = self.alg // 2
        nsrc = max(2, -(-2 * LLC_BYTES // half)) if nl >= 1 << 20 else 2
        self.csrc = torch.randint(0, 255, (nsrc, half), dtype=torch.uint8, device="cuda", generator=g)
        self.cdst = torch.empty(half, dtype=torch.uint8, device="cuda")
        self.ql, self.rl = ql, rl
        self.path = h.poly_divide_path(self.den, nl)

    def short(self, i, s=None):
        s = (3 * i) % self.sets if s is None else s
        h.poly_divide_short_batch_dev([(self.nums[s, b], self.nl, self.den, self.q[0, b], self.r[0, b])
                                       for b in range(self.batch)], self.lens[0], self.work)

    def divide(self, i, s=None):
        s = (3 * i + 1) % self.sets if s is None else s
        for b in range(self.batch):
            h.poly_divide_dev(self.nums[s, b], self.nl, self.den, self.q[1, b], self.r[1, b], self.lens[1, b], self.dwork)

    def copy(self, i):
        self.cdst.copy_(self.csrc[i % self.csrc.shape[0]])

    def measure(self, reps):
        self.short(0, 2)
        self.divide(0, 2)
        torch.cuda.synchronize()
        assert torch.equal(self.q[0, :, :self.ql], self.q[1, :, :self.ql]), "quotients disagree"
        assert torch.equal(self.r[0, :, :self.rl], self.r[1, :, :self.rl]), "remainders disagree"
        assert torch.equal(self.lens[0, :, :2], self.lens[1, :, :2]) and not self.lens[0, :, 2].any(), "length words"
        return timed({"short": self.short, "divide": self.divide, "copy": self.copy}, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_divide_short_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    h.init(0)
    rows = []
    for nl in LENGTHS:
        for dl in DLS:
            for batch in BATCHES:
                c = Case(nl, dl, batch)
                med, mn = c.measure(a.reps if nl < 1 << 24 else max(5, a.reps // 2))
                row = {"nl": nl, "dl": dl, "batch": batch, "buffer_sets": c.sets, "cache_resident": nl < 1 << 20,
                       "divide_path": c.path, "plan": h.poly_divide_short_plan(nl, dl), "alg_bytes": c.alg,
                       "short_us": med["short"], "divide_us": med["divide"], "copy_us": med["copy"],
                       "short_min_us": mn["short"], "divide_min_us": mn["divide"], "copy_min_us": mn["copy"],
                       "divide_over_short": med["divide"] / med["short"], "short_over_copy": med["short"] / med["copy"],
                       "fraction_of_hbm_peak": c.alg / (med["short"] * 1e-6) / HBM_PEAK}
                rows.append(row)
                print("nl 2^%d dl %2d batch %d: short %9.1f us  divide (path %d) %10.1f us (x%.2f)  copy %8.1f us (short x%.2f)"
                      % (nl.bit_length() - 1, dl, batch, med["short"], c.path, med["divide"], row["divide_over_short"],
                         med["copy"], row["short_over_copy"]), flush=True)
                del c
                torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around one variant (the Python binding's job marshalling included for short and "
                     "divide alike), variants alternating, median of the repeats after warm-up",
           "alg_bytes": "3 nl batch (two reads and one write of every numerator); copy: one device-to-device copy of "
                        "alg_bytes / 2 bytes",
           "divide": "plk_poly_divide_dev once per job; divide_path as plk_poly_divide_path reports it (2 binomial "
                     "chain scans, 4 Newton inverse)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1)[:-2])
        f.write(',\n "rows": [\n  %s\n ]\n}\n' % ",\n  ".join(json.dumps(r) for r in rows))


if __name__ == "__main__":
    main()
