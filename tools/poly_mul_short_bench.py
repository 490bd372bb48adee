#!/usr/bin/env python3
"""plk_poly_mul_short_batch_dev against the same products through plk_poly_mul_batch_dev in chunks of 64 and
against a device-to-device copy of the same traffic, in one process on the same device
buffers.

Shapes: 2^16 products of 48 x 48 as one run; 2^12 products of 1024 x 1024 as one run; single products of
2^24 x 17, 2^24 x 64 and 2^24 x 1024 coefficients; a ragged list of 200 runs of one product each (multipliers
of 1 .. 1024 coefficients against 1 .. 20000).  Variants, alternating:
  short   one plk_poly_mul_short_batch_dev call for the whole shape
  batch   plk_poly_mul_batch_dev over the same products, 64 jobs a call (the call's limit), its workspace
          plk_poly_mul_batch_workspace of the largest chunk
  copy    one device-to-device copy whose read + write traffic equals the products' algorithmic bytes (every
          operand read once, every product written once): a copy of half of them
The descriptor arrays of short and batch are built once, outside the timed region.  Each time is a pair of
device events around one variant, after warm-up; the median of the repeats is kept.  The operands rotate
through distinct buffer sets -- at least twice the 256 MB last-level cache in all for the 2^24 shapes, three
sets otherwise (those rows are cache resident and say so) -- and consecutive calls take different sets.
short and batch are compared byte for byte at every shape before the timing.

  python tools/poly_mul_short_bench.py [--out profiles/poly_mul_short_bench.json] [--reps 20]
"""
import argparse
import ctypes as C
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
CHUNK = 64


def timed(fns, reps, warm=2):
    for i in range(warm):
        for f in fns.values():
            f(i)
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for i in range(reps[max(reps, key=reps.get)]):
        for name, f in fns.items():   # alternate
            if i >= reps[name]:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}


class Case:
    """runs: (la, lb, count) in call order, operands tight in one buffer per set"""

    def __init__(self, name, runs, big):
        self.name, self.runs = name, runs
        in_bytes = sum((la + lb) * c for la, lb, c in runs)
        out_bytes = sum((la + lb - 1) * c for la, lb, c in runs)
        self.products = sum(c for _, _, c in runs)
        self.alg = in_bytes + out_bytes
        self.sets = max(3, -(-2 * LLC_BYTES // in_bytes)) if big else 3
        g = torch.Generator(device="cuda")
        g.manual_seed(len(runs) + in_bytes)
        pad = (in_bytes + 15) & ~15
        self.inp = torch.randint(0, 17, (self.sets, pad), dtype=torch.uint8, device="cuda", generator=g)
        self.out = torch.empty((2, (out_bytes + 15) & ~15), dtype=torch.uint8, device="cuda")   # [0] short, [1] batch
        self.nz = torch.zeros(self.products, dtype=torch.int32, device="cuda")
        self.short_runs, self.jobs = [], []
        for s in range(self.sets):
            base, o0, o1 = self.inp[s].data_ptr(), self.out[0].data_ptr(), self.out[1].data_ptr()
            arr = (h.MulShortRun * len(runs))()
            jobs = (h.PolyMulJob * self.products)()
            k = 0
            for r, (la, lb, c) in enumerate(runs):
                lo = la + lb - 1
                arr[r] = h.MulShortRun(base, la, la, base + la * c, lb, lb, o0, lo, c)
                for i in range(c):
                    jobs[k] = h.PolyMulJob(base + i * la, la, base + la * c + i * lb, lb, o1 + i * lo, 0)
                    k += 1
                base += (la + lb) * c
                o0 += lo * c
                o1 += lo * c
            self.short_runs.append(arr)
            self.jobs.append(jobs)
        L = h.lib()
        self.chunks = [(i, min(CHUNK, self.products - i)) for i in range(0, self.products, CHUNK)]
        step = C.sizeof(h.PolyMulJob)
        # (a shape of one run: every chunk but the last is the same)
        sized = self.chunks if len(runs) > 1 else [self.chunks[0], self.chunks[-1]]
        self.ws = int(max(L.plk_poly_mul_batch_workspace(C.addressof(self.jobs[0]) + i * step, n) for i, n in sized))
        self.work = torch.empty(max(self.ws, 16), dtype=torch.uint8, device="cuda")
        half = self.alg // 2
        nsrc = max(2, -(-2 * LLC_BYTES // half)) if big else 2
        self.csrc = torch.randint(0, 255, (nsrc, half), dtype=torch.uint8, device="cuda", generator=g)
        self.cdst = torch.empty(half, dtype=torch.uint8, device="cuda")
        self.step = step

    def short(self, i, s=None):
        s = (3 * i) % self.sets if s is None else s
        rc = h.lib().plk_poly_mul_short_batch_dev(self.short_runs[s], len(self.runs), self.nz.data_ptr(), None)
        assert rc == 0, h.last_error()

    def batch(self, i, s=None):
        s = (3 * i + 1) % self.sets if s is None else s
        L, base = h.lib(), C.addressof(self.jobs[s])
        for k, n in self.chunks:
            rc = L.plk_poly_mul_batch_dev(base + k * self.step, n, self.work.data_ptr(), self.ws, None)
            assert rc == 0, h.last_error()

    def copy(self, i):
        self.cdst.copy_(self.csrc[i % self.csrc.shape[0]])

    def measure(self, reps):
        self.short(0, 2)
        self.batch(0, 2)
        torch.cuda.synchronize()
        n = sum((la + lb - 1) * c for la, lb, c in self.runs)
        assert torch.equal(self.out[0][:n], self.out[1][:n]), "the products disagree"
        return timed({"short": self.short, "batch": self.batch, "copy": self.copy}, reps)


def ragged_runs():
    rng = np.random.default_rng(200)
    return [(int(rng.integers(1, 1025)), int(rng.integers(1, 20001)), 1) if k % 2 else
            (int(rng.integers(1, 20001)), int(rng.integers(1, 1025)), 1) for k in range(200)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_mul_short_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    h.init(0)
    cases = [("2^16 x (48 x 48)", [(48, 48, 1 << 16)], False, 3),
             ("2^12 x (1024 x 1024)", [(1024, 1024, 1 << 12)], False, 5),
             ("2^24 x 17", [(1 << 24, 17, 1)], True, a.reps),
             ("2^24 x 64", [(1 << 24, 64, 1)], True, a.reps),
             ("2^24 x 1024", [(1 << 24, 1024, 1)], True, a.reps),
             ("ragged 200", ragged_runs(), False, a.reps)]
    rows = []
    for name, runs, big, breps in cases:
        c = Case(name, runs, big)
        med, mn = c.measure({"short": a.reps, "batch": breps, "copy": a.reps})
        la, lb, cnt = runs[0]
        row = {"shape": name, "runs": len(runs), "products": c.products, "buffer_sets": c.sets, "cache_resident": not big,
               "plan": h.poly_mul_short_plan(la, lb, cnt) if len(runs) == 1 else None, "alg_bytes": c.alg,
               "batch_calls": len(c.chunks), "batch_workspace": c.ws,
               "short_us": med["short"], "batch_us": med["batch"], "copy_us": med["copy"],
               "short_min_us": mn["short"], "batch_min_us": mn["batch"], "copy_min_us": mn["copy"],
               "batch_over_short": med["batch"] / med["short"], "short_over_copy": med["short"] / med["copy"],
               "fraction_of_hbm_peak": c.alg / (med["short"] * 1e-6) / HBM_PEAK,
               "mac_per_s": sum(la * lb * n for la, lb, n in runs) / (med["short"] * 1e-6)}
        rows.append(row)
        print("%-22s short %10.1f us  batch (%d calls) %12.1f us (x%.2f)  copy %8.1f us (short x%.2f)"
              % (name, med["short"], len(c.chunks), med["batch"], row["batch_over_short"], med["copy"],
                 row["short_over_copy"]), flush=True)
        del c
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around one variant, descriptor arrays prebuilt, variants alternating, median of the "
                     "repeats after warm-up",
           "alg_bytes": "every operand read once and every product written once; copy: one device-to-device copy of "
                        "alg_bytes / 2 bytes",
           "batch": "plk_poly_mul_batch_dev over the same products, 64 jobs a call"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1)[:-2])
        f.write(',\n "rows": [\n  %s\n ]\n}\n' % ",\n  ".join(json.dumps(r) for r in rows))


if __name__ == "__main__":
    main()
