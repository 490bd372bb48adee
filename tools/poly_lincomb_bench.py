#!/usr/bin/env python3
"""plk_poly_lincomb_batch_dev against a device-to-device copy and against the same combination written
as PyTorch tensor ops, in one process on the same inputs.

One job of k terms of n coefficients each (shift 0, canonical bytes: the fast path):
  k = 2    two raw terms: the poly_add shape
  k = 9    the round-5 shape (src/plonk.h:582-604): t_lo raw, eight scaled terms, poly_add_hf at the end
  k = 16   sixteen terms, scaled, a third of them subtracted or negated
n in 2^16, 2^20, 2^22, 2^24, each with and without the d_nz word.  Variants, alternating:
  lincomb       plk_poly_lincomb_batch_dev with d_nz
  lincomb_nonz  the same with d_nz = NULL
  copy          one device-to-device copy whose read + write traffic equals the job's algorithmic bytes
                sum len_i + L = (k + 1) n (a copy of (k + 1) n / 2 bytes): the floor
  torch         k = 2: torch.remainder(a + b, 17) on uint8; otherwise the weighted sum over the stacked
                terms in int16, remainder 17, back to uint8 (+ the constant on coefficient 0)
Each time is a pair of device events around one variant, after warm-up; the median of the repeats is
kept.  From 2^20 coefficients up the inputs rotate through distinct buffer sets of at least twice the
256 MB last-level cache in all, and consecutive calls -- the variants included -- take different sets, so a
call never finds its input cached; at 2^16 the whole working set is cache resident and the row says so.  lincomb and torch are compared byte for byte at every shape.

  python tools/poly_lincomb_bench.py [--out profiles/poly_lincomb_bench.json] [--reps 30]
"""
import argparse
import ctypes as C
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
KS, LENGTHS = (2, 9, 16), (1 << 16, 1 << 20, 1 << 22, 1 << 24)


def shape_terms(k):
    """per term (scale or None for raw, sub, neg) and the job's add_hf"""
    if k == 2:
        return [(None, 0, 0), (None, 0, 0)], None
    if k == 9:
        return [(None, 0, 0)] + [(1 + (5 * i) % 16, 0, 0) for i in range(1, 9)], 11
    return [(None, 0, 0)] + [(1 + (3 * i) % 16, 1 if i % 3 == 1 else 0, 1 if i % 3 == 2 else 0) for i in range(1, k)], 3


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
    def __init__(self, n, k):
        self.n, self.k = n, k
        self.terms, self.add_hf = shape_terms(k)
        self.sets = max(2, min(-(-2 * LLC_BYTES // (n * k)), 8 if n < 1 << 20 else 1 << 20))
        g = torch.Generator(device="cuda")
        g.manual_seed(n + k)
        self.stride = (n + 15) & ~15
        self.polys = torch.randint(0, 17, (self.sets, k, self.stride), dtype=torch.uint8, device="cuda", generator=g)
        self.polys[:, :, n - 1] = 1
        self.out = torch.empty(self.stride, dtype=torch.uint8, device="cuda")
        self.nz = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.alg = (k + 1) * n
        half = self.alg // 2
        self.csrc = torch.randint(0, 255, (max(2, -(-2 * LLC_BYTES // half)), half), dtype=torch.uint8, device="cuda",
                                  generator=g) if n >= 1 << 20 else torch.zeros((2, half), dtype=torch.uint8, device="cuda")
        self.cdst = torch.empty(half, dtype=torch.uint8, device="cuda")
        w = [((1 if s is None else s) * (16 if sub ^ neg else 1)) % 17 for s, sub, neg in self.terms]
        self.w16 = torch.tensor(w, dtype=torch.int16, device="cuda").view(-1, 1)
        self.t_out = None
        self.cjobs = {}

    def job(self, i):
        """the plk_lc_job_t of buffer set i, built once (the timed call is the C entry point alone)"""
        i %= self.sets
        if i not in self.cjobs:
            p = self.polys[i]
            arr = (h.LcTerm * self.k)(*[h.LcTerm(p[t].data_ptr(), self.n, 0, sub, h.PLK_LC_RAW if s is None else s, neg, 0)
                                        for t, (s, sub, neg) in enumerate(self.terms)])
            self.cjobs[i] = (h.LcJob(arr, self.k, -1 if self.add_hf is None else self.add_hf, self.out.data_ptr()), arr)
        return C.byref(self.cjobs[i][0])

    def lincomb(self, i):
        assert h.lib().plk_poly_lincomb_batch_dev(self.job(3 * i), 1, self.nz.data_ptr(), None) == 0, h.last_error()

    def lincomb_nonz(self, i):
        assert h.lib().plk_poly_lincomb_batch_dev(self.job(3 * i + 1), 1, None, None) == 0, h.last_error()

    def copy(self, i):
        self.cdst.copy_(self.csrc[i % self.csrc.shape[0]])

    def torch_form(self, i):
        p = self.polys[(3 * i + 2) % self.sets][:, :self.n]
        if self.k == 2:
            self.t_out = torch.remainder(p[0] + p[1], 17)
        else:
            self.t_out = torch.remainder((p.to(torch.int16) * self.w16).sum(0), 17).to(torch.uint8)
            self.t_out[0] = (self.t_out[0] + self.add_hf) % 17

    def measure(self, reps):
        h.lib().plk_poly_lincomb_batch_dev(self.job(2), 1, self.nz.data_ptr(), None)
        self.torch_form(0)          # (buffer set 2, as the call above)
        torch.cuda.synchronize()
        assert torch.equal(self.out[:self.n], self.t_out), "lincomb and the torch form disagree"
        assert int(self.nz.item()) == self.n
        return timed({"lincomb": self.lincomb, "lincomb_nonz": self.lincomb_nonz, "copy": self.copy,
                      "torch": self.torch_form}, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_lincomb_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    h.init(0)
    rows = []
    for n in LENGTHS:
        for k in KS:
            c = Case(n, k)
            med, mn = c.measure(a.reps)
            row = {"len": n, "terms": k, "buffer_sets": c.sets, "cache_resident": n < 1 << 20, "alg_bytes": c.alg,
                   "lincomb_us": med["lincomb"], "lincomb_nonz_us": med["lincomb_nonz"], "copy_us": med["copy"],
                   "torch_us": med["torch"], "lincomb_min_us": mn["lincomb"], "lincomb_nonz_min_us": mn["lincomb_nonz"],
                   "copy_min_us": mn["copy"], "torch_min_us": mn["torch"],
                   "fraction_of_hbm_peak": c.alg / (med["lincomb"] * 1e-6) / HBM_PEAK,
                   "fraction_of_hbm_peak_nonz": c.alg / (med["lincomb_nonz"] * 1e-6) / HBM_PEAK,
                   "copy_fraction_of_hbm_peak": c.alg / (med["copy"] * 1e-6) / HBM_PEAK,
                   "lincomb_over_copy": med["lincomb"] / med["copy"], "torch_over_lincomb": med["torch"] / med["lincomb"]}
            rows.append(row)
            print("len 2^%d k %2d: lincomb %8.1f us (no nz %8.1f)  copy %8.1f us (x%.2f)  torch %9.1f us (x%.2f)  %.3f of 8 TB/s"
                  % (n.bit_length() - 1, k, med["lincomb"], med["lincomb_nonz"], med["copy"], row["lincomb_over_copy"],
                     med["torch"], row["torch_over_lincomb"], row["fraction_of_hbm_peak"]), flush=True)
            del c
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around one call (job structures built beforehand), variants alternating, median of "
                     "the repeats after warm-up",
           "alg_bytes": "sum len_i + L = (terms + 1) len; copy: one device-to-device copy of alg_bytes / 2 bytes",
           "torch": "terms 2: torch.remainder(a + b, 17) on uint8; else the int16 weighted sum over the stacked terms, "
                    "remainder 17, to uint8, the constant added to coefficient 0"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1)[:-2])
        f.write(',\n "rows": [\n  %s\n ]\n}\n' % ",\n  ".join(json.dumps(r) for r in rows))


if __name__ == "__main__":
    main()
