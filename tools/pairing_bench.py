#!/usr/bin/env python3
"""Throughput of plk_pairing_batch_dev and plk_kzg_verify_batch_dev.

Batches of 2^10, 2^16, 2^20 and 2^24 random valid jobs.  Each time is a pair of device events around
one call on the stream, after warm-up; the median of the repeats is kept.  At 2^20 and above the
inputs rotate through enough distinct buffer sets (twice the 256 MB last-level cache) that a launch
never finds its input cached.  Per size the record holds jobs/s, the achieved bytes/s at 5 B per
pairing job (its input bytes) and 9 B per verify job (8 in, 1 out) as a fraction of the 8 TB/s HBM peak, and the ratio to the reference's single-core time recorded in
tests/golden/pairing.json -- a CROSS-MACHINE ratio: that time was taken on the CPU of the machine
that generated the goldens, not on this host.

  python tools/pairing_bench.py [--out profiles/kzg_verify_bench.json] [--reps 25]
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
SIZES = (1 << 10, 1 << 16, 1 << 20, 1 << 24)
BYTES = {"pairing": 5, "verify": 9}


def random_g1(n, g):
    """n valid encodings: coordinates < 101, a quarter flagged"""
    t = torch.randint(0, 101, (n, 3), dtype=torch.uint8, device="cuda", generator=g)
    t[:, 2] = (torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g) == 0).to(torch.uint8)
    return t.reshape(-1)


class Case:
    def __init__(self, n):
        self.n = n
        g = torch.Generator(device="cuda")
        g.manual_seed(n)
        self.sets = {k: (-(-2 * LLC_BYTES // (b * n)) if n >= 1 << 20 else 4) for k, b in BYTES.items()}
        self.p_in = [(random_g1(n, g), torch.randint(0, 101, (2 * n,), dtype=torch.uint8, device="cuda", generator=g))
                     for _ in range(self.sets["pairing"])]
        self.v_in = [(random_g1(n, g), torch.randint(0, 17, (n,), dtype=torch.uint8, device="cuda", generator=g),
                      torch.randint(0, 17, (n,), dtype=torch.uint8, device="cuda", generator=g), random_g1(n, g))
                     for _ in range(self.sets["verify"])]
        self.gt = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
        self.ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.vk = h.KzgVk((1, 2, 0), (36, 31), (90, 82))

    def pairing(self, k):
        a, b = self.p_in[k % len(self.p_in)]
        h.pairing_dev(a, b, self.n, self.gt)

    def verify(self, k):
        c, z, y, w = self.v_in[k % len(self.v_in)]
        h.kzg_verify_dev(self.vk, c, z, y, w, self.n, self.ok)

    def measure(self, reps, warm=5):
        out = {}
        for name, f in (("pairing", self.pairing), ("verify", self.verify)):
            for k in range(warm):
                f(k)
            torch.cuda.synchronize()
            us = []
            for k in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f(k)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            out[name] = (statistics.median(us), min(us))
        assert int(self.gt.max()) < 101 and int(self.ok.max()) < 2     # valid inputs: no FF, no 2
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_verify_bench.json"))
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 launches per size")
    h.init(0)
    with open(os.path.join(ROOT, "tests", "golden", "pairing.json")) as f:
        ref = json.load(f)["reference_ns"]
    rows = []
    for n in SIZES:
        c = Case(n)
        m = c.measure(a.reps)
        row = {"n": n, "buffer_sets": c.sets}
        for name, (med, mn) in m.items():
            per_s = n / (med * 1e-6)
            row[name] = {"median_us": med, "min_us": mn, "jobs_per_s": per_s, "ns_per_job": 1e9 / per_s,
                         "bytes_per_s": BYTES[name] * per_s, "fraction_of_hbm_peak": BYTES[name] * per_s / HBM_PEAK,
                         "x_reference_one_core_cross_machine": ref[name] / (1e9 / per_s)}
            print("n 2^%d %-8s %10.1f us  %.3e jobs/s  %.4f of 8 TB/s  x%.0f the reference's core (cross-machine)" %
                  (n.bit_length() - 1, name, med, per_s, row[name]["fraction_of_hbm_peak"],
                   row[name]["x_reference_one_core_cross_machine"]), flush=True)
        rows.append(row)
        del c
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "bytes_per_job": BYTES,
           "timing": "device events around one call, median of %d launches after 5 warm-up launches" % a.reps,
           "reference_ns": ref, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
