#!/usr/bin/env python3
"""Measurements behind PLK_OPT_DIVIDE_FAST_MIN, through plk_poly_divide_dev in one process.

  crossover: general canonical divisors with dl ~ nl / 2 on a ladder of sizes, the reference's loop
             on one thread (DIVIDE_FAST_MIN = 0) against the Newton path (= 1), alternating; the
             ladder ends once the loop takes more than half a second.  The default of the option
             is the smallest measured (nl - dl + 1) * dl from which Newton wins at every larger
             rung, rounded up to a power of two.
  scale:     the Newton path alone at nl = 2^20, dl = 2^19 + 1 and nl = 2^21, dl = 2^20 + 1 against
             the sum of the standalone plk_poly_mul_dev times of its product shapes.

Every time is a host clock around one call that ends in a device synchronise (so the divisor's
classification and copy are in it), after warm-up, median of the repeats.

  python tools/divide_fast_bench.py --out profiles [--skip-scale] [--skip-crossover]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk.c_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import plonkhip as h  # noqa: E402

B0 = 1024   # polyops.hip INV_B0


def inputs(seed, nl, dl):
    rng = np.random.default_rng(seed)
    num = rng.integers(0, 17, nl).astype(np.uint8)
    den = rng.integers(0, 17, dl).astype(np.uint8)
    den[1] = 3
    den[-1] = 5
    return num, den


class Division:
    def __init__(self, nl, dl):
        self.nl, self.dl = nl, dl
        num, self.den = inputs(nl + dl, nl, dl)
        self.num = torch.from_numpy(num).cuda()
        self.q = torch.zeros(nl - dl + 1, dtype=torch.uint8, device="cuda")
        self.r = torch.zeros(dl - 1, dtype=torch.uint8, device="cuda")
        self.lens = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.work = torch.zeros(h.poly_divide_workspace(nl, dl), dtype=torch.uint8, device="cuda")

    def run(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.poly_divide_dev(self.num, self.nl, self.den, self.q, self.r, self.lens, self.work)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def result(self):
        return self.q.cpu().numpy().tobytes(), self.r.cpu().numpy().tobytes(), self.lens.cpu().tolist()


def crossover(max_serial_s=0.5):
    rows = []
    ladder = [6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 12288, 16384,
              24576, 32768]
    for nl in ladder:
        dl = nl // 2 + 1
        d = Division(nl, dl)
        times = {0: [], 1: []}
        outs = {}
        with h.options(DIVIDE_FAST_MIN=0):
            assert h.poly_divide_path(d.den, nl) == 3
            first = d.run()
        reps = max(2, min(20, int(0.3 / max(first, 1e-6))))
        for rnd in range(3):   # alternate the two paths
            for mode in (0, 1):
                with h.options(DIVIDE_FAST_MIN=mode):
                    assert h.poly_divide_path(d.den, nl) == (4 if mode else 3)
                    d.run()   # warm-up of this shape and path
                    times[mode] += [d.run() for _ in range(reps if mode == 0 else 20)]
                    outs[mode] = d.result()
        assert outs[0] == outs[1], "paths disagree at nl %d" % nl
        ser, newt = statistics.median(times[0]), statistics.median(times[1])
        rows.append({"nl": nl, "dl": dl, "steps": (nl - dl + 1) * dl, "serial_us": ser * 1e6, "newton_us": newt * 1e6,
                     "serial_min_us": min(times[0]) * 1e6, "newton_min_us": min(times[1]) * 1e6,
                     "serial_reps": len(times[0]), "newton_reps": len(times[1])})
        print("crossover nl %6d dl %6d steps %11d serial %12.1f us newton %10.1f us" %
              (nl, dl, rows[-1]["steps"], ser * 1e6, newt * 1e6), flush=True)
        if ser > max_serial_s:
            break
    win = None
    for r in reversed(rows):
        if r["newton_us"] < r["serial_us"]:
            win = r["steps"]
        else:
            break
    default = None if win is None else 1 << (win - 1).bit_length()
    return {"rows": rows, "first_winning_steps": win, "default": default}


def product_shapes(nl, dl):
    """the products of one Newton division (polyops.hip newton_divide), in launch order"""
    m = dl - 1
    k = nl - m
    fl = min(dl, k)
    t = k
    while t > B0:
        t = (t + 1) // 2
    shapes = []
    while t < k:
        n2 = min(2 * t, k)
        shapes += [(min(fl, n2), t), (t, n2 - t)]
        t = n2
    return shapes + [(k, k), (min(k, m), m)]


def time_product(la, lb, reps=10):
    rng = np.random.default_rng(la ^ lb)
    a = torch.from_numpy(rng.integers(0, 17, la).astype(np.uint8)).cuda()
    b = torch.from_numpy(rng.integers(0, 17, lb).astype(np.uint8)).cuda()
    out = torch.zeros(la + lb - 1, dtype=torch.uint8, device="cuda")
    work = torch.zeros(max(h.poly_mul_workspace(la, lb), 16), dtype=torch.uint8, device="cuda")
    ts = []
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.poly_mul_dev(a, la, b, lb, out, None, work)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[2:])


def scale():
    rows = []
    for nl, dl in (((1 << 20), (1 << 19) + 1), ((1 << 21), (1 << 20) + 1)):
        d = Division(nl, dl)
        assert h.poly_divide_path(d.den, nl) == 4
        for _ in range(3):
            d.run()
        ts = [d.run() for _ in range(15)]
        shapes = product_shapes(nl, dl)
        prods = [{"la": la, "lb": lb, "us": time_product(la, lb) * 1e6} for la, lb in shapes]
        ts += [d.run() for _ in range(15)]   # (again after the products: the spread over the run)
        div_us, psum = statistics.median(ts) * 1e6, sum(p["us"] for p in prods)
        rows.append({"nl": nl, "dl": dl, "divide_us": div_us, "divide_min_us": min(ts) * 1e6, "products": prods,
                     "products_sum_us": psum, "glue_share_of_sum": div_us / psum - 1.0})
        print("scale nl %d dl %d: divide %.1f us (min %.1f), %d products sum %.1f us, glue + gaps %+.1f %%" %
              (nl, dl, div_us, min(ts) * 1e6, len(prods), psum, 100 * (div_us / psum - 1)), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--skip-crossover", action="store_true")
    ap.add_argument("--skip-scale", action="store_true")
    ap.add_argument("--only-divide", type=int, default=0, metavar="LOG2_NL",
                    help="run just the Newton division at nl = 2^LOG2_NL, dl = nl / 2 + 1 (for a kernel trace)")
    a = ap.parse_args()
    h.init(0)
    if a.only_divide:
        d = Division(1 << a.only_divide, (1 << (a.only_divide - 1)) + 1)
        assert h.poly_divide_path(d.den, d.nl) == 4
        print("divide us:", ["%.1f" % (d.run() * 1e6) for _ in range(13)])
        return
    os.makedirs(a.out, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "option_default_at_run": h.get_option("DIVIDE_FAST_MIN")}
    if not a.skip_crossover:
        res["crossover"] = crossover()
    if not a.skip_scale:
        res["scale"] = scale()
    with open(os.path.join(a.out, "divide_fast_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "scale"})[:400])


if __name__ == "__main__":
    main()
