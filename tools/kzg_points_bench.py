#!/usr/bin/env python3
"""The per-point KZG openings against the same jobs listed one by one, in one process on
the same inputs.

Per shape: polynomials p_i, each opened at every point of its set with a proof per point.
  points    plk_kzg_open_points_batch_dev: a polynomial's bytes and the SRS logs loaded once for all its
            points (an aggregates launch in front past 4096 coefficients, a finish launch behind)
  expanded  plk_kzg_open_batch_dev on the expanded job list (the polynomial repeated once per point), an
            unchanged function: every job reads its polynomial twice and the logs once
Both run this commit's public _dev calls, through argument blocks built before the clock starts.  Each time is
a pair of device events around one call on the stream, after warm-up; the variants alternate -- the baseline
twice per round, as expanded and expanded_b -- and the median of the repeats is kept.  The spread of the baseline
is the larger of the gap between its two interleaved medians and its own 10th-to-90th percentile width, over its
median; the new call counts as a win only when it is faster by more than that.  The inputs rotate through enough
distinct buffer sets (twice the 256 MB last-level cache where memory allows) that a call never finds its
polynomials cached (the SRS is resident by design and stays warm).  ys and proof bytes of the two are compared
byte for byte at every shape.  `copy` is a device copy of the new call's algorithmic traffic -- the
polynomials' bytes (rotating) and as many log bytes (warm) -- timed the same way; a copy also writes what it
reads, so it is a generous stand-in for a pure read.

  python tools/kzg_points_bench.py [--out profiles/kzg_points_bench.json] [--reps 30]
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
MAX_SETS = 256
REC = h.MSM_RESULT_BYTES
FULL = (1 << 17) - 1


def shapes():
    """(name, lengths, sets as masks)"""
    n = 1 << 22
    return [
        ("1 of 2^22 at 1 point", [n], [1 << 3]),
        ("1 of 2^22 at 2 points", [n], [1 << 3 | 1 << 12]),
        ("1 of 2^22 at 4 points", [n], [1 | 1 << 3 | 1 << 12 | 1 << 16]),
        ("1 of 2^22 at 17 points", [n], [FULL]),
        ("9 of 2^22 at 17 points", [n] * 9, [FULL] * 9),
        ("1024 of 4096 at 17 points", [4096] * 1024, [FULL] * 1024),
        ("1 of 2^20 at 17 points", [1 << 20], [FULL]),
        ("ragged, 9 polynomials up to 2^22, mixed sets",
         [n, (1 << 21) + 5, 1 << 20, 3 * (1 << 20) + 17, 4097, n - 3, 17, 1 << 19, 12345],
         [1 << 3, 1 << 3 | 1 << 12, 0b1110, 1, FULL, 1 << 3 | 1, 0xFFFF, 1 << 16, FULL]),
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


def check(fn, rc):
    if rc != h.PLK_OK:
        raise RuntimeError("%s failed (%d): %s" % (fn, rc, h.last_error()))


class Case:
    def __init__(self, srs, lens, sets):
        self.srs, self.lens, self.masks, self.n = srs, lens, sets, len(lens)
        n = self.n
        offs, total = [], 0
        for k in lens:
            offs.append(total)
            total += (k + 15) & ~15
        self.total = total
        self.nsets = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // total)))
        g = torch.Generator(device="cuda")
        g.manual_seed(total + n)
        self.bufs = [torch.randint(0, 17, (total,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(self.nsets)]
        last = torch.tensor([o + k - 1 for o, k in zip(offs, lens)], device="cuda")
        for b in self.bufs:
            b[last] = 1 + b[last] % 16   # (a non-zero leading coefficient)
        self.jobs = [(i, a) for i, m in enumerate(sets) for a in points(m)]
        J = self.J = len(self.jobs)
        assert J == h.kzg_points_count(sets)
        sz, vp = C.c_size_t, C.c_void_p
        # points: argument blocks per buffer set
        self.p_ptrs = [(vp * n)(*[b.data_ptr() + o for o in offs]) for b in self.bufs]
        self.p_lens = (sz * n)(*lens)
        self.p_sets = (C.c_uint32 * n)(*sets)
        self.p_zs, self.p_ys, self.p_st = (torch.zeros(J, dtype=torch.uint8, device="cuda") for _ in range(3))
        self.p_pf = torch.zeros(3 * J, dtype=torch.uint8, device="cuda")
        ws = h.kzg_points_workspace(lens, sets)
        self.p_work = torch.empty(max(ws, 16), dtype=torch.uint8, device="cuda")
        self.p_ws = ws
        # expanded: the same polynomials listed once per point
        elens = [lens[i] for i, _ in self.jobs]
        self.e_ptrs = [(vp * J)(*[b.data_ptr() + offs[i] for i, _ in self.jobs]) for b in self.bufs]
        self.e_lens = (sz * J)(*elens)
        self.e_zs = (C.c_uint8 * J)(*[a for _, a in self.jobs])
        self.e_ys = torch.zeros(J, dtype=torch.uint8, device="cuda")
        self.e_res = torch.zeros(J * REC, dtype=torch.uint8, device="cuda")
        self.e_work = torch.empty(max(h.kzg_workspace(elens), 16), dtype=torch.uint8, device="cuda")
        # copy: the polynomials' bytes and as many log bytes
        self.c_logs = torch.randint(0, 102, (total,), dtype=torch.uint8, device="cuda", generator=g)
        self.c_dst = torch.empty(2 * total, dtype=torch.uint8, device="cuda")
        self.lib = h.lib()
        self.sh = srs._h

    def points(self, i):
        check("plk_kzg_open_points_batch_dev", self.lib.plk_kzg_open_points_batch_dev(
            self.sh, self.p_ptrs[i % self.nsets], self.p_lens, self.p_sets, self.n, self.p_zs.data_ptr(), self.p_ys.data_ptr(),
            self.p_pf.data_ptr(), self.p_st.data_ptr(), self.p_work.data_ptr() if self.p_ws else None, None))

    def expanded(self, i):
        check("plk_kzg_open_batch_dev", self.lib.plk_kzg_open_batch_dev(
            self.sh, self.e_ptrs[i % self.nsets], self.e_lens, self.e_zs, self.J, self.e_ys.data_ptr(), self.e_res.data_ptr(),
            None, self.e_work.data_ptr(), None))

    def copy(self, i):
        self.c_dst[:self.total].copy_(self.bufs[i % self.nsets])
        self.c_dst[self.total:].copy_(self.c_logs)

    def measure(self, reps):
        self.points(0)
        self.expanded(0)
        torch.cuda.synchronize()
        rec = self.e_res.view(self.J, REC)
        assert int(self.p_st.max()) == 0 and int(rec[:, 12:16].max()) == 0, "a flagged job"
        assert torch.equal(self.p_ys, self.e_ys) and torch.equal(self.p_pf.view(self.J, 3), rec[:, 16:19]), \
            "points and expanded disagree"
        assert self.p_zs.cpu().tolist() == [a for _, a in self.jobs]
        return timed({"points": self.points, "expanded": self.expanded, "copy": self.copy, "expanded_b": self.expanded}, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_points_bench.json"))
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
        both = t["expanded"] + t["expanded_b"]
        emed = statistics.median(both)
        spread = max(abs(med["expanded"] - med["expanded_b"]), pct(both, 0.9) - pct(both, 0.1)) / emed
        alg = 2 * sum(lens) + sum(n for n in lens if n > 4096)   # polynomial and logs once, the aggregates' second read
        row = {"shape": name, "polynomials": c.n, "coefficients": sum(lens), "jobs": c.J, "buffer_sets": c.nsets,
               "points_us": med["points"], "expanded_us": emed, "expanded_a_us": med["expanded"],
               "expanded_b_us": med["expanded_b"], "points_min_us": min(t["points"]), "expanded_min_us": min(both),
               "expanded_spread": spread, "expanded_over_points": emed / med["points"],
               "points_wins_by_more_than_spread": bool(med["points"] < emed * (1 - spread)),
               "copy_us": med["copy"], "copy_bytes_read": 2 * c.total, "points_over_copy": med["points"] / med["copy"],
               "points_alg_bytes": alg, "points_fraction_of_hbm_peak": alg / (med["points"] * 1e-6) / HBM_PEAK}
        rows.append(row)
        print("%-46s points %9.1f us  expanded %9.1f us (x%.2f, spread %.3f)  copy %8.1f us (x%.2f)"
              % (name, med["points"], emed, row["expanded_over_points"], spread, med["copy"], row["points_over_copy"]), flush=True)
        del c
        torch.cuda.empty_cache()
    srs.close()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around one call, variants alternating (the baseline twice a round), median of the "
                     "repeats after warm-up; spread = max(gap of the baseline's two medians, its p90 - p10) / median",
           "baseline": "plk_kzg_open_batch_dev on the expanded job list (the polynomial once per point)",
           "copy": "two device copies in one window: the polynomials' bytes (rotating sets) and as many log bytes (warm)",
           "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1)[:-2])
        f.write(',\n "shapes": [\n  %s\n ]\n}\n' % ",\n  ".join(json.dumps(r) for r in rows))


if __name__ == "__main__":
    main()
