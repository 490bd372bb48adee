#!/usr/bin/env python3
"""KZG flat multi-point openings (plk_kzg_open_multi_flat_dev) against what a user had before
them, in one process on the same coefficients.

Canonical coefficients, the well-formed SRS srs[i] = (2^i mod 17) G of 4096 points, u = g mod 17, weights 0 .. 16.
  multi          the new call without commitments: one launch, flat outputs
  multi_commits  the new call with commitments
  batch          (a) plk_kzg_open_multi_batch_dev, unchanged, on the same groups: host arrays of device pointers, host
                 masks, weights and challenges, four groups a launch of its own kernels plus the folded opening group
                 by group, two 2176-byte records per group.  A list of more than BASE_POLYS polynomials is timed on
                 its first BASE_POLYS polynomials' worth of groups and scaled by ngroups / groups timed (the record
                 says so): the call is a loop of identical launches.  The host arrays are built once, outside the
                 timing.  Its proofs and ys are compared with the new call's at every shape.
  fold_flat      a reference line, not a target: plk_kzg_open_fold_flat_dev on the same polynomials and weights at the
                 one point us[g] -- what the multi-point scheme costs over a plain fold
  copy           a device copy (torch copy_) of as many bytes as the new call touches
Each time is a pair of device events around one variant on the stream, after warm-up; the variants alternate, the
baseline twice per round, and the median of the repeats is kept.  The baseline's spread is the larger of the gap
between its two interleaved medians and its own 10th-to-90th percentile width, over its median; the new call is held
to be faster only where it wins by more than that.  The coefficients rotate through distinct buffer sets of more than
twice the 256 MB last-level cache in all where the list is large enough for that to matter.

  python tools/kzg_multi_flat_bench.py [--out profiles/kzg_multi_flat_bench.json] [--reps 15] [--only 0,1,...]
  python tools/kzg_multi_flat_bench.py --resources   (no GPU: compiles csrc/kzg_multi_flat.hip for gfx950 and records
                                                      the kernels' register, LDS and scratch figures in the same file)
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk.c_amd"))

HBM_PEAK = 8e12
LLC_BYTES = 256 << 20
MAX_SETS = 12
BASE_POLYS = 4096
SRS_N = 4096
FULL = (1 << 17) - 1
# (name, kind, groups, k, m, sets)
SHAPES = [("PLONK 2^20 x 9 x 16", "uniform", 1 << 20, 9, 16, "plonk"), ("PLONK 2^18 x 9 x 32", "uniform", 1 << 18, 9, 32, "plonk"),
          ("PLONK 2^14 x 9 x 256", "uniform", 1 << 14, 9, 256, "plonk"), ("PLONK 2^12 x 9 x 1024", "uniform", 1 << 12, 9, 1024, "plonk"),
          ("PLONK 2^10 x 9 x 4096", "uniform", 1 << 10, 9, 4096, "plonk"), ("nine pairs 2^18 x 9 x 32", "uniform", 1 << 18, 9, 32, "pairs"),
          ("wide set 2^18 x 1 x 32", "uniform", 1 << 18, 1, 32, "sixteen"), ("k = 15 2^18 x 15 x 32", "uniform", 1 << 18, 15, 32, "random"),
          ("k = 15 2^10 x 15 x 4096", "uniform", 1 << 10, 15, 4096, "random"),
          ("ragged 2^18 x 9 x 1..32", "ragged", 1 << 18, 9, 32, "mixed"), ("ragged 2^12 x 9 x 1..1024", "ragged", 1 << 12, 9, 1024, "mixed"),
          ("launch-bound 4 x 9 x 4096", "uniform", 4, 9, 4096, "plonk")]


def resources():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy, spills}} from -Rpass-analysis=kernel-resource-usage"""
    src = os.path.join(ROOT, "plonk.c_amd", "csrc", "kzg_multi_flat.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    err = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-c", src, "-o",
                          os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "lds_bytes_per_block", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
            "VGPRs Spill": "vgpr_spills", "SGPRs Spill": "sgpr_spills"}
    for line in err.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
            name = re.sub(r"\(anonymous namespace\)::|\(.*$", "", name)
            name = re.sub(r"^void ", "", name)
            cur = out.setdefault(name, {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {}


def store(path, data):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def masks(np, rng, kind, ng, k):
    """(ng, k) uint32 masks.  plonk: eight polynomials at {z}, the ninth at {z, 2 z}, z = 1 + g mod 16 (fewer or
    more polynomials keep the pair last); pairs: polynomial i at {2 i mod 17, (2 i + 1) mod 17}, T = all 17 points at
    k = 9; sixteen: every point but g mod 17; random: 1 .. 16 random points; mixed: the five kinds by turns"""
    g = np.arange(ng, dtype=np.int64)[:, None]
    i = np.arange(k, dtype=np.int64)[None, :]
    z = 1 + g % 16
    plonk = np.where(i == k - 1, (1 << z) | (1 << (2 * z % 17)), 1 << z)
    pairs = (1 << (2 * i % 17)) | (1 << ((2 * i + 1) % 17)) | 0 * g
    sixteen = FULL & ~(1 << (g % 17)) | 0 * i
    bits = rng.integers(0, 2, (ng, k, 17))
    rnd = (bits << np.arange(17)).sum(axis=2)
    rnd = np.where((rnd == 0) | (rnd == FULL), 1 << (g % 17), rnd)
    if kind == "mixed":
        sel = (g + i) % 5
        out = np.select([sel == 0, sel == 1, sel == 2, sel == 3], [1 + 0 * rnd, plonk, pairs, sixteen], rnd)
    else:
        out = {"plonk": plonk, "pairs": pairs, "sixteen": sixteen, "random": rnd}[kind]
    return np.ascontiguousarray(np.broadcast_to(out, (ng, k)).astype(np.uint32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_multi_flat_bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default="")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        data = load(a.out)
        data["kernel_resources"] = resources()
        store(a.out, data)
        for k, v in data["kernel_resources"].items():
            print(k, v)
        return

    import numpy as np
    import torch

    import plonkhip as h

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen

    REC = h.MSM_RESULT_BYTES
    h.init(0)
    L = h.lib()
    srs_pts = np.array([gen.KG[pow(2, i, 17)] for i in range(SRS_N)], np.uint8)
    srs = h.Srs(srs_pts)

    def timed(fns, reps, warm):
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

    def u8(n):
        return torch.empty(n, dtype=torch.uint8, device="cuda")

    class Case:
        def __init__(self, kind, ng, k, m, setkind):
            self.kind, self.ng, self.k, self.m = kind, ng, k, m
            self.npoly = npoly = k * ng
            rng = np.random.default_rng(ng + k + m)
            if kind == "uniform":
                lens = np.full(npoly, m, np.int64)
                self.off = None
            else:
                lens = rng.integers(1, m + 1, npoly)
            off = np.concatenate([[0], np.cumsum(lens)])
            self.total = total = int(off[-1])
            if kind == "ragged":
                self.off = torch.from_numpy(off.astype(np.uint32).view(np.int32).copy()).cuda()
            hu = (np.arange(ng) % 17).astype(np.uint8)
            hw = rng.integers(0, 17, npoly).astype(np.uint8)
            hs = masks(np, rng, setkind, ng, k)
            self.us, self.w = torch.from_numpy(hu).cuda(), torch.from_numpy(hw).cuda()
            self.masks = torch.from_numpy(hs.reshape(-1).view(np.int32).copy()).cuda()
            # the coefficients, a mask, a weight and a 17-byte row per polynomial, a u, a status and six proof bytes
            # per group, the offset words
            self.bytes = total + 22 * npoly + 8 * ng + (4 * (npoly + 1) if kind == "ragged" else 0)
            self.nsets = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // total) + 1))
            g = torch.Generator(device="cuda")
            g.manual_seed(total + npoly)
            self.sets = [torch.randint(0, 17, (total,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(self.nsets)]
            self.ys, self.commits, self.proofs, self.status = u8(17 * npoly), u8(3 * npoly), u8(6 * ng), u8(ng)
            # (a) the multi-point batch call: host arrays of the first `groups` groups of every buffer set, built once
            self.groups = gr = min(ng, max(1, BASE_POLYS // k))
            jobs = gr * k
            self.ptrs = [(C.c_void_p * jobs)(*[s.data_ptr() + int(o) for o in off[:jobs]]) for s in self.sets]
            self.lens = (C.c_size_t * jobs)(*[int(v) for v in lens[:jobs]])
            self.start = (C.c_int * (gr + 1))(*[k * g for g in range(gr + 1)])
            self.hs = (C.c_uint32 * jobs)(*hs.reshape(-1)[:jobs].tolist())
            self.hw = (C.c_uint8 * jobs)(*hw[:jobs].tolist())
            self.hus = (C.c_uint8 * gr)(*hu[:gr].tolist())
            self.res = torch.zeros(2 * gr * REC, dtype=torch.uint8, device="cuda")
            self.bys = u8(17 * jobs)
            ws = h.kzg_multi_workspace([int(v) for v in lens[:jobs]], hs.reshape(-1)[:jobs].tolist(), [k * g for g in range(gr + 1)])
            self.bwork = u8(max(ws, 256))
            self.batch_launches = -(-gr // 4)
            # the reference line
            self.fys, self.fpr, self.fst = u8(npoly), u8(3 * ng), u8(ng)
            ncp = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // self.bytes) + 1))
            self.cp = [(u8(self.bytes), u8(self.bytes)) for _ in range(ncp)]

        def multi(self, i, commits=None):
            h.kzg_open_multi_flat_dev(srs, self.sets[i % self.nsets], self.total, self.off, self.m, self.k, self.ng, self.masks, self.w,
                                      self.us, self.ys, self.proofs, commits, self.status)

        def multi_commits(self, i):
            self.multi(i, self.commits)

        def batch(self, i):
            rc = L.plk_kzg_open_multi_batch_dev(srs._h, self.ptrs[i % self.nsets], self.lens, self.hs, self.hw, self.start, self.hus,
                                                self.groups, self.bys.data_ptr(), self.res.data_ptr(), None, self.bwork.data_ptr(), None)
            assert rc == 0, rc

        def fold_flat(self, i):
            h.kzg_open_fold_flat_dev(srs, self.sets[i % self.nsets], self.total, self.off, self.m, self.k, self.ng, self.w, self.us,
                                     self.fys, self.fpr, None, self.fst)

        def copy(self, i):
            src, dst = self.cp[i % len(self.cp)]
            dst.copy_(src)

        def agree(self):
            """the new call's proofs and ys on set 0 against the multi-point batch call's on the groups it is timed on"""
            self.multi(0)
            self.batch(0)
            torch.cuda.synchronize()
            rec = self.res.view(self.groups, 2, REC)[:, :, h.MSM_G1_OFFSET:h.MSM_G1_OFFSET + 3].reshape(self.groups, 6)
            return (int(self.status.sum()) == 0 and bool(torch.equal(rec, self.proofs.view(-1, 6)[:self.groups]))
                    and bool(torch.equal(self.bys, self.ys[:17 * self.groups * self.k])))

    def spread_of(t, x, y):
        both = t[x] + t[y]
        med = statistics.median(both)
        return med, max(abs(statistics.median(t[x]) - statistics.median(t[y])), pct(both, 0.9) - pct(both, 0.1)) / med

    rows = {r["shape"]: r for r in load(a.out).get("shapes", [])}
    only = [int(v) for v in a.only.split(",") if v != ""] or list(range(len(SHAPES)))
    for i in only:
        name, kind, ng, k, m, setkind = SHAPES[i]
        c = Case(kind, ng, k, m, setkind)
        equal = c.agree()
        assert equal, "%s: the new call and plk_kzg_open_multi_batch_dev differ" % name
        t = timed({"multi": c.multi, "batch": c.batch, "fold_flat": c.fold_flat, "multi_commits": c.multi_commits, "copy": c.copy,
                   "batch_b": c.batch}, a.reps, 2)
        med = {n: statistics.median(v) for n, v in t.items()}
        scale = ng / c.groups
        ba, sa = spread_of(t, "batch", "batch_b")
        row = {"shape": name, "groups": ng, "k": k, "m": m, "sets": setkind, "polynomials": c.npoly, "coefficients": c.total,
               "bytes_touched": c.bytes, "plan": h.kzg_multi_flat_plan(m, k, ng, kind == "ragged"), "buffer_sets": c.nsets,
               "repeats": a.reps, "batch_groups_timed": c.groups, "batch_scaled_by": scale,
               "batch_own_kernel_launches_timed": c.batch_launches,
               "multi_us": med["multi"], "multi_min_us": min(t["multi"]), "multi_commits_us": med["multi_commits"],
               "copy_us": med["copy"], "multi_over_copy": med["multi"] / med["copy"],
               "multi_fraction_of_hbm_peak": c.bytes / (med["multi"] * 1e-6) / HBM_PEAK,
               "batch_us": ba * scale, "batch_timed_us": ba, "batch_spread": sa, "batch_over_multi": ba * scale / med["multi"],
               "multi_beats_batch_by_more_than_its_spread": bool(med["multi"] < ba * scale * (1 - sa)),
               "multi_slower_than_batch": bool(med["multi"] > ba * scale),
               "fold_flat_us": med["fold_flat"], "multi_over_fold_flat": med["multi"] / med["fold_flat"],
               "bytes_equal_batch": equal}
        rows[name] = row
        print("%-28s multi %9.1f us (x%.2f of a copy; with commitments %9.1f us)  batch %12.1f us (x%.1f, spread %.3f, scaled x%g)  "
              "fold_flat %9.1f us (multi x%.2f of it)  equal: %s"
              % (name, med["multi"], row["multi_over_copy"], med["multi_commits"], ba * scale, row["batch_over_multi"], sa, scale,
                 med["fold_flat"], row["multi_over_fold_flat"], equal), flush=True)
        del c
        torch.cuda.empty_cache()
        res = {n: v for n, v in load(a.out).items() if n == "kernel_resources"}
        res.update({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
                    "timing": "device events around one variant, variants alternating (the baseline twice a round), median of the "
                              "repeats after warm-up; spread = max(gap of the baseline's two medians, its p90 - p10) / median",
                    "baselines": {"batch": "plk_kzg_open_multi_batch_dev, host arrays built once; a list of more than %d polynomials is "
                                           "timed on its first %d polynomials' worth of groups and scaled by ngroups / groups timed "
                                           "(batch_scaled_by): batch_us is the scaled figure, batch_timed_us the measured one"
                                           % (BASE_POLYS, BASE_POLYS),
                                  "fold_flat": "a reference line, not a target: plk_kzg_open_fold_flat_dev on the same polynomials "
                                               "and weights at the one point us[g], no commitments",
                                  "copy": "torch copy_ of bytes_touched bytes (the coefficients, a mask, a weight and a 17-byte row "
                                          "per polynomial, a u, a status and six proof bytes per group, the offset words): reads that "
                                          "many and writes that many"},
                    "reps": a.reps, "shapes": [rows[s[0]] for s in SHAPES if s[0] in rows]})
        store(a.out, res)
    srs.close()


if __name__ == "__main__":
    main()
