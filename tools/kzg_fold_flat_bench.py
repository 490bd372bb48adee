#!/usr/bin/env python3
"""KZG flat folded openings (plk_kzg_open_fold_flat_dev) against what a user had before them,
in one process on the same coefficients.

Canonical coefficients, the well-formed SRS srs[i] = (2^i mod 17) G of 4096 points (the subgroup of order 17, where
baseline (b)'s weighted fold of single proofs equals the folded proof), z = g mod 17, weights 0 .. 16.
  fold          the new call without commitments: one launch, flat outputs
  fold_commits  the new call with commitments
  batch         (a) plk_kzg_open_fold_batch_dev, unchanged, on the same groups: host arrays of device pointers, host
                weights and points, 32 polynomials a launch, one 2176-byte record per group.  A list of more than
                BASE_POLYS polynomials is timed on its first BASE_POLYS polynomials' worth of groups and scaled by
                ngroups / groups timed (the record says so): the call is a loop of identical launches.  The host
                arrays are built once, outside the timing.
  two_launch    (b) the composition the library already allowed: plk_kzg_open_flat_dev over all k ngroups polynomials
                (z expanded per polynomial, outside the timing) + plk_msm_g1_segments_dev (m = k) over its proofs and
                the weights.  Its 4-byte words, ys and commitments are compared with the new call's at every shape.
  copy          a device copy (torch copy_) of as many bytes as the new call touches
Each time is a pair of device events around one variant on the stream, after warm-up; the variants alternate, each
baseline twice per round, and the median of the repeats is kept.  A baseline's spread is the larger of the gap
between its two interleaved medians and its own 10th-to-90th percentile width, over its median; the new call is held
to be faster only where it wins by more than that.  The coefficients rotate through distinct buffer sets of more than
twice the 256 MB last-level cache in all where the list is large enough for that to matter.

  python tools/kzg_fold_flat_bench.py [--out profiles/kzg_fold_flat_bench.json] [--reps 15] [--only 0,1,...]
  python tools/kzg_fold_flat_bench.py --resources   (no GPU: compiles csrc/kzg_fold_flat.hip for gfx950 and records
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
# (name, kind, groups, k, m)
SHAPES = [("2^20 x 9 x 16", "uniform", 1 << 20, 9, 16), ("2^18 x 9 x 32", "uniform", 1 << 18, 9, 32),
          ("2^14 x 9 x 256", "uniform", 1 << 14, 9, 256), ("2^12 x 9 x 1024", "uniform", 1 << 12, 9, 1024),
          ("2^10 x 9 x 4096", "uniform", 1 << 10, 9, 4096), ("2^18 x 2 x 32", "uniform", 1 << 18, 2, 32),
          ("2^18 x 16 x 32", "uniform", 1 << 18, 16, 32), ("ragged 2^18 x 9 x 1..32", "ragged", 1 << 18, 9, 32),
          ("ragged 2^12 x 9 x 1..1024", "ragged", 1 << 12, 9, 1024), ("3 x 9 x 4096", "uniform", 3, 9, 4096)]


def resources():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} from -Rpass-analysis=kernel-resource-usage"""
    src = os.path.join(ROOT, "plonk.c_amd", "csrc", "kzg_fold_flat.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    err = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-c", src, "-o",
                          os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "lds_bytes_per_block", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
            "VGPRs Spill": "vgpr_spills"}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_fold_flat_bench.json"))
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
    # srs[i] = (2^i mod 17) G, the well-formed SRS for s = 2: inside the subgroup of order 17, where the folded proof
    # equals the weighted fold of the single proofs (over all 102 elements baseline (b) computes other bytes)
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
        def __init__(self, kind, ng, k, m):
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
            hz = (np.arange(ng) % 17).astype(np.uint8)
            hw = rng.integers(0, 17, npoly).astype(np.uint8)
            self.zs, self.w = torch.from_numpy(hz).cuda(), torch.from_numpy(hw).cuda()
            self.zx = torch.from_numpy(np.repeat(hz, k)).cuda()      # (b): z per polynomial, built outside the timing
            self.bytes = total + 2 * npoly + 5 * ng + (4 * (npoly + 1) if kind == "ragged" else 0)
            self.nsets = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // total) + 1))
            g = torch.Generator(device="cuda")
            g.manual_seed(total + npoly)
            self.sets = [torch.randint(0, 17, (total,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(self.nsets)]
            self.ys, self.commits, self.proofs, self.status = u8(npoly), u8(3 * npoly), u8(3 * ng), u8(ng)
            # (a) the folded batch call: host arrays of the first `groups` groups of every buffer set, built once
            self.groups = gr = min(ng, max(1, BASE_POLYS // k))
            jobs = gr * k
            self.ptrs = [(C.c_void_p * jobs)(*[s.data_ptr() + int(o) for o in off[:jobs]]) for s in self.sets]
            self.lens = (C.c_size_t * jobs)(*[int(v) for v in lens[:jobs]])
            self.start = (C.c_int * (gr + 1))(*[k * g for g in range(gr + 1)])
            self.hw = (C.c_uint8 * jobs)(*hw[:jobs].tolist())
            self.hzs = (C.c_uint8 * gr)(*hz[:gr].tolist())
            self.res = torch.zeros(gr * REC, dtype=torch.uint8, device="cuda")
            self.bys = u8(jobs)
            ws = h.kzg_fold_workspace([int(v) for v in lens[:jobs]], [k * g for g in range(gr + 1)])
            self.bwork = u8(ws) if ws else None
            # (b) the two-launch composition
            self.ys1, self.pr1, self.cm1, self.st1, self.out4 = u8(npoly), u8(3 * npoly), u8(3 * npoly), u8(npoly), u8(4 * ng)
            ws = h.msm_g1_segments_workspace(npoly, k, ng, False)
            self.swork = u8(ws) if ws else None
            ncp = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // self.bytes) + 1))
            self.cp = [(u8(self.bytes), u8(self.bytes)) for _ in range(ncp)]

        def fold(self, i, commits=None):
            h.kzg_open_fold_flat_dev(srs, self.sets[i % self.nsets], self.total, self.off, self.m, self.k, self.ng, self.w, self.zs,
                                     self.ys, self.proofs, commits, self.status)

        def fold_commits(self, i):
            self.fold(i, self.commits)

        def batch(self, i):
            rc = L.plk_kzg_open_fold_batch_dev(srs._h, self.ptrs[i % self.nsets], self.lens, self.hw, self.start, self.hzs, self.groups,
                                               self.bys.data_ptr(), self.res.data_ptr(), None,
                                               self.bwork.data_ptr() if self.bwork is not None else None, None)
            assert rc == 0, rc

        def two_launch(self, i, commits=None):
            h.kzg_open_flat_dev(srs, self.sets[i % self.nsets], self.total, self.off, self.m, self.npoly, self.zx, self.ys1, self.pr1,
                                commits, self.st1)
            h.msm_g1_segments_dev(self.pr1, self.w, self.npoly, None, self.k, self.ng, self.out4, work=self.swork)

        def copy(self, i):
            src, dst = self.cp[i % len(self.cp)]
            dst.copy_(src)

        def agree(self):
            """the new call's proofs, ys and commitments on set 0 against the two-launch composition's, and against the
            folded batch call's on the groups it is timed on"""
            self.fold(0, self.commits)
            self.two_launch(0, self.cm1)
            self.batch(0)
            torch.cuda.synchronize()
            two = (bool(torch.equal(self.out4.view(-1, 4)[:, :3], self.proofs.view(-1, 3))) and int(self.out4.view(-1, 4)[:, 3].sum()) == 0
                   and bool(torch.equal(self.ys1, self.ys)) and bool(torch.equal(self.cm1, self.commits))
                   and int(self.status.sum()) == 0 and int(self.st1.sum()) == 0)
            rec = self.res.view(self.groups, REC)
            bat = (bool(torch.equal(rec[:, h.MSM_G1_OFFSET:h.MSM_G1_OFFSET + 3], self.proofs.view(-1, 3)[:self.groups]))
                   and bool(torch.equal(self.bys, self.ys[:self.groups * self.k])))
            return two, bat

    def spread_of(t, x, y):
        both = t[x] + t[y]
        med = statistics.median(both)
        return med, max(abs(statistics.median(t[x]) - statistics.median(t[y])), pct(both, 0.9) - pct(both, 0.1)) / med

    rows = {r["shape"]: r for r in load(a.out).get("shapes", [])}
    only = [int(v) for v in a.only.split(",") if v != ""] or list(range(len(SHAPES)))
    for i in only:
        name, kind, ng, k, m = SHAPES[i]
        c = Case(kind, ng, k, m)
        two_equal, batch_equal = c.agree()
        assert two_equal, "%s: the new call and the two-launch composition differ" % name
        assert batch_equal, "%s: the new call and plk_kzg_open_fold_batch_dev differ" % name
        t = timed({"fold": c.fold, "batch": c.batch, "two_launch": c.two_launch, "fold_commits": c.fold_commits, "copy": c.copy,
                   "batch_b": c.batch, "two_launch_b": c.two_launch}, a.reps, 2)
        med = {n: statistics.median(v) for n, v in t.items()}
        scale = ng / c.groups
        ba, sa = spread_of(t, "batch", "batch_b")
        tw, st = spread_of(t, "two_launch", "two_launch_b")
        row = {"shape": name, "groups": ng, "k": k, "m": m, "polynomials": c.npoly, "coefficients": c.total, "bytes_touched": c.bytes,
               "plan": h.kzg_fold_flat_plan(m, k, ng, kind == "ragged"), "buffer_sets": c.nsets, "repeats": a.reps,
               "batch_groups_timed": c.groups, "batch_scaled_by": scale, "batch_launches_scaled": -(-ng // (32 // k)),
               "fold_us": med["fold"], "fold_min_us": min(t["fold"]), "fold_commits_us": med["fold_commits"],
               "copy_us": med["copy"], "fold_over_copy": med["fold"] / med["copy"],
               "fold_fraction_of_hbm_peak": c.bytes / (med["fold"] * 1e-6) / HBM_PEAK,
               "batch_us": ba * scale, "batch_timed_us": ba, "batch_spread": sa,
               "two_launch_us": tw, "two_launch_spread": st,
               "batch_over_fold": ba * scale / med["fold"], "two_launch_over_fold": tw / med["fold"],
               "fold_beats_batch_by_more_than_its_spread": bool(med["fold"] < ba * scale * (1 - sa)),
               "fold_beats_two_launch_by_more_than_its_spread": bool(med["fold"] < tw * (1 - st)),
               "fold_slower_than_batch": bool(med["fold"] > ba * scale), "fold_slower_than_two_launch": bool(med["fold"] > tw),
               "bytes_equal_two_launch": two_equal, "bytes_equal_batch": batch_equal}
        rows[name] = row
        print("%-28s fold %9.1f us (x%.2f of a copy; with commitments %9.1f us)  batch %12.1f us (x%.1f, spread %.3f, scaled x%g)  "
              "two launches %9.1f us (x%.2f, spread %.3f)  equal: %s %s"
              % (name, med["fold"], row["fold_over_copy"], med["fold_commits"], ba * scale, row["batch_over_fold"], sa, scale, tw,
                 row["two_launch_over_fold"], st, two_equal, batch_equal), flush=True)
        del c
        torch.cuda.empty_cache()
        res = {n: v for n, v in load(a.out).items() if n == "kernel_resources"}
        res.update({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
                    "timing": "device events around one variant, variants alternating (each baseline twice a round), median of the "
                              "repeats after warm-up; spread = max(gap of the baseline's two medians, its p90 - p10) / median",
                    "baselines": {"batch": "plk_kzg_open_fold_batch_dev, host arrays built once; a list of more than %d polynomials is "
                                           "timed on its first %d polynomials' worth of groups and scaled by ngroups / groups timed "
                                           "(batch_scaled_by): batch_us is the scaled figure, batch_timed_us the measured one"
                                           % (BASE_POLYS, BASE_POLYS),
                                  "two_launch": "plk_kzg_open_flat_dev over k ngroups polynomials (z expanded outside the timing, no "
                                                "commitments) + plk_msm_g1_segments_dev (m = k) over its proofs and the weights",
                                  "copy": "torch copy_ of bytes_touched bytes (the coefficients, a weight and a y per polynomial, a z, "
                                          "a status and three proof bytes per group, the offset words): reads that many and writes "
                                          "that many"},
                    "reps": a.reps, "shapes": [rows[s[0]] for s in SHAPES if s[0] in rows]})
        store(a.out, res)
    srs.close()


if __name__ == "__main__":
    main()
