#!/usr/bin/env python3
"""KZG flat batches (plk_kzg_commit_flat_dev / plk_kzg_open_flat_dev) against what a user had
before them, in one process on the same coefficients.

Canonical coefficients, a regular SRS of 4096 points over all 102 group elements, z = g mod 17.
  flat_commit / flat_open   the new calls: one launch each, flat outputs (the opening without commitments)
  batch_commit / batch_open (a) plk_kzg_commit_batch_dev / plk_kzg_open_batch_dev on the same polynomials: host
                            arrays of device pointers, 32 jobs a launch, one 2176-byte record per job.  A list of
                            more than BASE_JOBS polynomials is timed on its first BASE_JOBS and scaled by npoly /
                            BASE_JOBS (the record says so): the call is a loop of identical launches.  The host
                            arrays are built once, outside the timing.  Its G1 bytes and ys are compared with the new
                            calls' on those polynomials.
  segments                  (b) commitments as plk_msm_g1_segments_dev over an SRS replicated once per polynomial
                            (3 bytes a coefficient more to read; the replica is built outside the timing)
  copy                      a device copy (torch copy_) of as many bytes as the opening touches: the coefficients,
                            one z and five output bytes per polynomial
Each time is a pair of device events around one variant on the stream, after warm-up; the variants alternate, the
two batch baselines twice per round, and the median of the repeats is kept.  A baseline's spread is the larger of
the gap between its two interleaved medians and its own 10th-to-90th percentile width, over its median; the new call
is held to be faster only where it wins by more than that.  The coefficients rotate through distinct buffer sets of
more than twice the 256 MB last-level cache in all where the list is large enough for that to matter.

  python tools/kzg_flat_bench.py [--out profiles/kzg_flat_bench.json] [--reps 15] [--only 0,1,...]
  python tools/kzg_flat_bench.py --resources   (no GPU: compiles csrc/kzg_flat.hip for gfx950 and records the
                                                kernels' register, LDS and scratch figures in the same file)
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
BASE_JOBS = 4096
SRS_N = 4096
# (name, kind, polynomials, m)
SHAPES = [("2^20 x 16", "uniform", 1 << 20, 16), ("2^20 x 32", "uniform", 1 << 20, 32),
          ("2^16 x 256", "uniform", 1 << 16, 256), ("2^16 x 1024", "uniform", 1 << 16, 1024),
          ("2^14 x 4096", "uniform", 1 << 14, 4096), ("ragged 2^20 x 1..32", "ragged", 1 << 20, 32),
          ("ragged 2^16 x 1..1024", "ragged", 1 << 16, 1024), ("32 x 4096", "uniform", 32, 4096),
          ("1024 x 4096", "uniform", 1024, 4096)]


def resources():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} from -Rpass-analysis=kernel-resource-usage"""
    src = os.path.join(ROOT, "plonk.c_amd", "csrc", "kzg_flat.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_flat_bench.json"))
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
    srs_pts, _ = gen.msm_inputs(0xF1A7, SRS_N, "full")
    srs = h.Srs(srs_pts)
    d_srs = torch.from_numpy(srs_pts).cuda()

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

    class Case:
        def __init__(self, kind, npoly, m):
            self.kind, self.npoly, self.m = kind, npoly, m
            rng = np.random.default_rng(npoly + m)
            if kind == "uniform":
                lens = np.full(npoly, m, np.int64)
                self.off = None
            else:
                lens = rng.integers(1, m + 1, npoly)
            off = np.concatenate([[0], np.cumsum(lens)])
            self.total = total = int(off[-1])
            if kind == "ragged":
                self.off = torch.from_numpy(off.astype(np.uint32).view(np.int32).copy()).cuda()
            self.zs = (torch.arange(npoly, device="cuda") % 17).to(torch.uint8)
            self.bytes = total + npoly + 5 * npoly + (4 * (npoly + 1) if kind == "ragged" else 0)
            self.nsets = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // total) + 1))
            g = torch.Generator(device="cuda")
            g.manual_seed(total + npoly)
            self.sets = [torch.randint(0, 17, (total,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(self.nsets)]
            self.ys, self.status = (torch.empty(npoly, dtype=torch.uint8, device="cuda") for _ in range(2))
            self.proofs, self.commits = (torch.empty(3 * npoly, dtype=torch.uint8, device="cuda") for _ in range(2))
            # (a) the batch calls: host arrays of the first `jobs` polynomials of every buffer set, built once
            self.jobs = jobs = min(npoly, BASE_JOBS)
            self.ptrs = [(C.c_void_p * jobs)(*[s.data_ptr() + int(o) for o in off[:jobs]]) for s in self.sets]
            self.lens = (C.c_size_t * jobs)(*[int(v) for v in lens[:jobs]])
            self.hzs = (C.c_uint8 * jobs)(*[g % 17 for g in range(jobs)])
            self.res = torch.zeros(jobs * REC, dtype=torch.uint8, device="cuda")
            self.bys = torch.empty(jobs, dtype=torch.uint8, device="cuda")
            # (b) the SRS replicated once per polynomial
            within = torch.arange(total, device="cuda") - torch.repeat_interleave(
                torch.from_numpy(off[:-1]).cuda(), torch.from_numpy(lens).cuda())
            self.rep = d_srs[within].reshape(-1).contiguous()
            del within
            self.out4 = torch.empty(4 * npoly, dtype=torch.uint8, device="cuda")
            ws = h.msm_g1_segments_workspace(total, m if kind == "uniform" else 0, npoly, kind == "ragged")
            self.work = torch.empty(ws, dtype=torch.uint8, device="cuda") if ws else None
            ncp = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // self.bytes) + 1))
            self.cp = [(torch.empty(self.bytes, dtype=torch.uint8, device="cuda"), torch.empty(self.bytes, dtype=torch.uint8, device="cuda"))
                       for _ in range(ncp)]

        def flat_open(self, i):
            h.kzg_open_flat_dev(srs, self.sets[i % self.nsets], self.total, self.off, self.m, self.npoly, self.zs, self.ys,
                                self.proofs, None, self.status)

        def flat_commit(self, i):
            h.kzg_commit_flat_dev(srs, self.sets[i % self.nsets], self.total, self.off, self.m, self.npoly, self.commits, self.status)

        def batch_open(self, i):
            rc = L.plk_kzg_open_batch_dev(srs._h, self.ptrs[i % self.nsets], self.lens, self.hzs, self.jobs, self.bys.data_ptr(),
                                          self.res.data_ptr(), None, None, None)
            assert rc == 0, rc

        def batch_commit(self, i):
            rc = L.plk_kzg_commit_batch_dev(srs._h, self.ptrs[i % self.nsets], self.lens, self.jobs, self.res.data_ptr(), None)
            assert rc == 0, rc

        def segments(self, i):
            h.msm_g1_segments_dev(self.rep, self.sets[i % self.nsets], self.total, self.off, self.m if self.kind == "uniform" else 0,
                                  self.npoly, self.out4, work=self.work)

        def copy(self, i):
            src, dst = self.cp[i % len(self.cp)]
            dst.copy_(src)

        def agree(self):
            """the batch calls' bytes on the first `jobs` polynomials of set 0 against the flat calls' and the segments'"""
            j = self.jobs
            rec = self.res.view(j, REC)
            self.flat_open(0)
            self.flat_commit(0)
            self.segments(0)
            self.batch_open(0)
            torch.cuda.synchronize()
            ok = bool(torch.equal(rec[:, h.MSM_G1_OFFSET:h.MSM_G1_OFFSET + 3], self.proofs.view(-1, 3)[:j]))
            ok = ok and bool(torch.equal(self.bys, self.ys[:j])) and int(self.status.sum()) == 0
            self.batch_commit(0)
            torch.cuda.synchronize()
            ok = ok and bool(torch.equal(rec[:, h.MSM_G1_OFFSET:h.MSM_G1_OFFSET + 3], self.commits.view(-1, 3)[:j]))
            return ok and bool(torch.equal(self.out4.view(-1, 4)[:, :3], self.commits.view(-1, 3)))

    def spread_of(t, a, b):
        both = t[a] + t[b]
        med = statistics.median(both)
        return med, max(abs(statistics.median(t[a]) - statistics.median(t[b])), pct(both, 0.9) - pct(both, 0.1)) / med

    rows = {r["shape"]: r for r in load(a.out).get("shapes", [])}
    only = [int(v) for v in a.only.split(",") if v != ""] or list(range(len(SHAPES)))
    for i in only:
        name, kind, npoly, m = SHAPES[i]
        c = Case(kind, npoly, m)
        agree = c.agree()
        t = timed({"flat_open": c.flat_open, "batch_open": c.batch_open, "flat_commit": c.flat_commit, "batch_commit": c.batch_commit,
                   "segments": c.segments, "copy": c.copy, "batch_open_b": c.batch_open, "batch_commit_b": c.batch_commit}, a.reps, 2)
        med = {k: statistics.median(v) for k, v in t.items()}
        scale = npoly / c.jobs
        bo, so = spread_of(t, "batch_open", "batch_open_b")
        bc, sc = spread_of(t, "batch_commit", "batch_commit_b")
        seg_spread = (pct(t["segments"], 0.9) - pct(t["segments"], 0.1)) / med["segments"]
        row = {"shape": name, "polynomials": npoly, "coefficients": c.total, "bytes_touched": c.bytes, "plan": h.kzg_flat_plan(m, npoly, kind == "ragged"),
               "buffer_sets": c.nsets, "repeats": a.reps,
               "batch_jobs_timed": c.jobs, "batch_scaled_by": scale, "batch_launches_scaled": -(-npoly // 32),
               "flat_open_us": med["flat_open"], "flat_open_min_us": min(t["flat_open"]), "flat_commit_us": med["flat_commit"],
               "copy_us": med["copy"], "flat_open_over_copy": med["flat_open"] / med["copy"],
               "flat_open_fraction_of_hbm_peak": c.bytes / (med["flat_open"] * 1e-6) / HBM_PEAK,
               "batch_open_us": bo * scale, "batch_open_timed_us": bo, "batch_open_spread": so,
               "batch_commit_us": bc * scale, "batch_commit_timed_us": bc, "batch_commit_spread": sc,
               "segments_commit_us": med["segments"], "segments_spread": seg_spread,
               "batch_open_over_flat_open": bo * scale / med["flat_open"], "batch_commit_over_flat_commit": bc * scale / med["flat_commit"],
               "segments_over_flat_commit": med["segments"] / med["flat_commit"],
               "flat_open_beats_batch_by_more_than_its_spread": bool(med["flat_open"] < bo * scale * (1 - so)),
               "flat_commit_beats_batch_by_more_than_its_spread": bool(med["flat_commit"] < bc * scale * (1 - sc)),
               "flat_commit_beats_segments_by_more_than_its_spread": bool(med["flat_commit"] < med["segments"] * (1 - seg_spread)),
               "flat_open_slower_than_batch": bool(med["flat_open"] > bo * scale),
               "flat_commit_slower_than_batch": bool(med["flat_commit"] > bc * scale),
               "bytes_equal": agree}
        rows[name] = row
        print("%-24s open: flat %9.1f us (x%.2f of a copy)  batch %12.1f us (x%.1f, spread %.3f)   commit: flat %9.1f us  batch %12.1f us "
              "(x%.1f, spread %.3f)  segments %9.1f us (x%.2f)   scaled x%g  equal: %s"
              % (name, med["flat_open"], row["flat_open_over_copy"], bo * scale, row["batch_open_over_flat_open"], so, med["flat_commit"],
                 bc * scale, row["batch_commit_over_flat_commit"], sc, med["segments"], row["segments_over_flat_commit"], scale, agree),
              flush=True)
        del c
        torch.cuda.empty_cache()
        res = {k: v for k, v in load(a.out).items() if k == "kernel_resources"}
        res.update({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
                    "timing": "device events around one variant, variants alternating (each batch baseline twice a round), median of the "
                              "repeats after warm-up; spread = max(gap of the baseline's two medians, its p90 - p10) / median",
                    "baselines": {"batch": "plk_kzg_commit_batch_dev / plk_kzg_open_batch_dev, host arrays built once; a list of more than "
                                           "%d polynomials is timed on its first %d and scaled by npoly / %d (batch_scaled_by): *_us is the "
                                           "scaled figure, *_timed_us the measured one" % (BASE_JOBS, BASE_JOBS, BASE_JOBS),
                                  "segments": "plk_msm_g1_segments_dev over an SRS replicated once per polynomial (one replica for all buffer sets)",
                                  "copy": "torch copy_ of bytes_touched bytes (the coefficients, a z and five output bytes per polynomial, "
                                          "the offset words): reads that many and writes that many"},
                    "reps": a.reps, "shapes": [rows[s[0]] for s in SHAPES if s[0] in rows]})
        store(a.out, res)
    srs.close()


if __name__ == "__main__":
    main()
