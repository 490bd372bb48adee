#!/usr/bin/env python3
"""Segmented MSM (plk_msm_g1_segments_dev) against what a user had before it, in one process on
the same points and scalars.

Points uniform over all 102 group elements, scalar bytes uniform over 0..255.
  segments  plk_msm_g1_segments_dev: one call, 4 bytes out per segment
  batch     (a) plk_msm_g1_batch_dev into 2176-byte records: the uniform shapes in chunks of at most 65535 MSMs a
            call; the ragged shapes as one call per run of consecutive equal-length segments (what the existing
            interface allows without moving the bytes).  Its G1 bytes are compared with the new call's.
  copy      (b) a device copy (torch copy_) of as many bytes as the call touches: 4 per point, 4 per segment out,
            4 per offset word -- the copy reads that many bytes and writes that many
Each time is a pair of device events around one variant on the stream, after warm-up; the variants alternate, the
batch baseline twice per round (batch and batch_b), and the median of the repeats is kept.  The baseline's spread is
the larger of the gap between its two interleaved medians and its own 10th-to-90th percentile width, over its median;
the new call is held to be faster only where it wins by more than that.  The inputs rotate through distinct buffer
sets of more than twice the 256 MB last-level cache in all, so a call never finds them cached.

  python tools/msm_segments_bench.py [--out profiles/msm_segments_bench.json] [--reps 20] [--only 0,1,...]
  python tools/msm_segments_bench.py --resources   (no GPU: compiles csrc/msm_seg.hip for gfx950 and records the
                                                    kernels' register, LDS and scratch figures in the same file)
"""
import argparse
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
MSM_BATCH_MAX = 65535
MAX_SETS = 80
# (name, kind, segments, points each / the length law)
SHAPES = [("uniform 2^20 x 2", "uniform", 1 << 20, 2), ("uniform 2^20 x 9", "uniform", 1 << 20, 9),
          ("uniform 2^20 x 16", "uniform", 1 << 20, 16), ("uniform 2^16 x 256", "uniform", 1 << 16, 256),
          ("uniform 64 x 2^18", "uniform", 64, 1 << 18), ("uniform 1 x 2^24", "uniform", 1, 1 << 24),
          ("ragged 2^20 x 1..16", "ragged", 1 << 20, "1..16"), ("ragged 4096 x log-uniform 1..2^16", "ragged", 4096, "log")]


def resources():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} from -Rpass-analysis=kernel-resource-usage"""
    src = os.path.join(ROOT, "plonk.c_amd", "csrc", "msm_seg.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_segments_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
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
    group = torch.from_numpy(gen.all_points()).cuda()

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
        def __init__(self, kind, nseg, law):
            self.kind, self.nseg = kind, nseg
            rng = np.random.default_rng(nseg)
            if kind == "uniform":
                self.m, lens = law, None
                self.total = nseg * law
                self.off = None
            else:
                self.m = 0
                lens = rng.integers(1, 17, nseg) if law == "1..16" else np.floor(2 ** rng.uniform(0, 16, nseg)).astype(np.int64)
                off = np.concatenate([[0], np.cumsum(lens)])
                self.total = int(off[-1])
                self.off = torch.from_numpy(off.astype(np.uint32).view(np.int32).copy()).cuda()
                # runs of consecutive equal-length segments: (first point, length, count)
                cut = np.flatnonzero(np.concatenate([[True], lens[1:] != lens[:-1]]))
                cnt = np.diff(np.concatenate([cut, [nseg]]))
                self.runs = []
                for g, c in zip(cut.tolist(), cnt.tolist()):
                    for b in range(0, c, MSM_BATCH_MAX):
                        self.runs.append((int(off[g + b]), int(lens[g]), min(MSM_BATCH_MAX, c - b), g + b))
            total = self.total
            self.bytes = 4 * total + 4 * nseg + (4 * (nseg + 1) if kind == "ragged" else 0)
            self.nsets = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // (4 * total)) + 1))
            g = torch.Generator(device="cuda")
            g.manual_seed(total + nseg)
            self.sets = []
            for _ in range(self.nsets):
                idx = torch.randint(0, 102, (total,), device="cuda", generator=g)
                sc = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda", generator=g)
                self.sets.append((group[idx].reshape(-1).contiguous(), sc))
            self.out4 = torch.empty(4 * nseg, dtype=torch.uint8, device="cuda")
            ws = h.msm_g1_segments_workspace(total, self.m, nseg, kind == "ragged")
            self.work = torch.empty(ws, dtype=torch.uint8, device="cuda") if ws else None
            self.res = torch.zeros(nseg * REC, dtype=torch.uint8, device="cuda")
            ncp = max(2, min(MAX_SETS, -(-2 * LLC_BYTES // self.bytes) + 1))
            self.cp = [(torch.empty(self.bytes, dtype=torch.uint8, device="cuda"), torch.empty(self.bytes, dtype=torch.uint8, device="cuda"))
                       for _ in range(ncp)]

        def segments(self, i):
            p, s = self.sets[i % self.nsets]
            h.msm_g1_segments_dev(p, s, self.total, self.off, self.m, self.nseg, self.out4, work=self.work)

        def batch(self, i):
            p, s = self.sets[i % self.nsets]
            pp, sp, rp = p.data_ptr(), s.data_ptr(), self.res.data_ptr()
            f = L.plk_msm_g1_batch_dev
            if self.kind == "uniform":
                m = self.m
                for b in range(0, self.nseg, MSM_BATCH_MAX):
                    k = min(MSM_BATCH_MAX, self.nseg - b)
                    rc = f(pp + 3 * m * b, 3 * m, sp + m * b, m, m, k, rp + REC * b, None)
                    assert rc == 0, rc
            else:
                for o, m, k, g in self.runs:
                    rc = f(pp + 3 * o, 3 * m, sp + o, m, m, k, rp + REC * g, None)
                    assert rc == 0, rc

        def copy(self, i):
            src, dst = self.cp[i % len(self.cp)]
            dst.copy_(src)

        def measure(self, reps):
            self.segments(0)
            self.batch(0)
            torch.cuda.synchronize()
            rec = self.res.view(self.nseg, REC)
            irregular = int(rec[:, h.MSM_IRREGULAR_OFFSET:h.MSM_IRREGULAR_OFFSET + 4].sum())
            o4 = self.out4.view(self.nseg, 4)
            agree = bool(torch.equal(rec[:, h.MSM_G1_OFFSET:h.MSM_G1_OFFSET + 3], o4[:, :3])) and irregular == 0 and int(o4[:, 3].sum()) == 0
            slow = self.kind == "ragged" and len(self.runs) > 100000     # a million launches a run: fewer repeats
            t = timed({"segments": self.segments, "batch": self.batch, "copy": self.copy, "batch_b": self.batch},
                      3 if slow else reps, 1 if slow else 2)
            return t, agree

    rows = {r["shape"]: r for r in load(a.out).get("shapes", [])}
    only = [int(v) for v in a.only.split(",") if v != ""] or list(range(len(SHAPES)))
    for i in only:
        name, kind, nseg, law = SHAPES[i]
        c = Case(kind, nseg, law)
        t, agree = c.measure(a.reps)
        med = {k: statistics.median(v) for k, v in t.items()}
        both = t["batch"] + t["batch_b"]
        bmed = statistics.median(both)
        spread = max(abs(med["batch"] - med["batch_b"]), pct(both, 0.9) - pct(both, 0.1)) / bmed
        row = {"shape": name, "segments": nseg, "points": c.total, "bytes_touched": c.bytes,
               "plan": h.msm_g1_segments_plan(c.total, c.m, nseg, kind == "ragged"), "buffer_sets": c.nsets, "repeats": len(t["segments"]),
               "batch_calls_per_run": (nseg + MSM_BATCH_MAX - 1) // MSM_BATCH_MAX if kind == "uniform" else len(c.runs),
               "segments_us": med["segments"], "segments_min_us": min(t["segments"]), "copy_us": med["copy"],
               "batch_us": bmed, "batch_a_us": med["batch"], "batch_b_us": med["batch_b"], "batch_spread": spread,
               "batch_over_segments": bmed / med["segments"], "segments_over_copy": med["segments"] / med["copy"],
               "segments_fraction_of_hbm_peak": c.bytes / (med["segments"] * 1e-6) / HBM_PEAK,
               "segments_beats_batch_by_more_than_its_spread": bool(med["segments"] < bmed * (1 - spread)),
               "segments_slower_than_batch": bool(med["segments"] > bmed), "batch_g1_bytes_equal_segments": agree}
        rows[name] = row
        print("%-36s segments %10.1f us (x%.2f of a copy, %.3f of 8 TB/s)  batch %12.1f us in %d calls (x%.2f, spread %.3f)  equal: %s"
              % (name, med["segments"], row["segments_over_copy"], row["segments_fraction_of_hbm_peak"], bmed,
                 row["batch_calls_per_run"], row["batch_over_segments"], spread, agree), flush=True)
        del c
        torch.cuda.empty_cache()
        res = {k: v for k, v in load(a.out).items() if k == "kernel_resources"}
        res.update({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
                    "timing": "device events around one variant, variants alternating (the batch baseline twice a round), median "
                              "of the repeats after warm-up; spread = max(gap of the baseline's two medians, its p90 - p10) / median",
                    "baselines": {"batch": "plk_msm_g1_batch_dev into 2176-byte records: uniform shapes in chunks of <= 65535 MSMs "
                                           "a call, ragged shapes one call per run of consecutive equal-length segments",
                                  "copy": "torch copy_ of bytes_touched bytes (4 per point, 4 per segment, 4 per offset word): "
                                          "reads that many and writes that many"},
                    "reps": a.reps, "shapes": [rows[s[0]] for s in SHAPES if s[0] in rows]})
        store(a.out, res)


if __name__ == "__main__":
    main()
