#!/usr/bin/env python3
"""KZG aggregate verification (plk_kzg_verify_agg_batch_dev) against what a user had before
it, in one process on the same jobs.

n groups of m regular jobs (points uniform over all 102 elements, z, y, r uniform below 17).
  fused     plk_kzg_verify_agg_batch_dev: one streaming pass over 9 bytes per job, two pairings per group
  per_job   (a) plk_kzg_verify_batch_dev on the same jobs -- two pairings per JOB -- and a device reduction of
            its ok bytes to one byte per group.  It answers a different question (every job, not the weighted
            sum), so only its time is compared.
  compose   (b) the public calls of the commit before: the scalars r, r z mod 102 and sum r y with tensor ops,
            three plk_msm_g1_batch_dev launches (sum r C, sum r z W, sum r W; at most 65535 groups a launch),
            the two logs combined with tensor ops, plk_msm_finalize_dev, plk_pairing_batch_dev on two pairs per
            group.  Its verdicts are compared with the fused call's at every shape.
  copy      a device copy moving the same traffic: 4.5 bytes per job read and 4.5 written
Each time is a pair of device events around one variant on the stream, after warm-up; the variants alternate,
each baseline twice per round (x and x_b), and the median of the repeats is kept.  A baseline's spread is the
larger of the gap between its two interleaved medians and its own 10th-to-90th percentile width, over its
median; the fused call is held to be faster only where it wins by more than that.  The job arrays rotate
through enough distinct buffer sets (twice the 256 MB last-level cache) that a call never finds them cached.

  python tools/kzg_agg_bench.py [--out profiles/kzg_agg_bench.json] [--reps 20]
  python tools/kzg_agg_bench.py --resources     (no GPU: compiles csrc/kzg_agg.hip for gfx950 and records the
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
JOB_BYTES = 9
MSM_BATCH_MAX = 65535
SHAPES = [(1 << 24, 1), (1 << 20, 1), (1 << 12, 1), (2, 1 << 20), (16, 1 << 20)]   # (m, n)


def resources():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} from -Rpass-analysis=kernel-resource-usage"""
    src = os.path.join(ROOT, "plonk.c_amd", "csrc", "kzg_agg.hip")
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


def merge_resources(path):
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data["kernel_resources"] = resources()
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    for k, v in data["kernel_resources"].items():
        print(k, v)


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_agg_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        merge_resources(a.out)
        return

    import torch

    import plonkhip as h

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen

    REC = h.MSM_RESULT_BYTES
    h.init(0)
    with open(os.path.join(ROOT, "tests", "golden", "pairing.json")) as f:
        g2m = json.load(f)["g2_multiples"]
    g1, h1, hs = (1, 2, 0), bytes.fromhex(g2m["1"]), bytes.fromhex(g2m["2"])
    vk = h.KzgVk(g1, h1, hs)
    pts = torch.from_numpy(gen.all_points()).cuda()
    # LOG of the key's g1: one MSM of one point
    rec0 = torch.zeros(REC, dtype=torch.uint8, device="cuda")
    h.msm_g1_dev(torch.tensor(g1, dtype=torch.uint8, device="cuda"), torch.ones(1, dtype=torch.uint8, device="cuda"), 1, rec0)
    torch.cuda.synchronize()
    lg = h.parse_result(rec0.cpu().numpy())["log"]

    def timed(fns, reps, warm=2):
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
        def __init__(self, m, n):
            self.m, self.n, e = m, n, m * n
            self.e = e
            self.nsets = max(2, min(16, -(-2 * LLC_BYTES // (JOB_BYTES * e))))
            g = torch.Generator(device="cuda")
            g.manual_seed(e + m)
            self.sets = []
            for _ in range(self.nsets):
                ic, iw = (torch.randint(0, 102, (e,), device="cuda", generator=g) for _ in range(2))
                z, y, r = (torch.randint(0, 17, (e,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3))
                self.sets.append({"c": pts[ic].reshape(-1).contiguous(), "w": pts[iw].reshape(-1).contiguous(), "z": z, "y": y,
                                  "r": r})
            self.ok = torch.empty(n, dtype=torch.uint8, device="cuda")
            ws = h.kzg_verify_agg_workspace(m, n)
            self.work = torch.empty(ws, dtype=torch.uint8, device="cuda") if ws else None
            self.ok_jobs = torch.empty(e, dtype=torch.uint8, device="cuda")
            self.ok_a = torch.empty(n, dtype=torch.uint8, device="cuda")
            self.res = [torch.zeros(n * REC, dtype=torch.uint8, device="cuda") for _ in range(3)]
            self.g2_1 = torch.tensor(list(h1), dtype=torch.uint8, device="cuda").repeat(n)
            self.g2_s = torch.tensor(list(hs), dtype=torch.uint8, device="cuda").repeat(n)
            self.out4 = [torch.empty(4 * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
            self.gt = [torch.empty(2 * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
            self.ok_b = torch.empty(n, dtype=torch.uint8, device="cuda")
            half = (JOB_BYTES * e // 2 + 15) & ~15
            self.cp = [(torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda"))
                       for _ in range(self.nsets)]

        def fused(self, i):
            d = self.sets[i % self.nsets]
            h.kzg_verify_agg_dev(vk, self.m, d["c"], d["z"], d["y"], d["w"], d["r"], self.n, self.ok, work=self.work)

        def per_job(self, i):
            d = self.sets[i % self.nsets]
            h.kzg_verify_dev(vk, d["c"], d["z"], d["y"], d["w"], self.e, self.ok_jobs)
            torch.amin(self.ok_jobs.view(self.n, self.m), 1, out=self.ok_a)

        def compose(self, i):
            d = self.sets[i % self.nsets]
            m, n = self.m, self.n
            r16 = d["r"].to(torch.int16)
            rz = ((r16 * d["z"]) % 102).to(torch.uint8)
            ry = (r16 * d["y"]).view(n, m).sum(1, dtype=torch.int64) % 102
            for b in range(0, n, MSM_BATCH_MAX):
                k = min(MSM_BATCH_MAX, n - b)
                h.msm_g1_batch_dev(d["c"][3 * m * b:], 3 * m, d["r"][m * b:], m, m, k, self.res[0][REC * b:])
                h.msm_g1_batch_dev(d["w"][3 * m * b:], 3 * m, rz[m * b:], m, m, k, self.res[1][REC * b:])
                h.msm_g1_batch_dev(d["w"][3 * m * b:], 3 * m, d["r"][m * b:], m, m, k, self.res[2][REC * b:])
            logs = [x.view(torch.int32).view(n, REC // 4)[:, h.MSM_LOG_OFFSET // 4].to(torch.int64) for x in self.res]
            s_l = ((logs[0] + logs[1] + 102 - (ry * lg) % 102) % 102).to(torch.int32)
            s_w = logs[2].to(torch.int32).contiguous()
            h.msm_finalize_dev(s_l, n, 1, self.out4[0])
            h.msm_finalize_dev(s_w, n, 1, self.out4[1])
            p_l = self.out4[0].view(n, 4)[:, :3].contiguous()
            p_w = self.out4[1].view(n, 4)[:, :3].contiguous()
            h.pairing_dev(p_l, self.g2_1, n, self.gt[0])
            h.pairing_dev(p_w, self.g2_s, n, self.gt[1])
            self.ok_b.copy_(torch.eq(self.gt[0].view(n, 2), self.gt[1].view(n, 2)).all(1))

        def copy(self, i):
            src, dst = self.cp[i % self.nsets]
            dst.copy_(src)

        def measure(self, reps):
            for x in self.res:
                x.zero_()
            self.fused(0)
            self.compose(0)
            torch.cuda.synchronize()
            irregular = sum(int(x.view(torch.int32).view(self.n, REC // 4)[:, h.MSM_IRREGULAR_OFFSET // 4].sum()) for x in self.res)
            agree = bool(torch.equal(self.ok, self.ok_b)) and irregular == 0
            accepts = int(self.ok.sum())
            assert int(self.ok.max()) <= 1
            t = timed({"fused": self.fused, "per_job": self.per_job, "compose": self.compose, "copy": self.copy,
                       "per_job_b": self.per_job, "compose_b": self.compose}, reps)
            return t, agree, accepts

    rows = []
    for m, n in SHAPES:
        c = Case(m, n)
        t, agree, accepts = c.measure(a.reps)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"m": m, "n": n, "jobs": m * n, "plan": h.kzg_verify_agg_plan(m, n), "buffer_sets": c.nsets, "fused_us": med["fused"],
               "fused_min_us": min(t["fused"]), "copy_us": med["copy"], "accepting_groups": accepts,
               "compose_verdicts_equal_fused": agree,
               "fused_fraction_of_hbm_peak": JOB_BYTES * m * n / (med["fused"] * 1e-6) / HBM_PEAK,
               "fused_over_copy_of_same_traffic": med["fused"] / med["copy"]}
        for name in ("per_job", "compose"):
            both = t[name] + t[name + "_b"]
            bmed = statistics.median(both)
            spread = max(abs(med[name] - med[name + "_b"]), pct(both, 0.9) - pct(both, 0.1)) / bmed
            row.update({name + "_us": bmed, name + "_a_us": med[name], name + "_b_us": med[name + "_b"], name + "_spread": spread,
                        name + "_over_fused": bmed / med["fused"],
                        "fused_beats_%s_by_more_than_its_spread" % name: bool(med["fused"] < bmed * (1 - spread))})
        rows.append(row)
        print("m %9d n %8d  fused %9.1f us (%.3f of 8 TB/s, x%.2f of a copy)  per_job %10.1f us (x%.2f, spread %.3f)  "
              "compose %10.1f us (x%.2f, spread %.3f)  verdicts equal: %s"
              % (m, n, med["fused"], row["fused_fraction_of_hbm_peak"], row["fused_over_copy_of_same_traffic"], row["per_job_us"],
                 row["per_job_over_fused"], row["per_job_spread"], row["compose_us"], row["compose_over_fused"],
                 row["compose_spread"], agree), flush=True)
        del c
        torch.cuda.empty_cache()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = {k: v for k, v in json.load(f).items() if k == "kernel_resources"}
    res.update({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "bytes_per_job": JOB_BYTES,
                "timing": "device events around one variant, variants alternating (each baseline twice a round), median of the "
                          "repeats after warm-up; spread = max(gap of a baseline's two medians, its p90 - p10) / median",
                "baselines": {"per_job": "plk_kzg_verify_batch_dev + torch.amin over each group's ok bytes",
                              "compose": "tensor ops for r z mod 102 and sum r y, 3 x plk_msm_g1_batch_dev (<= 65535 groups a "
                                         "launch), plk_msm_finalize_dev, 2 x plk_pairing_batch_dev, tensor compare",
                              "copy": "torch copy_ of 4.5 bytes per job (read 4.5 + write 4.5)"},
                "reps": a.reps, "shapes": rows})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
