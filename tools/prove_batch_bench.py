#!/usr/bin/env python3
"""Throughput of the batched small-circuit prover, in one process:

  fused n = 4:   plk_prover_prove_batch_dev on the reference's toy circuit (tests/golden/prove.json,
                 src/plonk-test.c) over a 9-point SRS, with random challenges and blinding per entry --
                 the draws the prover accepts (six in ten: the rest take the reference's remainder and
                 slice exits early), repeated up to the batch, so that every entry is a whole proof
  fused n = 16:  plk_prover_rounds_batch_dev on random polynomials
  loop:          256 plk_prover_prove calls on the same toy circuit, one after the other -- the per-proof
                 path this tool's subject leaves untouched (host wall time: the call is synchronous)

at batches 1, 64, 4096, 65536 and 2^20.  A fused time is a pair of device events around one _dev call
on a stream, after warm-up; the variants alternate and the median of the repeats is kept.  The first
entries of the n = 4 batch are compared with the single call.  The host reference's 17.72 us per proof
is quoted from profiles/r06_bench.json; where oracle/_ref is built, prove4_inproc is timed again on this
host.

  python tools/prove_batch_bench.py [--out profiles/prove_batch_bench.json] [--reps 9]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("plonk.c_amd", "oracle", os.path.join("tests", "golden")):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen  # noqa: E402
import plonkhip as h  # noqa: E402

BATCHES = (1, 64, 4096, 65536, 1 << 20)
LOOP = 256


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()


class Fused:
    """one (prover, batch): device inputs and outputs, and the _dev call on a stream"""

    def __init__(self, pr, circuit, each, batch, seed):
        rng = np.random.default_rng(seed)
        self.pr, self.circuit, self.batch = pr, circuit, batch
        # a pool of random draws, of which the accepted ones are kept and repeated up to the batch: every
        # entry then does a whole proof's work (a rejected draw leaves the kernel at its exit)
        pool = 4096
        draws = (each(rng, pool) if callable(each) else np.tile(each, (pool, 1)),
                 rng.integers(0, 17, (pool, 5), dtype=np.uint8), rng.integers(0, 17, (pool, 9), dtype=np.uint8))
        _, status = (pr.prove_batch if circuit else pr.rounds_batch)(*draws)
        ok = np.flatnonzero(status == 0)
        assert ok.size >= pool // 16, "too few accepted draws: %d of %d" % (ok.size, pool)
        self.accepted_fraction = ok.size / pool
        pick = ok[np.arange(batch) % ok.size]
        self.host = tuple(x[pick] for x in draws)
        self.d = [dev(x) for x in self.host]
        self.proofs = torch.zeros(34 * batch, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(batch, dtype=torch.int32, device="cuda")
        self.st = torch.cuda.Stream()

    def run(self):
        f = self.pr.prove_batch_dev if self.circuit else self.pr.rounds_batch_dev
        f(self.d[0], self.d[1], self.d[2], self.batch, self.proofs, self.status, stream=self.st)

    def timed(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.st)
        self.run()
        e1.record(self.st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_batch_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    h.init(0)
    with open(os.path.join(ROOT, "tests", "golden", "prove.json")) as f:
        g = json.load(f)
    toy = g["proofs"][0]
    with open(os.path.join(ROOT, "tests", "golden", "prove_edges.json")) as f:
        s = {k: bytes.fromhex(v) for k, v in json.load(f)["setups"]["8/0"].items()}   # 9 points: 2n + 1, every commitment fits
    pr4 = h.Prover(4, s["z_h"], s["g1s"], s["h"], s["k1_h"], s["k2_h"], s["h_pows_inv"])
    assert pr4.batch_path() == 1
    cir = np.array(toy["gates"] + toy["copies"] + toy["wires"], np.uint8)
    n16 = 16
    _, _, _, zh, pts = gen.prove_instance(n16, 1, 2 * n16 + 8)
    pr16 = h.Prover(n16, zh, pts)
    assert pr16.batch_path(circuit=False) == 1
    cases = {("n4", b): Fused(pr4, True, cir, b, b) for b in BATCHES}
    cases.update({("n16", b): Fused(pr16, False, lambda rng, b_: rng.integers(0, 17, (b_, 13 * n16), dtype=np.uint8), b, b + 1)
                  for b in BATCHES})
    # the per-proof loop: ctypes blocks built once, 256 synchronous calls
    arrs = [np.array(x, np.uint8) for x in (toy["gates"][0:4], toy["gates"][4:8], toy["gates"][8:12], toy["gates"][12:16],
                                            toy["gates"][16:20], toy["copies"][0:8], toy["copies"][8:16],
                                            toy["copies"][16:24], toy["wires"][0:4], toy["wires"][4:8], toy["wires"][8:12])]
    cstruct = h.Circuit(*(x.ctypes.data_as(C.POINTER(C.c_uint8)) for x in arrs))
    lch = cases["n4", 4096].host[1][:LOOP].copy()
    lrd = cases["n4", 4096].host[2][:LOOP].copy()
    lout = np.zeros((LOOP, 34), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    largs = [(lch[i].ctypes.data_as(u8p), lrd[i].ctypes.data_as(u8p), lout[i].ctypes.data_as(u8p)) for i in range(LOOP)]
    prove = h.lib().plk_prover_prove

    def loop():
        t0 = time.perf_counter()
        for ch, rd, out in largs:
            prove(pr4._h, C.byref(cstruct), ch, rd, out)   # (a rejected draw returns its code: the same work)
        return (time.perf_counter() - t0) * 1e6

    for _ in range(3):
        for c in cases.values():
            c.run()
    torch.cuda.synchronize()
    loop()
    # the fused answers of the first LOOP entries are the loop's
    c = cases["n4", 4096]
    c.run()
    torch.cuda.synchronize()
    fp = c.proofs.cpu().numpy().reshape(-1, 34)[:LOOP]
    fs = c.status.cpu().numpy()[:LOOP]
    differ = [i for i in range(LOOP) if not (fp[i] == lout[i]).all()]
    assert not differ and not fs.any() and lout.any(axis=1).all(), ("fused and single call disagree", differ[:8])
    times = {k: [] for k in cases}
    loops = []
    for _ in range(a.reps):
        for k, c in cases.items():   # alternate
            times[k].append(c.timed())
        loops.append(loop())
    rows = []
    for (kind, b), v in times.items():
        med = statistics.median(v)
        rows.append({"kernel": kind, "batch": b, "us": med, "min_us": min(v), "us_per_proof": med / b,
                     "proofs_per_s": b / (med * 1e-6), "accepted_fraction_of_random_draws": cases[kind, b].accepted_fraction})
        print("%-4s batch %8d: %11.1f us  %9.4f us/proof  %12.0f proofs/s" % (kind, b, med, med / b, b / (med * 1e-6)),
              flush=True)
    loop_us = statistics.median(loops) / LOOP
    print("loop of %d plk_prover_prove: %.1f us/proof" % (LOOP, loop_us))
    fused4096 = next(r for r in rows if r["kernel"] == "n4" and r["batch"] == 4096)["us_per_proof"]
    host = {"reference_cpu_us_quoted": 17.72, "quoted_from": "profiles/r06_bench.json cpu_reference_other"}
    from pyoracle import Reference
    if Reference.available():
        R = Reference()
        args = (toy["gates"], toy["copies"], toy["wires"], toy["chal"], toy["rand"], toy["secret"], toy["srs_n"],
                toy["srs_mode"])
        R.prove4_inproc(*args)
        t0 = time.perf_counter()
        for _ in range(20000):
            R.prove4_inproc(*args)
        host["reference_cpu_us_this_host"] = round((time.perf_counter() - t0) / 20000 * 1e6, 2)
    res = {"device": torch.cuda.get_device_name(0),
           "timing": "device events around one _dev call, variants alternating, median of %d; loop: host wall time" % a.reps,
           "rows": rows, "single_call_loop": {"calls": LOOP, "us_per_proof": loop_us, "min_us_per_proof": min(loops) / LOOP},
           "fused_n4_batch4096_below_loop": fused4096 < loop_us, "host_reference": host}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    assert fused4096 < loop_us, "the fused kernel at batch 4096 (%.3f us/proof) is not below the single-call loop (%.1f)" % (
        fused4096, loop_us)


if __name__ == "__main__":
    main()
