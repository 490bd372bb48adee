"""A plain `bench.py` run (no --full) does only what its headline needs -- set up, warm up, time the
steps, print the line -- and --dump-outputs DIR writes what the last timed step returned: the
step's commitments as DIR/msm_g1.npy (float32 rows {x, y, infinite}), from seeded inputs, so the
rows must equal the oracle's fold of the same input sets rebuilt here from their seeds."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_headline_and_dumped_outputs(tmp_path, oracle):
    W, K, B, log2n = 1, 2, 4, 20
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--log2n", str(log2n), "--msm-batch", str(B), "--rotate-mib", "32", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == K and d["warmup"] == W and d["unit"] == "Mpoint/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u8" and d["value"] > 0 and d["ms_per_step"] > 0
    # value and ms_per_step describe the same K timed steps of B MSMs
    assert abs(d["value"] - B * (1 << log2n) / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.002 * d["value"] + 0.1
    assert d["irregular_inputs"] == 0 and d["serial_fold_fallbacks"] == 0
    # what --full adds is absent
    for key in ("components", "cpu_baseline", "checks", "roofline"):
        assert key not in d, key
    assert sorted(os.listdir(out)) == ["msm_g1.npy"]
    got = np.load(out / "msm_g1.npy")
    assert got.dtype == np.float32 and got.shape == (B, 3)
    # the last timed step = MSMs (W + K - 1) B .. (W + K) B - 1, MSM i over input set i mod sets, seed 1234 + set
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    sets = 8                                  # 32 MiB of 4 MiB input sets (= 2 B, the minimum)
    dev = torch.device("cuda:0")
    for j in range(B):
        s = ((W + K - 1) * B + j) % sets
        pts, sc = bench.make_msm_set(torch, 1 << log2n, dev, 1234 + s)
        want = oracle.msm(pts.cpu().numpy().reshape(-1, 3), sc.cpu().numpy())
        assert bytes(got[j].astype(np.uint8)) == want, j
