"""Record tests/golden/msm_segments.json from the REAL reference: the srs_eval_at_s fold (src/srs.h:53-68) of every
segment of two ragged lists, computed with g1_mul / g1_add (src/g1.h, unmodified, taken by -I).

    python tests/golden/make_msm_segments_golden.py [reference src directory]

Runs only where the reference tree is present.  A small C driver is written to a temporary directory, compiled
with gcc against the reference's headers and fed the seeded inputs built here; only its output bytes reach the
JSON, next to the seeds.  The tests rebuild the inputs with list_inputs() (which needs no reference) and read the
JSON alone.

  "random"     SEGMENTS segments of seeded lengths 0..300 over one flat array; points uniform over all 102 group
               elements, scalar bytes over 0..255
  "irregular"  the near-misses of tests/g1_encoding_cases.py whose flag byte is 0 or 1 (the reference's G1 holds a
               bool: no other flag byte can reach it), every STRIDE-th of them, each planted at the first, a middle
               and the last position of a segment of its own among canonical fillers
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen  # noqa: E402

REF_SRC = "/root/reference/src"
OUT = os.path.join(HERE, "msm_segments.json")
SEGMENTS = 320
MAX_LEN = 300
STRIDE = 5
SEEDS = {"random": 0x5E60, "irregular": 0x5E61}

# The driver: one record on stdin, three bytes per segment on stdout.
#   nseg(u32), then per segment: len(u32), len x {x, y, flag}, len scalar bytes
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "hf.h"
#include "g1.h"

static unsigned rd_u32(void) {
  unsigned char b[4];
  if (fread(b, 1, 4, stdin) != 4) exit(2);
  return b[0] | b[1] << 8 | b[2] << 16 | (unsigned)b[3] << 24;
}

int main(void) {
  unsigned nseg = rd_u32();
  for (unsigned g = 0; g < nseg; g++) {
    unsigned len = rd_u32();
    unsigned char *p = malloc(3 * len + 1), *s = malloc(len + 1);
    if (fread(p, 1, 3 * len, stdin) != 3 * len || fread(s, 1, len, stdin) != len) return 2;
    G1 acc = g1_identity();
    for (unsigned i = 0; i < len; i++) {
      G1 pt;
      pt.x.value = p[3 * i]; pt.y.value = p[3 * i + 1]; pt.infinite = p[3 * i + 2] != 0;
      G1 term = g1_mul(&pt, s[i]);
      acc = g1_add(&acc, &term);
    }
    putchar(acc.x.value); putchar(acc.y.value); putchar(acc.infinite ? 1 : 0);
    free(p); free(s);
  }
  return 0;
}
"""


def irregular_candidates():
    import g1_encoding_cases as E
    nm = E.near_misses()
    return nm[nm[:, 2] <= 1][::STRIDE]


def list_inputs(kind):
    """(points (total, 3), scalars (total,), offsets (nseg + 1,) uint32) of one list, a pure function of its name"""
    seed = SEEDS[kind]
    if kind == "random":
        lens = (gen.splitmix64(seed, SEGMENTS) % np.uint64(MAX_LEN + 1)).astype(np.int64)
        lens[:4] = (0, 1, MAX_LEN, 0)
        lens[-1] = 0
        planted = None
    elif kind == "irregular":
        cands = irregular_candidates()
        lens = 3 + (gen.splitmix64(seed, 3 * len(cands)) % np.uint64(60)).astype(np.int64)
        planted = cands
    else:
        raise ValueError(kind)
    off = np.concatenate([[0], np.cumsum(lens)])
    total = int(off[-1])
    r = gen.splitmix64(seed + 0x100, 2 * total)
    pts = gen.all_points()[(r[:total] % np.uint64(102)).astype(np.int64)].copy()
    sc = (r[total:] & np.uint64(0xFF)).astype(np.uint8)
    if planted is not None:
        for i, c in enumerate(planted):
            for j in range(3):
                g = 3 * i + j
                pos = (off[g], off[g] + lens[g] // 2, off[g + 1] - 1)[j]
                pts[pos] = c
                sc[pos] = 1 + sc[pos] % 255
    return np.ascontiguousarray(pts), sc, off.astype(np.uint32)


def run_driver(exe, pts, sc, off):
    msg = [int(off.size - 1).to_bytes(4, "little")]
    for a, b in zip(off[:-1].tolist(), off[1:].tolist()):
        msg += [int(b - a).to_bytes(4, "little"), pts[a:b].tobytes(), sc[a:b].tobytes()]
    out = subprocess.run([exe], input=b"".join(msg), capture_output=True, check=True).stdout
    assert len(out) == 3 * (off.size - 1)
    return out.hex()


def generate(ref_src=REF_SRC):
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "msm_segments_driver.c"), os.path.join(tmp, "msm_segments_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-w", "-I", ref_src, src, "-o", exe], check=True)
        lists = {}
        for kind in sorted(SEEDS):
            pts, sc, off = list_inputs(kind)
            lists[kind] = {"segments": int(off.size - 1), "total": int(off[-1]), "out3": run_driver(exe, pts, sc, off)}
    return {
        "source": "reference src/g1.h (g1_mul, g1_add) folded as src/srs.h:53-68 (srs_eval_at_s), compiled unmodified",
        "inputs": "make_msm_segments_golden.list_inputs(kind): SplitMix64 streams, nothing else stored",
        "lists": lists,
    }


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else REF_SRC
    if not os.path.isdir(ref):
        sys.exit("the reference sources are not at %s" % ref)
    with open(OUT, "w") as f:
        json.dump(generate(ref), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
