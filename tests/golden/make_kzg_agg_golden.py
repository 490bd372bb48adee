"""Record tests/golden/kzg_agg.json from the REAL reference: the aggregate check of a group of KZG openings
(include/plonkhip.h, "KZG aggregate verification") folded with g1_mul / g1_add / g1_neg and decided with
pairing() and gtp_equal (src/pairing.h, src/g1.h, src/g2.h, src/gt.h, unmodified, taken by -I).

    python tests/golden/make_kzg_agg_golden.py [reference src directory]

Runs only where the reference tree is present.  A small C driver is written to a temporary directory,
compiled with gcc against the reference's headers and fed the seeded inputs built here; only its verdict
bits reach the JSON, next to the seeds.  The tests rebuild the inputs with case_inputs() (which needs no
reference: the G2 multiples come from pairing.json) and read the JSON alone.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen  # noqa: E402
from make_pairing_golden import random_g1, random_g2  # noqa: E402

REF_SRC = "/root/reference/src"
OUT = os.path.join(HERE, "kzg_agg.json")
GROUPS = 128                                   # per case
# regular: C and W uniform over all 102 group elements, the key's g1 one of them, its G2s multiples of the
# generator; raw: valid encodings, mostly off the curve, a quarter flagged (random_g1), a random key
CASES = [("regular", m, 0xA660 + m) for m in (1, 2, 3, 16, 17, 65)] + [("raw", m, 0xA6A0 + m) for m in (1, 2, 5, 33)]

# The driver: one record on stdin, the verdicts on stdout.
#   n(u32) m(u32) vk{g1 3, g2_1 2, g2_s 2} n m x {C 3, W 3, z, y, r}  -> n bytes, gtp_equal of the two pairings
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "hf.h"
#include "pairing.h"

static G1 rd_g1(const unsigned char *b) { G1 p; p.x.value = b[0]; p.y.value = b[1]; p.infinite = b[2] != 0; return p; }
static G2 rd_g2(const unsigned char *b) { G2 q; q.x.value = b[0]; q.y.value = b[1]; return q; }

static unsigned rd_u32(void) {
  unsigned char b[4];
  if (fread(b, 1, 4, stdin) != 4) exit(2);
  return b[0] | b[1] << 8 | b[2] << 16 | (unsigned)b[3] << 24;
}

int main(void) {
  unsigned n = rd_u32(), m = rd_u32();
  unsigned char vk[7];
  if (fread(vk, 1, 7, stdin) != 7) return 2;
  G1 G = rd_g1(vk);
  G2 h1 = rd_g2(vk + 3), hs = rd_g2(vk + 5);
  for (unsigned g = 0; g < n; g++) {
    G1 accL = g1_identity(), accW = g1_identity();
    for (unsigned i = 0; i < m; i++) {
      unsigned char j[9];
      if (fread(j, 1, 9, stdin) != 9) return 2;
      G1 C = rd_g1(j), W = rd_g1(j + 3);
      G1 yG = g1_mul(&G, j[7]);
      G1 nyG = g1_neg(&yG);
      G1 zW = g1_mul(&W, j[6]);
      G1 L = g1_add(&C, &nyG);
      L = g1_add(&L, &zW);
      G1 t = g1_mul(&L, j[8]);
      accL = g1_add(&accL, &t);
      G1 u = g1_mul(&W, j[8]);
      accW = g1_add(&accW, &u);
    }
    GTP a = pairing(&accL, &h1), b = pairing(&accW, &hs);
    putchar(gtp_equal(&a, &b));
  }
  return 0;
}
"""


def g2_multiples():
    with open(os.path.join(HERE, "pairing.json")) as f:
        g = json.load(f)["g2_multiples"]
    return np.array([list(bytes.fromhex(g[str(k)])) for k in range(1, 17)], np.uint8)


def case_inputs(kind, m, seed, n=GROUPS):
    """the seeded inputs of one case: vk (7 bytes) and the flat arrays c, w (n m x 3), z, y, r (n m)"""
    e = m * n
    r = gen.splitmix64(seed, 9 * e + 7)
    k = r[9 * e:]
    if kind == "regular":
        pts = gen.all_points()
        c, w = pts[(r[:e] % np.uint64(102)).astype(np.int64)], pts[(r[e:2 * e] % np.uint64(102)).astype(np.int64)]
        h = g2_multiples()
        vk = np.concatenate([pts[int(k[0] % np.uint64(102))], h[int(k[1] % np.uint64(16))], h[int(k[2] % np.uint64(16))]])
    elif kind == "raw":
        cw = random_g1(r[:6 * e]).reshape(e, 6)
        c, w = cw[:, :3], cw[:, 3:]
        vk = np.concatenate([random_g1(k[:3])[0], random_g2(k[3:7]).reshape(-1)])
    else:
        raise ValueError(kind)
    z, y, rr = ((r[(6 + i) * e:(7 + i) * e] % np.uint64(17)).astype(np.uint8) for i in range(3))
    return {"vk": np.ascontiguousarray(vk, np.uint8), "c": np.ascontiguousarray(c), "w": np.ascontiguousarray(w), "z": z,
            "y": y, "r": rr}


def key_of(vk):
    vk = [int(v) for v in vk]
    return (tuple(vk[0:3]), tuple(vk[3:5]), tuple(vk[5:7]))


class Driver:
    def __init__(self, ref_src, tmp):
        src = os.path.join(tmp, "kzg_agg_driver.c")
        self.exe = os.path.join(tmp, "kzg_agg_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-w", "-I", ref_src, src, "-o", self.exe], check=True)

    def run(self, m, d):
        n = d["z"].size // m
        jobs = np.concatenate([d["c"], d["w"], d["z"][:, None], d["y"][:, None], d["r"][:, None]], 1).astype(np.uint8)
        msg = int(n).to_bytes(4, "little") + int(m).to_bytes(4, "little") + d["vk"].tobytes() + jobs.tobytes()
        out = subprocess.run([self.exe], input=msg, capture_output=True, check=True).stdout
        assert len(out) == n and max(out) <= 1
        return "".join(str(b) for b in out)


def generate(ref_src=REF_SRC):
    with tempfile.TemporaryDirectory() as tmp:
        d = Driver(ref_src, tmp)
        cases = []
        for kind, m, seed in CASES:
            inp = case_inputs(kind, m, seed)
            cases.append({"kind": kind, "m": m, "seed": seed, "groups": GROUPS, "vk": inp["vk"].tobytes().hex(),
                          "bits": d.run(m, inp)})
    return {
        "source": "reference src/g1.h (g1_mul, g1_add, g1_neg), src/pairing.h:66-83 (pairing, gtp_equal), compiled unmodified",
        "inputs": "make_kzg_agg_golden.case_inputs(kind, m, seed): SplitMix64 streams, nothing else stored",
        "cases": cases,
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
