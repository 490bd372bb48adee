"""Record tests/golden/pairing.json from the REAL reference: pairing() and the KZG opening check
built from it (src/pairing.h, src/g1.h, src/g2.h, src/gt.h, unmodified, taken by -I).

    python tests/golden/make_pairing_golden.py [reference src directory]

Runs only where the reference tree is present.  A small C driver is written to a temporary
directory, compiled with gcc against the reference's headers and fed the seeded inputs built here;
only its outputs reach the JSON.  The tests read the JSON alone.  Everything but `reference_ns`
(single-core timings of the generating machine) is a pure function of the seeds below.
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

REF_SRC = "/root/reference/src"
OUT = os.path.join(HERE, "pairing.json")
RAW_SEED, VERIFY_SEED = 0x5041, 0x4B5A
N_RAW, N_VERIFY = 1024, 2048

# The driver: a stream of records on stdin, the answers on stdout.
#   'G'                      -> 32 bytes, k * g2_generator() for k = 1 .. 16
#   'P' n(u32) n x {g1 3, g2 2}                        -> n x 2 bytes, pairing()
#   'V' n(u32) n x {vk.g1 3, g2_1 2, g2_s 2, C 3, W 3, z, y}  -> n bytes, the accept bit
#   'T' n(u32)               -> two doubles: ns per pairing, ns per verification (n of each)
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include "hf.h"
#include "pairing.h"

static G1 rd_g1(const unsigned char *b) { G1 p; p.x.value = b[0]; p.y.value = b[1]; p.infinite = b[2] != 0; return p; }
static G2 rd_g2(const unsigned char *b) { G2 q; q.x.value = b[0]; q.y.value = b[1]; return q; }

static int verify(const unsigned char *j) {
  G1 G = rd_g1(j), C = rd_g1(j + 7), W = rd_g1(j + 10);
  G2 h1 = rd_g2(j + 3), hs = rd_g2(j + 5);
  G1 yG = g1_mul(&G, j[14]);
  G1 nyG = g1_neg(&yG);
  G1 zW = g1_mul(&W, j[13]);
  G1 L = g1_add(&C, &nyG);
  L = g1_add(&L, &zW);
  GTP a = pairing(&L, &h1), b = pairing(&W, &hs);
  return gtp_equal(&a, &b);
}

static double now_ns(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return 1e9 * (double)t.tv_sec + (double)t.tv_nsec;
}

static unsigned rd_u32(void) {
  unsigned char b[4];
  if (fread(b, 1, 4, stdin) != 4) exit(2);
  return b[0] | b[1] << 8 | b[2] << 16 | (unsigned)b[3] << 24;
}

int main(void) {
  int c;
  while ((c = getchar()) != EOF) {
    if (c == 'G') {
      for (unsigned k = 1; k <= 16; k++) {
        G2 q = g2_mul(g2_generator(), k);
        putchar(q.x.value);
        putchar(q.y.value);
      }
    } else if (c == 'P') {
      unsigned n = rd_u32();
      for (unsigned i = 0; i < n; i++) {
        unsigned char j[5];
        if (fread(j, 1, 5, stdin) != 5) return 2;
        G1 p = rd_g1(j);
        G2 q = rd_g2(j + 3);
        GTP e = pairing(&p, &q);
        putchar(e.a.value);
        putchar(e.b.value);
      }
    } else if (c == 'V') {
      unsigned n = rd_u32();
      for (unsigned i = 0; i < n; i++) {
        unsigned char j[15];
        if (fread(j, 1, 15, stdin) != 15) return 2;
        putchar(verify(j));
      }
    } else if (c == 'T') {
      unsigned n = rd_u32(), acc = 0;
      unsigned char j[15] = {1, 2, 0, 36, 31, 90, 82, 26, 45, 0, 68, 74, 0, 5, 3};
      double t0 = now_ns();
      for (unsigned i = 0; i < n; i++) {
        G1 p = rd_g1(j);
        G2 q = rd_g2(j + 3);
        p.x.value = (unsigned char)((i + acc) % 101);
        GTP e = pairing(&p, &q);
        acc += e.a.value;
      }
      double t1 = now_ns();
      for (unsigned i = 0; i < n; i++) {
        j[13] = (unsigned char)((i + acc) % 17);
        acc += (unsigned)verify(j);
      }
      double t2 = now_ns();
      double out[2] = {(t1 - t0) / n, (t2 - t1) / n};
      fwrite(out, sizeof(double), 2, stdout);
      if (acc == 0xFFFFFFFFu) putchar(0);
    } else {
      return 3;
    }
  }
  return 0;
}
"""


def hx(a):
    return np.asarray(a, dtype=np.uint8).reshape(-1).tobytes().hex()


class Driver:
    def __init__(self, ref_src, tmp):
        src = os.path.join(tmp, "pairing_driver.c")
        self.exe = os.path.join(tmp, "pairing_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-w", "-I", ref_src, src, "-o", self.exe], check=True)

    def run(self, tag, payload=b"", n=None):
        msg = tag + (b"" if n is None else int(n).to_bytes(4, "little")) + payload
        return subprocess.run([self.exe], input=msg, capture_output=True, check=True).stdout


def random_g1(r):
    """valid encodings from three random words per point: coordinates < 101 (mostly off the curve), the
    flag set on a quarter of them"""
    return np.stack([(r[0::3] % np.uint64(101)), (r[1::3] >> np.uint64(8)) % np.uint64(101),
                     ((r[2::3] >> np.uint64(16)) % np.uint64(4) == 0)], 1).astype(np.uint8)


def random_g2(r):
    return np.stack([r[0::2] % np.uint64(101), (r[1::2] >> np.uint64(8)) % np.uint64(101)], 1).astype(np.uint8)


def raw_inputs():
    r = gen.splitmix64(RAW_SEED, 5 * N_RAW)
    return np.concatenate([random_g1(r[:3 * N_RAW]), random_g2(r[3 * N_RAW:])], 1)


def verify_raw_inputs():
    """N_VERIFY x 15 bytes {vk.g1 3, g2_1 2, g2_s 2, C 3, W 3, z, y}"""
    n = N_VERIFY
    r = gen.splitmix64(VERIFY_SEED, 13 * n)
    base = gen.all_points()[(r[:n] % np.uint64(102)).astype(np.int64)]
    h = random_g2(r[n:5 * n]).reshape(n, 4)
    cw = random_g1(r[5 * n:11 * n]).reshape(n, 6)
    zy = np.stack([r[11 * n:12 * n] % np.uint64(17), r[12 * n:] % np.uint64(17)], 1).astype(np.uint8)
    return np.concatenate([base, h, cw, zy], 1)


def exhaustive_inputs(g2m):
    """every (c, w, z, y) in [0, 17)^4, y fastest, for vk = {(1, 2), H, 2 H}, C = c G, W = w G"""
    kg = np.array(gen.KG, dtype=np.uint8)
    c, w, z, y = (v.reshape(-1) for v in np.meshgrid(*[np.arange(17)] * 4, indexing="ij"))
    n = c.size
    vk = np.tile(np.array([1, 2, 0, *g2m[0], *g2m[1]], dtype=np.uint8), (n, 1))
    return np.concatenate([vk, kg[c], kg[w], z[:, None].astype(np.uint8), y[:, None].astype(np.uint8)], 1)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def generate(ref_src=REF_SRC, timing=True):
    with tempfile.TemporaryDirectory() as tmp:
        d = Driver(ref_src, tmp)
        g2m = np.frombuffer(d.run(b"G"), np.uint8).reshape(16, 2)
        pts = gen.all_points()
        tab = np.concatenate([np.repeat(pts, 16, 0), np.tile(g2m, (len(pts), 1))], 1)   # point major, k = 1 .. 16
        table = d.run(b"P", tab.tobytes(), len(tab))
        raw = raw_inputs()
        raw_out = d.run(b"P", raw.tobytes(), len(raw))
        ex = exhaustive_inputs(g2m)
        ex_bits = np.frombuffer(d.run(b"V", ex.tobytes(), len(ex)), np.uint8)
        vr = verify_raw_inputs()
        vr_bits = np.frombuffer(d.run(b"V", vr.tobytes(), len(vr)), np.uint8)
        ns = {"cpu": cpu_model(), "pairing": None, "verify": None, "note": "one core, gcc -O2, the generating machine"}
        if timing:
            t = np.frombuffer(d.run(b"T", n=20000), np.float64)
            ns["pairing"], ns["verify"] = round(float(t[0]), 1), round(float(t[1]), 1)
    assert len(table) == 2 * len(tab) and len(raw_out) == 2 * N_RAW
    assert ex_bits.max() <= 1 and vr_bits.max() <= 1
    return {
        "source": "reference src/pairing.h:66-83 (pairing, gtp_equal), src/g1.h, src/g2.h, src/gt.h, compiled unmodified",
        "g2_multiples": {str(k + 1): hx(q) for k, q in enumerate(g2m)},   # keyed by k
        "table": table.hex(),
        "raw": {"seed": RAW_SEED, "inputs": hx(raw), "out": raw_out.hex()},
        "verify_exhaustive": {"vk": hx(ex[0, :7]), "order": "bit ((c*17 + w)*17 + z)*17 + y, LSB first",
                              "bits": np.packbits(ex_bits, bitorder="little").tobytes().hex()},
        "verify_raw": {"seed": VERIFY_SEED, "jobs": hx(vr), "bits": "".join(str(int(b)) for b in vr_bits)},
        "reference_ns": ns,
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
