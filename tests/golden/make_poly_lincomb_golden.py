"""Record tests/golden/poly_lincomb.json from the REAL reference: compositions of poly_scale, poly_negate,
poly_shift, poly_add, poly_sub, poly_add_hf and the hf_mul(., hf_pow(omega, i)) coefficient loop of
src/plonk.h:466-470, from src/poly.h and src/hf.h, unmodified, taken by -I.

    python tests/golden/make_poly_lincomb_golden.py <reference src directory>

Runs only where the reference tree is present.  A small C driver is written to a temporary directory,
compiled with gcc against the reference's headers and fed the seeded jobs built here; only its outputs
(the result bytes, whose count is the reference's trimmed length) reach the JSON.  The inputs are not
stored: they are a pure function of the seed below (random_jobs), which the tests call to rebuild them
-- that needs numpy alone, not the reference.
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

OUT = os.path.join(HERE, "poly_lincomb.json")
SEED, N_JOBS = 0x4C434F4D, 512
MAX_LEN, MAX_SHIFT, MAX_TERMS = 40, 24, 16
RAW = 0xFF

# The driver: jobs on stdin, answers on stdout.
#   job     nterms(u8) add_hf(u8, 255: none) nterms x {len, shift, sub, scale, neg, twist, len coefficient bytes}
#   answer  len(u8) of the reference's (trimmed) result, its bytes
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "hf.h"
#include "poly.h"

static HF hf(unsigned v) { HF r; r.value = (unsigned char)v; return r; }
static unsigned rd_u8(void) {
  int c = getchar();
  if (c == EOF) exit(2);
  return (unsigned)c;
}

int main(void) {
  int c;
  while ((c = getchar()) != EOF) {
    unsigned nterms = (unsigned)c, add_hf = rd_u8();
    POLY acc = poly_zero();
    for (unsigned t = 0; t < nterms; t++) {
      unsigned len = rd_u8(), shift = rd_u8(), sub = rd_u8(), scale = rd_u8(), neg = rd_u8(), twist = rd_u8();
      HF cf[256];
      for (unsigned i = 0; i < len; i++) cf[i] = hf(rd_u8());
      POLY p = poly_new(cf, len);
      if (twist) {
        for (size_t i = 0; i < p.len; i++) cf[i] = hf_mul(p.coeffs[i], hf_pow(hf(twist), i));
        p = poly_new(cf, p.len);
      }
      if (scale != 255) p = poly_scale(&p, hf(scale));
      if (neg) p = poly_negate(&p);
      if (shift) p = poly_shift(&p, shift);
      if (t == 0) acc = p;
      else acc = sub ? poly_sub(&acc, &p) : poly_add(&acc, &p);
    }
    if (add_hf != 255) acc = poly_add_hf(&acc, hf(add_hf));
    putchar((int)acc.len);
    for (size_t j = 0; j < acc.len; j++) putchar(acc.coeffs[j].value);
  }
  return 0;
}
"""


def random_jobs(seed=SEED, n=N_JOBS):
    """n jobs (terms, add_hf); a term is a dict p (list of bytes), shift, sub, scale, neg, twist; add_hf is
    None or 0 .. 16.  Job g by its number:
      g % 3 == 2    arbitrary bytes 0 .. 255 in every raw term (scale RAW and twist 0; one term at least is
                    made raw), else canonical bytes
      g % 16        fixes the term count: 1 + g % 16, so every count 1 .. 16 and single-term jobs occur
      g % 8 == 5    one term has scale 0
      g % 16 == 11  the terms cancel in pairs: term 2i+1 subtracts a copy of term 2i
    lengths 1 .. 40 (top coefficients may be zero), shifts 0 .. 24 on about half of the terms."""
    per = 2 + MAX_TERMS * (8 + MAX_LEN)
    r = gen.splitmix64(seed, n * per).reshape(n, per)
    jobs = []
    for g in range(n):
        x = [int(v >> np.uint64(8)) for v in r[g]]
        k = 1 + g % 16
        wild = g % 3 == 2
        terms = []
        for i in range(k):
            o = 2 + i * (8 + MAX_LEN)
            ln = 1 + x[o] % MAX_LEN
            shift = x[o + 1] % (MAX_SHIFT + 1) if x[o + 1] & 0x100 else 0
            scale = RAW if x[o + 2] % 3 == 0 else x[o + 2] // 3 % 17
            twist = x[o + 3] // 4 % 17 if x[o + 3] % 4 == 0 else 0
            if wild and i == x[0] // 7 % k:
                scale, twist = RAW, 0
            sub = (x[o + 4] & 1) if i else 0
            neg = 1 if x[o + 5] % 4 == 0 else 0
            raw = scale == RAW and twist == 0
            p = [(v % 256 if wild and (raw or x[o + 6] & 1) else v % 17) for v in x[o + 8:o + 8 + ln]]
            if x[o + 7] % 4 == 0:
                p[-1] = 0
            terms.append({"p": p, "shift": shift, "sub": sub, "scale": scale, "neg": neg, "twist": twist})
        if g % 8 == 5:
            terms[x[0] % k]["scale"] = 0
        if g % 16 == 11:
            for i in range(1, k, 2):
                terms[i] = dict(terms[i - 1], sub=1 - terms[i - 1]["sub"])
            if k % 2:
                terms[-1]["scale"] = 0
            terms[0]["sub"] = 0
            if k > 1:
                terms[1]["sub"] = 1
        add_hf = x[1] // 2 % 17 if x[1] % 2 else None
        jobs.append((terms, add_hf))
    return jobs


def job_record(terms, add_hf):
    out = bytes([len(terms), 255 if add_hf is None else add_hf])
    for t in terms:
        out += bytes([len(t["p"]), t["shift"], t["sub"], t["scale"], t["neg"], t["twist"]]) + bytes(t["p"])
    return out


def generate(ref_src):
    jobs = random_jobs()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "poly_lincomb_driver.c"), os.path.join(tmp, "poly_lincomb_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-w", "-I", ref_src, src, "-o", exe], check=True)
        out = subprocess.run([exe], input=b"".join(job_record(*j) for j in jobs), capture_output=True, check=True).stdout
    res, o = [], 0
    for _ in jobs:
        ln = out[o]
        res.append(out[o + 1:o + 1 + ln].hex())
        o += 1 + ln
    assert o == len(out)
    return {
        "source": "reference src/poly.h (poly_scale, poly_negate, poly_shift, poly_add, poly_sub, poly_add_hf), "
                  "src/hf.h (hf_mul, hf_pow), compiled unmodified",
        "inputs": "not stored: random_jobs(seed, n) of this script",
        "seed": SEED, "n": N_JOBS,
        "out": ",".join(res),
    }


def expand(gold):
    """the committed record joined with the jobs it was taken on -> [(terms, add_hf, the reference's trimmed bytes)]"""
    outs = [bytes.fromhex(t) for t in gold["out"].split(",")]
    jobs = random_jobs(gold["seed"], gold["n"])
    assert len(outs) == len(jobs)
    return [(t, a, o) for (t, a), o in zip(jobs, outs)]


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_poly_lincomb_golden.py <reference src directory>")
    with open(OUT, "w") as f:
        json.dump(generate(sys.argv[1]), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
