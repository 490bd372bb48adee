"""Record tests/golden/kzg_fold.json from the REAL reference: folded KZG openings (poly_scale /
poly_add, poly_eval, poly_divide, srs_eval_at_s) and their verification (g1_mul / g1_add, pairing),
from src/poly.h, src/srs.h, src/pairing.h and what they include, unmodified, taken by -I.

    python tests/golden/make_kzg_fold_golden.py [reference src directory]

Runs only where the reference tree is present.  A small C driver is written to a temporary
directory, compiled with gcc against the reference's headers and fed the seeded inputs built here;
only its outputs reach the JSON.  The inputs are not stored: they are pure functions of the seeds
below (random_groups, verify_jobs, e2e_variants), which the tests call to rebuild them -- that needs
numpy alone, not the reference.
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
OUT = os.path.join(HERE, "kzg_fold.json")
OPEN_SEED, VERIFY_SEED, E2E_SEED = 0x464F4C44, 0x564F4C44, 0x45324532
N_OPEN, N_VERIFY, N_E2E = 256, 2048, 40
MAX_LEN, SRS_LEN = 40, 48
VERIFY_KS = (1, 2, 3, 9, 16)
G2_1, G2_2 = (36, 31), (90, 82)          # g2_generator() and twice it (tests/golden/pairing.json pins both)
STD_KEY = (1, 2, 0) + G2_1 + G2_2        # s = 2

# The driver: a stream of records on stdin, the answers on stdout.
#   'S' n(u32) n x 3 bytes                 the SRS of the records that follow; no output
#   'C' n(u32) n x {len(u8), coeffs}       -> n x 3 bytes, srs_eval_at_s
#   'O' n(u32) n x {k, z, k x {w, len, coeffs}} -> per group: k ys, len(F), F, the proof's 3 bytes
#   'W' n(u32) k(u8) n x {vk 7, k x {C 3, w, y}, W 3, z} -> n bytes, the accept bit
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "hf.h"
#include "poly.h"
#include "srs.h"
#include "pairing.h"

static SRS srs;

static G1 rd_g1(const unsigned char *b) { G1 p; p.x.value = b[0]; p.y.value = b[1]; p.infinite = b[2] != 0; return p; }
static G2 rd_g2(const unsigned char *b) { G2 q; q.x.value = b[0]; q.y.value = b[1]; return q; }
static HF hf(unsigned v) { HF r; r.value = (unsigned char)v; return r; }
static void put_g1(G1 p) { putchar(p.x.value); putchar(p.y.value); putchar(p.infinite ? 1 : 0); }

static unsigned rd_u8(void) {
  int c = getchar();
  if (c == EOF) exit(2);
  return (unsigned)c;
}
static unsigned rd_u32(void) {
  unsigned char b[4];
  if (fread(b, 1, 4, stdin) != 4) exit(2);
  return b[0] | b[1] << 8 | b[2] << 16 | (unsigned)b[3] << 24;
}
static POLY rd_poly(void) {
  unsigned len = rd_u8();
  HF c[256];
  for (unsigned i = 0; i < len; i++) c[i] = hf(rd_u8());
  return poly_new(c, len);
}

int main(void) {
  int c;
  while ((c = getchar()) != EOF) {
    if (c == 'S') {
      srs.len = rd_u32();
      srs.g1s = (G1 *)malloc(srs.len * sizeof(G1));
      for (size_t i = 0; i < srs.len; i++) {
        unsigned char b[3];
        if (fread(b, 1, 3, stdin) != 3) return 2;
        srs.g1s[i] = rd_g1(b);
      }
    } else if (c == 'C') {
      unsigned n = rd_u32();
      for (unsigned i = 0; i < n; i++) {
        POLY p = rd_poly();
        put_g1(srs_eval_at_s(&srs, &p));
      }
    } else if (c == 'O') {
      unsigned n = rd_u32();
      for (unsigned g = 0; g < n; g++) {
        unsigned k = rd_u8();
        HF z = hf(rd_u8());
        POLY F = poly_zero();
        for (unsigned i = 0; i < k; i++) {
          HF w = hf(rd_u8());
          POLY p = rd_poly();
          putchar(poly_eval(&p, z).value);
          POLY sp = poly_scale(&p, w);
          F = poly_add(&F, &sp);
        }
        putchar((int)F.len);
        for (size_t j = 0; j < F.len; j++) putchar(F.coeffs[j].value);
        HF dc[2] = {hf_neg(z), hf_one()};
        POLY den = poly_new(dc, 2), q, rem;
        poly_divide(&F, &den, &q, &rem);
        put_g1(srs_eval_at_s(&srs, &q));
      }
    } else if (c == 'W') {
      unsigned n = rd_u32(), k = rd_u8();
      for (unsigned b = 0; b < n; b++) {
        unsigned char key[7], e[5], t[4];
        if (fread(key, 1, 7, stdin) != 7) return 2;
        G1 acc = g1_identity();
        HF y = hf_zero();
        for (unsigned i = 0; i < k; i++) {
          if (fread(e, 1, 5, stdin) != 5) return 2;
          G1 ci = rd_g1(e);
          G1 term = g1_mul(&ci, e[3]);
          acc = g1_add(&acc, &term);
          y = hf_add(y, hf_mul(hf(e[3]), hf(e[4])));
        }
        if (fread(t, 1, 4, stdin) != 4) return 2;
        G1 G = rd_g1(key), W = rd_g1(t);
        G2 h1 = rd_g2(key + 3), hs = rd_g2(key + 5);
        G1 yG = g1_mul(&G, y.value);
        G1 nyG = g1_neg(&yG);
        G1 zW = g1_mul(&W, t[3]);
        G1 L = g1_add(&acc, &nyG);
        L = g1_add(&L, &zW);
        GTP lhs = pairing(&L, &h1), rhs = pairing(&W, &hs);
        putchar(gtp_equal(&lhs, &rhs));
      }
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
        src = os.path.join(tmp, "kzg_fold_driver.c")
        self.exe = os.path.join(tmp, "kzg_fold_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-w", "-I", ref_src, src, "-o", self.exe], check=True)

    def run(self, msg):
        return subprocess.run([self.exe], input=msg, capture_output=True, check=True).stdout


def u32(n):
    return int(n).to_bytes(4, "little")


def srs_points(n=SRS_LEN):
    """srs[i] = (2^i mod 17) G: a well-formed SRS for s = 2"""
    return np.array([gen.KG[pow(2, i, 17)] for i in range(n)], np.uint8)


def srs_record(pts):
    return b"S" + u32(len(pts)) + pts.tobytes()


def poly_record(p):
    return bytes([len(p)]) + bytes(p)


def group_record(polys, weights, z):
    return bytes([len(polys), z]) + b"".join(bytes([w]) + poly_record(p) for p, w in zip(polys, weights))


def random_groups(seed, n, max_len=MAX_LEN):
    """n groups (polys, weights, z): k cycles through 1 .. 16, ragged lengths 1 .. max_len (the longest
    rarely first), weights with zeros (every eighth group all zero), canonical coefficients whose top one
    may be zero; every sixteenth group ends in a pair w p + (17 - w) p that cancels"""
    per = 2 + 16 * (2 + max_len)
    r = gen.splitmix64(seed, n * per).reshape(n, per)
    out = []
    for g in range(n):
        k = 1 + g % 16
        x = [int(v >> np.uint64(8)) for v in r[g]]
        z = x[0] % 17
        polys, weights = [], []
        for i in range(k):
            o = 2 + i * (2 + max_len)
            ln = 1 + x[o] % max_len
            polys.append([v % 17 for v in x[o + 2:o + 2 + ln]])
            weights.append(0 if g % 8 == 7 else x[o + 1] % 17)
        if g % 16 == 9 and k >= 2:
            polys[-1] = list(polys[-2])
            weights[-2] = 1 + weights[-2] % 16
            weights[-1] = 17 - weights[-2]
        out.append((polys, weights, z))
    return out


def parse_open(out, groups):
    res, o = [], 0
    for polys, _, _ in groups:
        k = len(polys)
        ys = list(out[o:o + k])
        fl = out[o + k]
        F = list(out[o + k + 1:o + k + 1 + fl])
        proof = tuple(out[o + k + 1 + fl:o + k + 4 + fl])
        o += k + 4 + fl
        res.append((ys, F, proof))
    assert o == len(out)
    return res


def groups_json(res):
    """the reference's answers alone; the inputs are random_groups(seed, n)"""
    return {"ys": ",".join(bytes(ys).hex() for ys, _, _ in res), "F": ",".join(bytes(F).hex() for _, F, _ in res),
            "proofs": b"".join(bytes(p) for _, _, p in res).hex()}


def random_g1(r):
    """valid encodings from three random words per point: coordinates < 101 (mostly off the curve), the
    flag set on a quarter of them"""
    return np.stack([(r[0::3] % np.uint64(101)), (r[1::3] >> np.uint64(8)) % np.uint64(101),
                     ((r[2::3] >> np.uint64(16)) % np.uint64(4) == 0)], 1).astype(np.uint8)


def verify_jobs(seed, k, n):
    """n jobs of 7 + 5 k + 4 bytes {vk 7, k x {C 3, w, y}, W 3, z}.  Job b by b % 4:
    0  random valid encodings (a quarter flagged, most off the curve) under its own random key
    1  random valid encodings under the s = 2 key
    2  subgroup points C_i = c_i G, W = w G under the s = 2 key with the ys solved so that the opening
       equation holds whenever some weight is non-zero
    3  as 2 with random ys"""
    per = 8 + 5 * k + 4 + 3 * (k + 1)
    r = gen.splitmix64(seed + k, n * per).reshape(n, per)
    kg = np.array(gen.KG, np.uint8)
    pts = gen.all_points()
    jobs = np.zeros((n, 7 + 5 * k + 4), np.uint8)
    for b in range(n):
        x = r[b]
        v = [int(t >> np.uint64(8)) for t in x[:8 + 5 * k + 4]]
        enc = random_g1(x[8 + 5 * k + 4:])
        kind = b % 4
        key = list(STD_KEY)
        if kind == 0:
            key = list(pts[v[0] % 102]) + [v[1] % 101, v[2] % 101, v[3] % 101, v[4] % 101]
        ws = [v[8 + 5 * i] % 17 for i in range(k)]
        ysv = [v[9 + 5 * i] % 17 for i in range(k)]
        z = v[5] % 17
        if kind < 2:
            cs, W = [list(e) for e in enc[:k]], list(enc[k])
        else:
            ce = [v[10 + 5 * i] % 17 for i in range(k)]
            we = v[6] % 17
            cs, W = [list(kg[c]) for c in ce], list(kg[we])
            if kind == 2:
                ysv = list(ce)
                nz = [i for i in range(k) if ws[i]]
                if nz:
                    # sum w_i c_i - sum w_i y_i + (z - 2) w = 0: put the whole correction on one entry
                    j = nz[v[7] % len(nz)]
                    ysv[j] = (ce[j] + (z - 2) * we * pow(ws[j], 15, 17)) % 17
        row = key
        for i in range(k):
            row = row + cs[i] + [ws[i], ysv[i]]
        jobs[b] = row + W + [z]
    return jobs


def e2e_variants(g, weights, ys, proof):
    """the four (weights, ys, proof) variants of end-to-end group g: honest, one y_i, one weight, the proof
    altered (a pure function of the seed and the honest opening)"""
    x = [int(t >> np.uint64(8)) for t in gen.splitmix64(E2E_SEED ^ 0xA17E, 4, 4 * g)]
    ws, ys, proof = list(weights), list(ys), tuple(proof)
    i = x[0] % len(ws)
    alt_y, alt_w = list(ys), list(ws)
    alt_y[i] = (ys[i] + 1 + x[1] % 16) % 17
    alt_w[i] = (ws[i] + 1 + x[2] % 16) % 17
    alt_p = tuple(gen.KG[1 + x[3] % 16])
    if alt_p == proof:
        alt_p = tuple(gen.KG[0])
    return [(ws, ys, proof), (ws, alt_y, proof), (alt_w, ys, proof), (ws, ys, alt_p)]


def e2e_cases(d, pts):
    """honest groups for s = 2 and their three altered variants: the reference's commitments, openings and
    the verdicts of all four"""
    groups = random_groups(E2E_SEED, N_E2E)
    res = parse_open(d.run(srs_record(pts) + b"O" + u32(len(groups)) + b"".join(group_record(*g) for g in groups)), groups)
    flat = [p for polys, _, _ in groups for p in polys]
    cm = d.run(srs_record(pts) + b"C" + u32(len(flat)) + b"".join(poly_record(p) for p in flat))
    cases, o = [], 0
    for g, ((polys, ws, z), (ys, F, proof)) in enumerate(zip(groups, res)):
        k = len(polys)
        commits = cm[3 * o:3 * (o + k)]
        o += k
        bits = []
        for w_, y_, p_ in e2e_variants(g, ws, ys, proof):
            job = list(STD_KEY)
            for j in range(k):
                job += list(commits[3 * j:3 * j + 3]) + [w_[j], y_[j]]
            job += list(p_) + [z]
            bits.append(d.run(b"W" + u32(1) + bytes([k]) + bytes(job))[0])
        cases.append((commits.hex(), bytes(ys).hex(), bytes(proof).hex(), "".join(str(int(b)) for b in bits)))
    # one comma-separated entry per group (the proofs: 3 bytes each, run together)
    return {"commits": ",".join(c[0] for c in cases), "ys": ",".join(c[1] for c in cases),
            "proofs": "".join(c[2] for c in cases), "bits": ",".join(c[3] for c in cases)}


def expand(gold):
    """the committed record joined with the inputs it was taken on ->
    (opening groups [dict], {k: (job rows n x (7 + 5 k + 4), verdict bits)}, end-to-end cases [dict])"""
    def unhex(t):
        return list(bytes.fromhex(t))

    o = gold["open"]
    ys, F, pr = o["ys"].split(","), o["F"].split(","), unhex(o["proofs"])
    opened = [{"polys": p, "weights": w, "z": z, "ys": unhex(ys[i]), "F": unhex(F[i]), "proof": tuple(pr[3 * i:3 * i + 3])}
              for i, (p, w, z) in enumerate(random_groups(o["seed"], o["n"]))]
    v = gold["verify"]
    verify = {int(k): (verify_jobs(v["seed"], int(k), v["n_per_k"]), np.array([int(c) for c in bits], np.uint8))
              for k, bits in v["bits_by_k"].items()}
    e = gold["e2e"]
    cm, ys, pr, bits = e["commits"].split(","), e["ys"].split(","), unhex(e["proofs"]), e["bits"].split(",")
    cases = []
    for g, (p, w, z) in enumerate(random_groups(e["seed"], e["n"])):
        c = unhex(cm[g])
        cases.append({"polys": p, "weights": w, "z": z, "commits": [tuple(c[3 * i:3 * i + 3]) for i in range(len(p))],
                      "ys": unhex(ys[g]), "proof": tuple(pr[3 * g:3 * g + 3]), "bits": bits[g],
                      "variants": e2e_variants(g, w, unhex(ys[g]), pr[3 * g:3 * g + 3])})
    return opened, verify, cases


def generate(ref_src=REF_SRC):
    pts = srs_points()
    with tempfile.TemporaryDirectory() as tmp:
        d = Driver(ref_src, tmp)
        groups = random_groups(OPEN_SEED, N_OPEN)
        out = d.run(srs_record(pts) + b"O" + u32(len(groups)) + b"".join(group_record(*g) for g in groups))
        opened = groups_json(parse_open(out, groups))
        verify = {}
        per = -(-N_VERIFY // len(VERIFY_KS))
        for k in VERIFY_KS:
            jobs = verify_jobs(VERIFY_SEED, k, per)
            bits = d.run(b"W" + u32(len(jobs)) + bytes([k]) + jobs.tobytes())
            assert len(bits) == len(jobs) and max(bits) <= 1
            verify[str(k)] = "".join(str(int(b)) for b in bits)
        e2e = e2e_cases(d, pts)
    return {
        "source": "reference src/poly.h (poly_scale, poly_add, poly_eval, poly_divide), src/srs.h (srs_eval_at_s), "
                  "src/pairing.h, src/g1.h (g1_mul, g1_add, g1_neg), compiled unmodified",
        "srs": hx(pts),
        "key": bytes(STD_KEY).hex(),
        "inputs": "not stored: random_groups(seed, n) / verify_jobs(seed, k, n) / e2e_variants of this script",
        "open": dict(opened, seed=OPEN_SEED, n=N_OPEN),
        "verify": {"seed": VERIFY_SEED, "n_per_k": -(-N_VERIFY // len(VERIFY_KS)), "bits_by_k": verify},
        "e2e": dict(e2e, seed=E2E_SEED, n=N_E2E, variants="honest, y, weight, proof"),
    }


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else REF_SRC
    if not os.path.isdir(ref):
        sys.exit("the reference sources are not at %s" % ref)
    with open(OUT, "w") as f:
        json.dump(generate(ref), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
