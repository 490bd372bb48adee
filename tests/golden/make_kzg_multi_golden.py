"""Record tests/golden/kzg_multi.json from the REAL reference: multi-point KZG openings (poly_z,
poly_divide, poly_scale, poly_add, poly_eval, srs_eval_at_s) and their verification (g1_mul, g1_add,
pairing), from src/poly.h, src/srs.h, src/pairing.h and what they include, unmodified, taken by -I.

    python tests/golden/make_kzg_multi_golden.py <reference src directory>

Runs only where the reference tree is present.  A small C driver is written to a temporary directory,
compiled with gcc against the reference's headers and fed the seeded inputs built here; only its outputs
reach the JSON.  The inputs are not stored: they are pure functions of the seeds below (random_groups,
verify_jobs, e2e_variants), which the tests call to rebuild them -- that needs numpy alone, not the
reference.  To keep the file small an opening's evaluations and h are stored as one short digest; W and
W' are stored as they are.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen  # noqa: E402

OUT = os.path.join(HERE, "kzg_multi.json")
OPEN_SEED, VERIFY_SEED, E2E_SEED = 0x4D554C54, 0x564D554C, 0x45324D55
N_OPEN, N_VERIFY, N_E2E = 200, 2000, 30
MAX_LEN, SRS_LEN = 40, 48
KS = (1, 2, 3, 9, 15)
FULL = (1 << 17) - 1
G2_1, G2_2 = (36, 31), (90, 82)          # g2_generator() and twice it (tests/golden/pairing.json pins both)
STD_KEY = (1, 2, 0) + G2_1 + G2_2        # s = 2

# The driver: a stream of records on stdin, the answers on stdout.
#   'S' n(u32) n x 3 bytes                                   the SRS of the records that follow; no output
#   'C' n(u32) n x {len(u8), coeffs}                         -> n x 3 bytes, srs_eval_at_s
#   'M' n(u32) n x {k, u, k x {w, mask(u32), len, coeffs}}   -> per group: 17 k ys (0xFF off the set), len(h), h, W, W'
#   'V' n(u32) k(u8) n x {vk 7, k x {C 3, mask(u32), w, ys 17}, W 3, W' 3, u} -> n bytes, the accept bit
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
/* prod_{a in mask} (x - a) at x */
static HF vanish(unsigned mask, HF x) {
  HF r = hf_one();
  for (unsigned a = 0; a < 17; a++)
    if ((mask >> a) & 1u) r = hf_mul(r, hf_sub(x, hf(a)));
  return r;
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
    } else if (c == 'M') {
      unsigned n = rd_u32();
      for (unsigned g = 0; g < n; g++) {
        unsigned k = rd_u8();
        HF u = hf(rd_u8());
        POLY ps[16];
        HF ws[16];
        unsigned masks[16], T = 0;
        POLY h = poly_zero();
        for (unsigned i = 0; i < k; i++) {
          ws[i] = hf(rd_u8());
          masks[i] = rd_u32();
          T |= masks[i];
          ps[i] = rd_poly();
          HF pts[17];
          size_t t = 0;
          for (unsigned a = 0; a < 17; a++) {
            if ((masks[i] >> a) & 1u) {
              pts[t++] = hf(a);
              putchar(poly_eval(&ps[i], hf(a)).value);
            } else {
              putchar(0xFF);
            }
          }
          POLY z = poly_z(pts, t), q, rem;
          poly_divide(&ps[i], &z, &q, &rem);
          POLY sq = poly_scale(&q, ws[i]);
          h = poly_add(&h, &sq);
        }
        putchar((int)h.len);
        for (size_t j = 0; j < h.len; j++) putchar(h.coeffs[j].value);
        put_g1(srs_eval_at_s(&srs, &h));
        POLY F = poly_zero();
        for (unsigned i = 0; i < k; i++) {
          POLY sp = poly_scale(&ps[i], hf_mul(ws[i], vanish(T & ~masks[i], u)));
          F = poly_add(&F, &sp);
        }
        POLY sh = poly_scale(&h, hf_neg(vanish(T, u)));
        F = poly_add(&F, &sh);
        HF dc[2] = {hf_neg(u), hf_one()};
        POLY den = poly_new(dc, 2), q, rem;
        poly_divide(&F, &den, &q, &rem);
        put_g1(srs_eval_at_s(&srs, &q));
      }
    } else if (c == 'V') {
      unsigned n = rd_u32(), k = rd_u8();
      for (unsigned b = 0; b < n; b++) {
        unsigned char key[7], e[3], ys[17], t[7];
        if (fread(key, 1, 7, stdin) != 7) return 2;
        G1 cs[16];
        unsigned masks[16], T = 0;
        HF ws[16], rs[16];
        unsigned char yall[16][17];
        for (unsigned i = 0; i < k; i++) {
          if (fread(e, 1, 3, stdin) != 3) return 2;
          cs[i] = rd_g1(e);
          masks[i] = rd_u32();
          T |= masks[i];
          ws[i] = hf(rd_u8());
          if (fread(ys, 1, 17, stdin) != 17) return 2;
          for (unsigned a = 0; a < 17; a++) yall[i][a] = ys[a];
        }
        if (fread(t, 1, 7, stdin) != 7) return 2;
        HF u = hf(t[6]);
        G1 acc = g1_identity();
        HF y = hf_zero();
        for (unsigned i = 0; i < k; i++) {
          HF r = hf_zero();
          for (unsigned a = 0; a < 17; a++) {
            if (!((masks[i] >> a) & 1u)) continue;
            unsigned rest = masks[i] & ~(1u << a);
            r = hf_add(r, hf_mul(hf(yall[i][a]), hf_div(vanish(rest, u), vanish(rest, hf(a)))));
          }
          rs[i] = r;
          HF ci = hf_mul(ws[i], vanish(T & ~masks[i], u));
          G1 term = g1_mul(&cs[i], ci.value);
          acc = g1_add(&acc, &term);
          y = hf_add(y, hf_mul(ci, rs[i]));
        }
        G1 G = rd_g1(key), W = rd_g1(t), Wp = rd_g1(t + 3);
        HF ch = hf_neg(vanish(T, u));
        G1 term = g1_mul(&W, ch.value);
        acc = g1_add(&acc, &term);
        y = hf_add(y, hf_mul(ch, hf_zero()));
        G2 h1 = rd_g2(key + 3), hs = rd_g2(key + 5);
        G1 yG = g1_mul(&G, y.value);
        G1 nyG = g1_neg(&yG);
        G1 zW = g1_mul(&Wp, u.value);
        G1 L = g1_add(&acc, &nyG);
        L = g1_add(&L, &zW);
        GTP lhs = pairing(&L, &h1), rhs = pairing(&Wp, &hs);
        putchar(gtp_equal(&lhs, &rhs));
      }
    } else {
      return 3;
    }
  }
  return 0;
}
"""


class Driver:
    def __init__(self, ref_src, tmp):
        src = os.path.join(tmp, "kzg_multi_driver.c")
        self.exe = os.path.join(tmp, "kzg_multi_driver")
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


def group_record(polys, sets, weights, u):
    return bytes([len(polys), u]) + b"".join(bytes([w]) + u32(m) + poly_record(p) for p, m, w in zip(polys, sets, weights))


def points(mask):
    return [a for a in range(17) if (mask >> a) & 1]


def random_mask(x0, x1, kind):
    """1 .. 16 points from two random words.  kind 0: a random subset, 1: without 0, 2: with 0, 3: one point,
    4: sixteen points, 5: a pair {z, 3 z} (z != 0)"""
    if kind == 3:
        return 1 << (x0 % 17)
    if kind == 4:
        return FULL & ~(1 << (x0 % 17))
    if kind == 5:
        z = 1 + x0 % 16
        return 1 << z | 1 << (3 * z % 17)
    m, v = 0, x0
    while bin(m).count("1") < 1 + x1 % 16:         # 1 .. 16 distinct points, every size as likely
        v = (v * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        m |= 1 << ((v >> 33) % 17)
    if kind == 1:
        m &= ~1
    if kind == 2:
        m |= 1
    if m == 0:
        m = 1 << (1 + x1 % 16)
    if m == FULL:
        m &= ~(1 << (1 + x1 % 16))
    return m


def random_groups(seed, n, max_len=MAX_LEN):
    """n groups (polys, sets, weights, u): k cycles through KS, ragged lengths 1 .. max_len (with len <= t,
    len = t + 1 and len = 1 among them), sets of 1 .. 16 points with and without 0, weights with zeros (every
    eighth group all zero), u alternately a point of T and (where T leaves one) a point outside it; every
    tenth group ends in a pair w p + (17 - w) p over one set, which cancels"""
    per = 4 + 15 * (4 + max_len)
    r = gen.splitmix64(seed, n * per).reshape(n, per)
    out = []
    for g in range(n):
        k = KS[g % len(KS)]
        x = [int(v >> np.uint64(8)) for v in r[g]]
        polys, sets, weights = [], [], []
        for i in range(k):
            o = 4 + i * (4 + max_len)
            m = random_mask(x[o + 2], x[o + 3], (g // len(KS) + i) % 6)
            t = bin(m).count("1")
            ln = 1 + x[o] % max_len
            if (g + i) % 7 == 3:
                ln = min(max_len, t + 1)
            elif (g + i) % 7 == 5:
                ln = max(1, t - x[o] % 2)
            polys.append([v % 17 for v in x[o + 4:o + 4 + ln]])
            sets.append(m)
            weights.append(0 if g % 8 == 7 else x[o + 1] % 17)
        if g % 10 == 6 and k >= 2:
            polys[-1], sets[-1] = list(polys[-2]), sets[-2]
            weights[-2] = 1 + weights[-2] % 16
            weights[-1] = 17 - weights[-2]
        T = 0
        for m in sets:
            T |= m
        inside, outside = points(T), points(FULL & ~T)
        u = inside[x[0] % len(inside)] if g % 2 == 0 or not outside else outside[x[0] % len(outside)]
        out.append((polys, sets, weights, u))
    return out


def digest(ys, h):
    """12 hex characters over a group's 17 k evaluation bytes and its trimmed h"""
    return hashlib.sha256(bytes(ys) + b"|" + bytes(h)).hexdigest()[:12]


def parse_open(out, groups):
    res, o = [], 0
    for polys, _, _, _ in groups:
        k = len(polys)
        ys = list(out[o:o + 17 * k])
        o += 17 * k
        hl = out[o]
        h = list(out[o + 1:o + 1 + hl])
        o += 1 + hl
        res.append((ys, h, tuple(out[o:o + 3]), tuple(out[o + 3:o + 6])))
        o += 6
    assert o == len(out)
    return res


def random_g1(r):
    """valid encodings from three random words per point: coordinates < 101 (mostly off the curve), the
    flag set on a quarter of them"""
    return np.stack([(r[0::3] % np.uint64(101)), (r[1::3] >> np.uint64(8)) % np.uint64(101),
                     ((r[2::3] >> np.uint64(16)) % np.uint64(4) == 0)], 1).astype(np.uint8)


def vanish(mask, x):
    r = 1
    for a in points(mask):
        r = r * (x - a) % 17
    return r


ENTRY = 3 + 4 + 1 + 17           # C, mask, w, ys


def verify_jobs(seed, k, n):
    """n jobs of 7 + 25 k + 7 bytes {vk 7, k x {C 3, mask (u32 little endian), w, ys 17}, W 3, W' 3, u}; the ys
    rows hold values at every position (the verifier reads the set's only).  Job b by b % 4:
    0  random valid encodings (a quarter flagged, most off the curve) under its own random key
    1  random valid encodings under the s = 2 key
    2  subgroup points C_i = c_i G, W = w G, W' = w' G under the s = 2 key, u outside T, non-zero weights, and
       one claimed value solved so that the pairing equation holds
    3  as 2 with that value left random"""
    per = 8 + (6 + 17) * k + 3 * (k + 2)
    r = gen.splitmix64(seed + k, n * per).reshape(n, per)
    kg = np.array(gen.KG, np.uint8)
    pts = gen.all_points()
    jobs = np.zeros((n, 7 + ENTRY * k + 7), np.uint8)
    for b in range(n):
        x = r[b]
        v = [int(t >> np.uint64(8)) for t in x[:8 + 23 * k]]
        enc = random_g1(x[8 + 23 * k:])
        kind = b % 4
        key = list(STD_KEY)
        if kind == 0:
            key = list(pts[v[0] % 102]) + [v[1] % 101, v[2] % 101, v[3] % 101, v[4] % 101]
        u = v[5] % 17
        masks = [random_mask(v[8 + 23 * i], v[9 + 23 * i], (b // 4 + i) % 6) for i in range(k)]
        ws = [v[10 + 23 * i] % 17 for i in range(k)]
        ys = [[v[14 + 23 * i + a] % 17 for a in range(17)] for i in range(k)]
        if kind < 2:
            cs, W, Wp = [list(e) for e in enc[:k]], list(enc[k]), list(enc[k + 1])
        else:
            for i in range(k):                       # u outside T, every set non-empty, weights non-zero
                masks[i] &= ~(1 << u)
                if masks[i] == 0:
                    masks[i] = 1 << ((u + 1 + v[11 + 23 * i] % 16) % 17)
                ws[i] = 1 + ws[i] % 16
            ce = [v[12 + 23 * i] % 17 for i in range(k)]
            we, wpe = v[6] % 17, v[7] % 17
            cs, W, Wp = [list(kg[c]) for c in ce], list(kg[we]), list(kg[wpe])
            if kind == 2:
                T = 0
                for m in masks:
                    T |= m
                c = [ws[i] * vanish(T & ~masks[i], u) % 17 for i in range(k)]

                def lag(i, a):
                    rest = masks[i] & ~(1 << a)
                    return vanish(rest, u) * pow(vanish(rest, a), 15, 17) % 17

                # sum c_i C_i - c_T w - sum c_i r_i(u) + (u - 2) w' = 0: put the whole correction on one value
                j = v[13] % k
                a0 = points(masks[j])[(v[13] // k) % len(points(masks[j]))]
                rest = sum(c[i] * lag(i, a) * ys[i][a] for i in range(k) for a in points(masks[i]) if (i, a) != (j, a0))
                want = (sum(c[i] * ce[i] for i in range(k)) - vanish(T, u) * we + (u - 2) * wpe - rest) % 17
                ys[j][a0] = want * pow(c[j] * lag(j, a0), 15, 17) % 17
        row = key
        for i in range(k):
            row = row + cs[i] + list(u32(masks[i])) + [ws[i]] + ys[i]
        jobs[b] = row + W + Wp + [u]
    return jobs


def e2e_groups():
    """honest groups with u outside T and non-zero weights (there an altered value provably moves the check)"""
    out = []
    for polys, sets, weights, u in random_groups(E2E_SEED, N_E2E):
        sets = [m & ~(1 << u) or 1 << ((u + 1) % 17) for m in sets]
        out.append((polys, sets, [1 + w % 16 for w in weights], u))
    return out


def e2e_variants(g, sets, ys, commits, W, Wp):
    """the six (sets, ys, commits, W, W') variants of end-to-end group g: honest, one value, one mask, W, W' and
    one commitment altered (a pure function of the seed and the honest opening)"""
    x = [int(t >> np.uint64(8)) for t in gen.splitmix64(E2E_SEED ^ 0xA17E, 6, 6 * g)]
    k = len(sets)
    i = x[0] % k
    a = points(sets[i])[x[1] % len(points(sets[i]))]
    alt_y = list(ys)
    alt_y[17 * i + a] = (ys[17 * i + a] + 1 + x[2] % 16) % 17
    alt_s = list(sets)
    flip = 1 << (x[3] % 17)
    alt_s[i] = sets[i] ^ flip
    if alt_s[i] == 0 or alt_s[i] == FULL:
        alt_s[i] = sets[i] ^ flip ^ (1 << ((x[3] + 1) % 17))
    alt_ys_s = [0 if v == 0xFF else v for v in ys]     # the added point reads a value: make it a valid byte

    def other(p, t):
        q = tuple(gen.KG[1 + t % 16])
        return q if q != tuple(p) else tuple(gen.KG[0])

    alt_c = [tuple(c) for c in commits]
    alt_c[i] = other(commits[i], x[5])
    hon = [tuple(c) for c in commits]
    return [(sets, ys, hon, W, Wp), (sets, alt_y, hon, W, Wp), (alt_s, alt_ys_s, hon, W, Wp),
            (sets, ys, hon, other(W, x[4]), Wp), (sets, ys, hon, W, other(Wp, x[4] >> 4)), (sets, ys, alt_c, W, Wp)]


def job_row(key, commits, sets, weights, ys, W, Wp, u):
    row = list(key)
    for i in range(len(commits)):
        row += list(commits[i]) + list(u32(sets[i])) + [weights[i]] + list(ys[17 * i:17 * i + 17])
    return bytes(row + list(W) + list(Wp) + [u])


def e2e_cases(d, pts):
    groups = e2e_groups()
    res = parse_open(d.run(srs_record(pts) + b"M" + u32(len(groups)) + b"".join(group_record(*g) for g in groups)), groups)
    flat = [p for polys, _, _, _ in groups for p in polys]
    cm = d.run(srs_record(pts) + b"C" + u32(len(flat)) + b"".join(poly_record(p) for p in flat))
    cases, o = [], 0
    for g, ((polys, sets, ws, u), (ys, h, W, Wp)) in enumerate(zip(groups, res)):
        k = len(polys)
        commits = [tuple(cm[3 * (o + j):3 * (o + j) + 3]) for j in range(k)]
        o += k
        bits = []
        for s_, y_, c_, w_, p_ in e2e_variants(g, sets, ys, commits, W, Wp):
            bits.append(d.run(b"V" + u32(1) + bytes([k]) + job_row(STD_KEY, c_, s_, ws, y_, w_, p_, u))[0])
        cases.append((b"".join(bytes(c) for c in commits).hex(), digest(ys, h), bytes(W + Wp).hex(),
                      "".join(str(int(b)) for b in bits)))
    return {"commits": ",".join(c[0] for c in cases), "digests": ",".join(c[1] for c in cases),
            "proofs": "".join(c[2] for c in cases), "bits": ",".join(c[3] for c in cases)}


def expand(gold):
    """the committed record joined with the inputs it was taken on ->
    (opening groups [dict], {k: (job rows, verdict bits)}, end-to-end cases [dict])"""
    def unhex(t):
        return list(bytes.fromhex(t))

    o = gold["open"]
    dg, pr = o["digests"].split(","), unhex(o["proofs"])
    opened = [{"polys": p, "sets": s, "weights": w, "u": u, "digest": dg[i], "W": tuple(pr[6 * i:6 * i + 3]),
               "Wp": tuple(pr[6 * i + 3:6 * i + 6])} for i, (p, s, w, u) in enumerate(random_groups(o["seed"], o["n"]))]
    v = gold["verify"]
    verify = {int(k): (verify_jobs(v["seed"], int(k), v["n_per_k"]), np.array([int(c) for c in bits], np.uint8))
              for k, bits in v["bits_by_k"].items()}
    e = gold["e2e"]
    cm, dg, pr, bits = e["commits"].split(","), e["digests"].split(","), unhex(e["proofs"]), e["bits"].split(",")
    cases = []
    for g, (p, s, w, u) in enumerate(e2e_groups()):
        c = unhex(cm[g])
        cases.append({"polys": p, "sets": s, "weights": w, "u": u, "digest": dg[g],
                      "commits": [tuple(c[3 * i:3 * i + 3]) for i in range(len(p))],
                      "W": tuple(pr[6 * g:6 * g + 3]), "Wp": tuple(pr[6 * g + 3:6 * g + 6]), "bits": bits[g]})
    return opened, verify, cases


def generate(ref_src):
    pts = srs_points()
    with tempfile.TemporaryDirectory() as tmp:
        d = Driver(ref_src, tmp)
        groups = random_groups(OPEN_SEED, N_OPEN)
        res = parse_open(d.run(srs_record(pts) + b"M" + u32(len(groups)) + b"".join(group_record(*g) for g in groups)), groups)
        opened = {"digests": ",".join(digest(ys, h) for ys, h, _, _ in res),
                  "proofs": b"".join(bytes(W + Wp) for _, _, W, Wp in res).hex()}
        verify = {}
        per = -(-N_VERIFY // len(KS))
        for k in KS:
            jobs = verify_jobs(VERIFY_SEED, k, per)
            bits = d.run(b"V" + u32(len(jobs)) + bytes([k]) + jobs.tobytes())
            assert len(bits) == len(jobs) and max(bits) <= 1
            verify[str(k)] = "".join(str(int(b)) for b in bits)
        e2e = e2e_cases(d, pts)
    return {
        "source": "reference src/poly.h (poly_z, poly_divide, poly_scale, poly_add, poly_eval), src/srs.h "
                  "(srs_eval_at_s), src/pairing.h, src/g1.h (g1_mul, g1_add, g1_neg), compiled unmodified",
        "srs": pts.reshape(-1).tobytes().hex(),
        "key": bytes(STD_KEY).hex(),
        "inputs": "not stored: random_groups(seed, n) / verify_jobs(seed, k, n) / e2e_groups, e2e_variants of this script",
        "open": dict(opened, seed=OPEN_SEED, n=N_OPEN, digest="sha256(17 k ys bytes | trimmed h)[:12]"),
        "verify": {"seed": VERIFY_SEED, "n_per_k": per, "bits_by_k": verify},
        "e2e": dict(e2e, seed=E2E_SEED, n=N_E2E, variants="honest, value, mask, W, W', commitment"),
    }


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_kzg_multi_golden.py <reference src directory>")
    with open(OUT, "w") as f:
        json.dump(generate(sys.argv[1]), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
