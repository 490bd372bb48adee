"""Which round-3 plan the device prover takes at n gates (binomial Z_H = x^n - 1, default options,
one device), restated from the rules of plonk.c_amd/csrc/prove.hip (rounds()) and ntt.hip
(product_plan, plk_poly_mul_batch_launch, ntt_group), and the table of expected centre launches
for the gate counts of tests/golden/prove_large.json.  tests/test_prove_large_cpu.py checks the
table against the restated rules; tests/test_prove_large_gpu.py checks the device's launch log
(PLK_OPT_NTT_LAUNCH_LOG) against the table.

The switches and the first n on their other side (la = n + 2, lzx = n + 3, the 2n products have
2n + 1 .. 2n + 4 coefficients, (a b) q_m 3n + 2, t_2 / t_3 4n + 6):

  2^12 -> 2^13 tiles (transforms of 2^21 points and up), both inside one proof     n = 2^19
  (a b) q_m leaves the t_2 sum group: the transform sizes differ                   600000, 1223336
  a q_l + b q_r + c q_o stops being one sum group, 3 (n + 2) 128 >= p29            1,223,337
  t_2 group refused on range, (3n + 3) 128 >= p29, although the plans agree again
  (3n + 2 > 2^22 + 16)                                                             1,398,107
  4n products leave F29 for BabyBear, (2n + 3) 128 >= p29, and (a b) q_m's launch
  chunk goes with them (a q_m transform preprocessed for F29 is stale)             1,835,007
  2n products leave F29 too, (n + 2) 128 >= p29                                    3,670,015
  a 4n product leaves BabyBear's exact range, (2n + 3) 256 >= pBB: PLK_ERR_RANGE   3,932,159
"""
P29 = 7 * (1 << 26) + 1          # F29, centred residues: 64 sum(min) <= (p - 1) / 2
PBB = 15 * (1 << 27) + 1         # BabyBear, bytes as they are: 256 sum(min) < p
SMALL_LOG, DIRECT_MAX, WRAP_MAX, MAX_JOBS, T13_MIN_K = 12, 32, 16, 12, 21
F29, BABYBEAR = 0, 1             # LaunchRec's field code
N_MAX = 3932158                  # (2n + 3) 256 < pBB


def product_plan(la, lb):
    """(log2 of the transform size, wrapped top coefficients)"""
    rl = la + lb - 1
    k = (rl - 1).bit_length()
    if k - 1 > SMALL_LOG:
        ex = rl - (1 << (k - 1))
        if ex <= WRAP_MAX and ex < max(la, lb):
            return k - 1, ex
    return k, 0


def batch_launches(jobs):
    """jobs: (la, lb, acc).  The centre launches of one plk_poly_mul_batch_launch call in launch
    order as (k, tile bits, field, products, products with inverse passes), or None where a
    product is outside BabyBear's exact range (PLK_ERR_RANGE before any launch)."""
    ks = []
    for la, lb, _ in jobs:
        assert min(la, lb) > DIRECT_MAX and product_plan(la, lb)[0] > SMALL_LOG
        if min(la, lb) * 256 >= PBB:
            return None
        ks.append(product_plan(la, lb)[0])
    out, done = [], [False] * len(jobs)
    for i, k in enumerate(ks):
        if done[i]:
            continue
        groups, m = [], 0                         # one launch chunk: sum groups of size k, <= 12 jobs
        for q in range(i, len(jobs)):
            if done[q] or ks[q] != k or jobs[q][2]:
                continue
            gs = 1
            while q + gs < len(jobs) and jobs[q + gs][2]:
                gs += 1
            if m + gs > MAX_JOBS:
                break
            groups.append(sum(min(la, lb) for la, lb, _ in jobs[q:q + gs]))
            for u in range(gs):
                done[q + u] = True
            m += gs
        f29 = k <= 26 and all(mn * 128 < P29 for mn in groups)
        assert f29 or all(mn * 256 < PBB for mn in groups)
        out.append((k, 13 if k >= T13_MIN_K else 12, F29 if f29 else BABYBEAR, m, len(groups)))
    return out


def prover_batches(n):
    """centre launches of round 3's two product batches at n gates, PROVE_DERIVE_T2A at its default
    (A2 B2 is not a product of the first batch)"""
    la, lzx, lab, t2b = n + 2, n + 3, 2 * n + 3, 2 * n + 4
    lin = 1 if 3 * la * 128 < P29 else 0
    grp = 1 if (product_plan(lab, n)[0] == product_plan(lab, t2b)[0] and
                (min(lab, t2b) + min(lab, n)) * 128 < P29) else 0
    g1 = [(la, n, 0), (la, n, lin), (la, n, lin), (lzx, n, 0), (la, la, 0), (lzx, n, 0), (la, lzx, 0), (la, la, 0),
          (la, lzx, 0)]
    g2 = [(lab, t2b, 0), (lab, n, grp), (lab, t2b, 0)]
    return batch_launches(g1), batch_launches(g2)


def prover_launches(n):
    """centre launches of one plain proof, or None where a product is out of range"""
    a, b = prover_batches(n)
    return None if a is None or b is None else a + b


# n: the centre launches (kind 2 records) of a plain proof in launch order, each
# (k, tile bits, field, products, products with inverse passes -- fewer where a sum group formed)
LAUNCHES = {
    131072: [(18, 12, F29, 9, 7), (19, 12, F29, 3, 2)],
    262144: [(19, 12, F29, 9, 7), (20, 12, F29, 3, 2)],
    524288: [(20, 12, F29, 9, 7), (21, 13, F29, 3, 2)],                          # both tile widths
    600000: [(21, 13, F29, 9, 7), (22, 13, F29, 2, 2), (21, 13, F29, 1, 1)],     # (a b) q_m apart: 2^21 / 2^22
    1223336: [(22, 13, F29, 9, 7), (23, 13, F29, 2, 2), (22, 13, F29, 1, 1)],    # last n with the linear sum group
    1223337: [(22, 13, F29, 9, 9), (23, 13, F29, 2, 2), (22, 13, F29, 1, 1)],
    1400000: [(22, 13, F29, 9, 9), (23, 13, F29, 3, 3)],                         # one size, no t_2 group (range)
    1835006: [(22, 13, F29, 9, 9), (23, 13, F29, 3, 3)],                         # last n all in F29
    1835007: [(22, 13, F29, 9, 9), (23, 13, BABYBEAR, 3, 3)],
    2097152: [(22, 13, F29, 9, 9), (23, 13, BABYBEAR, 3, 3)],
    3932158: [(23, 13, BABYBEAR, 9, 9), (24, 13, BABYBEAR, 3, 3)],               # the largest n
}

# preprocessed circuits: is q_m's recorded transform (its own plan: 2^k points of (2n + 3) x n, F29
# while n 128 < p29) the one its launch runs in?  Where it is, that launch runs one lo = 0 pass fewer.
QM_TRANSFORM_USED = {524288: True, 1223337: True, 1835007: False, 2097152: False}


def qm_transform_used(n):
    k = product_plan(2 * n + 3, n)[0]
    mine = F29 if k <= 26 and n * 128 < P29 else BABYBEAR
    return any(lk == k and lf == mine for lk, _, lf, _, _ in prover_batches(n)[1])
