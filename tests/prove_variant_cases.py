"""Which kernels the device prover takes for one placement of the caller's 13 polynomials, restated
from plonk.c_amd/csrc/prove.hip (rounds(), lincomb_batch, make_evargs, divide_zh,
divide_linear), and the placements and sizes that tests/test_prove_variants_gpu.py runs.
tests/test_prove_variants_cpu.py checks that the lists reach every variant; the GPU file checks
the counted launches (plk_prover_launches) against launch_delta.

Besides n, rounds() chooses from the address of each caller polynomial mod 16 and mod 4, n % 4 and
n % 16 (binomial Z_H = x^n - 1 of n + 1 coefficients, one device, no helpers; the prover's own
buffers -- Z_H's copy, the commitment arena, every intermediate -- are 16-byte aligned and padded):

  prep    rounds 1-3 preparation in one launch (prep_kernel): f_a f_b f_c acc_x s_sigma_1..3 all
          16-byte aligned (the lengths satisfy la <= lzx <= la + 1 at every n and Z_H, n + 2 <= n + 3
          <= n + 3 for this Z_H: lens_for).  Else scalars_init_kernel, 4 blinding products
          (direct kernel, one launch each), a lincomb_batch of 3 (one lincomb16_batch launch when
          f_a f_b f_c are aligned, else 3 lincomb_kernel), a lincomb_batch of 1 (acc_x: one launch
          either way), a lincomb_batch of 8 (one launch when s_sigma_1..3 are aligned, else 8).
  numdiv  t(x)'s numerator and its division by Z_H in one launch (numdiv_kernel): n % 4 == 0 and q_c
          4-byte aligned.  Else lincomb_batch({num}) (one launch either way), divide_zh
          (divide_binomial4_kernel when n % 4 == 0, else divide_binomial_kernel: one launch),
          copy3_kernel.
  fuse5   round 5's numerators computed inside the division launch, ONE launch
          (lincomb_agg_divide_kernel): n % 16 == 0 and q_m q_l q_r q_o s_sigma_1 s_sigma_2 16-byte
          aligned.  Else a lincomb_batch of 2 first (one launch when those six are aligned, else 2) and
          the two-launch scan (lin_scan_sums_kernel, lin_scan_apply_kernel).  No option is involved.
  agg     round 4's evaluation rows store the chunk aggregates: exactly with fuse5 (every aggregated
          caller row is then aligned with n % 16 == 0: vec == 2, so make_evargs' agg_ok holds).
  vec     per evaluated caller polynomial (s_sigma_1 s_sigma_2 l_1 q_m q_l q_r q_o): 0 bytes, 1 aligned
          (the tail of the last 16-byte load masked), 2 aligned and n % 16 == 0.

The round-3 products (their NTT pass launches), the evaluation launch and the commitments depend
on lengths and options only, so they cancel in launch_delta; no option moves a switch listed
above, so the `options` arguments below change nothing (the GPU file passes the sets it runs).
"""
import numpy as np

FA, FB, FC, QO, QM, QL, QR, QC, S1, S2, S3, ACC, L1 = range(13)
NAMES = ("f_a", "f_b", "f_c", "q_o", "q_m", "q_l", "q_r", "q_c", "s1", "s2", "s3", "acc_x", "l_1")
PREP_INPUTS = (FA, FB, FC, ACC, S1, S2, S3)
FUSE5_INPUTS = (QM, QL, QR, QO, S1, S2)
EVAL_INPUTS = (S1, S2, L1, QM, QL, QR, QO)
ALIGNED = (0,) * 13


def _al(residues, idx, m=16):
    return all(residues[i] % m == 0 for i in idx)


def variants(n, residues, options=None):
    """{prep, numdiv, fuse5, agg} of rounds() at n gates for the 13 address residues (mod 16, in
    d_polys order); `options` move no switch"""
    assert len(residues) == 13
    la, lzx = n + 2, n + 3
    prep = _al(residues, PREP_INPUTS) and la <= lzx <= la + 1
    numdiv = n % 4 == 0 and residues[QC] % 4 == 0
    fuse5 = n % 16 == 0 and _al(residues, FUSE5_INPUTS)
    agg = fuse5
    return dict(prep=prep, numdiv=numdiv, fuse5=fuse5, agg=agg)


def vec_modes(n, residues):
    """make_evargs' vec of each evaluated caller polynomial, by d_polys index"""
    return {i: 0 if residues[i] % 16 else (2 if n % 16 == 0 else 1) for i in EVAL_INPUTS}


def switched_launches(n, residues, options=None):
    """kernel launches of the parts of rounds() that depend on the placement"""
    v = variants(n, residues, options)
    k = 0
    if v["prep"]:
        k += 1                                              # prep_kernel
    else:
        k += 1 + 4                                          # scalars_init_kernel, 4 blinding products
        k += 1 if _al(residues, (FA, FB, FC)) else 3        # a_x b_x c_x
        k += 1                                              # z_x
        k += 1 if _al(residues, (S1, S2, S3)) else 8        # round 3's linear factors
    k += 1 if v["numdiv"] else 3                            # numdiv | lincomb, divide, copy3
    if v["fuse5"]:
        k += 1                                              # lincomb_agg_divide
    else:
        k += 1 if _al(residues, FUSE5_INPUTS) else 2        # W and ZZ numerators
        k += 2                                              # lin_scan_sums, lin_scan_apply
    return k


def launch_delta(n, residues, options=None):
    """kernel launches of a proof from this placement minus those from the all-aligned placement at
    the same n and options"""
    return switched_launches(n, residues, options) - switched_launches(n, ALIGNED, options)


# ---- sizes (Z_H = x^n - 1): seed of a gen.prove_instance whose oracle proof has no reference exit
SIZES = {
    1008: 101,     # n % 16 == 0
    1000: 101,     # n % 16 == 8, n % 4 == 0: fuse5 off, numdiv on
    1004: 101,     # n % 16 == 12
    1001: 101,     # n % 4 != 0: numdiv off, divide_binomial_kernel
    1023: 102,
    4112: 101,     # evaluations past 4096: the row split, more than one AGG_CHUNK
    8200: 101,
    20000: 101,    # several scan chunks per division
}
SINGLE_SIZES = (1008, 1000, 1001)                  # list (a)
STRICT = {1008: 201, 1000: 201, 1001: 201, 4112: 201}   # prove_strict_case.strict_case seeds
OPTION_SIZES = (1008, 1000, 4112)
PREPROCESSED_SIZES = (1008, 8200)
SPLIT_SIZES = (1000, 4112)


def _one(i, r):
    res = [0] * 13
    res[i] = r
    return tuple(res)


# (a) each polynomial alone at residue 1, 4 and 8, the other twelve at 0
SINGLE = [("%s@%d" % (NAMES[i], r), _one(i, r)) for i in range(13) for r in (1, 4, 8)]
# (b) all thirteen at one residue
TOGETHER = [("all@%d" % r, (r,) * 13) for r in (1, 2, 4, 8, 15)]


def _mixes():
    rng = np.random.default_rng(0x13A11)
    pool = np.array([0, 1, 4, 8, 12, 15])
    return [("mix%d" % k, tuple(int(x) for x in rng.choice(pool, 13))) for k in range(16)]


# (c) 16 seeded mixes of residues from {0, 1, 4, 8, 12, 15}
MIXES = _mixes()


def only(*idx, r=1):
    """the named polynomials at residue r, the others aligned (q_c-only, q_m-only, ...)"""
    res = [0] * 13
    for i in idx:
        res[i] = r
    return tuple(res)


def placements(n):
    """(name, residues) run at n by the single-polynomial-and-mixes test"""
    return (SINGLE if n in SINGLE_SIZES else []) + TOGETHER + MIXES


# the option values of test_round5_divisions_vs_oracle (EARLY_COMMITS) ...
DIVISION_OPTIONS = [dict(PROVE_EARLY_COMMITS=e) for e in (1, 0)]
# ... of test_commitments_srs_log_form (SRS_LOGS, PACK_FUSE, EARLY_COMMITS) ...
COMMIT_OPTIONS = [dict(PROVE_SRS_LOGS=s, PROVE_PACK_FUSE=p, PROVE_EARLY_COMMITS=e)
                  for s, p, e in ((1, 1, 0), (1, 0, 1), (0, 1, 1))]
# ... and of test_derive_t2a_modes_vs_oracle
DERIVE_OPTIONS = [dict(PROVE_DERIVE_T2A=m) for m in (0, 1, 2)]
OPTION_SETS = DIVISION_OPTIONS + COMMIT_OPTIONS + DERIVE_OPTIONS
OPTION_PLACEMENTS = TOGETHER + [("q_c@1", only(QC)), ("q_m@1", only(QM)), ("s1@1", only(S1))]
