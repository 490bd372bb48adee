"""plk_msm_plan without a GPU: the launch plan (threads per block, blocks per MSM, groups in flight,
table copies, half groups) that plk_msm_g1_dev / plk_msm_g1_batch_dev take for a shape under the
current options.  The plan is computed by the helper the launch itself uses, so what is pinned
here is what tests/test_msm_batch_gpu.py runs: a retune of the geometry that moves one of these
shapes to another block count fails here, instead of silently emptying the batch tests.

The pinned values were worked out by hand from plk_msm_geometry (msm.hip):
    groups = n >> 4;  threads = 512 from 2^16 groups, else 256
    fill   = max(1, (MSM_MAX_BLOCKS or 512) // batch)
    blocks = min(fill, ceil(groups / threads)); with no MSM_MAX_BLOCKS, when that is below
             ceil(groups / 2 threads): ceil(groups / threads) for a batch, ceil(groups / 2 threads)
             for a single MSM;  at least 1
    groups in flight: doubled from 1 while 2 g <= groups // (blocks threads), up to MSM_GROUPS or 2
    half:  a single aligned MSM with groups <= blocks threads: twice the blocks, g = 1, one copy
    byte-wise form: no half groups (blocks halved back), g = 1
"""
import numpy as np
import pytest

import plonkhip as h
from test_msm_gpu import _GEOM

SHAPE_A = 37461      # 2341 groups of 16 + a 5-point tail; 256-thread blocks, 10 for one group per thread
SHAPE_B = 1059785    # 66236 groups + a 9-point tail; 512-thread blocks
MSM_OPTS = ("MSM_THREADS", "MSM_MAX_BLOCKS", "MSM_GROUPS", "MSM_COPIES", "MSM_HALF")


def test_shapes_are_what_the_pins_assume():
    assert (SHAPE_A >> 4, SHAPE_A & 15) == (2341, 5) and -(-2341 // 256) == 10
    assert (SHAPE_B >> 4, SHAPE_B & 15) == (66236, 9) and 66236 >= 1 << 16


@pytest.mark.parametrize("X", range(1, 10))
def test_shape_a_blocks_per_row_1_to_9(X):
    with h.options(MSM_MAX_BLOCKS=11 * X):
        p = h.msm_plan(SHAPE_A, 11)
        assert p == {"threads": 256, "blocks": X, "groups": 2 if X <= 4 else 1, "copies": 8, "half": 0}
        # the byte-wise form of the same rows: the same blocks, one group in flight
        assert h.msm_plan(SHAPE_A, 11, aligned=False) == dict(p, groups=1)
        if X == 1:
            with h.options(MSM_GROUPS=4):
                assert h.msm_plan(SHAPE_A, 11) == dict(p, groups=4)
        if X == 3:
            with h.options(MSM_THREADS=1024):
                assert h.msm_plan(SHAPE_A, 11) == dict(p, threads=1024, groups=1)   # 2341 // 3072 = 0 per thread


@pytest.mark.parametrize("batch,blocks", [(2, 10), (64, 8), (100, 5), (160, 10)])
def test_shape_a_default_batches(batch, blocks):
    assert h.msm_plan(SHAPE_A, batch) == {"threads": 256, "blocks": blocks, "groups": 1, "copies": 8, "half": 0}


def test_shape_a_single_msm():
    assert h.msm_plan(SHAPE_A, 1) == {"threads": 256, "blocks": 20, "groups": 1, "copies": 1, "half": 1}
    assert h.msm_plan(SHAPE_A, 1, aligned=False) == {"threads": 256, "blocks": 10, "groups": 1, "copies": 1,
                                                     "half": 0}


@pytest.mark.parametrize("X", (3, 7))
def test_shape_b_512_thread_rows(X):
    with h.options(MSM_MAX_BLOCKS=3 * X):
        assert h.msm_plan(SHAPE_B, 3) == {"threads": 512, "blocks": X, "groups": 2, "copies": 8, "half": 0}


@pytest.mark.parametrize("X", (15, 16, 17, 33))
def test_shape_c_blocks_around_the_shard_count(X):
    """n = 135205: 8450 groups, up to 34 blocks of 256 threads -- block counts on both sides of
    PLK_MSM_SHARDS = 16 (plk_internal.h), which shape A (at most 10 blocks) cannot reach"""
    n = 135205
    assert (n >> 4, n & 15) == (8450, 5) and -(-8450 // 256) == 34
    with h.options(MSM_MAX_BLOCKS=5 * X):
        want_g = 2 if 8450 // (256 * X) >= 2 else 1
        assert want_g == (2 if X <= 16 else 1)
        assert h.msm_plan(n, 5) == {"threads": 256, "blocks": X, "groups": want_g, "copies": 8, "half": 0}


@pytest.mark.parametrize("n", (0, 1, 15, 16, 17, 255))
def test_tiny_rows_one_block(n):
    p = h.msm_plan(n, 9)
    assert (p["threads"], p["blocks"], p["groups"], p["half"]) == (256, 1, 1, 0)
    assert h.msm_plan(n, 9, aligned=False)["blocks"] == 1


def test_headline_shape():
    """160 MSMs of 2^22 points per launch: msm_dlog_kernel<true, 512, 1, 8, false>, 512 blocks per row"""
    assert h.msm_plan(1 << 22, 160) == {"threads": 512, "blocks": 512, "groups": 1, "copies": 8, "half": 0}


def _option_sets(rng, count):
    """_GEOM's settings alone, then random unions of them (a later entry overrides an earlier one)"""
    sets = list(_GEOM)
    while len(sets) < count:
        merged = {}
        for i in rng.choice(len(_GEOM), size=int(rng.integers(2, 4)), replace=False):
            merged.update(_GEOM[int(i)])
        sets.append(merged)
    return sets


def test_invariants_over_a_seeded_sweep():
    """what the kernels rely on, for ~2000 (n, batch, options, aligned) draws: the finish's 16-bit
    per-shard ticket bounds the blocks; the instantiated template values; half groups only for a
    single aligned MSM of one resident round with at most one half group per thread; several groups
    in flight only where every thread has that many whole groups (the kernel's unmasked iterations)"""
    rng = np.random.default_rng(0x9E0)
    before = {k: h.get_option(k) for k in MSM_OPTS}
    draws = 2000
    sets = _option_sets(rng, 40)
    seen_half = seen_multi = seen_bytewise = 0
    for i in range(draws):
        n = int(2.0 ** rng.uniform(0, 26)) - 1 if i % 50 else (0, 1 << 26)[(i // 50) & 1]
        batch = (1, int(2.0 ** rng.uniform(0, 16)), int(rng.integers(1, 65536)))[i % 3]
        batch = min(max(batch, 1), 65535)
        aligned = bool(i % 4)
        opts = sets[i % len(sets)]
        with h.options(**opts):
            p = h.msm_plan(n, batch, aligned)
        ctx = (n, batch, aligned, opts, p)
        groups = n >> 4
        assert 1 <= p["blocks"] <= 8 * 65535, ctx
        assert p["threads"] in (256, 512, 1024), ctx
        assert p["groups"] in (1, 2, 4), ctx
        assert p["copies"] in (1, 8), ctx
        assert p["half"] in (0, 1), ctx
        if "MSM_THREADS" in opts:
            assert p["threads"] == opts["MSM_THREADS"], ctx
        if p["half"]:
            assert batch == 1 and aligned and 2 * groups <= p["blocks"] * p["threads"], ctx
            assert opts.get("MSM_HALF", 1) == 1 and p["groups"] == 1, ctx
            seen_half += 1
        if p["groups"] > 1:
            assert aligned and groups // (p["blocks"] * p["threads"]) >= p["groups"], ctx
            seen_multi += 1
        seen_bytewise += not aligned
    assert seen_half > 20 and seen_multi > 100 and seen_bytewise > 400   # the sweep reaches every form
    assert {k: h.get_option(k) for k in MSM_OPTS} == before


def test_argument_errors():
    import ctypes as C
    out = (C.c_int * 5)(*[-7] * 5)
    lib = h.lib()
    for batch in (0, -1, -65536):
        assert lib.plk_msm_plan(100, batch, 1, out) == h.PLK_ERR_ARG
    assert lib.plk_msm_plan(100, 1, 1, None) == h.PLK_ERR_ARG
    assert "plk_msm_plan" in h.last_error()
    for batch in (65536, 1 << 20, 2 ** 31 - 1):
        assert lib.plk_msm_plan(100, batch, 1, out) == h.PLK_ERR_RANGE
    assert list(out) == [-7] * 5                      # nothing written on an error
    with pytest.raises(h.PlonkHipError) as e:
        h.msm_plan(100, 65536)
    assert e.value.code == h.PLK_ERR_RANGE
    with pytest.raises(h.PlonkHipError) as e:
        h.msm_plan(100, 0)
    assert e.value.code == h.PLK_ERR_ARG
    assert lib.plk_msm_plan(100, 65535, 1, out) == h.PLK_OK and out[1] == 1
