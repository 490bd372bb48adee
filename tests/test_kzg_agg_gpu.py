"""KZG aggregate verification (plk_kzg_verify_agg_batch*) on the GPU.

Expected values are the reference's verdicts recorded in tests/golden/kzg_agg.json and the two Python models
of tests/kzg_agg_model.py (pinned to that file by tests/test_kzg_agg_cpu.py) where a test needs a shape the
file does not hold; every expectation is asserted on the model before the library is asked.  Everything is
exact: bytes are compared for equality.  Group sizes at which the code takes another path are found by
calling the plan, never copied from the source."""
import numpy as np
import pytest

import gen
import kzg_agg_model as A
import make_kzg_agg_golden as mk
from conftest import load_golden

pytestmark = pytest.mark.gpu

GUARD = 32
MAX_JOBS = 1 << 30
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257]
NS = [1, 2, 257]
OFF_CURVE, FLAGGED = (5, 5, 0), (1, 2, 1)      # valid encodings that are no canonical group element


# ------------------------------------------------------------------ inputs, shared and never modified
class Pool:
    """2^20 + 1 seeded regular jobs over all 102 elements under the key {(1, 2), H, 2 H}; every test takes a
    prefix or a slice of it (copies), so the bytes are built once"""

    def __init__(self):
        g = load_golden("pairing.json")["g2_multiples"]
        self.key = ((1, 2, 0), tuple(bytes.fromhex(g["1"])), tuple(bytes.fromhex(g["2"])))
        e = (1 << 20) + 1
        r = gen.splitmix64(0xA66, 5 * e)
        pts = gen.all_points()
        self.c = pts[(r[:e] % np.uint64(102)).astype(np.int64)]
        self.w = pts[(r[e:2 * e] % np.uint64(102)).astype(np.int64)]
        self.z, self.y, self.r = ((r[(2 + i) * e:(3 + i) * e] % np.uint64(17)).astype(np.uint8) for i in range(3))
        assert {tuple(p) for p in self.c[:4096].tolist()} == {tuple(p) for p in pts.tolist()}

    def take(self, e, start=0):
        s = slice(start, start + e)
        return {"c": self.c[s].copy(), "w": self.w[s].copy(), "z": self.z[s].copy(), "y": self.y[s].copy(),
                "r": self.r[s].copy()}


@pytest.fixture(scope="module")
def pool():
    return Pool()


def vk_of(hip, key):
    return hip.KzgVk(*key)


def model_log(key, m, d):
    return A.agg_log(key, m, d["c"], d["z"], d["y"], d["w"], d["r"])


def model_raw(key, m, d):
    return A.agg_raw_flat(key, m, d["c"], d["z"], d["y"], d["w"], d["r"])


def on_device(a, offset=0, fill=None, guard=0):
    """a byte array on the device starting `offset` bytes past a 16-byte boundary (fill: an output block of
    that many 0xEE bytes instead, with `guard` more behind it)"""
    import torch
    n = a if fill else a.size
    t = torch.full((offset + n + guard + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    if not fill:
        t[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    return t[offset:]


def taken(t, n):
    """the n output bytes of block t, after checking that the guard behind them is untouched"""
    h = t[:n + GUARD].cpu().numpy()
    assert (h[n:n + GUARD] == 0xEE).all(), "wrote past the output"
    return h[:n].copy()


def poisoned_work(hip, m, n):
    import torch
    ws = hip.kzg_verify_agg_workspace(m, n)
    assert (ws == 0) == (hip.kzg_verify_agg_plan(m, n)["launches"] == 1)
    return torch.full((ws,), 0xEE, dtype=torch.uint8, device="cuda") if ws else None


def stage(d, offset=0):
    return {k: on_device(d[k], offset) for k in ("c", "z", "y", "w", "r")}


def launch(hip, vk, m, n, dd, ok, work, stream=None):
    hip.kzg_verify_agg_dev(vk, m, dd["c"], dd["z"], dd["y"], dd["w"], dd["r"], n, ok, work=work, stream=stream)


def agg_dev(hip, key, m, d, offset=0, stream=None):
    import torch
    n = d["z"].size // m
    dd = stage(d, offset)
    ok = on_device(n, offset, fill=True, guard=GUARD)
    work = poisoned_work(hip, m, n)
    torch.cuda.synchronize()
    launch(hip, vk_of(hip, key), m, n, dd, ok, work, stream)
    torch.cuda.synchronize()
    return taken(ok, n)


def agg_host(hip, key, m, d):
    return hip.kzg_verify_agg(vk_of(hip, key), m, d["c"], d["z"], d["y"], d["w"], d["r"])


def agg_both(hip, key, m, d, form):
    return agg_host(hip, key, m, d) if form == "host" else agg_dev(hip, key, m, d)


def path_bounds(hip):
    """{path: (smallest m, largest m)} by bisection on the plan (the path never falls as m grows)"""
    def first_with(pred):
        lo, hi = 1, MAX_JOBS + 1            # pred is false below the answer, true from it on; hi: none
        while lo < hi:
            mid = (lo + hi) // 2
            if pred(hip.kzg_verify_agg_plan(mid, 1)):
                hi = mid
            else:
                lo = mid + 1
        return lo
    paths = sorted({hip.kzg_verify_agg_plan(m, 1)["path"] for m in (1, MAX_JOBS)} |
                   {hip.kzg_verify_agg_plan(1 << k, 1)["path"] for k in range(31)})
    starts = {p: first_with(lambda pl, p=p: pl["path"] >= p) for p in paths}
    return {p: (starts[p], (starts[paths[i + 1]] - 1) if i + 1 < len(paths) else MAX_JOBS) for i, p in enumerate(paths)}


def first_m_with_slices(hip, k):
    lo, hi = 1, MAX_JOBS
    while lo < hi:
        mid = (lo + hi) // 2
        if hip.kzg_verify_agg_plan(mid, 1)["slices"] >= k:
            hi = mid
        else:
            lo = mid + 1
    assert hip.kzg_verify_agg_plan(lo, 1)["slices"] >= k
    return lo


def one_m_per_path(hip):
    """a group size inside every path the plan reports, none a multiple of 16, plus one of three blocks"""
    ms = []
    for lo, hi in path_bounds(hip).values():
        m = min(lo + 37, hi)
        ms.append(m if m % 16 else m - 1)
    return sorted(set(ms + [first_m_with_slices(hip, 3) + 5]))


def positions(hip, m):
    """first job, last job, and the jobs on either side of a thread-step, block-step and slice edge"""
    b = hip.kzg_verify_agg_plan(m, 1)["slices"]
    per = ((-(-m // b) + 15) & ~15) if b else m
    edge = [p for p in (255, 256, 4095, 4096, per - 1, per) if 0 < p < m - 1]
    return {"first": [0], "block_edge": edge[-2:] if edge else [m // 2], "last": [m - 1]}


# ------------------------------------------------------------------ the goldens
@pytest.fixture(scope="module")
def gold():
    cases = []
    for c in load_golden("kzg_agg.json")["cases"]:
        d = mk.case_inputs(c["kind"], c["m"], c["seed"], c["groups"])
        cases.append((c["kind"], c["m"], mk.key_of(d["vk"]), d, np.array([int(b) for b in c["bits"]], np.uint8)))
    return cases


@pytest.mark.parametrize("form", ["host", "dev"])
def test_golden_groups(hip, gold, form):
    """regular groups: the reference's bit in both forms; raw groups: 3 from the _dev form, the bit from the host form"""
    assert sorted({(k, m) for k, m, *_ in gold}) == sorted([("regular", m) for m in (1, 2, 3, 16, 17, 65)] +
                                                           [("raw", m) for m in (1, 2, 5, 33)])
    for kind, m, key, d, bits in gold:
        log = model_log(key, m, d)
        if kind == "regular":
            assert np.array_equal(log, bits)
        else:
            assert (log == A.UNDECIDED).sum() > len(bits) * 3 // 4 and np.array_equal(model_raw(key, m, d), bits)
        exp = bits if form == "host" else np.where(log == A.UNDECIDED, A.UNDECIDED, bits)
        got = agg_both(hip, key, m, d, form)
        assert np.array_equal(got, exp), (kind, m, np.flatnonzero(got != exp)[:8], got[got != exp][:8])


# ------------------------------------------------------------------ group sizes
@pytest.mark.parametrize("m", SIZES)
def test_group_sizes(hip, pool, m):
    for n in NS:
        d = pool.take(m * n, start=3 * n)
        exp = model_log(pool.key, m, d)
        if n == 257:
            assert 0 < int(exp.sum()) < n and exp.max() == 1
        assert np.array_equal(agg_dev(hip, pool.key, m, d), exp), (m, n)
    assert np.array_equal(agg_host(hip, pool.key, m, d), exp), m


def test_every_path_at_its_edges(hip, pool):
    """the smallest and the largest m of every path the plan reports, and their neighbours, n = 1 and 2; group
    sizes beyond the pool (the last path ends at 2^30 jobs) repeat the pool's bytes on the device and take
    the model's sums tile by tile"""
    import torch
    bounds = path_bounds(hip)
    assert len(bounds) >= 2 and min(lo for lo, _ in bounds.values()) == 1 and max(hi for _, hi in bounds.values()) == MAX_JOBS
    ms = sorted({m for lo, hi in bounds.values() for m in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1) if 1 <= m <= MAX_JOBS})
    assert {hip.kzg_verify_agg_plan(m, 1)["path"] for m in ms} == set(bounds)
    tile = 1 << 20
    for m in ms:
        for n in (1, 2):
            if m * n <= pool.z.size:
                d = pool.take(m * n, start=n)
                exp = model_log(pool.key, m, d)
                assert np.array_equal(agg_dev(hip, pool.key, m, d), exp), (m, n)
            elif n == 1:
                t = pool.take(tile)
                exp = A.agg_log_tiled(pool.key, m, t["c"], t["z"], t["y"], t["w"], t["r"])
                reps = -(-m // tile)
                dd = {k: torch.from_numpy(t[k].reshape(-1)).cuda().repeat(reps) for k in t}
                ok = on_device(1, fill=True, guard=GUARD)
                work = poisoned_work(hip, m, 1)
                torch.cuda.synchronize()
                launch(hip, vk_of(hip, pool.key), m, 1, dd, ok, work)
                torch.cuda.synchronize()
                assert np.array_equal(taken(ok, 1), exp), m
                del dd, work


def test_slice_counts_at_their_edges(hip, pool):
    """where the plan goes from one block per group to two and from two to three"""
    for k in (2, 3):
        m0 = first_m_with_slices(hip, k)
        for m in (m0 - 1, m0, m0 + 1):
            for n in (1, 2):
                d = pool.take(m * n, start=7)
                assert np.array_equal(agg_dev(hip, pool.key, m, d), model_log(pool.key, m, d)), (m, n)


def test_a_group_of_at_least_three_blocks(hip, pool):
    m = first_m_with_slices(hip, 3) + 5
    p = hip.kzg_verify_agg_plan(m, 2)
    assert p["slices"] >= 3 and p["launches"] == 2 and m * 2 <= pool.z.size
    d = pool.take(2 * m)
    exp = model_log(pool.key, m, d)
    for form in ("dev", "host"):
        assert np.array_equal(agg_both(hip, pool.key, m, d, form), exp), form


def test_a_million_jobs_as_one_group_and_as_pairs(hip, pool):
    e = (1 << 20) + 1
    d = pool.take(e)
    exp = model_log(pool.key, e, d)
    assert np.array_equal(agg_dev(hip, pool.key, e, d), exp)
    d = pool.take(e - 1)
    exp = model_log(pool.key, 2, d)
    assert 0 < int(exp.sum()) < exp.size and exp.max() == 1
    got = agg_dev(hip, pool.key, 2, d)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]


def test_many_groups_on_the_two_launch_paths(hip, pool):
    """thousands of groups on every path with a second launch (one lane per group finishes them there, a wave
    per group where the groups are few); the larger call repeats the pool's bytes"""
    bounds = path_bounds(hip)
    for path, n in ((1, 20000), (2, 4500)):
        m = bounds[path][0] + 3
        assert hip.kzg_verify_agg_plan(m, n) == dict(hip.kzg_verify_agg_plan(m, 1), blocks=hip.kzg_verify_agg_plan(m, n)["blocks"])
        d = {k: np.resize(v, (m * n,) + v.shape[1:]) for k, v in pool.take(pool.z.size).items()}
        exp = model_log(pool.key, m, d)
        assert 0 < int(exp.sum()) < n and exp.max() == 1
        got = agg_dev(hip, pool.key, m, d)
        assert np.array_equal(got, exp), (m, n, np.flatnonzero(got != exp)[:8])


# ------------------------------------------------------------------ m = 1, r = 1
def test_groups_of_one_under_weight_one_are_verify_batch(hip):
    g = load_golden("pairing.json")
    bits = np.unpackbits(np.frombuffer(bytes.fromhex(g["verify_exhaustive"]["bits"]), np.uint8), bitorder="little")[:17 ** 4]
    kg = np.array(gen.KG, np.uint8)
    c, w, z, y = (v.reshape(-1) for v in np.meshgrid(*[np.arange(17)] * 4, indexing="ij"))
    key = mk.key_of(bytes.fromhex(g["verify_exhaustive"]["vk"]))
    d = {"c": kg[c], "w": kg[w], "z": z.astype(np.uint8), "y": y.astype(np.uint8), "r": np.ones(z.size, np.uint8)}
    assert np.array_equal(model_log(key, 1, d), bits)
    per_job = hip.kzg_verify(vk_of(hip, key), d["c"], d["z"], d["y"], d["w"])
    assert np.array_equal(per_job, bits)
    for form in ("dev", "host"):
        assert np.array_equal(agg_both(hip, key, 1, d, form), per_job), form


# ------------------------------------------------------------------ end to end with commit and open
E2E_LENGTHS = [1, 2, 3, 17, 4097]
E2E_ZS = [0, 1, 2, 5, 16]


@pytest.fixture(scope="module")
def e2e(hip, pool):
    """a well-formed SRS for s = 2, srs[i] = (2^i mod 17) G, and the library's own commitments and openings of
    every (polynomial, z), as flat job arrays with seeded non-zero weights"""
    g1 = load_golden("g1.json")["kG_k0_17"]
    srs_pts = np.array([list(bytes.fromhex(g1[pow(2, i, 17)])) for i in range(max(E2E_LENGTHS))], np.uint8)
    polys = [gen.poly_inputs(0xE2E + n, n, 0)[0] for n in E2E_LENGTHS]
    with hip.Srs(srs_pts) as srs:
        assert not srs.irregular
        commits = hip.kzg_commit(srs, polys)
        jobs = [(i, z) for i in range(len(polys)) for z in E2E_ZS]
        ys, proofs = hip.kzg_open(srs, [polys[i] for i, _ in jobs], [z for _, z in jobs])
    r = (gen.splitmix64(0xE2E, len(jobs)) % np.uint64(16)).astype(np.uint8) + np.uint8(1)
    return {"c": np.array([list(commits[i]) for i, _ in jobs], np.uint8), "w": np.array([list(p) for p in proofs], np.uint8),
            "z": np.array([z for _, z in jobs], np.uint8), "y": np.array(ys, np.uint8), "r": r}


@pytest.mark.parametrize("form", ["host", "dev"])
def test_the_librarys_openings_aggregate(hip, pool, e2e, form):
    k = e2e["z"].size
    assert k == 25 and e2e["r"].min() >= 1
    for m in (k, 5, 1):
        assert model_raw(pool.key, m, e2e).tolist() == [1] * (k // m)
        assert agg_both(hip, pool.key, m, e2e, form).tolist() == [1] * (k // m), m


@pytest.mark.parametrize("form", ["host", "dev"])
def test_a_wrong_value_counts_only_under_a_non_zero_weight(hip, pool, e2e, form):
    for j in (0, 12, 24):
        bad = {k: v.copy() for k, v in e2e.items()}
        bad["y"][j] = (bad["y"][j] + 1) % 17
        assert bad["r"][j] != 0
        assert model_raw(pool.key, 25, bad).tolist() == [0]
        assert agg_both(hip, pool.key, 25, bad, form).tolist() == [0], j
        exp5 = [int(g != j // 5) for g in range(5)]
        assert model_raw(pool.key, 5, bad).tolist() == exp5
        assert agg_both(hip, pool.key, 5, bad, form).tolist() == exp5, j
        bad["r"][j] = 0
        assert model_raw(pool.key, 25, bad).tolist() == [1]
        assert agg_both(hip, pool.key, 25, bad, form).tolist() == [1], j


# ------------------------------------------------------------------ invalid bytes, non-canonical points and keys
INVALID = {"c_x_101": ("c", 0, 101), "c_flag_2": ("c", 2, 2), "w_y_255": ("w", 1, 255), "w_flag_2": ("w", 2, 2),
           "z_17": ("z", None, 17), "y_255": ("y", None, 255), "r_17": ("r", None, 17)}


def three_groups(hip, pool, m, which, where, edit):
    """(inputs, model bytes of the untouched call, the touched group) for the three-group call with `edit` applied at
    every job position `where` names in group `which`"""
    d = pool.take(3 * m, start=11)
    base = model_log(pool.key, m, d)
    for p in positions(hip, m)[where]:
        edit(d, which * m + p)
    return d, base


@pytest.mark.parametrize("where", ["first", "block_edge", "last"])
@pytest.mark.parametrize("kind", sorted(INVALID))
def test_invalid_byte_marks_its_group_only(hip, pool, kind, where):
    arr, col, val = INVALID[kind]

    def edit(d, j):
        if col is None:
            d[arr][j] = val
        else:
            d[arr][j, col] = val

    for i, m in enumerate(one_m_per_path(hip)):
        which = i % 3
        d, exp = three_groups(hip, pool, m, which, where, edit)
        exp = exp.copy()
        exp[which] = 2
        assert np.array_equal(model_log(pool.key, m, d), exp)
        for form in ("dev", "host"):
            assert np.array_equal(agg_both(hip, pool.key, m, d, form), exp), (m, form)


@pytest.mark.parametrize("where", ["first", "block_edge", "last"])
@pytest.mark.parametrize("kind", ["c_off_curve", "w_flagged"])
def test_non_canonical_point_leaves_its_group_undecided(hip, pool, kind, where):
    arr, val = ("c", OFF_CURVE) if kind == "c_off_curve" else ("w", FLAGGED)

    def edit(d, j):
        d[arr][j] = val

    for i, m in enumerate(one_m_per_path(hip)):
        which = (i + 1) % 3
        d, exp = three_groups(hip, pool, m, which, where, edit)
        dev = exp.copy()
        dev[which] = A.UNDECIDED
        assert np.array_equal(model_log(pool.key, m, d), dev)
        assert np.array_equal(agg_dev(hip, pool.key, m, d), dev), m
        host = exp.copy()
        g = slice(which * m, (which + 1) * m)
        host[which] = A.agg_raw(pool.key, list(zip(d["c"][g], d["w"][g], d["z"][g], d["y"][g], d["r"][g])))
        assert np.array_equal(agg_host(hip, pool.key, m, d), host), m


@pytest.mark.parametrize("g1", [OFF_CURVE, FLAGGED])
def test_non_canonical_key(hip, pool, g1):
    key = (g1,) + pool.key[1:]
    for m, n in ((3, 9), (70, 5)):
        d = pool.take(m * n, start=5)
        d["z"][0] = 17                                    # an invalid byte is still 2
        dev = np.full(n, A.UNDECIDED, np.uint8)
        dev[0] = 2
        assert np.array_equal(model_log(key, m, d), dev)
        assert np.array_equal(agg_dev(hip, key, m, d), dev), m
        exp = model_raw(key, m, d)
        assert exp[0] == 2 and exp[1:].max() <= 1
        assert np.array_equal(agg_host(hip, key, m, d), exp), m


# ------------------------------------------------------------------ device-buffer edges
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_unaligned_device_buffers_and_guards(hip, pool, offset):
    """all five inputs and ok `offset` bytes past a 16-byte boundary, 0xEE behind ok and all over the workspace"""
    for m in one_m_per_path(hip) + [16, 64]:
        d = pool.take(3 * m, start=offset)
        assert np.array_equal(agg_dev(hip, pool.key, m, d, offset), model_log(pool.key, m, d)), m


# ------------------------------------------------------------------ streams, workspaces, determinism
def test_non_default_stream(hip, pool):
    import torch
    s = torch.cuda.Stream()
    for m in one_m_per_path(hip):
        d = pool.take(3 * m)
        assert np.array_equal(agg_dev(hip, pool.key, m, d, stream=s), model_log(pool.key, m, d)), m


def test_two_streams_two_workspaces(hip, pool):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    m = first_m_with_slices(hip, 3) + 5
    a, b = pool.take(3 * m), pool.take(3 * m, start=3 * m)
    da, db = stage(a), stage(b)
    oa, ob = on_device(3, fill=True, guard=GUARD), on_device(3, fill=True, guard=GUARD)
    wa, wb = poisoned_work(hip, m, 3), poisoned_work(hip, m, 3)
    vk = vk_of(hip, pool.key)
    torch.cuda.synchronize()
    launch(hip, vk, m, 3, da, oa, wa, s1)
    launch(hip, vk, m, 3, db, ob, wb, s2)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(taken(oa, 3), model_log(pool.key, m, a))
    assert np.array_equal(taken(ob, 3), model_log(pool.key, m, b))


def test_workspace_reused_by_a_call_of_another_shape(hip, pool):
    import torch
    m1, n1 = first_m_with_slices(hip, 3) + 5, 3
    m2, n2 = path_bounds(hip)[1][0] + 3, 700
    work = torch.full((max(hip.kzg_verify_agg_workspace(m1, n1), hip.kzg_verify_agg_workspace(m2, n2)),), 0xEE,
                      dtype=torch.uint8, device="cuda")
    a, b = pool.take(m1 * n1), pool.take(m2 * n2, start=9)
    da, db = stage(a), stage(b)
    oa, ob, oc = (on_device(n, fill=True, guard=GUARD) for n in (n1, n2, n1))
    vk = vk_of(hip, pool.key)
    torch.cuda.synchronize()
    launch(hip, vk, m1, n1, da, oa, work)
    launch(hip, vk, m2, n2, db, ob, work)
    launch(hip, vk, m1, n1, da, oc, work)
    torch.cuda.synchronize()
    assert np.array_equal(taken(oa, n1), model_log(pool.key, m1, a))
    assert np.array_equal(taken(ob, n2), model_log(pool.key, m2, b))
    assert np.array_equal(taken(oc, n1), taken(oa, n1))


def test_repeated_calls_give_identical_bytes(hip, pool):
    for m in one_m_per_path(hip):
        d = pool.take(5 * m, start=1)
        first = agg_dev(hip, pool.key, m, d)
        assert np.array_equal(agg_dev(hip, pool.key, m, d), first)
        assert np.array_equal(agg_dev(hip, pool.key, m, d, offset=1), first)
        assert np.array_equal(agg_host(hip, pool.key, m, d), first)
