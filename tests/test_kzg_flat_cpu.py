"""KZG flat batches (plk_kzg_flat_plan, plk_kzg_commit_flat*, plk_kzg_open_flat*) without a GPU: the Python model
against the oracle's composition and against the reference's recorded values, the plan, the exports, and every
argument check that comes before any device query."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import kzg_flat_model as FM
from conftest import ROOT, load_golden

NEW = ("plk_kzg_flat_plan", "plk_kzg_commit_flat_dev", "plk_kzg_open_flat_dev", "plk_kzg_commit_flat", "plk_kzg_open_flat")


def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("kzg_flat_plan", "kzg_commit_flat", "kzg_open_flat", "kzg_commit_flat_dev", "kzg_open_flat_dev"):
        assert hasattr(h, name), name
    assert len(h.SIGNATURES["plk_kzg_commit_flat_dev"][1]) == 9
    assert len(h.SIGNATURES["plk_kzg_open_flat_dev"][1]) == 12
    assert len(h.SIGNATURES["plk_kzg_commit_flat"][1]) == 7
    assert len(h.SIGNATURES["plk_kzg_open_flat"][1]) == 10
    with open(os.path.join(ROOT, "include", "plonkhip.h")) as f:
        txt = f.read()
    assert "#define PLK_KZG_FLAT_MAX %d " % h.PLK_KZG_FLAT_MAX in txt
    assert "#define PLK_KZG_FLAT_IRREGULAR %d " % h.PLK_KZG_FLAT_IRREGULAR in txt
    assert "#define PLK_KZG_FLAT_BAD       %d " % h.PLK_KZG_FLAT_BAD in txt
    assert (h.PLK_KZG_FLAT_MAX, h.PLK_KZG_FLAT_IRREGULAR, h.PLK_KZG_FLAT_BAD) == (FM.FLAT_MAX, FM.IRREGULAR, FM.BAD)


def test_model_tables_are_the_group():
    import gen
    assert FM.EXP[0].tolist() == [0, 0, 1]
    assert sorted(map(tuple, FM.EXP.tolist())) == sorted(map(tuple, gen.all_points().tolist()))
    assert [tuple(r) for r in FM.rule_srs(6).tolist()] == [gen.KG[pow(2, i, 17)] for i in range(6)]
    assert FM.srs_logs(FM.rule_srs(40)) is not None
    for bad in ((1, 3, 0), (0, 0, 0), (101, 2, 0), (1, 2, 1), (1, 2, 2)):
        s = FM.rule_srs(5).copy()
        s[3] = bad
        assert FM.srs_logs(s) is None, bad


def test_model_equals_the_oracle_composition(oracle):
    """every length 1 .. 40 at every z: y = poly_eval, q = poly_divide by x - z, proof = msm over q, commitment = msm"""
    srs = FM.rule_srs(40)
    logs = FM.srs_logs(srs)
    for n in range(1, 41):
        r = np.random.default_rng(1000 + n)
        rows = r.integers(0, 17, (17, n)).astype(np.uint8)
        rows[5, -1] = 0                                # an untrimmed top coefficient
        if n > 2:
            rows[6, 1:] = 0                            # a constant in n coefficients
        ys, proofs, commits = FM.open_rows(rows, np.arange(17), logs)
        for z in range(17):
            p = rows[z]
            q, _ = oracle.poly_divide(p, [(17 - z) % 17, 1])
            assert int(ys[z]) == oracle.poly_eval(p, z), (n, z)
            assert proofs[z].tobytes() == oracle.msm(srs[:len(q)], q), (n, z)
            assert commits[z].tobytes() == oracle.msm(srs[:n], p), (n, z)


def test_model_commitment_takes_raw_bytes(oracle):
    srs = FM.rule_srs(40)
    rows = np.random.default_rng(7).integers(0, 256, (8, 40)).astype(np.uint8)
    got = FM.commit_rows(rows, FM.srs_logs(srs))
    for g in range(8):
        assert got[g].tobytes() == oracle.msm(srs, rows[g]), g


def test_model_equals_the_reference_golden():
    cases = load_golden("kzg_flat.json")["cases"]
    assert len(cases) >= 24
    lens = set()
    for c in cases:
        p = np.frombuffer(bytes.fromhex(c["coeffs"]), np.uint8)
        srs = np.frombuffer(bytes.fromhex(c["srs"]), np.uint8).reshape(-1, 3)
        assert srs.shape[0] == p.size and (srs == FM.rule_srs(p.size)).all()
        ys, proofs, commits = FM.open_rows(p[None, :], [c["z"]], FM.srs_logs(srs))
        assert (int(ys[0]), proofs[0].tobytes().hex(), commits[0].tobytes().hex()) == (c["y"], c["proof"], c["commit"]), \
            (p.size, c["z"])
        lens.add(p.size)
    assert {1, 16, 17, 32, 33, 1024, 1025, 4096} <= lens
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kzg_flat.json")) < (1 << 20)


def test_model_device_rules():
    srs = FM.rule_srs(8)
    co = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.uint8)
    # segments: fine, empty, falling, above total, longer than m = 4, fine
    off = [0, 3, 3, 2, 14, 5, 9, 12]
    r = FM.flat_dev(co, 4, 7, srs, zs=[1, 1, 1, 1, 1, 17, 255], offsets=off)
    assert r["status"].tolist() == [0, 2, 2, 2, 2, 2, 2]
    assert all(tuple(x) == FM.FLAGGED for x in r["proofs"][1:].tolist())
    assert all(tuple(x) == FM.FLAGGED for x in r["commits"][1:].tolist())
    r = FM.flat_dev(np.array([1, 2, 200, 4, 5, 6], np.uint8), 3, 2, srs, zs=[3, 4])
    assert r["status"].tolist() == [1, 0] and tuple(r["proofs"][0]) == FM.FLAGGED and tuple(r["commits"][0]) != FM.FLAGGED
    assert r["ys_exact"].tolist() == [False, True]
    bad = srs.copy()
    bad[1] = (1, 3, 0)
    r = FM.flat_dev(np.array([1, 2, 3, 4, 5, 6], np.uint8), 3, 2, bad, zs=[3, 4])
    assert r["status"].tolist() == [1, 1] and r["ys_exact"].all()
    assert r["ys"].tolist() == [(1 + 2 * 3 + 3 * 9) % 17, (4 + 5 * 4 + 6 * 16) % 17]
    assert (r["proofs"] == 0xFF).all() and (r["commits"] == 0xFF).all()
    r = FM.flat_dev(np.array([1, 2, 200, 4, 5, 6], np.uint8), 3, 2, srs)   # commitments only: any byte is exact
    assert r["status"].tolist() == [0, 0] and r["ys"] is None and r["proofs"] is None


def test_model_is_fast_enough_for_the_grid_stride_cases():
    n = 1 << 19
    co = (np.arange(n * 32, dtype=np.uint32) * 2654435761 >> 13).astype(np.uint8) % 17
    t = time.perf_counter()
    r = FM.flat_dev(co, 32, n, FM.rule_srs(32), zs=np.arange(n) % 17)
    dt = time.perf_counter() - t
    assert r["status"].sum() == 0
    assert dt < 5.0, dt          # (well under a second on an idle core; the bound only catches a de-vectorised model)


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("ragged", [0, 1])
@pytest.mark.parametrize("m,path,per", [(1, 0, 256), (32, 0, 256), (33, 1, 4), (1024, 1, 4), (1025, 2, 1), (4096, 2, 1)])
def test_plan_paths(m, path, per, ragged):
    import plonkhip as h
    for npoly in (1, 3, per, per + 1, 3 * per + 1, per * 2048, per * 2048 + 1, 1 << 19):
        p = h.kzg_flat_plan(m, npoly, ragged)
        assert p == FM.plan(m, npoly), (m, npoly)
        assert (p["path"], p["per_block"], p["launches"]) == (path, per, 1)
        assert p["blocks"] == min(-(-npoly // per), 2048)


def test_plan_errors():
    import plonkhip as h
    lib = h.lib()
    out = (C.c_int64 * 4)()
    assert lib.plk_kzg_flat_plan(16, 8, 0, None) == h.PLK_ERR_ARG
    for m, npoly in ((0, 8), (16, 0), (0, 0)):
        for ragged in (0, 1):
            assert lib.plk_kzg_flat_plan(m, npoly, ragged, out) == h.PLK_ERR_ARG, (m, npoly)
    for ragged in (0, 1):
        assert lib.plk_kzg_flat_plan(4097, 8, ragged, out) == h.PLK_ERR_RANGE
        assert "PLK_KZG_FLAT_MAX" in h.last_error()
        assert lib.plk_kzg_flat_plan(1, (1 << 30) + 1, ragged, out) == h.PLK_ERR_RANGE
        assert lib.plk_kzg_flat_plan(1, 1 << 30, ragged, out) == h.PLK_OK
    # uniform: total = m npoly must stay below 2^32; a ragged list's total is not the plan's business
    assert lib.plk_kzg_flat_plan(4096, 1 << 20, 0, out) == h.PLK_ERR_RANGE
    assert "2^32" in h.last_error()
    assert lib.plk_kzg_flat_plan(4096, (1 << 20) - 1, 0, out) == h.PLK_OK
    assert lib.plk_kzg_flat_plan(4096, 1 << 20, 1, out) == h.PLK_OK


# ------------------------------------------------------------------ argument checks, no device
def _opaque_handle():
    """a non-NULL handle of zero bytes (an SRS of no points): shape and pointer checks return before it is read"""
    return (C.c_uint8 * 256)()


class FlatArgs:
    """host blocks standing in for every array: a failing call never reads them"""

    def __init__(self):
        self.co = (C.c_uint8 * 64)()
        self.off = (C.c_uint32 * 5)(0, 16, 32, 48, 64)
        self.zs = (C.c_uint8 * 4)()
        self.ys = (C.c_uint8 * 4)()
        self.pr = (C.c_uint8 * 12)()
        self.cm = (C.c_uint8 * 12)()
        self.st = (C.c_uint8 * 4)()

    def call(self, h, fn, s, total=64, m=16, npoly=4, ragged=False, drop=()):
        a = {k: (None if k in drop else C.addressof(getattr(self, k))) for k in ("co", "zs", "ys", "pr", "cm", "st")}
        p = {k: (None if k in drop else C.cast(getattr(self, k), C.POINTER(C.c_uint8))) for k in ("co", "zs", "ys", "pr", "cm")}
        off_a = C.addressof(self.off) if ragged and "off" not in drop else None
        off_p = self.off if ragged and "off" not in drop else None
        L = h.lib()
        if fn == "commit_dev":
            return L.plk_kzg_commit_flat_dev(s, a["co"], total, off_a, m, npoly, a["cm"], a["st"], None)
        if fn == "open_dev":
            return L.plk_kzg_open_flat_dev(s, a["co"], total, off_a, m, npoly, a["zs"], a["ys"], a["pr"], a["cm"], a["st"], None)
        if fn == "commit":
            return L.plk_kzg_commit_flat(s, p["co"], total, off_p, m, npoly, p["cm"])
        return L.plk_kzg_open_flat(s, p["co"], total, off_p, m, npoly, p["zs"], p["ys"], p["pr"], p["cm"])


FNS = ("commit_dev", "open_dev", "commit", "open")


@pytest.mark.parametrize("fn", FNS)
def test_null_handle_is_arg_error(fn):
    import plonkhip as h
    assert FlatArgs().call(h, fn, None) == h.PLK_ERR_ARG
    assert "plk_kzg_%s_flat" % fn.split("_")[0] in h.last_error()


SHAPES = {
    "npoly0": (dict(npoly=0, total=64), "ARG"),
    "total0": (dict(total=0), "ARG"),
    "m0": (dict(m=0), "ARG"),
    "m0_ragged": (dict(m=0, ragged=True), "ARG"),
    "mismatch": (dict(total=63), "ARG"),
    "mismatch_up": (dict(total=65), "ARG"),
    "m4097": (dict(m=4097, npoly=1, total=4097), "RANGE"),
    "m4097_ragged": (dict(m=4097, ragged=True), "RANGE"),
    "total_2_32": (dict(m=4096, npoly=1 << 20, total=1 << 32), "RANGE"),
    "total_2_32_ragged": (dict(total=1 << 32, ragged=True), "RANGE"),
    "npoly_2_30_1": (dict(m=1, npoly=(1 << 30) + 1, total=(1 << 30) + 1), "RANGE"),
    "npoly_2_30_1_ragged": (dict(npoly=(1 << 30) + 1, ragged=True), "RANGE"),
}


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("case", sorted(SHAPES))
@pytest.mark.parametrize("handle", ["null", "opaque"])
def test_shape_errors_come_before_any_device_query(case, fn, handle):
    """the shape is checked first: the same code with a NULL handle and with one the call must not look into"""
    import plonkhip as h
    fake = _opaque_handle()
    kw, code = SHAPES[case]
    rc = FlatArgs().call(h, fn, None if handle == "null" else C.addressof(fake), **kw)
    assert rc == {"ARG": h.PLK_ERR_ARG, "RANGE": h.PLK_ERR_RANGE}[code], (case, fn)
    assert "plk_kzg_%s_flat" % fn.split("_")[0] in h.last_error()


@pytest.mark.parametrize("fn,drop", [("commit_dev", "co"), ("commit_dev", "cm"), ("commit_dev", "st"), ("open_dev", "co"),
                                     ("open_dev", "zs"), ("open_dev", "ys"), ("open_dev", "pr"), ("open_dev", "st"),
                                     ("commit", "co"), ("commit", "cm"), ("open", "co"), ("open", "zs"), ("open", "ys"),
                                     ("open", "pr")])
def test_null_pointers_are_arg_errors(fn, drop):
    import plonkhip as h
    fake = _opaque_handle()
    assert FlatArgs().call(h, fn, C.addressof(fake), drop=(drop,)) == h.PLK_ERR_ARG
    assert "required" in h.last_error()


@pytest.mark.parametrize("fn", ("commit_dev", "open_dev"))
def test_misaligned_offsets_are_arg_errors(fn):
    import plonkhip as h
    fake = _opaque_handle()
    a = FlatArgs()
    L = h.lib()
    off = C.addressof(a.off) + 2
    if fn == "commit_dev":
        rc = L.plk_kzg_commit_flat_dev(C.addressof(fake), C.addressof(a.co), 64, off, 16, 2, C.addressof(a.cm), C.addressof(a.st), None)
    else:
        rc = L.plk_kzg_open_flat_dev(C.addressof(fake), C.addressof(a.co), 64, off, 16, 2, C.addressof(a.zs), C.addressof(a.ys),
                                     C.addressof(a.pr), None, C.addressof(a.st), None)
    assert rc == h.PLK_ERR_ARG and "4-byte aligned" in h.last_error()


HOST_LISTS = {
    "empty": ([0, 16, 16, 48, 64], None),
    "falling": ([0, 16, 8, 48, 64], None),
    "above_total": ([0, 16, 32, 48, 65], None),
    "longer_than_m": ([0, 16, 33, 48, 64], None),
    "z17": (None, [0, 17, 0, 0]),
    "z255": (None, [0, 0, 0, 255]),
}


@pytest.mark.parametrize("case,fn", [(c, f) for c in sorted(HOST_LISTS) for f in ("commit", "open")
                                     if f == "open" or HOST_LISTS[c][1] is None])   # (a commitment takes no z)
def test_host_forms_validate_offsets_and_points_before_any_device_query(case, fn):
    import plonkhip as h
    off, zs = HOST_LISTS[case]
    fake = _opaque_handle()
    a = FlatArgs()
    if off is not None:
        a.off[:] = off
    if zs is not None:
        a.zs[:] = zs
    assert a.call(h, fn, C.addressof(fake), ragged=True) == h.PLK_ERR_ARG, case
    assert "plk_kzg_%s_flat" % fn in h.last_error()


@pytest.mark.parametrize("fn", FNS)
def test_range_error_of_a_zeroed_handle(fn):
    """a call that passes every argument check reaches the SRS bound, which a handle of zero bytes (an SRS of no
    points) fails with the reference's text -- still before any device query"""
    import plonkhip as h
    fake = _opaque_handle()
    assert FlatArgs().call(h, fn, C.addressof(fake)) == h.PLK_ERR_RANGE
    assert "degree exceeds SRS size" in h.last_error()
