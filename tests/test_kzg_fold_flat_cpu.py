"""KZG flat folded openings (plk_kzg_fold_flat_plan, plk_kzg_open_fold_flat*) without a GPU: the Python model
against kzg_fold_model.open_fold (which tests/golden/kzg_fold.json pins to the compiled reference) and against the
oracle's composition, the model's linearity identity and status rules, the plan, the exports, and every argument
check that comes before any device query, in the order the header states."""
import ctypes as C
import os

import numpy as np
import pytest

import kzg_flat_model as FM
import kzg_fold_flat_model as FF
import kzg_fold_model as F
from conftest import ROOT

NEW = ("plk_kzg_fold_flat_plan", "plk_kzg_open_fold_flat_dev", "plk_kzg_open_fold_flat")


def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("kzg_fold_flat_plan", "kzg_open_fold_flat", "kzg_open_fold_flat_dev"):
        assert hasattr(h, name), name
    assert len(h.SIGNATURES["plk_kzg_fold_flat_plan"][1]) == 5
    assert len(h.SIGNATURES["plk_kzg_open_fold_flat_dev"][1]) == 14
    assert len(h.SIGNATURES["plk_kzg_open_fold_flat"][1]) == 12
    with open(os.path.join(ROOT, "include", "plonkhip.h")) as f:
        txt = f.read()
    assert "#define PLK_KZG_FOLD_MAX %d " % FF.FOLD_MAX in txt
    assert "KZG flat folded openings" in txt
    assert (FF.LANE_MAX, FF.WAVE_MAX, FF.GRID_CAP, FF.PER_BLOCK) == (32, 1024, 2048, (256, 4, 1))


def test_python_wrapper_checks_its_lists():
    import plonkhip as h
    with pytest.raises(ValueError):
        h.kzg_open_fold_flat(None, np.zeros(12, np.uint8), 5, [1] * 3, [0], m=4)      # k does not divide npoly
    with pytest.raises(ValueError):
        h.kzg_open_fold_flat(None, np.zeros(12, np.uint8), 3, [1] * 2, [0], m=4)      # a weight per polynomial
    with pytest.raises(ValueError):
        h.kzg_open_fold_flat(None, np.zeros(12, np.uint8), 3, [1] * 3, [0, 1], m=4)   # a z per group


# ------------------------------------------------------------------ the model
def mixed_group(seed, k, maxlen=40):
    """k polynomials of lengths 1 .. maxlen (mixed, the longest first or last by turns), weights with zeros"""
    r = np.random.default_rng(0xF01D + seed)
    lens = r.integers(1, maxlen + 1, k).tolist()
    lens[seed % k] = maxlen if seed % 3 else 1 + seed % maxlen
    polys = [r.integers(0, 17, n).astype(np.uint8) for n in lens]
    w = r.integers(0, 17, k).astype(np.uint8)
    if seed % 4 == 0:
        w[r.integers(0, k)] = 0
    return polys, w


def as_flat(groups):
    polys = [p for g in groups for p in g]
    off = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.uint32)
    return np.concatenate(polys).astype(np.uint8), off


def model_of(groups, weights, zs, srs, m):
    co, off = as_flat(groups)
    k = len(groups[0])
    return FF.fold_flat_dev(co, m, k, len(groups), srs, np.concatenate(weights), zs, offsets=off)


def check_group(oracle, srs, polys, w, z, ys, proof, commits, what):
    """one group of the model against kzg_fold_model.open_fold and against the oracle's composition"""
    eys, Fb, eproof = F.open_fold(srs, polys, w, z)
    assert ys.tolist() == eys and tuple(proof.tolist()) == tuple(eproof), what
    for p, y, c in zip(polys, ys, commits):
        assert int(y) == oracle.poly_eval(p, z), what
        assert c.tobytes() == oracle.msm(srs[:len(p)], p), what
    q, _ = oracle.poly_divide(Fb, [(17 - z) % 17, 1])
    q = np.frombuffer(bytes(q), np.uint8) if len(q) else np.zeros(1, np.uint8)
    assert proof.tobytes() == oracle.msm(srs[:len(q)], q), what


@pytest.mark.parametrize("k", range(1, 17))
def test_model_equals_the_fold_model_and_the_oracle(oracle, k):
    """every k, lengths 1 .. 40 mixed inside a group, every z, weights with zeros"""
    srs = FM.rule_srs(40)
    groups, weights = zip(*[mixed_group(100 * k + z, k) for z in range(17)])
    zs = np.arange(17)
    r = model_of(groups, weights, zs, srs, 40)
    assert r["status"].sum() == 0 and r["ys_exact"].all()
    for g in range(17):
        sl = slice(k * g, k * (g + 1))
        check_group(oracle, srs, groups[g], weights[g], g, r["ys"][sl], r["proofs"][g], r["commits"][sl], (k, g))


def test_model_degenerate_groups(oracle):
    """all weights zero, the cancelling pair (p, p under 1 and 16), F cancelling only its top, L = 1"""
    srs = FM.rule_srs(40)
    r = np.random.default_rng(5)
    p = r.integers(1, 17, 23).astype(np.uint8)
    top = p.copy()
    top[:9] = r.integers(0, 17, 9)                        # equal above coefficient 8: F keeps degree <= 8
    one = [np.array([5], np.uint8), np.array([7], np.uint8)]
    for z in range(17):
        groups = [[p, r.integers(0, 17, 30).astype(np.uint8)], [p, p], [p, top], one]
        weights = [np.array(w, np.uint8) for w in ([0, 0], [1, 16], [1, 16], [3, 4])]
        res = model_of(groups, weights, [z] * 4, srs, 40)
        assert res["status"].sum() == 0
        for g in range(4):
            sl = slice(2 * g, 2 * g + 2)
            check_group(oracle, srs, groups[g], weights[g], z, res["ys"][sl], res["proofs"][g], res["commits"][sl], (z, g))
        assert res["proofs"][[0, 1, 3]].tolist() == [[0, 0, 1]] * 3      # F = 0, F = 0, L = 1: the identity
        assert res["ys"][6:8].tolist() == [5, 7]


def test_model_linearity_identity():
    """over a regular SRS the folded proof is the raw fold of g1_mul(W_i, w_i) over the per-polynomial proofs"""
    srs = FM.rule_srs(40)
    logs = FM.srs_logs(srs)
    for k in (1, 2, 9, 16):
        groups, weights = zip(*[mixed_group(7000 + 31 * k + z, k) for z in range(17)])
        r = model_of(groups, weights, np.arange(17), srs, 40)
        for g in range(17):
            rows = np.zeros((k, 40), np.uint8)
            for i, p in enumerate(groups[g]):
                rows[i, :len(p)] = p
            ys, W, _ = FM.open_rows(rows, [g] * k, logs, want_commits=False)
            assert ys.tolist() == r["ys"][k * g:k * (g + 1)].tolist()
            assert tuple(r["proofs"][g].tolist()) == tuple(F.fold_commitments(W.tolist(), weights[g].tolist())), (k, g)


def test_model_status_rules():
    srs = FM.rule_srs(8)
    co = (np.arange(24) % 17).astype(np.uint8)
    # k = 2, m = 4; groups: fine, an empty polynomial, a falling one, above total, longer than m, z = 17, weight 17,
    # weight 255, fine
    off = np.array([0, 3, 4, 4, 6, 5, 7, 30, 9, 14, 15, 17, 18, 19, 20, 21, 22, 23, 24], np.uint32)
    zs = np.array([1, 1, 1, 1, 1, 17, 2, 3, 4])
    w = np.ones(18, np.uint8)
    w[12], w[15] = 17, 255
    r = FF.fold_flat_dev(co, 4, 2, 9, srs, w, zs, offsets=off)
    assert r["status"].tolist() == [0, 2, 2, 2, 2, 2, 2, 2, 0]
    bad = list(range(1, 8))
    assert (r["proofs"][bad] == 0xFF).all()
    assert (r["ys"].reshape(9, 2)[bad] == 0xFF).all() and (r["commits"].reshape(9, 2, 3)[bad] == 0xFF).all()
    assert (r["commits"].reshape(9, 2, 3)[[0, 8]] != 0xFF).any(axis=2).all()
    # a coefficient byte >= 17: the group IRREGULAR, its commitments exact, its ys unspecified
    co2 = np.array([1, 2, 200, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.uint8)
    r = FF.fold_flat_dev(co2, 3, 2, 2, srs, [1, 2, 3, 4], [3, 4])
    assert r["status"].tolist() == [1, 0] and tuple(r["proofs"][0]) == FF.FLAGGED
    assert (r["commits"] != 0xFF).any(axis=1).all()
    assert r["commits"].tolist() == FM.commit_rows(co2.reshape(4, 3), FM.srs_logs(srs)).tolist()
    assert r["ys_exact"].tolist() == [False, False, True, True]
    # an SRS without log form: every group IRREGULAR, every G1 FF FF FF, the ys exact
    bad_srs = srs.copy()
    bad_srs[1] = (1, 3, 0)
    co3 = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.uint8)
    r = FF.fold_flat_dev(co3, 3, 2, 2, bad_srs, [1, 2, 3, 4], [3, 4])
    assert r["status"].tolist() == [1, 1] and r["ys_exact"].all()
    assert r["ys"].tolist() == [(1 + 2 * 3 + 3 * 9) % 17, (4 + 5 * 3 + 6 * 9) % 17, (7 + 8 * 4 + 9 * 16) % 17,
                                (10 + 11 * 4 + 12 * 16) % 17]
    assert (r["proofs"] == 0xFF).all() and (r["commits"] == 0xFF).all()


def test_model_expanded():
    co = np.arange(12, dtype=np.uint8)
    g = FF.expanded(co, 2, 3, 2)
    assert [[p.tolist() for p in grp] for grp in g] == [[[0, 1], [2, 3], [4, 5]], [[6, 7], [8, 9], [10, 11]]]


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("ragged", [0, 1])
@pytest.mark.parametrize("m,path", [(1, 0), (FF.LANE_MAX, 0), (FF.LANE_MAX + 1, 1), (FF.WAVE_MAX, 1), (FF.WAVE_MAX + 1, 2),
                                    (FM.FLAT_MAX, 2)])
def test_plan_paths(m, path, ragged):
    import plonkhip as h
    per = FF.PER_BLOCK[path]
    for k in (1, 9, 16):
        for ng in (1, 3, per, per + 1, 3 * per + 1, per * FF.GRID_CAP, per * FF.GRID_CAP + 1):
            if m * k * ng >= 1 << 32 and not ragged:
                continue
            p = h.kzg_fold_flat_plan(m, k, ng, ragged)
            assert p == FF.plan(m, k, ng), (m, k, ng)
            assert (p["path"], p["per_block"], p["launches"]) == (path, per, 1)
            assert p["blocks"] == min(-(-ng // per), FF.GRID_CAP)


def test_plan_errors():
    import plonkhip as h
    lib = h.lib()
    out = (C.c_int64 * 4)()
    assert lib.plk_kzg_fold_flat_plan(16, 2, 8, 0, None) == h.PLK_ERR_ARG
    for ragged in (0, 1):
        for m, k, ng in ((0, 2, 8), (16, 0, 8), (16, 2, 0), (0, 0, 0), (16, 17, 8)):
            assert lib.plk_kzg_fold_flat_plan(m, k, ng, ragged, out) == h.PLK_ERR_ARG, (m, k, ng)
        assert "PLK_KZG_FOLD_MAX" in h.last_error()
        assert lib.plk_kzg_fold_flat_plan(4097, 2, 8, ragged, out) == h.PLK_ERR_RANGE
        assert "PLK_KZG_FLAT_MAX" in h.last_error()
        assert lib.plk_kzg_fold_flat_plan(1, 16, (1 << 26) + 1, ragged, out) == h.PLK_ERR_RANGE
        assert lib.plk_kzg_fold_flat_plan(1, 16, 1 << 26, ragged, out) == h.PLK_OK
        assert lib.plk_kzg_fold_flat_plan(1, 3, (1 << 30) // 3 + 1, ragged, out) == h.PLK_ERR_RANGE
        assert lib.plk_kzg_fold_flat_plan(1, 3, (1 << 30) // 3, ragged, out) == h.PLK_OK
        assert lib.plk_kzg_fold_flat_plan(1, 1, (1 << 64) - 1, ragged, out) == h.PLK_ERR_RANGE
    # uniform: total = m k ngroups must stay below 2^32; a ragged list's total is not the plan's business
    assert lib.plk_kzg_fold_flat_plan(4096, 16, 1 << 16, 0, out) == h.PLK_ERR_RANGE
    assert "2^32" in h.last_error()
    assert lib.plk_kzg_fold_flat_plan(4096, 16, (1 << 16) - 1, 0, out) == h.PLK_OK
    assert lib.plk_kzg_fold_flat_plan(4096, 16, 1 << 16, 1, out) == h.PLK_OK


# ------------------------------------------------------------------ argument checks, no device
def _opaque_handle():
    """a non-NULL handle of zero bytes (an SRS of no points): shape and pointer checks return before it is read"""
    return (C.c_uint8 * 256)()


class FoldArgs:
    """host blocks standing in for every array: a failing call never reads them.  Two groups of two polynomials
    of sixteen coefficients."""

    def __init__(self):
        self.co = (C.c_uint8 * 64)()
        self.off = (C.c_uint32 * 5)(0, 16, 32, 48, 64)
        self.w = (C.c_uint8 * 4)()
        self.zs = (C.c_uint8 * 2)()
        self.ys = (C.c_uint8 * 4)()
        self.pr = (C.c_uint8 * 6)()
        self.cm = (C.c_uint8 * 12)()
        self.st = (C.c_uint8 * 2)()

    def call(self, h, fn, s, total=64, m=16, k=2, ngroups=2, ragged=False, drop=(), off_shift=0):
        names = ("co", "w", "zs", "ys", "pr", "cm", "st")
        a = {n: (None if n in drop else C.addressof(getattr(self, n))) for n in names}
        p = {n: (None if n in drop else C.cast(getattr(self, n), C.POINTER(C.c_uint8))) for n in names}
        L = h.lib()
        if fn == "dev":
            off = C.addressof(self.off) + off_shift if ragged else None
            return L.plk_kzg_open_fold_flat_dev(s, a["co"], total, off, m, k, ngroups, a["w"], a["zs"], a["ys"], a["pr"], a["cm"],
                                                a["st"], None)
        return L.plk_kzg_open_fold_flat(s, p["co"], total, self.off if ragged else None, m, k, ngroups, p["w"], p["zs"], p["ys"],
                                        p["pr"], p["cm"])


FNS = ("dev", "host")


@pytest.mark.parametrize("fn", FNS)
def test_null_handle_is_arg_error(fn):
    import plonkhip as h
    assert FoldArgs().call(h, fn, None) == h.PLK_ERR_ARG
    assert "plk_kzg_open_fold_flat" in h.last_error()


SHAPES = {
    "ngroups0": (dict(ngroups=0), "ARG"),
    "k0": (dict(k=0), "ARG"),
    "total0": (dict(total=0), "ARG"),
    "m0": (dict(m=0), "ARG"),
    "m0_ragged": (dict(m=0, ragged=True), "ARG"),
    "k17": (dict(k=17, ngroups=1, total=16 * 17), "ARG"),
    "k17_ragged": (dict(k=17, ragged=True), "ARG"),
    "mismatch": (dict(total=63), "ARG"),
    "mismatch_up": (dict(total=65), "ARG"),
    "m4097": (dict(m=4097, k=1, ngroups=1, total=4097), "RANGE"),
    "m4097_ragged": (dict(m=4097, ragged=True), "RANGE"),
    "total_2_32": (dict(m=4096, k=16, ngroups=1 << 16, total=1 << 32), "RANGE"),
    "total_2_32_ragged": (dict(total=1 << 32, ragged=True), "RANGE"),
    "npoly_2_30_1": (dict(m=1, k=1, ngroups=(1 << 30) + 1, total=(1 << 30) + 1), "RANGE"),
    "npoly_2_30_16_ragged": (dict(k=16, ngroups=(1 << 26) + 1, ragged=True), "RANGE"),
}


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("case", sorted(SHAPES))
@pytest.mark.parametrize("handle", ["null", "opaque"])
def test_shape_errors_come_before_any_device_query(case, fn, handle):
    """the shape is checked first: the same code with a NULL handle and with one the call must not look into"""
    import plonkhip as h
    fake = _opaque_handle()
    kw, code = SHAPES[case]
    rc = FoldArgs().call(h, fn, None if handle == "null" else C.addressof(fake), **kw)
    assert rc == {"ARG": h.PLK_ERR_ARG, "RANGE": h.PLK_ERR_RANGE}[code], (case, fn)
    assert "plk_kzg_open_fold_flat" in h.last_error()


@pytest.mark.parametrize("fn,drop", [("dev", d) for d in ("co", "w", "zs", "ys", "pr", "st")] +
                         [("host", d) for d in ("co", "w", "zs", "ys", "pr")])
def test_null_pointers_are_arg_errors(fn, drop):
    """pointers come after the shape and before the SRS bound (a zeroed handle would fail that with RANGE)"""
    import plonkhip as h
    fake = _opaque_handle()
    assert FoldArgs().call(h, fn, C.addressof(fake), drop=(drop,)) == h.PLK_ERR_ARG
    assert "required" in h.last_error()


def test_misaligned_offsets_are_arg_errors():
    import plonkhip as h
    fake = _opaque_handle()
    assert FoldArgs().call(h, "dev", C.addressof(fake), ragged=True, ngroups=1, off_shift=2) == h.PLK_ERR_ARG
    assert "4-byte aligned" in h.last_error()


HOST_LISTS = {
    "empty": ([0, 16, 16, 48, 64], None, None),
    "falling": ([0, 16, 8, 48, 64], None, None),
    "above_total": ([0, 16, 32, 48, 65], None, None),
    "longer_than_m": ([0, 16, 33, 48, 64], None, None),
    "z17": (None, [0, 17], None),
    "z255": (None, [255, 0], None),
    "w17": (None, None, [1, 17, 1, 1]),
    "w255": (None, None, [1, 1, 1, 255]),
}


@pytest.mark.parametrize("case", sorted(HOST_LISTS))
def test_host_form_validates_its_lists_before_any_device_query(case):
    """each BAD case of the _dev form is PLK_ERR_ARG in the host form, before the SRS bound (RANGE with this handle)"""
    import plonkhip as h
    off, zs, w = HOST_LISTS[case]
    fake = _opaque_handle()
    a = FoldArgs()
    if off is not None:
        a.off[:] = off
    if zs is not None:
        a.zs[:] = zs
    if w is not None:
        a.w[:] = w
    assert a.call(h, "host", C.addressof(fake), ragged=True) == h.PLK_ERR_ARG, case
    assert "plk_kzg_open_fold_flat" in h.last_error()


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("ragged", [False, True])
def test_range_error_of_a_zeroed_handle(fn, ragged):
    """a call that passes every argument check reaches the SRS bound, which a handle of zero bytes (an SRS of no
    points) fails with the reference's text -- still before any device query"""
    import plonkhip as h
    fake = _opaque_handle()
    assert FoldArgs().call(h, fn, C.addressof(fake), ragged=ragged) == h.PLK_ERR_RANGE
    assert "degree exceeds SRS size" in h.last_error()
