"""KZG flat multi-point openings (plk_kzg_multi_flat_plan, plk_kzg_open_multi_flat*) without a GPU: the Python
model against kzg_multi_model.open_multi (which tests/golden/kzg_multi.json pins to the compiled reference), the
model's status rules, the plan, the exports, and every argument check that comes before any device query, in the
order the header states."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kzg_flat_model as FM
import kzg_multi_flat_model as MF
import kzg_multi_model as MM
from conftest import ROOT

NEW = ("plk_kzg_multi_flat_plan", "plk_kzg_open_multi_flat_dev", "plk_kzg_open_multi_flat")
PLONK_PAIR = MM.mask_of([3, 6])


def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("kzg_multi_flat_plan", "kzg_open_multi_flat", "kzg_open_multi_flat_dev"):
        assert hasattr(h, name), name
    assert len(h.SIGNATURES["plk_kzg_multi_flat_plan"][1]) == 5
    assert len(h.SIGNATURES["plk_kzg_open_multi_flat_dev"][1]) == 15
    assert len(h.SIGNATURES["plk_kzg_open_multi_flat"][1]) == 13
    with open(os.path.join(ROOT, "include", "plonkhip.h")) as f:
        txt = f.read()
    assert "#define PLK_KZG_MULTI_MAX %d " % MF.MULTI_MAX in txt
    assert "KZG flat multi-point openings" in txt
    assert (MF.LANE_MAX, MF.WAVE_MAX, MF.GRID_CAP, MF.PER_BLOCK) == (32, 1024, 2048, (256, 4, 1))


def test_python_wrapper_checks_its_lists():
    import plonkhip as h
    co = np.zeros(12, np.uint8)
    with pytest.raises(ValueError):
        h.kzg_open_multi_flat(None, co, 5, [1] * 3, [1] * 3, [0], m=4)      # k does not divide npoly
    with pytest.raises(ValueError):
        h.kzg_open_multi_flat(None, co, 3, [1] * 2, [1] * 3, [0], m=4)      # a set per polynomial
    with pytest.raises(ValueError):
        h.kzg_open_multi_flat(None, co, 3, [1] * 3, [1] * 2, [0], m=4)      # a weight per polynomial
    with pytest.raises(ValueError):
        h.kzg_open_multi_flat(None, co, 3, [1] * 3, [1] * 3, [0, 1], m=4)   # a u per group


# ------------------------------------------------------------------ the model
def mixed_group(seed, k, maxlen=40):
    """k polynomials of lengths 1 .. maxlen mixed, sets from one point to sixteen (the point 0, the pair, random),
    weights with zeros"""
    r = np.random.default_rng(0x3F17 + seed)
    lens = r.integers(1, maxlen + 1, k).tolist()
    lens[seed % k] = maxlen if seed % 3 else 1 + seed % maxlen
    polys = [r.integers(0, 17, n).astype(np.uint8) for n in lens]
    sets = []
    for i in range(k):
        kind = (seed + i) % 5
        if kind == 0:
            sets.append(1)
        elif kind == 1:
            sets.append(1 << int(r.integers(1, 17)))
        elif kind == 2:
            sets.append(PLONK_PAIR)
        elif kind == 3:
            sets.append(MM.FULL & ~(1 << int(r.integers(0, 17))))
        else:
            sets.append(MM.mask_of(r.choice(17, int(r.integers(1, 17)), replace=False)))
    w = r.integers(0, 17, k).astype(np.uint8)
    if seed % 4 == 0:
        w[r.integers(0, k)] = 0
    return polys, sets, w


def as_flat(groups):
    polys = [p for g in groups for p in g]
    off = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.uint32)
    return np.concatenate(polys).astype(np.uint8), off


def model_of(groups, sets, weights, us, srs, m):
    co, off = as_flat(groups)
    k = len(groups[0])
    return MF.multi_flat_dev(co, m, k, len(groups), srs, np.concatenate(sets), np.concatenate(weights), us, offsets=off)


def check_group(srs, polys, sets, w, u, ys, proofs, commits, what):
    """one group of the model (commitments by logs) against kzg_multi_model.open_multi (the raw fold)"""
    eys, _, W, Wp = MM.open_multi(srs, polys, sets, w, u)
    assert ys.reshape(-1).tolist() == eys, what
    assert tuple(proofs.tolist()) == tuple(W) + tuple(Wp), what
    for p, c in zip(polys, commits):
        assert tuple(c.tolist()) == tuple(MM.F.msm(srs[:len(p)], p)), what


@pytest.mark.parametrize("k", range(1, 16))
def test_model_equals_the_multi_model(k):
    """every k, lengths 1 .. 40 mixed inside a group, every u (inside and outside T), weights with zeros"""
    srs = FM.rule_srs(40)
    groups, sets, weights = zip(*[mixed_group(100 * k + u, k) for u in range(17)])
    us = np.arange(17)
    r = model_of(groups, sets, weights, us, srs, 40)
    assert r["status"].sum() == 0 and r["ys_exact"].all()
    for g in range(17):
        sl = slice(k * g, k * (g + 1))
        check_group(srs, groups[g], sets[g], weights[g], g, r["ys"][sl], r["proofs"][g], r["commits"][sl], (k, g))


def test_model_status_rules():
    srs = FM.rule_srs(8)
    co = (np.arange(32) % 17).astype(np.uint8)
    # k = 2, m = 4; groups: fine, an empty polynomial, a falling one, above total, longer than m, u = 17, weight 17,
    # mask 0, a mask bit 17, the full mask, fine
    off = np.array([0, 3, 4, 4, 6, 5, 7, 40, 9, 14, 15, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28], np.uint32)
    us = np.array([1, 1, 1, 1, 1, 17, 2, 3, 4, 5, 6])
    w = np.ones(22, np.uint8)
    w[12] = 17
    s = np.full(22, 0b110, np.int64)
    s[14], s[17], s[18] = 0, 1 << 17, MM.FULL
    r = MF.multi_flat_dev(co, 4, 2, 11, srs, s, w, us, offsets=off)
    assert r["status"].tolist() == [0] + [2] * 9 + [0]
    bad = list(range(1, 10))
    assert (r["proofs"][bad] == 0xFF).all()
    assert (r["ys"].reshape(11, 34)[bad] == 0xFF).all() and (r["commits"].reshape(11, 2, 3)[bad] == 0xFF).all()
    assert (r["commits"].reshape(11, 2, 3)[[0, 10]] != 0xFF).any(axis=2).all()
    assert (r["ys"].reshape(11, 2, 17)[[0, 10]][:, :, [1, 2]] < 17).all()
    assert (r["ys"].reshape(11, 2, 17)[[0, 10]][:, :, [0] + list(range(3, 17))] == 0xFF).all()
    # a coefficient byte >= 17: the group IRREGULAR, its commitments exact, its ys unspecified
    co2 = np.array([1, 2, 200, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.uint8)
    r = MF.multi_flat_dev(co2, 3, 2, 2, srs, [2, 6, 1, 3], [1, 2, 3, 4], [3, 4])
    assert r["status"].tolist() == [1, 0] and (r["proofs"][0] == 0xFF).all() and (r["proofs"][1] != 0xFF).any()
    assert r["commits"].tolist() == FM.commit_rows(co2.reshape(4, 3), FM.srs_logs(srs)).tolist()
    assert r["ys_exact"].tolist() == [False, True]
    # an SRS without log form: every group IRREGULAR, every G1 FF FF FF, the ys exact
    bad_srs = srs.copy()
    bad_srs[1] = (1, 3, 0)
    co3 = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.uint8)
    r = MF.multi_flat_dev(co3, 3, 2, 2, bad_srs, [1 << 3, 1 << 3, 1, 1 << 4], [1, 2, 3, 4], [3, 4])
    assert r["status"].tolist() == [1, 1] and r["ys_exact"].all()
    assert r["ys"][[0, 1, 2, 3], [3, 3, 0, 4]].tolist() == [(1 + 2 * 3 + 3 * 9) % 17, (4 + 5 * 3 + 6 * 9) % 17, 7,
                                                             (10 + 11 * 4 + 12 * 16) % 17]
    assert (r["ys"] != 0xFF).sum() == 4
    assert (r["proofs"] == 0xFF).all() and (r["commits"] == 0xFF).all()


def test_model_expanded():
    co = np.arange(12, dtype=np.uint8)
    g = MF.expanded(co, 2, 3, 2)
    assert [[p.tolist() for p in grp] for grp in g] == [[[0, 1], [2, 3], [4, 5]], [[6, 7], [8, 9], [10, 11]]]
    g = MF.expanded(co, 5, 2, 2, offsets=[1, 2, 5, 6, 11])
    assert [[p.tolist() for p in grp] for grp in g] == [[[1], [2, 3, 4]], [[5], [6, 7, 8, 9, 10]]]


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("ragged", [0, 1])
@pytest.mark.parametrize("m,path", [(1, 0), (MF.LANE_MAX, 0), (MF.LANE_MAX + 1, 1), (MF.WAVE_MAX, 1), (MF.WAVE_MAX + 1, 2),
                                    (FM.FLAT_MAX, 2)])
def test_plan_paths(m, path, ragged):
    import plonkhip as h
    per = MF.PER_BLOCK[path]
    for k in (1, 9, 15):
        for ng in (1, 3, per, per + 1, 3 * per + 1, per * MF.GRID_CAP, per * MF.GRID_CAP + 1):
            if m * k * ng >= 1 << 32 and not ragged:
                continue
            p = h.kzg_multi_flat_plan(m, k, ng, ragged)
            assert p == MF.plan(m, k, ng), (m, k, ng)
            assert (p["path"], p["per_block"], p["launches"]) == (path, per, 1)
            assert p["blocks"] == min(-(-ng // per), MF.GRID_CAP)


def test_plan_errors():
    import plonkhip as h
    lib = h.lib()
    out = (C.c_int64 * 4)()
    assert lib.plk_kzg_multi_flat_plan(16, 2, 8, 0, None) == h.PLK_ERR_ARG
    for ragged in (0, 1):
        for m, k, ng in ((0, 2, 8), (16, 0, 8), (16, 2, 0), (0, 0, 0), (16, 16, 8)):
            assert lib.plk_kzg_multi_flat_plan(m, k, ng, ragged, out) == h.PLK_ERR_ARG, (m, k, ng)
        assert "PLK_KZG_MULTI_MAX" in h.last_error()
        assert lib.plk_kzg_multi_flat_plan(16, 15, 8, ragged, out) == h.PLK_OK
        assert lib.plk_kzg_multi_flat_plan(4097, 2, 8, ragged, out) == h.PLK_ERR_RANGE
        assert "PLK_KZG_FLAT_MAX" in h.last_error()
        assert lib.plk_kzg_multi_flat_plan(1, 8, (1 << 27) + 1, ragged, out) == h.PLK_ERR_RANGE
        assert lib.plk_kzg_multi_flat_plan(1, 8, 1 << 27, ragged, out) == h.PLK_OK
        assert lib.plk_kzg_multi_flat_plan(1, 3, (1 << 30) // 3 + 1, ragged, out) == h.PLK_ERR_RANGE
        assert lib.plk_kzg_multi_flat_plan(1, 3, (1 << 30) // 3, ragged, out) == h.PLK_OK
        assert lib.plk_kzg_multi_flat_plan(1, 1, (1 << 64) - 1, ragged, out) == h.PLK_ERR_RANGE
    # uniform: total = m k ngroups must stay below 2^32; a ragged list's total is not the plan's business
    assert lib.plk_kzg_multi_flat_plan(4096, 8, 1 << 17, 0, out) == h.PLK_ERR_RANGE
    assert "2^32" in h.last_error()
    assert lib.plk_kzg_multi_flat_plan(4096, 8, (1 << 17) - 1, 0, out) == h.PLK_OK
    assert lib.plk_kzg_multi_flat_plan(4096, 8, 1 << 17, 1, out) == h.PLK_OK


# ------------------------------------------------------------------ argument checks, no device
def _opaque_handle():
    """a non-NULL handle of zero bytes (an SRS of no points): shape and pointer checks return before it is read"""
    return (C.c_uint8 * 256)()


class MultiArgs:
    """host blocks standing in for every array: a failing call never reads them.  Two groups of two polynomials
    of sixteen coefficients, every set the point 1."""

    def __init__(self):
        self.co = (C.c_uint8 * 64)()
        self.off = (C.c_uint32 * 5)(0, 16, 32, 48, 64)
        self.sets = (C.c_uint32 * 5)(2, 2, 2, 2, 2)
        self.w = (C.c_uint8 * 4)()
        self.us = (C.c_uint8 * 2)()
        self.ys = (C.c_uint8 * 68)()
        self.pr = (C.c_uint8 * 12)()
        self.cm = (C.c_uint8 * 12)()
        self.st = (C.c_uint8 * 2)()

    def call(self, h, fn, s, total=64, m=16, k=2, ngroups=2, ragged=False, drop=(), off_shift=0, sets_shift=0):
        names = ("co", "sets", "w", "us", "ys", "pr", "cm", "st")
        a = {n: (None if n in drop else C.addressof(getattr(self, n))) for n in names}
        p = {n: (None if n in drop else C.cast(getattr(self, n), C.POINTER(C.c_uint8))) for n in names}
        L = h.lib()
        if fn == "dev":
            off = C.addressof(self.off) + off_shift if ragged else None
            sets = None if a["sets"] is None else a["sets"] + sets_shift
            return L.plk_kzg_open_multi_flat_dev(s, a["co"], total, off, m, k, ngroups, sets, a["w"], a["us"], a["ys"], a["pr"],
                                                 a["cm"], a["st"], None)
        return L.plk_kzg_open_multi_flat(s, p["co"], total, self.off if ragged else None, m, k, ngroups,
                                         None if "sets" in drop else self.sets, p["w"], p["us"], p["ys"], p["pr"], p["cm"])


FNS = ("dev", "host")


@pytest.mark.parametrize("fn", FNS)
def test_null_handle_is_arg_error(fn):
    import plonkhip as h
    assert MultiArgs().call(h, fn, None) == h.PLK_ERR_ARG
    assert "plk_kzg_open_multi_flat" in h.last_error()


SHAPES = {
    "ngroups0": (dict(ngroups=0), "ARG"),
    "k0": (dict(k=0), "ARG"),
    "total0": (dict(total=0), "ARG"),
    "m0": (dict(m=0), "ARG"),
    "m0_ragged": (dict(m=0, ragged=True), "ARG"),
    "k16": (dict(k=16, ngroups=1, total=16 * 16), "ARG"),
    "k16_ragged": (dict(k=16, ragged=True), "ARG"),
    "mismatch": (dict(total=63), "ARG"),
    "mismatch_up": (dict(total=65), "ARG"),
    "m4097": (dict(m=4097, k=1, ngroups=1, total=4097), "RANGE"),
    "m4097_ragged": (dict(m=4097, ragged=True), "RANGE"),
    "total_2_32": (dict(m=4096, k=8, ngroups=1 << 17, total=1 << 32), "RANGE"),
    "total_2_32_ragged": (dict(total=1 << 32, ragged=True), "RANGE"),
    "npoly_2_30_1": (dict(m=1, k=1, ngroups=(1 << 30) + 1, total=(1 << 30) + 1), "RANGE"),
    "npoly_2_30_8_ragged": (dict(k=8, ngroups=(1 << 27) + 1, ragged=True), "RANGE"),
}


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("case", sorted(SHAPES))
@pytest.mark.parametrize("handle", ["null", "opaque"])
def test_shape_errors_come_before_any_device_query(case, fn, handle):
    """the shape is checked first: the same code with a NULL handle and with one the call must not look into"""
    import plonkhip as h
    fake = _opaque_handle()
    kw, code = SHAPES[case]
    rc = MultiArgs().call(h, fn, None if handle == "null" else C.addressof(fake), **kw)
    assert rc == {"ARG": h.PLK_ERR_ARG, "RANGE": h.PLK_ERR_RANGE}[code], (case, fn)
    assert "plk_kzg_open_multi_flat" in h.last_error()


@pytest.mark.parametrize("fn,drop", [("dev", d) for d in ("co", "sets", "w", "us", "ys", "pr", "st")] +
                         [("host", d) for d in ("co", "sets", "w", "us", "ys", "pr")])
def test_null_pointers_are_arg_errors(fn, drop):
    """pointers come after the shape and before the SRS bound (a zeroed handle would fail that with RANGE)"""
    import plonkhip as h
    fake = _opaque_handle()
    assert MultiArgs().call(h, fn, C.addressof(fake), drop=(drop,)) == h.PLK_ERR_ARG
    assert "required" in h.last_error()


def test_misaligned_offsets_and_sets_are_arg_errors():
    import plonkhip as h
    fake = _opaque_handle()
    assert MultiArgs().call(h, "dev", C.addressof(fake), ragged=True, ngroups=1, off_shift=2) == h.PLK_ERR_ARG
    assert "4-byte aligned" in h.last_error()
    for shift in (1, 2, 3):
        assert MultiArgs().call(h, "dev", C.addressof(fake), sets_shift=shift) == h.PLK_ERR_ARG
        assert "4-byte aligned" in h.last_error()
    assert MultiArgs().call(h, "dev", C.addressof(fake), sets_shift=4) == h.PLK_ERR_RANGE   # aligned: on to the SRS bound


HOST_LISTS = {
    "empty": ("off", [0, 16, 16, 48, 64]),
    "falling": ("off", [0, 16, 8, 48, 64]),
    "above_total": ("off", [0, 16, 32, 48, 65]),
    "longer_than_m": ("off", [0, 16, 33, 48, 64]),
    "mask0": ("sets", [2, 0, 2, 2, 2]),
    "mask_bit17": ("sets", [2, 2, 1 << 17, 2, 2]),
    "mask_full": ("sets", [2, 2, 2, (1 << 17) - 1, 2]),
    "w17": ("w", [1, 17, 1, 1]),
    "w255": ("w", [1, 1, 1, 255]),
    "u17": ("us", [0, 17]),
    "u255": ("us", [255, 0]),
}


@pytest.mark.parametrize("case", sorted(HOST_LISTS))
def test_host_form_validates_its_lists_before_any_device_query(case):
    """each BAD case of the _dev form is PLK_ERR_ARG in the host form, before the SRS bound (RANGE with this handle)"""
    import plonkhip as h
    name, vals = HOST_LISTS[case]
    fake = _opaque_handle()
    a = MultiArgs()
    getattr(a, name)[:] = vals
    assert a.call(h, "host", C.addressof(fake), ragged=True) == h.PLK_ERR_ARG, case
    assert "plk_kzg_open_multi_flat" in h.last_error()


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("ragged", [False, True])
def test_range_error_of_a_zeroed_handle(fn, ragged):
    """a call that passes every argument check reaches the SRS bound, which a handle of zero bytes (an SRS of no
    points) fails with the reference's text -- still before any device query"""
    import plonkhip as h
    fake = _opaque_handle()
    assert MultiArgs().call(h, fn, C.addressof(fake), ragged=ragged) == h.PLK_ERR_RANGE
    assert "degree exceeds SRS size" in h.last_error()


_NODEV_CHILD = r"""
import sys
sys.path[:0] = %r
import test_kzg_multi_flat_cpu as t
import plonkhip as h
assert h.device_count() == 0, "the device is still visible"
print("code", t.open_without_device(h))
"""


def open_without_device(h):
    try:
        with h.Srs([1, 2, 0] * 4) as s:
            h.kzg_open_multi_flat(s, [1, 2, 3, 4, 5, 6], 2, [2, 6], [1, 1], [3], m=3)
    except h.PlonkHipError as e:
        return e.code
    return h.PLK_OK


def test_no_cpu_fallback():
    """a valid call without a GPU is PLK_ERR_NODEV: in this process when it has no device; otherwise in one child
    process that hides it"""
    import plonkhip as h
    if h.device_count() == 0:
        code = open_without_device(h)
    else:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        paths = [os.path.dirname(os.path.abspath(__file__))] + [p for p in sys.path if p.startswith(ROOT)]
        out = subprocess.run([sys.executable, "-c", _NODEV_CHILD % (paths,)], env=env, capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        code = int(out.stdout.split("code", 1)[1].split()[0])
    assert code == h.PLK_ERR_NODEV
