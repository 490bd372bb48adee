"""The builders of tests/g1_encoding_cases.py and the expected values they take from the oracle,
without a GPU: the independent canonical predicate against the oracle's discrete-log table over the
whole encoding space, the family sizes, determinism, and -- for flag bytes 0 / 1 -- the oracle
(oracle/oracle.c) against the reference compiled from its unmodified headers
(oracle/_ref/libplonkref.so) at the very inputs tests/test_g1_encodings_gpu.py sends to the kernels.
A flag byte outside {0, 1} is a C bool with undefined behaviour in the reference build (ADVICE.md,
oracle/sanitize_main.c): those encodings are compared device against oracle only."""
import os

import numpy as np
import pytest

import g1_encoding_cases as ge
from conftest import ROOT

REFLIB = os.path.join(ROOT, "oracle", "_ref", "libplonkref.so")
NEAR_MISSES = 1228          # len(near_misses()), counted here
BOUNDARY_CASES = 1012       # len(boundary_states())


@pytest.fixture(scope="module")
def ref():
    assert os.path.exists(REFLIB), "%s missing: `make -C oracle` where /root/reference exists" % REFLIB
    from pyoracle import Reference
    return Reference(REFLIB)


def _all_xy(flag):
    v = np.arange(1 << 16)
    return np.stack([v >> 8, v & 0xFF, np.full(v.size, flag)], axis=1).astype(np.uint8)


@pytest.mark.parametrize("flag", [0, 1, 2, 255])
def test_canonical_mask_is_the_oracles_dlog(oracle, flag):
    t = _all_xy(flag)
    assert np.array_equal(ge.canonical_mask(t), oracle.dlog_many(t) != 0xFF)
    for p in t[::257]:                                       # the bulk form is the single call
        assert (oracle.dlog(p) is not None) == bool(ge.canonical_mask(p)[0])


def test_canonical_mask_on_the_other_flag_bytes(oracle):
    t = ge.seeded_triples(list(range(3, 255)), 1 << 16)
    assert set(np.unique(t[:, 2])) == set(range(3, 255))
    assert not ge.canonical_mask(t).any()
    assert (oracle.dlog_many(t) == 0xFF).all()


def test_exactly_102_of_all_encodings_are_canonical():
    total = 0
    for flag in range(256):
        m = ge.canonical_mask(_all_xy(flag))
        total += int(m.sum())
        assert int(m.sum()) == {0: 101, 1: 1}.get(flag, 0)
    assert total == 102
    assert ge.canonical_mask(ge.GROUP).all() and len(ge.GROUP) == 102


def test_sweep_candidates_cover_every_xy_once():
    for flag in (0, 7):
        both = np.concatenate([ge.sweep_candidates(flag, h) for h in (0, 1)])
        assert np.array_equal(both, _all_xy(flag))


def test_near_misses(oracle):
    nm = ge.near_misses()
    assert len(nm) == NEAR_MISSES
    assert len({tuple(p) for p in nm.tolist()}) == len(nm)
    assert not ge.canonical_mask(nm).any() and (oracle.dlog_many(nm) == 0xFF).all()
    have = {tuple(p) for p in nm.tolist()}
    # the shapes the decode must reject, for an affine point, the 2-torsion point and the identity
    for p in [(0, 2, 0), (2, 2, 0), (102, 2, 0), (203, 2, 0), (1, 103, 0), (1, 204, 0), (1, 254, 0), (1, 2, 1), (1, 2, 2),
              (1, 2, 3), (1, 2, 128), (1, 2, 254), (1, 2, 255), (48, 101, 0), (48, 202, 0), (49, 0, 0), (149, 0, 0),
              (0, 0, 0), (0, 0, 2), (0, 0, 3), (0, 0, 255), (1, 0, 1), (0, 1, 1), (101, 0, 1), (0, 101, 1)]:
        assert p in have, p
    sp = ge.special_candidates()
    assert ge.canonical_mask(sp[:3]).all() and not ge.canonical_mask(sp[3:]).any()
    assert {tuple(p) for p in sp[3:].tolist()} <= have


def test_family_sizes(oracle):
    assert len(ge.Y47) == 47 and len(set(ge.Y47)) == 47
    assert len(ge.pairs_same_x(oracle)[0]) == 7 * 47 * 47 == 15463
    assert [len(ge.pairs_chord(oracle, w)[0]) for w in (0, 1)] == [65536, 65536]
    assert len(ge.flag_coordinate_pairs()) == 100 and len(ge.pairs_flags(oracle)[0]) == 1600
    assert len(ge.pairs_mul(oracle)[0]) == (102 + NEAR_MISSES) * 256
    S, T, c = ge.boundary_cases()
    assert len(S) == BOUNDARY_CASES and T.shape == (BOUNDARY_CASES, 3, 3) and c.shape == (BOUNDARY_CASES, 3)
    ids = ge.canonical_mask(S)
    low = (S[:, 2] == 0) & (S[:, 0] < 101) & (S[:, 1] < 101)
    assert ids.sum() == 102                                              # group elements
    assert (low & ~ids).sum() >= 300                                     # off-curve, with a state id
    assert ((S[:, 2] == 0) & ~low).sum() >= 300                          # raw: no state id
    assert (S[:, 2] != 0).sum() >= 300                                   # flagged
    a, b = ge.CHORD_YS
    assert max(a) < 101 and min(b) >= 101


def test_boundary_layout_puts_the_terms_at_the_chunk_starts():
    S, T, c = ge.boundary_cases()
    pts, sc = ge.boundary_layout(S[:5], T[:5], c[:5])
    assert pts.shape == (5, 8192, 3) and ge.BOUNDARY_N >= ge.FOLD_CHUNKED_MIN
    where = [0, 2048, 4096, 6144]
    other = np.setdiff1d(np.arange(8192), where)
    assert (pts[:, other] == np.array(ge.IDENT, np.uint8)).all()
    assert np.array_equal(pts[:, 0], S[:5]) and (sc[:, 0] == 1).all()
    fl = np.flatnonzero(S[:, 2] != 0)[:5]                      # a flagged state: again before the second chunk
    fp, fs = ge.boundary_layout(S[fl], T[fl], c[fl])
    assert np.array_equal(fp[:, 2047], S[fl]) and (fs[:, 2047] == 1).all() and np.array_equal(fp[:, 0], S[fl])
    assert (fp[:, np.setdiff1d(other, [2047])] == np.array(ge.IDENT, np.uint8)).all()
    assert np.array_equal(pts[:, where[1:]], T[:5]) and np.array_equal(sc[:, where[1:]], c[:5])
    # the chunk length the launcher derives: ceil(n / 256) rounded up to 1024, at least 2048
    for n, L in ((ge.BOUNDARY_N, ge.BOUNDARY_L), (ge.BIG_N - 1, 2048), (ge.BIG_N, ge.BIG_L)):
        assert max(2048, ((n + 255) // 256 + 1023) // 1024 * 1024) == L
    bp, bs = ge.big_layout()
    assert bs.size == ge.BIG_N and (~ge.canonical_mask(bp)).sum() >= 5
    assert set(np.flatnonzero(~ge.canonical_mask(bp)) % ge.BIG_L) == {0}


def test_builders_are_pure(oracle):
    def same(f, *a):
        x, y = f(*a), f(*a)
        x, y = (x, y) if isinstance(x, tuple) else ((x,), (y,))
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), f.__name__
    same(ge.near_misses)
    same(ge.sweep_rows, oracle, 0, 0)
    same(ge.sweep_rows, oracle, 1, 0, 21)
    same(ge.seeded_triples, [4, 5], 1000)
    same(ge.pairs_same_x, oracle)
    same(ge.pairs_flags, oracle)
    same(ge.boundary_cases)
    same(ge.big_layout)
    same(ge.prefix_cases, ge.near_misses()[:8], [0] * 8)
    a = ge.sweep_rows(oracle, 0, 0)
    b = ge.sweep_rows(oracle, 0, 1)
    assert not np.array_equal(a[1], b[1])                      # another half: other fillers


def test_sweep_rows_expectation(oracle):
    """the candidate sits where the docstring says, every filler is canonical, and the rows expected
    regular are exactly those whose candidate is canonical"""
    for flag, half, n in ((0, 0, 16), (0, 1, 16), (1, 0, 16), (0, 0, 21), (2, 0, 16)):
        pts, sc, irregular, logs, g1 = ge.sweep_rows(oracle, flag, half, n)
        cands = ge.sweep_candidates(flag, half)
        r = np.arange(ge.SWEEP_ROWS)
        pos = r % 16 if n == 16 else 16 + r % 5
        assert np.array_equal(pts[r, pos], cands) and (sc[r, pos] != 0).all()
        canon = ge.canonical_mask(pts.reshape(-1, 3)).reshape(ge.SWEEP_ROWS, n)
        canon[r, pos] = True
        assert canon.all()
        assert np.array_equal(irregular, ~ge.canonical_mask(cands))
        want = {(0, 0): None, (1, 0): 1, (2, 0): 0}.get((flag, half))
        if want is not None:
            assert (~irregular).sum() == want
        if flag == 0:
            assert sum((~ge.sweep_rows(oracle, 0, h, n)[2]).sum() for h in (0, 1)) == 101
        for row in np.flatnonzero(~irregular):
            assert bytes(g1[row]) == oracle.msm(pts[row], sc[row]) == oracle.dlog_exp(int(logs[row]))


FAMILIES = {"same_x": ge.pairs_same_x, "chord0": lambda o: ge.pairs_chord(o, 0),
            "chord1": lambda o: ge.pairs_chord(o, 1), "flags": ge.pairs_flags, "mul": ge.pairs_mul}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_pair_family_expectations_are_the_references(oracle, ref, name):
    """flag bytes 0 / 1: the fold that observes a pair on the device (srs_eval_at_s over [A, 1], [T, c],
    or [T, c] alone) gives, in the reference, the committed expectation g1_add(A, g1_mul(T, c)) -- every
    such pair; the two reference calls themselves on a sample"""
    fam = FAMILIES[name](oracle)
    pts, sc = ge.pair_folds(fam)
    assert np.array_equal(oracle.msm_many(pts, sc), fam[3])              # every flag byte: the fold is the pair
    keep = (fam[0][:, 2] <= 1) & (fam[1][:, 2] <= 1)
    assert keep.sum() >= {"flags": 400}.get(name, len(keep) // 2)
    assert np.array_equal(ref.msm_many(pts[keep], sc[keep]), fam[3][keep])
    for i in np.flatnonzero(keep)[::max(1, int(keep.sum()) // 3000)]:
        assert ref.g1_add(fam[0][i], ref.g1_mul(fam[1][i], int(fam[2][i]))) == bytes(fam[3][i]), (name, i)


def test_near_misses_and_boundary_terms_against_the_reference(oracle, ref):
    nm = ge.near_misses()
    nm = nm[nm[:, 2] <= 1]
    assert len(nm) == 720
    for n in (1, 16, 17):
        pts, sc = ge.placed("host/%d" % n, nm, n, np.arange(len(nm)) % n)
        want = oracle.msm_many(pts, sc)
        for i in range(0, len(nm), 3):
            assert ref.msm(pts[i], sc[i]) == bytes(want[i]), (n, i)
    S, T, c = ge.boundary_cases()
    keep = np.flatnonzero((S[:, 2] <= 1) & (T[:, :, 2] <= 1).all(axis=1))
    assert keep.size > 300 and (S[keep, 2] == 1).sum() > 20
    pts, sc = ge.boundary_layout(S[keep], T[keep], c[keep])
    want = oracle.msm_many(pts, sc)
    for i in range(keep.size):
        assert ref.msm(pts[i], sc[i]) == bytes(want[i]), i
    bp, bs = ge.big_layout()
    assert oracle.msm(bp, bs) == oracle.msm(bp[::ge.BIG_L], bs[::ge.BIG_L])   # identities pass a flag-0 state through


def test_same_x_family_sees_a_wrong_branch(oracle):
    """sensitivity: the Python restatement of the raw addition reproduces the family's expected bytes,
    and the same code doubling b instead of a in the a.x == b.x branch does not"""
    A, T, c, want = ge.pairs_same_x(oracle)
    assert (c == 1).all()
    right = wrong = 0
    for a, t, w in zip(A.tolist(), T.tolist(), want.tolist()):
        term = ge.py_add(ge.IDENT, tuple(t))                             # g1_mul(T, 1)
        right += ge.py_add(tuple(a), term) == tuple(w)
        wrong += ge.py_add(tuple(a), term, same_x_uses_b=True) != tuple(w)
    assert right == len(A)
    print("same-x pairs on which the altered branch differs: %d of %d" % (wrong, len(A)))
    assert wrong >= 1
