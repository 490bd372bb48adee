"""Python model of the KZG flat batches (plk_kzg_commit_flat*, plk_kzg_open_flat*): numpy, vectorised over the
polynomials, so that 2^19 short polynomials cost well under a second.

A canonical SRS is a list of group elements of E(F101): y^2 = x^3 + 3, cyclic of order 102, so a commitment is
EXP[(sum c_j LOG(srs_j)) mod 102] for ANY coefficient byte (g1_mul takes the raw byte).  The tables are built here
from the group law itself.  An opening is plain synthetic division by x - z from the top coefficient down:
q[j - 1] = p[j] + z q[j], y = p[0] + z q[0]; the proof is the commitment of q.  The status rules are those of
include/plonkhip.h ("KZG flat batches")."""
import numpy as np

R = 17
P = 101
ORD = 102
FLAT_MAX = 4096
IRREGULAR, BAD = 1, 2
FLAGGED = (0xFF, 0xFF, 0xFF)
LANE_MAX, WAVE_MAX = 32, 1024
GRID_CAP = 2048


def _add(a, b):
    """the group law on (x, y) tuples, None the identity"""
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2 and (y1 + y2) % P == 0:
        return None
    if a == b:
        lam = 3 * x1 * x1 * pow(2 * y1, P - 2, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, P - 2, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def _tables():
    pts = [(x, y) for x in range(P) for y in range(P) if (y * y - x * x * x - 3) % P == 0]
    assert len(pts) == ORD - 1
    for g in pts:
        seq, acc = [None], g
        while acc is not None:
            seq.append(acc)
            acc = _add(acc, g)
        if len(seq) == ORD:
            break
    else:
        raise AssertionError("no generator")
    exp = np.array([(0, 0, 1) if e is None else (e[0], e[1], 0) for e in seq], np.uint8)
    log = np.full(1 << 17, -1, np.int64)   # index x | y << 8 | flag << 16
    for k, e in enumerate(exp):
        log[int(e[0]) | int(e[1]) << 8 | int(e[2]) << 16] = k
    return exp, log


EXP, _LOG = _tables()


def rule_srs(n):
    """srs[i] = (2^i mod 17) G, G = (1, 2): the well-formed SRS for s = 2"""
    g = int(_LOG[1 | 2 << 8])
    k = np.array([pow(2, i, R) for i in range(n)], np.int64)
    return EXP[(k * g) % ORD]


def srs_logs(srs_pts):
    """the discrete logs of an SRS (n, 3), or None when some encoding is no canonical group element (the
    library's `irregular`)"""
    s = np.asarray(srs_pts, np.uint8).reshape(-1, 3).astype(np.int64)
    idx = s[:, 0] | s[:, 1] << 8 | np.minimum(s[:, 2], 1) << 16
    lg = _LOG[idx]
    if (lg < 0).any() or (s[:, 2] > 1).any():
        return None
    return lg


def plan(m, npoly):
    """plk_kzg_flat_plan's four numbers"""
    path = 0 if m <= LANE_MAX else 1 if m <= WAVE_MAX else 2
    per = (256, 4, 1)[path]
    return {"path": path, "per_block": per, "blocks": min(-(-npoly // per), GRID_CAP), "launches": 1}


def open_rows(rows, zs, logs, want_commits=True):
    """rows: (npoly, m) bytes, polynomial g in row g, zero padded at the top (padding changes nothing); zs: npoly
    values < 17; logs: srs_logs of at least m points (m - 1 without commitments).
    -> (ys, proofs (npoly, 3), commits (npoly, 3) or None), exact where the row's bytes are < 17; the commitments
    exact for every byte"""
    rows = np.asarray(rows, np.uint8)
    n, m = rows.shape
    z = np.asarray(zs, np.int32).reshape(n)
    lg = _padded_logs(logs, m)
    rt = np.ascontiguousarray(rows.T)         # (m, npoly): one coefficient position per row
    q = np.zeros(n, np.int32)
    sq = np.zeros(n, np.int32)                # (<= 4096 x 16 x 101)
    for j in range(m - 1, 0, -1):
        q = (rt[j] + z * q) % R               # q[j - 1]
        sq += q * lg[j - 1]
    ys = ((rt[0] + z * q) % R).astype(np.uint8)
    return ys, EXP[sq % ORD], commit_rows(rows, logs) if want_commits else None


def _padded_logs(logs, m):
    lg = np.zeros(m, np.int32)
    k = min(m, len(logs))
    lg[:k] = np.asarray(logs, np.int32)[:k]
    return lg


def commit_rows(rows, logs):
    """EXP[sum_j byte j x log j]: exact in float64 (<= 4096 x 255 x 101 < 2^53)"""
    rows = np.asarray(rows, np.uint8)
    s = rows.astype(np.float64) @ _padded_logs(logs, rows.shape[1]).astype(np.float64)
    return EXP[s.astype(np.int64) % ORD]


def segments(total, npoly, m, offsets=None):
    """(lo, length, ok) per polynomial as the kernels read them: offsets as min(o, total); ok False for a ragged
    polynomial that is empty, falls, has an offset above total or is longer than m"""
    if offsets is None:
        lo = np.arange(npoly, dtype=np.int64) * m
        return lo, np.full(npoly, m, np.int64), np.ones(npoly, bool)
    o = np.asarray(offsets, np.int64)
    a, b = o[:-1], o[1:]
    ok = (a < b) & (b <= total) & (b - a <= m)
    return np.minimum(a, total), np.where(ok, b - a, 0), ok


def rows_of(coeffs, lo, ln, width):
    """(npoly, width) matrix: row g = coeffs[lo[g]:lo[g] + ln[g]], zero above"""
    co = np.asarray(coeffs, np.uint8).reshape(-1)
    j = np.arange(width, dtype=np.int64)[None, :]
    idx = np.minimum(lo[:, None] + j, max(co.size - 1, 0))
    return np.where(j < ln[:, None], co[idx], 0).astype(np.uint8)


def flat_dev(coeffs, m, npoly, srs_pts, zs=None, offsets=None, want_commits=True):
    """the _dev forms: dict(status, ys, proofs, commits, ys_exact); zs None: plk_kzg_commit_flat_dev (no ys, no
    proofs).  ys_exact: where the header specifies y (everything but a polynomial with a byte >= 17); BAD rows
    hold y = 0xFF."""
    co = np.asarray(coeffs, np.uint8).reshape(-1)
    lo, ln, ok = segments(co.size, npoly, m, offsets)
    width = int(ln.max()) if npoly else 1
    rows = co.reshape(npoly, m) if offsets is None else rows_of(co, lo, ln, max(width, 1))
    logs = srs_logs(srs_pts)
    irregular = logs is None
    opening = zs is not None
    z = np.asarray(zs, np.int64).reshape(npoly) if opening else np.zeros(npoly, np.int64)
    if opening:
        ok = ok & (z < R)
    noncanon = (rows >= R).any(axis=1)
    status = np.where(~ok, BAD, np.where(irregular | (opening & noncanon), IRREGULAR, 0)).astype(np.uint8)
    lg = np.zeros(max(width, 1), np.int64) if irregular else logs
    out = {"status": status, "ys": None, "proofs": None, "commits": None, "ys_exact": None}
    if opening:
        ys, proofs, commits = open_rows(rows, np.where(ok, z, 0), lg, want_commits)
        ys = np.where(ok, ys, 0xFF).astype(np.uint8)
        proofs = np.where((status != 0)[:, None], np.array(FLAGGED, np.uint8), proofs)
        out.update(ys=ys, proofs=proofs, ys_exact=~(ok & noncanon))
    elif want_commits:
        commits = commit_rows(rows, lg)
    if want_commits:
        out["commits"] = np.where((~ok | irregular)[:, None], np.array(FLAGGED, np.uint8), commits)
    return out


def expanded(coeffs, m, npoly, offsets=None):
    """the list of polynomials a valid call stands for (the specification's expanded list)"""
    co = np.asarray(coeffs, np.uint8).reshape(-1)
    lo, ln, ok = segments(co.size, npoly, m, offsets)
    assert ok.all()
    return [co[a:a + k] for a, k in zip(lo.tolist(), ln.tolist())]
