"""Python model of the KZG flat folded openings (plk_kzg_fold_flat_plan, plk_kzg_open_fold_flat*): numpy,
vectorised over the groups, on the tables and the segment helpers of tests/kzg_flat_model.py.

Group g = polynomials [k g, k (g + 1)) of a flat list under weights [k g, k (g + 1)) at the one point zs[g]:
y_i = p_i(z); F[j] = sum_i w_i p_i[j] mod 17 over L = the longest length; the proof is the commitment of
F's quotient by x - z, which over a canonical SRS is EXP[(sum_j q_j LOG(srs_j)) mod 102]; the commitment of
polynomial i is kzg_flat_model.commit_rows' (exact for any byte).  The status rules are those of
include/plonkhip.h ("KZG flat folded openings")."""
import numpy as np

import kzg_flat_model as FM

R = FM.R
FOLD_MAX = 16
LANE_MAX, WAVE_MAX, GRID_CAP = FM.LANE_MAX, FM.WAVE_MAX, FM.GRID_CAP
PER_BLOCK = (256, 4, 1)
IRREGULAR, BAD = FM.IRREGULAR, FM.BAD
FLAGGED = FM.FLAGGED


def plan(m, k, ngroups):
    """plk_kzg_fold_flat_plan's four numbers: a function of (m, ngroups); k changes nothing"""
    path = 0 if m <= LANE_MAX else 1 if m <= WAVE_MAX else 2
    per = PER_BLOCK[path]
    return {"path": path, "per_block": per, "blocks": min(-(-ngroups // per), GRID_CAP), "launches": 1}


def fold_rows(rows, weights, zs, logs):
    """rows: (ngroups, k, width) bytes, zero above each polynomial's length; weights (ngroups, k) and zs (ngroups)
    values < 17; logs: at least width - 1 SRS logs.  -> (ys (ngroups, k), proofs (ngroups, 3)), exact where the
    bytes are < 17"""
    rows = np.asarray(rows, np.uint8)
    ng, k, width = rows.shape
    w = np.asarray(weights, np.int64).reshape(ng, k)
    z = np.asarray(zs, np.int64).reshape(ng)
    F = (np.einsum("gkj,gk->gj", rows.astype(np.int64), w) % R).astype(np.uint8)    # (<= 16 x 16 x 255 a sum)
    _, proofs, _ = FM.open_rows(F, z, logs, want_commits=False)
    ys = np.zeros((ng, k), np.int64)
    for j in range(width - 1, -1, -1):                                               # Horner, every polynomial at once
        ys = (ys * z[:, None] + rows[:, :, j]) % R
    return ys.astype(np.uint8), proofs


def fold_flat_dev(coeffs, m, k, ngroups, srs_pts, weights, zs, offsets=None, want_commits=True):
    """the _dev form: dict(status (ngroups), ys (k ngroups), proofs (ngroups, 3), commits (k ngroups, 3) or None,
    ys_exact (k ngroups)).  ys_exact: where the header specifies y (everything but a valid group with a byte >= 17);
    BAD groups hold y = 0xFF."""
    co = np.asarray(coeffs, np.uint8).reshape(-1)
    npoly = k * ngroups
    lo, ln, ok = FM.segments(co.size, npoly, m, offsets)
    width = max(int(ln.max()), 1)
    rows = co.reshape(npoly, m) if offsets is None else FM.rows_of(co, lo, ln, width)
    w = np.asarray(weights, np.int64).reshape(ngroups, k)
    z = np.asarray(zs, np.int64).reshape(ngroups)
    gok = ok.reshape(ngroups, k).all(axis=1) & (z < R) & (w < R).all(axis=1)
    logs = FM.srs_logs(srs_pts)
    irregular = logs is None
    noncanon = (rows >= R).any(axis=1).reshape(ngroups, k).any(axis=1)
    status = np.where(~gok, BAD, np.where(irregular | noncanon, IRREGULAR, 0)).astype(np.uint8)
    lg = np.zeros(width, np.int64) if irregular else logs
    g3 = rows.reshape(ngroups, k, -1)
    ys, proofs = fold_rows(g3, np.where(gok[:, None], w, 0), np.where(gok, z, 0), lg)
    ys = np.where(gok[:, None], ys, 0xFF).astype(np.uint8).reshape(-1)
    proofs = np.where((status != 0)[:, None], np.array(FLAGGED, np.uint8), proofs)
    out = {"status": status, "ys": ys, "proofs": proofs, "commits": None, "ys_exact": np.repeat(~(gok & noncanon), k)}
    if want_commits:
        flag = np.repeat(~gok | irregular, k)
        out["commits"] = np.where(flag[:, None], np.array(FLAGGED, np.uint8), FM.commit_rows(rows, lg))
    return out


def expanded(coeffs, m, k, ngroups, offsets=None):
    """the groups a valid call stands for: a list of ngroups lists of k polynomials (the specification's expanded
    groups)"""
    polys = FM.expanded(coeffs, m, k * ngroups, offsets)
    return [polys[k * g:k * (g + 1)] for g in range(ngroups)]
