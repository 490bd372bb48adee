"""Python model of the KZG flat multi-point openings (plk_kzg_multi_flat_plan, plk_kzg_open_multi_flat*): the
_dev form's outputs and status rules in numpy, on tests/kzg_multi_model.py (the opening of one group) and the
tables and segment helpers of tests/kzg_flat_model.py.

Group g = polynomials, masks and weights [k g, k (g + 1)) of a flat list under the challenge us[g]: its 17-byte
ys rows and its six proof bytes W, W' are kzg_multi_model.open_multi's, the commitment over a canonical SRS taken
as EXP[(sum_j c_j LOG(srs_j)) mod 102]; the commitment of polynomial i is kzg_flat_model.commit_rows' (exact for
any byte).  Groups repeat in the tiled batches the tests build, so results are remembered per distinct group.
The status rules are those of include/plonkhip.h ("KZG flat multi-point openings")."""
import numpy as np

import kzg_flat_model as FM
import kzg_multi_model as MM

R = FM.R
MULTI_MAX = MM.MULTI_MAX
LANE_MAX, WAVE_MAX, GRID_CAP = FM.LANE_MAX, FM.WAVE_MAX, FM.GRID_CAP
PER_BLOCK = (256, 4, 1)
IRREGULAR, BAD = FM.IRREGULAR, FM.BAD
FLAGGED = FM.FLAGGED


def plan(m, k, ngroups):
    """plk_kzg_multi_flat_plan's four numbers: a function of (m, ngroups); k changes nothing"""
    path = 0 if m <= LANE_MAX else 1 if m <= WAVE_MAX else 2
    per = PER_BLOCK[path]
    return {"path": path, "per_block": per, "blocks": min(-(-ngroups // per), GRID_CAP), "launches": 1}


def log_msm(logs):
    """the commitment over an SRS in log form, as kzg_multi_model.open_multi's msm"""
    lg = np.asarray(logs, np.int64)

    def msm(points, scalars):
        sc = np.asarray(scalars, np.int64).reshape(-1)
        return tuple(int(v) for v in FM.EXP[int(sc @ lg[:sc.size]) % FM.ORD])
    return msm


def masks_ok(sets):
    s = np.asarray(sets, np.int64)
    return (s != 0) & (s & ~np.int64(MM.FULL) == 0) & (s != MM.FULL)


def multi_flat_dev(coeffs, m, k, ngroups, srs_pts, sets, weights, us, offsets=None, want_commits=True):
    """the _dev form: dict(status (ngroups), ys (k ngroups, 17), proofs (ngroups, 6), commits (k ngroups, 3) or
    None, ys_exact (ngroups)).  ys_exact: where the header specifies the group's ys (everything but a valid group
    with a byte >= 17); BAD groups hold 0xFF throughout."""
    co = np.asarray(coeffs, np.uint8).reshape(-1)
    npoly = k * ngroups
    lo, ln, ok = FM.segments(co.size, npoly, m, offsets)
    s = np.asarray(sets, np.int64).reshape(ngroups, k)
    w = np.asarray(weights, np.int64).reshape(ngroups, k)
    u = np.asarray(us, np.int64).reshape(ngroups)
    gok = ok.reshape(ngroups, k).all(axis=1) & (u < R) & (w < R).all(axis=1) & masks_ok(s).all(axis=1)
    logs = FM.srs_logs(srs_pts)
    irregular = logs is None
    width = max(int(ln.max()), 1)
    rows = co.reshape(npoly, m) if offsets is None else FM.rows_of(co, lo, ln, width)
    noncanon = (rows >= R).any(axis=1).reshape(ngroups, k).any(axis=1)
    status = np.where(~gok, BAD, np.where(irregular | noncanon, IRREGULAR, 0)).astype(np.uint8)
    msm = (lambda points, scalars: FLAGGED) if irregular else log_msm(logs)
    ys = np.full((npoly, R), 0xFF, np.uint8)
    proofs = np.full((ngroups, 6), 0xFF, np.uint8)
    seen = {}
    for g in np.flatnonzero(gok & ~noncanon).tolist():
        polys = [co[lo[e]:lo[e] + ln[e]] for e in range(k * g, k * (g + 1))]
        key = (tuple(p.tobytes() for p in polys), s[g].tobytes(), w[g].tobytes(), int(u[g]))
        if key not in seen:
            gy, _, W, Wp = MM.open_multi(srs_pts, polys, s[g].tolist(), w[g].tolist(), int(u[g]), msm=msm)
            seen[key] = (np.array(gy, np.uint8).reshape(k, R), np.array(list(W) + list(Wp), np.uint8))
        ys[k * g:k * (g + 1)], proofs[g] = seen[key]
    proofs[status != 0] = 0xFF
    out = {"status": status, "ys": ys, "proofs": proofs, "commits": None, "ys_exact": ~(gok & noncanon)}
    if want_commits:
        flag = np.repeat(~gok | irregular, k)
        lg = np.zeros(width, np.int64) if irregular else logs
        out["commits"] = np.where(flag[:, None], np.array(FLAGGED, np.uint8), FM.commit_rows(rows, lg))
    return out


def expanded(coeffs, m, k, ngroups, offsets=None):
    """the groups a valid call stands for: a list of ngroups lists of k polynomials (the specification's expanded
    groups)"""
    polys = FM.expanded(coeffs, m, k * ngroups, offsets)
    return [polys[k * g:k * (g + 1)] for g in range(ngroups)]
