"""numpy restatement of step20's leave-one-out outlier fits (XvalOutlier.run_xval_stn, optimize.py:113-153): the
neighbourhoods come from the CPU oracle (``pyoracle.select``: StationSelect.set_ngh_stns with rm_zero_dist_stns and
stns_rm), each of the 13 fits is an ``np.linalg.lstsq`` on sqrt(w)-scaled rows after dropping the rows with a NaN.
Independent of libtwxqa's formulation (shifted normal equations + Cholesky) and of the golden maker's pandas frames."""
import warnings

import numpy as np

from topowx_amd import stationdb as sdb


def annual(cols12):
    """[n, 12] -> [n]: pandas' mean(axis=1) (NaN skipped; NaN where a row has none)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # all-NaN rows: NaN
        return np.nanmean(cols12, axis=1)


def tables(stns):
    """(lst13, norm13), each [n, 13]: the 12 months then the annual mean."""
    lst = np.column_stack([stns[sdb.get_lst_varname(m)] for m in range(1, 13)]).astype(np.float64)
    norm = np.column_stack([stns[sdb.get_norm_varname(m)] for m in range(1, 13)]).astype(np.float64)
    return np.column_stack([lst, annual(lst)]), np.column_stack([norm, annual(norm)])


def fit_err(X, y, w, x0, y0):
    """prediction at x0 minus y0 of the WLS fit y ~ 1 + X (rows with a NaN dropped); NaN for a rank-deficient fit."""
    A = np.column_stack([np.ones(len(y)), X])
    keep = np.isfinite(y) & np.isfinite(A).all(axis=1)
    A, y, w = A[keep], y[keep], w[keep]
    if not (np.isfinite(x0).all() and np.isfinite(y0)):
        return np.nan
    sw = np.sqrt(w)
    beta, _, rank, _ = np.linalg.lstsq(A * sw[:, None], y * sw, rcond=None)
    if rank < A.shape[1]:
        return np.nan
    return float(np.concatenate([[1.0], x0]) @ beta) - y0


def xval_errs(orc, stn_da, stn_ids=None, k=100):
    """errs[13, n] of ``find_xval_outliers(stn_ids)`` (None: every station) and the per-station selection status."""
    stns = stn_da.stns
    good = np.isnan(stns[sdb.BAD])
    db = orc.Db(stn_da)                                    # pool: the good stations
    pool_pos = np.full(stns.size, -1)
    pool_pos[good] = np.arange(good.sum())
    lst13, norm13 = tables(stns)
    ids = stn_da.stn_ids if stn_ids is None else np.asarray(stn_ids)
    errs = np.full((13, ids.size), np.nan)
    status = np.zeros(ids.size, np.int32)
    geo = np.column_stack([stns[sdb.ELEV], stns[sdb.LON], stns[sdb.LAT]]).astype(np.float64)
    gi = np.nonzero(good)[0]
    for i, sid in enumerate(ids):
        r = stn_da.stn_idxs[sid]
        rc, idx, _, wgt = orc.select(db, float(stns[sdb.LAT][r]), float(stns[sdb.LON][r]), k, int(pool_pos[r]),
                                     rm_zero_dist=True)
        if rc != 0:
            status[i] = rc
            continue
        rows = gi[idx]
        for t in range(13):
            X = np.column_stack([lst13[rows, t], geo[rows]])
            x0 = np.concatenate([[lst13[r, t]], geo[r]])
            errs[t, i] = fit_err(X, norm13[rows, t], wgt, x0, norm13[r, t])
    return errs, status
