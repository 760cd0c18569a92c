"""Plain-numpy restatement of the rest of step08's spatial stage (include/twx_qa.h, ``twxqa_doy_norms`` and
``twxqa_spatial_only``): the day-of-year normals, the corroboration check and the mega-inconsistency check, with the
regression check taken from ``restate_spatial``.  The checker on inputs too large for the executed reference
(tests/golden/make_golden_corrob.py); agreement with the golden is tested on the CPU (test_corrob_host.py).

Independent of the kernels' formulation and of the golden maker's exec: the window of a table row comes from
``datetime`` arithmetic on the dates of 2003 / 2004; all rows of a table are computed at once from a padded
[row, value] matrix sorted twice with ``np.sort`` (the kernel sorts once and counts for the second median, and works
year by year); sums run in series order (the kernel's in sorted order); the neighbours of a day are taken with
cumulative counts over the distance-sorted columns instead of a walk with early exit.
"""
import datetime as dt

import numpy as np

import restate_spatial as RS

ANOMALY_CUTOFF, MIN_NORM_VALUES, MIN_NGHS, MAX_NGHS = 10.0, 100, 3, 7
QA_OK, QA_MISSING, QA_SPATIAL_REGRESS, QA_SPATIAL_CORROB, QA_MEGA_INCONSIST = 1, 2, 16, 17, 18
OK, FEW_NGHS, NGH_CAP = RS.OK, RS.FEW_NGHS, RS.NGH_CAP
NORM_ROWS = 731


def window_table(year):
    """[rows, 15] of month * 100 + day: the dates from 7 days before to 7 days after each date of ``year`` (2003 for the
    365-row table, 2004 for the 366-row table)."""
    d0 = dt.date(year, 1, 1)
    n = (dt.date(year + 1, 1, 1) - d0).days
    out = np.empty((n, 15), np.int32)
    for x in range(n):
        for j in range(15):
            d = d0 + dt.timedelta(days=x + j - 7)
            out[x, j] = d.month * 100 + d.day
    return out


_TABLES = {}


def _day_index(ymd):
    """Per table the series days of each row, [rows, K] padded with ndays (a slot that reads NaN); cached per axis."""
    ymd = np.asarray(ymd, np.int64)
    key = (int(ymd[0]), ymd.size)
    if key not in _TABLES:
        md = ymd % 10000
        out = []
        for year in (2003, 2004):
            member = (md[None, None, :] == window_table(year)[:, :, None]).any(1)          # [rows, ndays]
            K = int(member.sum(1).max())
            idx = np.full((member.shape[0], K), ymd.size, np.int64)
            for x in range(member.shape[0]):
                d = np.nonzero(member[x])[0]
                idx[x, :d.size] = d
            out.append(idx)
        _TABLES[key] = out
    return _TABLES[key]


def biweight_rows(X):
    """X [rows, K] with NaN padding: the biweight mean of each row's finite values, NaN below MIN_NORM_VALUES; also
    whether the row took the MAD == 0 branch."""
    n = np.isfinite(X).sum(1)
    ok = n >= MIN_NORM_VALUES
    out, mad0 = np.full(X.shape[0], np.nan), np.zeros(X.shape[0], bool)
    if not ok.any():
        return out, mad0
    X, n = X[ok], n[ok]
    r = np.arange(X.shape[0])

    def median(A):
        S = np.sort(A, axis=1)                                                       # NaN last
        return (S[r, (n - 1) // 2] + S[r, n // 2]) / 2.0

    M = median(X)
    D = X - M[:, None]
    MAD = median(np.abs(D))
    zero = MAD == 0
    with np.errstate(all="ignore"):
        u = D / (7.5 * MAD)[:, None]
        u = np.where(np.abs(u) >= 1.0, 1.0, u)
        w = (1.0 - u ** 2) ** 2
        bi = M + np.nansum(D * w, axis=1) / np.nansum(np.where(np.isfinite(D), w, np.nan), axis=1)
    res = np.where(zero, np.nansum(X, axis=1) / n, bi)
    out[ok], mad0[ok] = res, zero
    return out, mad0


def doy_norms(series, ymd, with_mad0=False):
    """The 731 normals of one series [ndays] (NaN = missing): the 365-row table, then the 366-row table."""
    pad = np.append(np.asarray(series, np.float64), np.nan)
    pad[~np.isfinite(pad)] = np.nan
    parts = [biweight_rows(pad[idx]) for idx in _day_index(ymd)]
    norms = np.concatenate([p[0] for p in parts])
    return (norms, np.concatenate([p[1] for p in parts])) if with_mad0 else norms


def norm_rows(ymd):
    """Per series day its row of the 731: yday - 1, plus 365 in a leap year."""
    ymd = np.asarray(ymd, np.int64)
    yr = ymd // 10000
    d = np.array([np.datetime64("%04d-%02d-%02d" % (v // 10000, v // 100 % 100, v % 100)) for v in (ymd[0],)])[0]
    dates = d + np.arange(ymd.size)
    yday0 = (dates - dates.astype("datetime64[Y]").astype("datetime64[D]")).astype(np.int64)
    leap = ((yr % 4 == 0) & (yr % 100 != 0)) | (yr % 400 == 0)
    return yday0 + np.where(leap, 365, 0)


def sorted_neighbours(lon, lat, i):
    """Rows within the radius of station i without i, ascending distance (equal distances: table order), and the distances."""
    d = RS.distances_km(lon, lat, i)
    j = np.nonzero(d <= RS.RADIUS_KM)[0]
    j = j[j != i]
    o = np.argsort(d[j], kind="stable")
    return j[o], d[j][o]


def corrob_station(vals, tnorm, nobs, nnorm, rows):
    """One target and variable.  vals [ndays] after the regression check's removal, tnorm [731], nobs [ndays, K] the
    neighbours in distance order, nnorm [731, K].  Returns (flag [ndays] bool, smallest |dif - cutoff| of a dif that
    was looked at, tested [ndays] bool, empty [ndays] bool: tested days without any neighbour anomaly)."""
    nd = vals.size
    flag, tested, empty = np.zeros(nd, bool), np.zeros(nd, bool), np.zeros(nd, bool)
    margin = np.inf
    if nd < 3:
        return flag, margin, tested, empty
    with np.errstate(all="ignore"):
        anom = np.abs(vals - tnorm[rows])
        A = np.abs(nobs - np.take_along_axis(nnorm, np.broadcast_to(rows[:, None], nobs.shape), 0))
    enough = np.isfinite(nobs).sum(1) >= MIN_NGHS
    V = np.isfinite(A)
    take = V & (np.cumsum(V, axis=1) <= MAX_NGHS)
    x = np.arange(1, nd - 1)
    tested[x] = np.isfinite(anom[x]) & enough[x - 1] & enough[x] & enough[x + 1]
    corr, nany = np.zeros(x.size, bool), np.zeros(x.size, bool)
    for c in (-1, 0, 1):
        with np.errstate(all="ignore"):
            dif = np.abs(A[x + c] - anom[x, None])
        look = take[x + c] & tested[x, None]
        corr |= (look & (dif < ANOMALY_CUTOFF)).any(1)
        nany |= look.any(1)
        if look.any():
            margin = min(margin, np.abs(dif[look] - ANOMALY_CUTOFF).min())
    flag[x] = tested[x] & ~corr
    empty[x] = tested[x] & ~nany
    return flag, margin, tested, empty


def mega_inconsist(tmin, tmax, ymd):
    """(flag_tmin, flag_tmax) [ndays] bool of the series as they are (NaN = missing or removed)."""
    mth = np.asarray(ymd, np.int64) // 100 % 100
    f0, f1 = np.zeros(tmin.size, bool), np.zeros(tmax.size, bool)
    for m in range(1, 13):
        a, b = (mth == m) & np.isfinite(tmin), (mth == m) & np.isfinite(tmax)
        if not a.any() or not b.any():
            continue
        f0 |= a & (tmin > tmax[b].max())
        f1 |= b & (tmax < tmin[a].min())
    return f0, f1


def run(lon, lat, tmin, tmax, ymd, targets=None, cap=None, regress=None):
    """All targets.  tmin / tmax [ndays, n] float32 / float64.  ``regress``: the result of ``restate_spatial.run`` for
    the same targets (computed if None).  Returns a dict of flags_tmin / flags_tmax [ndays, ntarget] uint8 (final), the
    boolean stage masks reg / cor / mega [2, ndays, ntarget], norms [ntarget, 2, 731], status [ntarget], near [2, ndays,
    ntarget] bool (days whose decision lies within 1e-5 of a threshold: a regression margin of the day's item or a
    corroboration dif), tested [2, ndays, ntarget], empty (tested days with an empty list of anomalies) and
    ``cutoff_margin``."""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    ymd = np.asarray(ymd, np.int64)
    targets = np.arange(lon.size) if targets is None else np.asarray(targets)
    nd, nt = ymd.size, targets.size
    if regress is None:
        regress = RS.run(lon, lat, tmin, tmax, ymd, targets=targets, cap=cap)
    obs = (np.asarray(tmin, np.float64), np.asarray(tmax, np.float64))
    rows = norm_rows(ymd)
    res = dict(reg=regress["flags"].copy(), cor=np.zeros((2, nd, nt), bool), mega=np.zeros((2, nd, nt), bool),
               norms=np.full((nt, 2, NORM_ROWS), np.nan), status=np.zeros(nt, np.int32), tested=np.zeros((2, nd, nt), bool),
               empty=np.zeros((2, nd, nt), bool), near=np.zeros((2, nd, nt), bool))
    cache = {}

    def ngh_norm(v, j):
        if (v, j) not in cache:
            cache[(v, j)] = doy_norms(obs[v][:, j], ymd)
        return cache[(v, j)]

    cutoff_margin = np.inf
    for k, i in enumerate(targets):
        i = int(i)
        ngh, _ = sorted_neighbours(lon, lat, i)
        over = cap is not None and ngh.size > cap
        res["status"][k] = NGH_CAP if over else (FEW_NGHS if ngh.size < MIN_NGHS else OK)
        after = []
        for v in range(2):
            vals = obs[v][:, i].copy()
            vals[res["reg"][v, :, k]] = np.nan
            tn = doy_norms(vals, ymd)
            res["norms"][k, v] = tn
            if res["status"][k] == OK:
                nn = np.column_stack([ngh_norm(v, int(j)) for j in ngh])
                f, margin, tested, empty = corrob_station(vals, tn, obs[v][:, ngh], nn, rows)
                res["cor"][v, :, k], res["tested"][v, :, k], res["empty"][v, :, k] = f, tested, empty
                cutoff_margin = min(cutoff_margin, margin)
                if margin < 1e-5:                               # which days: redo per day is not needed, mark by recomputation
                    res["near"][v, :, k] |= _near_days(vals, tn, obs[v][:, ngh], nn, rows)
                vals[f] = np.nan
            after.append(vals)
        m0, m1 = mega_inconsist(after[0], after[1], ymd)
        res["mega"][0, :, k], res["mega"][1, :, k] = m0, m1
    for v, name in enumerate(("flags_tmin", "flags_tmax")):
        f = np.where(np.isnan(obs[v][:, targets]), QA_MISSING, QA_OK).astype(np.uint8)
        for mask, num in ((res["reg"][v], QA_SPATIAL_REGRESS), (res["cor"][v], QA_SPATIAL_CORROB),
                          (res["mega"][v], QA_MEGA_INCONSIST)):
            f[mask & (f == QA_OK)] = num
        res[name] = f
    res["cutoff_margin"] = cutoff_margin
    res["regress_margins"] = regress["margins"]
    return res


def _near_days(vals, tnorm, nobs, nnorm, rows, eps=1e-5):
    """The days of one target and variable on which some dif that was looked at lies within eps of the cutoff."""
    nd = vals.size
    out = np.zeros(nd, bool)
    with np.errstate(all="ignore"):
        anom = np.abs(vals - tnorm[rows])
        A = np.abs(nobs - np.take_along_axis(nnorm, np.broadcast_to(rows[:, None], nobs.shape), 0))
    V = np.isfinite(A)
    take = V & (np.cumsum(V, axis=1) <= MAX_NGHS)
    x = np.arange(1, nd - 1)
    for c in (-1, 0, 1):
        with np.errstate(all="ignore"):
            dif = np.abs(A[x + c] - anom[x, None])
            out[x] |= (take[x + c] & np.isfinite(dif) & (np.abs(dif - ANOMALY_CUTOFF) < eps)).any(1)
    return out
