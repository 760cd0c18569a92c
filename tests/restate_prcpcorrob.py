"""A numpy restatement of the precipitation QA's spatial corroboration check (flag 17) as include/twx_qa.h states it for
``twxpc_spatial_corrob``: cumulative counts over distance-sorted neighbour columns, no per-day Python loop.  It is written
from that statement, not from the library's kernels: the tests compare the two, and the executed-reference golden
(tests/golden/make_golden_prcpcorrob.py) pins the restatement.

``run(lon, lat, prcp, ymd, targets, flags)``: prcp [ndays, nstn] (the pool as it is), flags [ndays, ntarget] the flags of
the checks before (a target's series is its pool value where the flag is 1).  Returns a dict: ``flags``, ``status``,
``abs_dif``, ``pctile``, ``thres`` [ndays, ntarget] (NaN where the day did not get that far), ``margin`` [ndays, ntarget]
(the relative distance of abs_dif from thres where both exist, inf elsewhere) and ``nngh``."""
import numpy as np

RADIAN = 0.017453292519943295
EARTH_KM = 6371.009
NGH_RADIUS = 75.0
MIN_NGHS, MAX_NGHS = 3, 7
MIN_PERCENTILE_VALUES = 20
THRES = 26.924
THRES_MM = 26.924 * 10.0
MAX_RADIUS_NGH = 256
SP_OK, SP_FEW_NGHS, SP_NGH_CAP = 0, 1, 7
QA_OK, QA_MISSING, QA_SPATIAL_CORROB = 1, 2, 17
_CUM = np.cumsum([0, 31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30])


def grt_circle_dist(lon1, lat1, lon2, lat2):
    lat1rad, lon1rad = lat1 * RADIAN, lon1 * RADIAN
    lat2rad, lon2rad = np.asarray(lat2) * RADIAN, np.asarray(lon2) * RADIAN
    a = np.sin((lat1rad - lat2rad) / 2.0) ** 2 + (np.cos(lat1rad) * np.cos(lat2rad)) * np.sin((lon1rad - lon2rad) / 2.0) ** 2
    return EARTH_KM * (2.0 * np.arcsin(np.sqrt(a)))


def calendar(ymd):
    """(row [ndays]: yday - 1 of the day's own year, mday [ndays]: the month-day's index among the dates of 2004)."""
    ymd = np.asarray(ymd, np.int64)
    y, m, d = ymd // 10000, (ymd // 100) % 100, ymd % 100
    mday = _CUM[m - 1] + d - 1
    leap = ((y % 4 == 0) & (y % 100 != 0)) | (y % 400 == 0)
    row = mday - ((m > 2) & ~leap)
    return row.astype(np.int64), mday.astype(np.int64)


def pors_counts(vals, ymd):
    """[366] or [366, n]: the finite values > 0 of each column within 14 days of each date of 2004."""
    v = np.asarray(vals)
    one = v.ndim == 1
    v = v.reshape(v.shape[0], -1)
    _, mday = calendar(ymd)
    wet = np.isfinite(v) & (v > 0)
    hist = np.zeros((366, v.shape[1]), np.int64)
    np.add.at(hist, mday, wet.astype(np.int64))
    out = np.zeros_like(hist)
    for j in range(-14, 15):
        out += np.roll(hist, -j, axis=0)
    return out[:, 0] if one else out


def neighbours(lon, lat, s):
    """Columns of the stations within 75 km of s, self excluded, ascending distance, equal distances in table order."""
    d = grt_circle_dist(lon[s], lat[s], lon, lat)
    idx = np.nonzero((d <= NGH_RADIUS) & (np.arange(lon.size) != s))[0]
    return idx[np.argsort(d[idx], kind="stable")], d


def _triple(a, fill):
    """a [ndays, ...] -> (a at x - 1, a at x, a at x + 1) for every x, ``fill`` beyond the ends."""
    pad = np.full((1,) + a.shape[1:], fill, a.dtype)
    return np.concatenate([pad, a[:-1]]), a, np.concatenate([a[1:], pad])


def check_target(x, obs, row, basis_t, basis_n, window_of):
    """x [ndays] float64 (NaN outside the series), obs [ndays, m] the neighbours in distance order, row [ndays], basis_t
    [366] bool, basis_n [366, m] bool, window_of(r) -> the sorted values of the target's row r."""
    nd = x.size
    fin = np.isfinite(obs)
    nfin = fin.sum(axis=1)
    first7 = fin & (np.cumsum(fin, axis=1) <= MAX_NGHS)
    o = obs.astype(np.float64)
    mx7 = np.where(first7, o, -np.inf).max(axis=1, initial=-np.inf)
    mn7 = np.where(first7, o, np.inf).min(axis=1, initial=np.inf)
    mxa = np.where(fin, o, -np.inf).max(axis=1, initial=-np.inf)
    mna = np.where(fin, o, np.inf).min(axis=1, initial=np.inf)
    nbas = (fin & basis_n[row, :]).sum(axis=1)                  # finite neighbours with a basis at the day's own row
    c3 = np.minimum.reduce(_triple(nfin, 0))
    b3 = np.minimum.reduce(_triple(nbas, 0))
    hi7, lo7 = np.maximum.reduce(_triple(mx7, -np.inf)), np.minimum.reduce(_triple(mn7, np.inf))
    hia, loa = np.maximum.reduce(_triple(mxa, -np.inf)), np.minimum.reduce(_triple(mna, np.inf))
    tested = ~np.isnan(x)
    tested[[0, -1]] = False
    tested &= c3 >= MIN_NGHS
    above, below = tested & (x > hi7), tested & (x < lo7)
    abs_dif = np.full(nd, np.nan)
    abs_dif[above] = np.abs(x[above] - hi7[above])
    abs_dif[below] = np.abs(x[below] - lo7[below])
    reach = above | below
    thres = np.full(nd, np.nan)
    thres[reach] = THRES
    pctile = np.full(nd, np.nan)
    ranked = reach & basis_t[row] & (b3 >= MIN_NGHS)
    for r in np.unique(row[ranked]):
        dd = np.nonzero(ranked & (row == r))[0]
        w = window_of(int(r))
        left, right = np.searchsorted(w, x[dd], "left"), np.searchsorted(w, x[dd], "right")
        pctile[dd] = (left + right + (left < right)) * (50.0 / w.size)
    dd = np.nonzero(ranked)[0]
    p = pctile[dd]
    dif = np.where(p > hia[dd], np.abs(p - hia[dd]), np.where(p < loa[dd], np.abs(p - loa[dd]), 0.0))
    with np.errstate(divide="ignore"):
        thres[dd] = np.where(dif == 0, THRES, (-45.72 * np.log(np.where(dif == 0, 1.0, dif)) + THRES_MM) / 10.0)
    flag = reach & (abs_dif > np.where(reach, thres, np.inf))
    return flag, abs_dif, pctile, thres


def run(lon, lat, prcp, ymd, targets, flags):
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    prcp = np.asarray(prcp, np.float32)
    nd, n = prcp.shape
    targets = np.asarray(targets, np.int64)
    flags = np.asarray(flags, np.uint8)
    row, mday = calendar(ymd)
    pool_cnt = pors_counts(prcp, ymd)
    out = {k: np.full((nd, targets.size), np.nan) for k in ("abs_dif", "pctile", "thres")}
    out["flags"] = flags.copy()
    out["status"] = np.zeros(targets.size, np.int32)
    out["nngh"] = np.zeros(targets.size, np.int32)
    out["margin"] = np.full((nd, targets.size), np.inf)
    dq = (mday[None, :] - np.arange(366)[:, None]) % 366
    inwin = (dq <= 14) | (dq >= 352)                             # [366, ndays]
    for k, s in enumerate(targets):
        ngh, _ = neighbours(lon, lat, int(s))
        out["nngh"][k] = ngh.size
        if ngh.size > MAX_RADIUS_NGH:
            out["status"][k] = SP_NGH_CAP
            continue
        if ngh.size < MIN_NGHS:
            out["status"][k] = SP_FEW_NGHS
            continue
        x = np.where(flags[:, k] == QA_OK, prcp[:, s], np.float32(np.nan)).astype(np.float64)
        if nd < 3:
            continue
        wet = np.isfinite(x) & (x > 0)
        cnt_t = pors_counts(x, ymd)

        def window_of(r, x=x, wet=wet):
            return np.sort(x[wet & inwin[r]])

        fl, ad, pc, th = check_target(x, prcp[:, ngh], row, cnt_t > MIN_PERCENTILE_VALUES,
                                      pool_cnt[:, ngh] > MIN_PERCENTILE_VALUES, window_of)
        out["abs_dif"][:, k], out["pctile"][:, k], out["thres"][:, k] = ad, pc, th
        both = np.isfinite(ad) & np.isfinite(th)
        with np.errstate(all="ignore"):
            out["margin"][both, k] = np.abs(ad[both] / th[both] - 1.0)
        col = out["flags"][:, k]
        col[fl & (col == QA_OK)] = QA_SPATIAL_CORROB
    return out
