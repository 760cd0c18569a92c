"""A numpy restatement of the non-spatial precipitation QA (twx/qa/qa_prcp.py:135-176, with _qa_streak and _qa_frequent in
their places when asked for), written from the description in include/twx_qa.h and independent of the kernels'
formulation: years and months are padded matrices compared pair against pair, streaks are run-length arrays, the
frequent-value windows are a sliding view, a row of the percentile table is a boolean mask over the month-day index and
a sort.  Used for the random pools the GPU tests compare against; tests/test_prcp_host.py checks it against the
executed-reference golden.

``run(prcp, tavg, ymd, streak=False, frequent=False)``: prcp, tavg [ndays, n] float32.  Returns a dict of ``flags``
[ndays, n] uint8, ``stages`` (the flags after each check, by the check's number), ``pctiles`` [n, 366, 5] (the table of
check 15), ``pctiles_frequent`` (that of check 19, or None), ``knife`` [n] bool (a comparison of check 15 or 19 within
KNIFE relative of equality without being a tie) and ``margin`` [n] (the smallest such relative distance)."""
import numpy as np

KNIFE = 1e-6
TIE = 1e-12            # a value equal to the order statistic the percentile is (or is 1e-13 below): decided alike in any precision
OK, MISSING, DUP_YEAR, DUP_MONTH, DUP_YEAR_MONTH, IMPOSS, STREAK, GAP, CLIM, FREQUENT = 1, 2, 4, 5, 6, 8, 9, 10, 15, 19
STAGE_ORDER = (MISSING, DUP_YEAR, DUP_YEAR_MONTH, DUP_MONTH, IMPOSS, STREAK, FREQUENT, GAP, CLIM)
QS = np.array([30.0, 50.0, 70.0, 90.0, 95.0]) / 100.0
_CUM_LEAP = np.cumsum([0, 31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30])


def stage_flags(final, upto):
    """The flags after the check numbered ``upto`` from the final ones: a later check's number is still 1 there (a check
    writes only where the flag is 1, so nothing an earlier check wrote is ever overwritten)."""
    later = STAGE_ORDER[STAGE_ORDER.index(upto) + 1:]
    out = np.array(final, np.uint8)
    out[np.isin(out, later)] = OK
    return out


class Calendar(object):
    def __init__(self, ymd):
        ymd = np.asarray(ymd, np.int64)
        self.year, self.month, self.day = ymd // 10000, (ymd // 100) % 100, ymd % 100
        self.q = _CUM_LEAP[self.month - 1] + self.day - 1                  # index of the month-day in a leap year
        leap = ((self.year % 4 == 0) & (self.year % 100 != 0)) | (self.year % 400 == 0)
        self.row = np.where(leap | (self.q < 59), self.q, self.q - 1)      # yday - 1 of the day's own year
        self.years = np.unique(self.year)
        self.months = np.unique(self.month)
        nd = ymd.size
        idx = np.arange(nd)
        # padded position tables: ypos [nyears, 366], mpos [nyears, 12, 31] hold day indices, -1 = none
        yk = np.searchsorted(self.years, self.year)
        self.yk = yk
        ystart = np.array([idx[yk == k][0] for k in range(self.years.size)])
        self.ypos = np.full((self.years.size, 366), -1)
        self.ypos[yk, idx - ystart[yk]] = idx
        self.mpos = np.full((self.years.size, 12, 31), -1)
        seg = yk * 12 + self.month - 1
        first = np.full(self.years.size * 12, -1)
        for s in np.unique(seg):
            first[s] = idx[seg == s][0]
        self.mpos[yk, self.month - 1, idx - first[seg]] = idx


def _wet(x):
    return np.isfinite(x) & (x > 0)


def _pairs_equal(M, L):
    """M [k, w] padded series (NaN where there is no day or no value), L [k] their lengths: E [k, k], E[a, b] = the first
    min(L[a], L[b]) entries are all ==."""
    pos = np.arange(M.shape[1])
    with np.errstate(invalid="ignore"):
        eq = M[:, None, :] == M[None, :, :]
    beyond = pos[None, None, :] >= np.minimum(L[:, None], L[None, :])[:, :, None]
    return (eq | beyond).all(axis=2)


def _take(x, pos):
    out = np.full(pos.shape, np.nan, x.dtype)
    out[pos >= 0] = x[pos[pos >= 0]]
    return out


def dup_year(x, cal):
    Y = _take(x, cal.ypos)
    L = (cal.ypos >= 0).sum(axis=1)
    ok = _wet(Y).sum(axis=1) >= 3
    E = _pairs_equal(Y, L) & ok[:, None] & ok[None, :] & ~np.eye(L.size, dtype=bool)
    return E.any(axis=1)[cal.yk]


def dup_year_month(x, cal):
    M = _take(x, cal.mpos)                                              # [ny, 12, 31]
    L = (cal.mpos >= 0).sum(axis=2)
    ok = _wet(M).sum(axis=2) >= 3
    skip = cal.months.size - 1                                          # the month NUMBER that is never the first of a pair
    hit = np.zeros(L.shape, bool)
    m1, m2 = np.triu_indices(12, 1)
    use = (m1 + 1) != skip
    m1, m2 = m1[use], m2[use]
    for k in range(L.shape[0]):
        E = _pairs_equal(M[k], L[k])
        d = E[m1, m2] & ok[k, m1] & ok[k, m2]
        hit[k, m1[d]] = True
        hit[k, m2[d]] = True
    return hit[cal.yk, cal.month - 1]


def dup_month(x, cal):
    M = _take(x, cal.mpos)
    L = (cal.mpos >= 0).sum(axis=2)
    ok = _wet(M).sum(axis=2) >= 3
    hit = np.zeros(L.shape, bool)
    for m in range(12):
        E = _pairs_equal(M[:, m], L[:, m]) & ok[:, m, None] & ok[None, :, m] & ~np.eye(L.shape[0], dtype=bool)
        hit[:, m] = E.any(axis=1)
    return hit[cal.yk, cal.month - 1]


def imposs(x):
    x32 = x.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (x32 < np.float32(0.0)) | (x32 > np.float32(182.88))


def streak_mask(x):
    idx = np.nonzero(_wet(x))[0]
    mask = np.zeros(x.size, bool)
    if idx.size == 0:
        return mask
    v = x[idx]
    starts = np.r_[0, np.nonzero(v[1:] != v[:-1])[0] + 1]
    lens = np.diff(np.r_[starts, v.size])
    for s, n in zip(starts[:-1], lens[:-1]):                            # the last run has no different value after it
        if n >= 20:
            mask[idx[s:s + n]] = True
    return mask


def frequent_mask(x, cal, table, margin):
    idx = np.nonzero(_wet(x))[0]
    mask = np.zeros(x.size, bool)
    n = idx.size
    if n == 0:
        return mask
    v = x[idx].astype(np.float64)
    P = table[cal.row[idx]][:, :4]                                      # the four columns at each value's own day
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(v[:, None] / P - 1.0)
    ge = v[:, None] >= P                                                # a NaN percentile: False
    pad = 9
    vp = np.r_[v, np.full(pad, np.nan)]
    gp = np.r_[ge, np.zeros((pad, 4), bool)]
    W = np.lib.stride_tricks.sliding_window_view(vp, 10)[:n]            # [n, 10] windows (NaN beyond the end)
    G = np.lib.stride_tricks.sliding_window_view(gp, 10, axis=0)[:n]    # [n, 4, 10]
    with np.errstate(invalid="ignore"):
        same = W[:, :, None] == W[:, None, :]                           # [n, i, j]: value j equals value i
    cnt = same.sum(axis=2)
    hold = np.zeros(cnt.shape, bool)
    used = np.zeros((n, 4), bool)                                       # the comparisons the check makes: tiers with cnt >= need
    for t, need in enumerate((9, 8, 7, 5)):
        w, i = np.nonzero((cnt >= need) & np.isfinite(W))
        used[w + i, t] = True
        allge = (~same | G[:, t][:, None, :]).all(axis=2)               # every occurrence of value i is >= its percentile
        hold |= (cnt >= need) & allge
    hold &= np.isfinite(W)
    rel = rel[used]
    margin.append(rel[np.isfinite(rel) & (rel > TIE)])
    w, i = np.nonzero(hold)
    mask[idx[w + i]] = True
    return mask


def gap(x, cal):
    mask = np.zeros(x.size, bool)
    x32 = x.astype(np.float32)
    wet = _wet(x)
    for m in cal.months:
        sel = wet & (cal.month == m)
        if not sel.any():
            continue
        s = np.sort(x32[sel])
        step = np.nonzero(np.diff(s) >= np.float32(30.0))[0]
        if step.size:
            mask |= sel & (x32 >= s[step[0] + 1])
    return mask


def percentiles(x, cal):
    """[366, 5] float64 from the values widened exactly; numpy's linear interpolation with the two-sided lerp."""
    out = np.full((366, 5), np.nan)
    wet = _wet(x)
    v, q = x[wet].astype(np.float64), cal.q[wet]
    for r in range(366):
        d = (q - r) % 366
        s = np.sort(v[(d <= 14) | (d >= 366 - 14)])
        n = s.size
        if n < 20:
            continue
        vi = (n - 1) * QS
        lo = np.floor(vi).astype(int)
        g = vi - lo
        a, b = s[lo], s[np.minimum(lo + 1, n - 1)]
        diff = b - a
        out[r] = np.where(g >= 0.5, b - diff * (1 - g), a + diff * g)
    return out


def clim(x, tavg, cal, table, margin):
    wet = _wet(x)
    with np.errstate(invalid="ignore"):
        m = np.where(tavg < 0, 5.0, 9.0)
    bound = m * table[cal.row, 4]
    v = x.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(v[wet] / bound[wet] - 1.0)
        margin.append(rel[np.isfinite(rel) & (rel > TIE)])
        return wet & (v >= bound)


def run(prcp, tavg, ymd, streak=False, frequent=False):
    prcp, tavg = np.asarray(prcp, np.float32), np.asarray(tavg, np.float32)
    cal = Calendar(ymd)
    nd, n = prcp.shape
    flags = np.ones((nd, n), np.uint8)
    stages = {k: np.ones((nd, n), np.uint8) for k in STAGE_ORDER}
    tables = np.full((n, 366, 5), np.nan)
    tables_f = np.full((n, 366, 5), np.nan) if frequent else None
    margins = np.full(n, np.inf)
    for s in range(n):
        x, f, mg = prcp[:, s].copy(), flags[:, s], []

        def update(mask, num):
            x[mask] = np.nan
            f[mask & (f == OK)] = num
            stages[num][:, s] = f

        update(np.isnan(x), MISSING)
        update(dup_year(x, cal), DUP_YEAR)
        update(dup_year_month(x, cal), DUP_YEAR_MONTH)
        update(dup_month(x, cal), DUP_MONTH)
        update(imposs(x), IMPOSS)
        update(streak_mask(x) if streak else np.zeros(nd, bool), STREAK)
        if frequent:
            tables_f[s] = percentiles(x, cal)
            update(frequent_mask(x, cal, tables_f[s], mg), FREQUENT)
        else:
            update(np.zeros(nd, bool), FREQUENT)
        update(gap(x, cal), GAP)
        tables[s] = percentiles(x, cal)
        update(clim(x, tavg[:, s], cal, tables[s], mg), CLIM)
        mg = np.concatenate(mg) if mg else np.zeros(0)
        if mg.size:
            margins[s] = mg.min()
    return dict(flags=flags, stages=stages, pctiles=tables, pctiles_frequent=tables_f, knife=margins < KNIFE, margin=margins)
