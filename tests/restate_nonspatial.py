"""Plain-numpy restatement of step08's non-spatial checks (include/twx_qa.h, ``twxqa_non_spatial``): the checker of the
GPU results on inputs too large for the executed reference (tests/golden/make_golden_nonspatial.py); agreement with
the golden is tested on the CPU (test_nonspatial_host.py).

Independent of the kernels' formulation and of the golden maker's exec: a removal really sets the working copy to NaN
(the kernels keep flags only); the duplicate checks compare padded [year, 366] and [year, 12, 31] matrices all pairs at
once (the kernels walk pairs with early exit); run lengths of the streak check come from cumulative counts over the
non-missing values (the kernel: ballots over blocks of 64 days); the gap check uses ``np.sort`` / ``np.diff`` per month
(the kernel: a bitonic sort of 31 slots per year); all rows of a day-of-year table are computed at once from a padded
[row, value] matrix sorted twice, sums in series order (the kernel: one row per workgroup, sorted once, sums in sorted
order); the lagged range is a scatter of the day's condition over its window (the kernel gathers).  float32 where the
specification says float32, fp64 elsewhere.
"""
import numpy as np

import restate_corrob as RC

(QA_OK, QA_MISSING, QA_NAUGHT, QA_DUP_YEAR, QA_DUP_MONTH, QA_DUP_YEAR_MONTH, QA_DUP_WITHIN_MONTH, QA_IMPOSS_VALUE, QA_STREAK,
 QA_GAP, QA_INTERNAL_INCONSIST, QA_LAGRANGE_INCONSIST, QA_SPIKE_DIP) = range(1, 14)
QA_CLIM_OUTLIER, QA_MEGA_INCONSIST = 15, 18
ORDER = (2, 3, 4, 6, 5, 7, 8, 9, 10, 15, 11, 13, 12, 18)
F32 = np.float32
KNIFE = 6.0e-7              # |z - 6| below this: the decision may fall either way between two fp64 formulations


class _Axis(object):
    """Calendar tables of a day axis, cached by (first day, length)."""
    _cache = {}

    def __init__(self, ymd):
        ymd = np.asarray(ymd, np.int64)
        self.year, self.month = ymd // 10000, ymd // 100 % 100
        self.yk = self.year - self.year[0]                                # year index
        self.ny = int(self.yk[-1]) + 1
        first_of_year = np.searchsorted(self.yk, np.arange(self.ny))
        self.ypos = np.arange(ymd.size) - first_of_year[self.yk]          # position among the year's days on the axis
        seg = self.yk * 12 + self.month - 1
        self.seg = seg
        first_of_seg = np.full(self.ny * 12, -1, np.int64)
        u, i = np.unique(seg, return_index=True)
        first_of_seg[u] = i
        self.mpos = np.arange(ymd.size) - first_of_seg[seg]
        self.ylen = np.bincount(self.yk, minlength=self.ny)
        self.mlen = np.bincount(seg, minlength=self.ny * 12).reshape(self.ny, 12)
        self.ndistinct = np.unique(self.month).size
        self.rows = RC.norm_rows(ymd)
        self.day_index = RC._day_index(ymd)

    @classmethod
    def of(cls, ymd):
        key = (int(ymd[0]), len(ymd))
        if key not in cls._cache:
            cls._cache[key] = cls(ymd)
        return cls._cache[key]


def _dup_pairs(P, lens):
    """P [k, L] padded with NaN, lens [k]: the boolean [k, k] of pairs whose first min(len, len) positions are all ==
    and that both hold a value."""
    k, L = P.shape
    has = np.isfinite(P).any(1) | np.isinf(P).any(1)
    with np.errstate(invalid="ignore"):
        eq = P[:, None, :] == P[None, :, :]
    n = np.minimum(lens[:, None], lens[None, :])
    inside = np.arange(L)[None, None, :] < n[:, :, None]
    return (eq | ~inside).all(2) & has[:, None] & has[None, :] & (n > 0)


def dup_year(v, ax):
    Y = np.full((ax.ny, 366), np.nan, F32)
    Y[ax.yk, ax.ypos] = v
    D = np.triu(_dup_pairs(Y, ax.ylen), 1)
    bad = D.any(0) | D.any(1)
    return bad[ax.yk]


def dup_year_month(v, ax):
    M = np.full((ax.ny, 12, 31), np.nan, F32)
    M[ax.yk, ax.month - 1, ax.mpos] = v
    bad = np.zeros((ax.ny, 12), bool)
    skip = ax.ndistinct - 1                                             # a month NUMBER (the reference's quirk)
    for k in range(ax.ny):
        D = np.triu(_dup_pairs(M[k], ax.mlen[k]), 1)
        if 1 <= skip <= 12:
            D[skip - 1, :] = False
        bad[k] = D.any(0) | D.any(1)
    return bad[ax.yk, ax.month - 1]


def dup_month(v, ax):
    M = np.full((ax.ny, 12, 31), np.nan, F32)
    M[ax.yk, ax.month - 1, ax.mpos] = v
    bad = np.zeros((ax.ny, 12), bool)
    for m in range(12):
        D = np.triu(_dup_pairs(M[:, m], ax.mlen[:, m]), 1)
        bad[:, m] = D.any(0) | D.any(1)
    return bad[ax.yk, ax.month - 1]


def dup_within_month(a, b, ax):
    with np.errstate(invalid="ignore"):
        same = a == b
    cnt = np.bincount(ax.seg[same], minlength=ax.ny * 12)
    return cnt[ax.seg] >= 10


def streaks(v):
    out = np.zeros(v.size, bool)
    idx = np.nonzero(~np.isnan(v))[0]
    if idx.size == 0:
        return out
    x = v[idx]
    run = np.cumsum(np.r_[True, x[1:] != x[:-1]]) - 1
    length = np.bincount(run)
    hit = (length[run] >= 20) & (run < run[-1])                         # the last run has no value that ends it
    out[idx[hit]] = True
    return out


def gap(v, ax):
    out = np.zeros(v.size, bool)
    for m in range(1, 13):
        sel = ax.month == m
        s = np.sort(v[sel & ~np.isnan(v)]).astype(F32)
        n = s.size
        if n == 0:
            continue
        med = s[n // 2] if n & 1 else F32(F32(s[n // 2 - 1] + s[n // 2]) / F32(2))
        top, bot = s[s >= med], s[s <= med]
        i = np.nonzero(np.diff(top) >= F32(10))[0]
        if i.size:
            out |= sel & (v >= top[i[0] + 1])
        i = np.nonzero(np.diff(bot) >= F32(10))[0]
        if i.size:
            out |= sel & (v <= bot[i[-1]])
    return out


def biweight_rows(X):
    """X [rows, K] with NaN padding: (mean, std, mad0) of each row's finite values, NaN below 100 values."""
    n = np.isfinite(X).sum(1)
    ok = n >= RC.MIN_NORM_VALUES
    mean, std, mad0 = np.full(X.shape[0], np.nan), np.full(X.shape[0], np.nan), np.zeros(X.shape[0], bool)
    if not ok.any():
        return mean, std, mad0
    X, n = X[ok], n[ok]
    r = np.arange(X.shape[0])

    def median(A):
        S = np.sort(A, axis=1)                                           # NaN last
        return (S[r, (n - 1) // 2] + S[r, n // 2]) / 2.0

    M = median(X)
    D = X - M[:, None]
    MAD = median(np.abs(D))
    zero = MAD == 0
    fin = np.isfinite(D)
    with np.errstate(all="ignore"):
        u = D / (7.5 * MAD)[:, None]
        u = np.where(np.abs(u) >= 1.0, 1.0, u)
        h = np.where(fin, 1.0 - u ** 2, 0.0)
        D0 = np.where(fin, D, 0.0)
        bi = M + (D0 * h ** 2).sum(1) / (h ** 2).sum(1)
        sbi = np.sqrt(n * (D0 ** 2 * h ** 4).sum(1)) / np.abs((h * np.where(fin, 1.0 - 5.0 * u ** 2, 0.0)).sum(1))
        pm = np.where(fin, X, 0.0).sum(1) / n
        ps = np.sqrt(np.where(fin, (X - pm[:, None]) ** 2, 0.0).sum(1) / (n - 1))
    mean[ok], std[ok], mad0[ok] = np.where(zero, pm, bi), np.where(zero, ps, sbi), zero
    return mean, std, mad0


def clim_rows(v, ax):
    """[731, 2] (mean, std) of one series and the rows that took the MAD == 0 branch."""
    pad = np.append(np.asarray(v, np.float64), np.nan)
    pad[~np.isfinite(pad)] = np.nan
    parts = [biweight_rows(pad[idx]) for idx in ax.day_index]
    return (np.stack([np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])], 1),
            np.concatenate([p[2] for p in parts]))


def clim_outliers(v, ax):
    norms, mad0 = clim_rows(v, ax)
    with np.errstate(all="ignore"):
        z = np.abs((v.astype(np.float64) - norms[ax.rows, 0]) / norms[ax.rows, 1])
    zf = z[np.isfinite(z)]
    margin = np.abs(zf - 6.0).min() if zf.size else np.inf
    return np.nan_to_num(z, nan=0.0) >= 6.0, norms, margin, mad0


def spikes(v):
    out = np.zeros(v.size, bool)
    if v.size >= 3:
        with np.errstate(invalid="ignore"):
            out[1:-1] = (np.abs(v[1:-1] - v[:-2]) >= F32(25)) & (np.abs(v[1:-1] - v[2:]) >= F32(25))
    return out


def lagrange(a, b):
    """(mask_tmin, mask_tmax, smallest distance of a comparison from equality)."""
    nd = a.size
    lo = np.r_[np.nan, a.astype(np.float64), np.nan]
    hi = np.r_[np.nan, b.astype(np.float64), np.nan]
    with np.errstate(all="ignore"):
        mx = np.fmax(np.fmax(lo[:-2], lo[1:-1]), lo[2:])
        mn = np.fmin(np.fmin(hi[:-2], hi[1:-1]), hi[2:])
        ok = ~np.isnan(mx) & ~np.isnan(mn)
        c_hi = ok & (hi[1:-1] >= mx + 40.0)
        c_lo = ok & (lo[1:-1] <= mn - 40.0)
        d = np.r_[(hi[1:-1] - (mx + 40.0))[ok], (lo[1:-1] - (mn - 40.0))[ok]]
    d = d[np.isfinite(d)]
    margin = np.abs(d).min() if d.size else np.inf

    def spread(c):
        w = np.r_[False, c, False]
        return w[:-2] | w[1:-1] | w[2:]

    assert c_hi.size == nd
    return c_lo | spread(c_hi), c_hi | spread(c_lo), margin


def station(tmin, tmax, ymd):
    """One station: (flags_tmin, flags_tmax [ndays] uint8, norms [2, 731, 2], info)."""
    ax = _Axis.of(ymd)
    v = [np.array(tmin, F32), np.array(tmax, F32)]
    f = [np.ones(v[0].size, np.uint8), np.ones(v[0].size, np.uint8)]

    def remove(masks, num):
        for k in range(2):
            f[k][masks[k] & (f[k] == QA_OK)] = num
            v[k][masks[k]] = np.nan

    remove([np.isnan(v[0]), np.isnan(v[1])], QA_MISSING)
    with np.errstate(invalid="ignore"):
        us = [np.rint(x * F32(10)) / F32(10) == F32(-17.8) for x in v]
        naught = (us[0] & us[1]) | ((v[0] == 0) & (v[1] == 0))
    remove([naught, naught], QA_NAUGHT)
    remove([dup_year(x, ax) for x in v], QA_DUP_YEAR)
    remove([dup_year_month(x, ax) for x in v], QA_DUP_YEAR_MONTH)
    remove([dup_month(x, ax) for x in v], QA_DUP_MONTH)
    m = dup_within_month(v[0], v[1], ax)
    remove([m, m], QA_DUP_WITHIN_MONTH)
    with np.errstate(invalid="ignore"):
        remove([(x < F32(-89.4)) | (x > F32(57.7)) for x in v], QA_IMPOSS_VALUE)
    remove([streaks(x) for x in v], QA_STREAK)
    remove([gap(x, ax) for x in v], QA_GAP)
    res = [clim_outliers(x, ax) for x in v]
    norms = np.stack([r[1] for r in res])
    z_margin = min(r[2] for r in res)
    remove([r[0] for r in res], QA_CLIM_OUTLIER)
    with np.errstate(invalid="ignore"):
        m = v[0] > v[1]
    remove([m, m], QA_INTERNAL_INCONSIST)
    remove([spikes(x) for x in v], QA_SPIKE_DIP)
    m0, m1, lag_margin = lagrange(v[0], v[1])
    remove([m0, m1], QA_LAGRANGE_INCONSIST)
    remove(list(RC.mega_inconsist(v[0], v[1], ymd)), QA_MEGA_INCONSIST)
    info = dict(z_margin=z_margin, lag_margin=lag_margin, knife=bool(z_margin < KNIFE), mad0=int(res[0][3].sum() + res[1][3].sum()),
                std0=bool((norms[:, :, 1] == 0).any()))
    return f[0], f[1], norms, info


def run(tmin, tmax, ymd):
    """tmin / tmax [ndays, n].  Returns a dict of flags_tmin / flags_tmax [ndays, n] uint8, norms [n, 2, 731, 2], knife
    [n] bool (some |z - 6| within 1e-7 * 6 of the threshold: the series is to be left out of an exact comparison),
    z_margin / lag_margin [n], mad0 [n] (rows that took the MAD == 0 branch) and std0 [n] bool."""
    tmin, tmax = np.asarray(tmin, F32), np.asarray(tmax, F32)
    nd, n = tmin.shape
    out = dict(flags_tmin=np.zeros((nd, n), np.uint8), flags_tmax=np.zeros((nd, n), np.uint8),
               norms=np.full((n, 2, 731, 2), np.nan), knife=np.zeros(n, bool), z_margin=np.zeros(n), lag_margin=np.zeros(n),
               mad0=np.zeros(n, np.int64), std0=np.zeros(n, bool))
    for s in range(n):
        f0, f1, norms, info = station(tmin[:, s], tmax[:, s], ymd)
        out["flags_tmin"][:, s], out["flags_tmax"][:, s], out["norms"][s] = f0, f1, norms
        for k in ("knife", "z_margin", "lag_margin", "mad0", "std0"):
            out[k][s] = info[k]
    return out
