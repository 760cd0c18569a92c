"""numpy restatement of the twxhm_* entries (include/twx_qa.h): observation counts, monthly means, the time-of-observation
shift of Tmax and the daily homogenisation.  Written from the header's statement; tests/golden/make_golden_homog.py refuses a
fixture in which it differs from the executed reference in any bit, and the GPU tests compare the kernels with it bit for bit.

Records are station-major [nstn, ndays] float32 with NaN for "no value".
"""
import numpy as np

OK, NO_ADJ, OVERLAP = 0, 33, 34
PHA_MISSING = -9999
NAN32 = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def month_groups(year, month):
    """(mth_first, mth_ndays, mth_ymd) of a gap-free day axis."""
    ym = np.asarray(year, np.int64) * 12 + np.asarray(month, np.int64) - 1
    u, first, cnt = np.unique(ym, return_index=True, return_counts=True)
    return first.astype(np.int32), cnt.astype(np.int32), ((u // 12) * 10000 + (u % 12 + 1) * 100 + 1).astype(np.int32)


def obs_cnt(obs, day_month, first_day, last_day):
    obs, day_month = np.asarray(obs, np.float32), np.asarray(day_month)
    fin = np.isfinite(obs[:, first_day:last_day + 1])
    mon = day_month[first_day:last_day + 1]
    return np.stack([fin[:, mon == m].sum(axis=1) for m in range(1, 13)], axis=1).astype(np.int32)


def monthly_means(obs, mth_first, mth_ndays, max_miss=9):
    """The fp64 sum in day order with a non-finite day as +0.0 and the first day's value as the start, over the count."""
    obs = np.asarray(obs, np.float32)
    ns, nm = obs.shape[0], len(mth_first)
    mean, miss = np.full((ns, nm), NAN32, np.float32), np.zeros((ns, nm), np.int16)
    for g in range(nm):
        blk = obs[:, mth_first[g]:mth_first[g] + mth_ndays[g]]
        fin = np.isfinite(blk)
        val = np.where(fin, blk.astype(np.float64), 0.0)
        s = val[:, 0].copy()
        for j in range(1, blk.shape[1]):
            s = s + val[:, j]
        n = fin.sum(axis=1)
        ms = blk.shape[1] - n
        masked = (n == 0) | ((ms > max_miss) if (max_miss is not None and max_miss >= 0) else False)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = (s / n).astype(np.float32)
        mean[:, g] = np.where(masked, NAN32, m)
        miss[:, g] = ms
    return mean, miss


def tobs_shift(tmax, tobs):
    tmax, tobs = np.asarray(tmax, np.float32), np.asarray(tobs, np.float32)
    out, nshift = tmax.copy(), np.zeros(tmax.shape[0], np.int32)
    with np.errstate(invalid="ignore"):
        am = (tobs > 0) & (tobs < 1100)
    ok = ~am & np.isfinite(tmax)
    for s in range(tmax.shape[0]):
        ins = np.zeros(tmax.shape[1], bool)
        ins[1:] = am[s, 1:] & ~ok[s, :-1]
        nshift[s] = ins.sum()
        if nshift[s] > 1:
            row = np.full(tmax.shape[1], NAN32, np.float32)
            row[ok[s]] = tmax[s, ok[s]]
            idx = np.nonzero(ins)[0]
            row[idx - 1] = tmax[s, idx]
            out[s] = row
    return out, nshift


def round2(x):
    return np.rint(np.asarray(x, np.float64) * 100.0) / 100.0


def homog_daily(obs, mth_mean, mth_miss, pha, mth_ymd, mth_first, mth_ndays, adj_off, adj_ymd_start, adj_ymd_end, adj):
    obs = np.asarray(obs, np.float32)
    ns, nm = obs.shape[0], len(mth_first)
    delta = np.full((ns, nm), np.nan)
    out = obs.copy()
    status, nchanged = np.zeros(ns, np.int32), np.zeros(ns, np.int32)
    for s in range(ns):
        a0, a1 = int(adj_off[s]), int(adj_off[s + 1])
        st, en, ad = adj_ymd_start[a0:a1], adj_ymd_end[a0:a1], np.asarray(adj[a0:a1], np.float64)
        bad = OK
        for g in range(nm):
            has_m, has_h = not np.isnan(mth_mean[s, g]), pha[s, g] != PHA_MISSING
            if has_m and has_h:
                m, h = round2(np.float64(mth_mean[s, g])), round2(np.float64(pha[s, g]) / 100.0)
                if m != h:
                    delta[s, g] = h - m
                    nchanged[s] += 1
            elif has_h and mth_miss[s, g] < mth_ndays[g]:
                if a1 <= a0:
                    bad = max(bad, NO_ADJ)
                elif mth_ymd[g] < st[0]:
                    delta[s, g] = round2(-ad[0])
                else:
                    cover = np.nonzero((st <= mth_ymd[g]) & (en >= mth_ymd[g]))[0]
                    if cover.size > 1:
                        bad = max(bad, OVERLAP)
                    else:
                        delta[s, g] = round2(-ad[cover[0]] if cover.size else 0.0)
        status[s] = bad
        if bad != OK:
            delta[s], out[s], nchanged[s] = np.nan, NAN32, 0
            continue
        for g in np.nonzero(~np.isnan(delta[s]))[0]:
            sl = slice(mth_first[g], mth_first[g] + mth_ndays[g])
            out[s, sl] = (obs[s, sl].astype(np.float64) + delta[s, g]).astype(np.float32)
    return dict(delta=delta, out=out, status=status, nchanged=nchanged)
