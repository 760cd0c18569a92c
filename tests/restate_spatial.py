"""Plain-numpy restatement of step08's spatial regression check (include/twx_qa.h, ``twxqa_spatial_regress``): the
checker on inputs too large for the executed reference (tests/golden/make_golden_spatial.py), as
``outlier_restatement`` is for the outlier screen.

Independent of the kernel's formulation and of the golden maker's exec: one station and variable at a time, vectorised
over ALL of its months and window days at once ([neighbour, month, slot] arrays) instead of a walk per item; the
regression and Pearson's r from raw moments of data shifted by the item's first observation (the kernel centres on
the means); the seven heaviest contributing neighbours of a day by a cumulative count over the weight-sorted list
instead of a sequential walk with early exit.  Agreement with the golden is tested on the CPU (test_spatial_host.py).
"""
import numpy as np

RADIUS_KM, EARTH_KM = 75.0, 6371.009
MIN_DAYS, MIN_NGHS, MAX_NGHS, BUFFER = 40, 3, 7, 15
NGH_CORR, RESID_CUTOFF, RESID_STD_CUTOFF = 0.8, 8.0, 4.0
OK, FEW_NGHS, DEGENERATE, NGH_CAP, FEW_DAYS, FEW_VALID = 0, 1, 4, 7, 16, 17
NSLOT = 63


def distances_km(lon, lat, i):
    """Haversine distance of station i to every station."""
    p1, p2 = np.radians(lat[i]), np.radians(lat)
    h = np.sin((p1 - p2) / 2.0) ** 2 + np.cos(p1) * np.cos(p2) * np.sin((np.radians(lon[i]) - np.radians(lon)) / 2.0) ** 2
    return EARTH_KM * 2.0 * np.arcsin(np.sqrt(h))


def neighbours(lon, lat, i):
    """Table rows within the radius of station i, ascending, without i."""
    j = np.nonzero(distances_km(lon, lat, i) <= RADIUS_KM)[0]
    return j[j != i]


def month_table(ymd):
    """(ws, we, ms, me) per calendar month from that of the first to that of the last day: window and month as
    half-open ranges of series indices, clipped to the series."""
    ymd = np.asarray(ymd, np.int64)
    nd = ymd.size
    iso = lambda v: "%04d-%02d-%02d" % (v // 10000, v // 100 % 100, v % 100)  # noqa: E731
    d0, d1 = np.datetime64(iso(ymd[0])), np.datetime64(iso(ymd[-1]))
    starts = np.arange(d0.astype("datetime64[M]"), d1.astype("datetime64[M]") + 2).astype("datetime64[D]")
    a = (starts - d0).astype(np.int64)
    a, b = a[:-1], a[1:]
    return np.maximum(0, a - BUFFER), np.minimum(nd, b + BUFFER), np.maximum(0, a), np.minimum(nd, b)


def check_station(obs, ymd, i, ngh, cap=None):
    """One target and variable.  obs [ndays, n] (NaN = missing), ngh: its radius list.  Returns a dict of flag [ndays]
    bool, est [ndays], r / nvalid / status [nmonths] and the weight-sorted models w / slope / icpt / col [K, nmonths]
    (rows past nvalid are NaN / -1), resid / resid_std [ndays] (NaN where not computed)."""
    obs = np.asarray(obs, np.float64)
    nd = obs.shape[0]
    ws, we, ms, me = month_table(ymd)
    nm, K = ws.size, ngh.size
    out = dict(flag=np.zeros(nd, bool), est=np.full(nd, np.nan), r=np.full(nm, np.nan), nvalid=np.zeros(nm, np.int32),
               status=np.zeros(nm, np.int32), resid=np.full(nd, np.nan), resid_std=np.full(nd, np.nan),
               w=np.full((K, nm), np.nan), slope=np.full((K, nm), np.nan), icpt=np.full((K, nm), np.nan),
               col=np.full((K, nm), -1, np.int64))
    if cap is not None and K > cap:
        out["status"][:] = NGH_CAP
        return out
    if K < MIN_NGHS:
        out["status"][:] = FEW_NGHS
        return out
    slot = np.arange(NSLOT)
    day = ws[:, None] - 1 + slot[None, :]                                  # [nm, 63] series day of a slot
    nwin = (we - ws)[:, None]
    in_win = (slot[None, :] >= 1) & (slot[None, :] <= nwin)
    in_ser = (slot[None, :] <= nwin + 1) & (day >= 0) & (day < nd)
    pad = np.vstack([obs, np.full((1, obs.shape[1]), np.nan)])             # row nd: a day outside the series
    didx = np.where(in_ser, day, nd)
    T = np.where(in_win, pad[didx, i], np.nan)                             # [nm, 63]
    tf = np.isfinite(T)
    N = np.moveaxis(pad[didx][:, :, ngh], 2, 0)                            # [K, nm, 63]
    ov = tf[None] & np.isfinite(N)
    cnt = ov.sum(2)
    with np.errstate(all="ignore"):
        spread = lambda a: np.where(ov, a, -np.inf).max(2) != np.where(ov, a, np.inf).min(2)  # noqa: E731
        valid = (cnt >= MIN_DAYS) & spread(np.broadcast_to(T, N.shape)) & spread(N)
        # raw moments of the data shifted by the item's first finite observation
        first = np.take_along_axis(T, np.argmax(tf, axis=1)[:, None], 1)   # [nm, 1]
        shift = np.where(np.isfinite(first), first, 0.0)
        y = np.where(ov, T[None] - shift[None], 0.0)
        x = np.where(ov, N - shift[None], 0.0)
        n = cnt.astype(np.float64)
        sx, sy, sxx, sxy = x.sum(2), y.sum(2), (x * x).sum(2), (x * y).sum(2)
        slope = (n * sxy - sx * sy) / (n * sxx - sx * sx)
        icpt_shifted = (sy - slope * sx) / n                               # y' = icpt' + slope x'  with x' = x - c, y' = y - c
        icpt = icpt_shifted + shift[:, 0][None] - slope * shift[:, 0][None]
        o_mean = (sy / n)[:, :, None] + shift[None]
        num = np.where(ov, np.abs(N - T[None]), 0.0).sum(2)
        den = np.where(ov, np.abs(N - o_mean) + np.abs(T[None] - o_mean), 0.0).sum(2)
        w = 1.0 - num / den
    w = np.where(valid, w, -np.inf)
    nvalid = valid.sum(0)
    order = np.argsort(-w, axis=0, kind="stable")                          # heaviest first; equal weights: table order
    take = lambda a: np.take_along_axis(a, order, 0)  # noqa: E731
    ws_, sl_, ic_, va_ = take(w), take(slope), take(icpt), take(valid)
    Ns = np.take_along_axis(N, order[:, :, None], 0)
    nanc = np.full(Ns.shape[:2] + (1,), np.nan)
    cand = np.stack([np.concatenate([nanc, Ns[:, :, :-1]], 2), Ns, np.concatenate([Ns[:, :, 1:], nanc], 2)])  # prev, own, next
    with np.errstate(all="ignore"):
        dif = np.where(np.isfinite(cand), np.abs(cand - T[None, None]), np.inf)
        pick = np.argmin(dif, axis=0)                                      # the first of equals
        val = np.take_along_axis(cand, pick[None], 0)[0]
        contrib = np.isfinite(val) & va_[:, :, None] & tf[None]
        use = contrib & (np.cumsum(contrib, axis=0) <= MAX_NGHS)
        wk = np.where(va_, ws_, 0.0)[:, :, None]
        term = np.where(use, (ic_[:, :, None] + sl_[:, :, None] * val) * wk, 0.0)
        nuse = use.sum(0)
        has = tf & (nuse >= MIN_NGHS)
        est = np.where(has, term.sum(0) / np.where(use, wk, 0.0).sum(0), np.nan)     # [nm, 63]
    ntw = tf.sum(1)
    in_mth = in_win & (day >= ms[:, None]) & (day < me[:, None])
    for m in range(nm):
        if ntw[m] < MIN_DAYS:
            out["status"][m] = FEW_DAYS
            continue
        out["nvalid"][m] = nvalid[m]
        k = nvalid[m]
        out["w"][:k, m], out["slope"][:k, m], out["icpt"][:k, m] = ws_[:k, m], sl_[:k, m], ic_[:k, m]
        out["col"][:k, m] = ngh[order[:k, m]]
        if k < MIN_NGHS:
            out["status"][m] = FEW_VALID
            continue
        h = has[m]
        own = h & in_mth[m]
        out["est"][day[m][own]] = est[m][own]
        if h.sum() < 2:
            out["status"][m] = DEGENERATE
            continue
        o, e = T[m][h], est[m][h]
        c = o[0]
        po, pe, q = o - c, e - c, float(h.sum())
        with np.errstate(all="ignore"):
            r = (q * (po * pe).sum() - po.sum() * pe.sum()) / np.sqrt(
                (q * (po * po).sum() - po.sum() ** 2) * (q * (pe * pe).sum() - pe.sum() ** 2))
        out["r"][m] = r
        if not np.isfinite(r):
            out["status"][m] = DEGENERATE
            continue
        if r >= NGH_CORR:
            res = np.abs(o - e)
            sd = np.std(res)
            if not (sd > 0.0 and np.isfinite(sd)):
                out["status"][m] = DEGENERATE
                continue
            rm = np.abs(T[m][own] - est[m][own])
            rs = np.abs(rm - res.mean()) / sd
            out["resid"][day[m][own]], out["resid_std"][day[m][own]] = rm, rs
            out["flag"][day[m][own]] = (rm >= RESID_CUTOFF) & (rs >= RESID_STD_CUTOFF)
    return out


def run(lon, lat, tmin, tmax, ymd, targets=None, cap=None):
    """All targets, both variables.  tmin / tmax [ndays, n].  Returns a dict of flags [2, ndays, ntarget] bool, est
    [ntarget, 2, ndays], r / nvalid / status [ntarget, 2, nmonths], and the smallest distances of r, of a tested residual
    and of a tested standardised residual from their thresholds and of a station distance from the radius (``margins``: r, resid, resid_std, km)."""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    targets = np.arange(lon.size) if targets is None else np.asarray(targets)
    nd, nt = len(ymd), targets.size
    nm = month_table(ymd)[0].size
    res = dict(flags=np.zeros((2, nd, nt), bool), est=np.full((nt, 2, nd), np.nan), r=np.full((nt, 2, nm), np.nan),
               nvalid=np.zeros((nt, 2, nm), np.int32), status=np.zeros((nt, 2, nm), np.int32))
    margins = np.full(4, np.inf)
    for k, i in enumerate(targets):
        d = distances_km(lon, lat, i)
        margins[3] = min(margins[3], np.abs(np.delete(d, i) - RADIUS_KM).min()) if d.size > 1 else margins[3]
        ngh = neighbours(lon, lat, i)
        for v, obs in enumerate((tmin, tmax)):
            o = check_station(obs, ymd, int(i), ngh, cap)
            res["flags"][v, :, k], res["est"][k, v] = o["flag"], o["est"]
            res["r"][k, v], res["nvalid"][k, v], res["status"][k, v] = o["r"], o["nvalid"], o["status"]
            with np.errstate(all="ignore"):
                for q, (a, thr) in enumerate(((o["r"], NGH_CORR), (o["resid"], RESID_CUTOFF), (o["resid_std"], RESID_STD_CUTOFF))):
                    a = a[np.isfinite(a)]
                    if a.size:
                        margins[q] = min(margins[q], np.abs(a - thr).min())
    res["margins"] = margins
    return res
