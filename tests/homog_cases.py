"""Scripted inputs of the homogenisation tests: the database of tests/golden/make_golden_homog.py (``db_case``), the PHA
output files the maker writes for it (``pha_output``, in the column layout the reference's parsers read), and seeded cases of
any shape for the comparison of the kernels with tests/restate_homog.py (``random_case``)."""
import datetime as dt
import os

import numpy as np

import restate_homog as RH

START, END = dt.date(1979, 1, 1), dt.date(1984, 12, 31)
NSTN = 51


TENTHS_NAN = -32768
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_homog_v1.npz")


def to_tenths(a):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), TENTHS_NAN, np.rint(np.float64(a) * 10.0)).astype(np.int16)


def from_tenths(t):
    return np.where(t == TENTHS_NAN, np.nan, t / 10.0).astype(np.float32)


def load_fixture():
    """The fixture as a dict, with raw_tmin / raw_tmax widened from their int16 tenths and the step09 inputs derived:
    ``obs_<var>`` = the raw values with flagged days as NaN."""
    z = np.load(FIXTURE)
    fx = dict((k, z[k]) for k in z.files)
    for v in ("tmin", "tmax"):
        fx["raw_" + v] = from_tenths(fx.pop("raw_tenths_" + v))
        fx["obs_" + v] = np.where(fx["flag_" + v], np.float32(np.nan), fx["raw_" + v]).astype(np.float32)
    return fx


def day_axis(start, end):
    d = np.arange(np.datetime64(start), np.datetime64(end) + 1)
    y = d.astype("datetime64[Y]").astype(np.int64) + 1970
    m = d.astype("datetime64[M]").astype(np.int64) % 12 + 1
    day = (d - d.astype("datetime64[M]")).astype(np.int64) + 1
    return y.astype(np.int32), m.astype(np.int32), day.astype(np.int32)


def _days_of(year, month, y, m):
    return np.nonzero((year == y) & (month == m))[0]


def db_case():
    rs = np.random.RandomState(91011)
    year, month, day = day_axis(START, END)
    ns, nd = NSTN, year.size
    kinds = ["GHCND_USC00%06d", "GHCND_USW000%05d", "NRCS_%d", "RAWS_%s", "USH00%06d"]
    ids = []
    for s in range(ns):
        k = s % 5
        ids.append(kinds[k] % (("T%03d" % s) if k == 3 else (240000 + 37 * s if k in (0, 4) else (300 + s if k == 2 else 24000 + s))))
    ids[7] = "NRCS_13C01S"                     # a letter id, padded to eight
    ids[12] = "NRCS_806:MT:SNTL"                                         # a triplet id
    ids = np.array(ids)
    lat = np.round(30 + 19 * rs.rand(ns), 4)
    lon = -np.round(95 + 29 * rs.rand(ns), 4)                            # on both sides of -100
    lat[3], lon[3], lon[4] = 45.5, -99.99995, -100.0
    elev = np.round(200 + 2500 * rs.rand(ns), 1)
    name = np.array(["STATION %02d" % s for s in range(ns)])
    doy = np.arange(nd) % 365.25
    clim = (4.0 - 11.0 * np.cos(2 * np.pi * doy / 365.25))[None, :] + rs.randn(ns, 1) * 3
    tmin = np.round(clim + rs.randn(ns, nd) * 4, 1).astype(np.float32)
    tmax = np.round(clim + 11 + rs.randn(ns, nd) * 4, 1).astype(np.float32)
    for a in (tmin, tmax):
        a[rs.rand(ns, nd) < 0.05] = np.nan
    flag_tmin, flag_tmax = rs.rand(ns, nd) < 0.01, rs.rand(ns, nd) < 0.01
    flag_tmin[:10], flag_tmax[:10] = False, False
    tobs = np.full((ns, nd), np.nan, np.float32)                          # stations 0 .. 9: no observation time, S empty

    def miss(s, y, m, n, where=None):
        d = _days_of(year, month, y, m)
        for a in (tmin, tmax):
            a[s, d] = np.round(clim[s, d] + 5, 1)
            a[s, d[rs.permutation(d.size)[:n]] if where is None else d[where]] = np.nan

    miss(0, 1980, 3, 9); miss(0, 1980, 4, 10); miss(0, 1980, 2, 10); miss(0, 1981, 2, 9); miss(0, 1982, 2, 10)
    miss(1, 1982, 6, 30)                                                 # no finite day: mth_miss == mth_ndays
    for s in (2, 3):                                                     # before, on a start, on an end, inside, after
        for y, m in ((1979, 3), (1980, 1), (1981, 6), (1982, 3), (1984, 5)):
            miss(s, y, m, 15)
    for y in range(1979, 1985):                                          # 20 finite days: means in steps of 0.005
        miss(4, y, 2, 9 if y % 4 == 0 else 8)
    miss(5, 1983, 4, 6, where=slice(0, 6))                               # mean 1.125: a tie of round(x, 2) that float32 holds
    d = _days_of(year, month, 1983, 4)[6:]
    for a in (tmin, tmax):
        a[5, d] = 1.0
        a[5, d[0]] = 4.0
    # ---- observation times ----
    tobs[10, 100] = 700; tmax[10, 99] = np.nan; tmax[10, 100] = 21.5      # |S| = 1: nothing moves
    tobs[11, 100:102] = 700; tmax[11, 99] = np.nan; tmax[11, 100:102] = (20.5, 22.5)      # |S| = 2
    tobs[12, 0:3] = 800; tobs[12, 500:502] = 730; tmax[12, 0:3] = (1.5, 2.5, 3.5)         # day 0, three in a row
    tobs[13, :] = 700
    tobs[13, 10:15] = (0, 1099, 1100, -1, np.nan)
    tobs[14, :] = 700; tmax[14, 50] = np.nan; tmax[14, 51] = np.nan; flag_tmax[14, 60] = True
    tobs[15:31] = 700
    tobs[31:41, : nd // 2], tobs[31:41, nd // 2:] = 1800, 700
    tobs[41:, :] = 1700
    tobs[20:45][rs.rand(25, nd) < 0.03] = np.nan
    tobs[25, ::7] = 2400
    # ---- short records ----
    tmin[50, 200:], tmax[50, 200:] = np.nan, np.nan
    tmin[49, :] = np.nan
    tmax[48, :] = np.nan
    tmin, tmax = tmin + np.float32(0.0), tmax + np.float32(0.0)             # no negative zero: the fixture stores int16 tenths
    hist = [(ids[7], "198109"), (ids[12], "198210"), (ids[2], "198001")]
    return dict(ids=ids, lat=lat, lon=lon, elev=elev, name=name, year=year, month=month, day=day, raw_tmin=tmin,
                raw_tmax=tmax, flag_tmin=flag_tmin, flag_tmax=flag_tmax, tobs=tobs,
                hist_ids=np.array([h[0] for h in hist]), hist_yyyymm=np.array([h[1] for h in hist]))


def fls_text(fid, years, vals):
    """``<id>.FLs.r00.<var>``: the year in columns 12-16, twelve values of width 5 every 9 columns from column 17."""
    out = []
    for y, row in zip(years, np.asarray(vals).reshape(len(years), 12)):
        out.append("%-11s %5d" % (fid, y) + "".join("%5d    " % v for v in row) + "\n")
    return "".join(out)


def adj_line(fid, ym_start, ym_end, adj):
    """A line of ``pha_adj_<var>.log``: id in 10-20, yyyymm in 25-30 and 45-50, the adjustment in 75-80."""
    c = [" "] * 90
    for at, text in ((0, "Adj write:"), (10, fid), (25, "%06d" % ym_start), (45, "%06d" % ym_end), (75, "%6.2f" % adj)):
        c[at:at + len(text)] = text
    return "".join(c).rstrip() + "\n"


def pha_output(case, fids, mean_tmin, mean_tmax, miss_tmin, miss_tmax):
    ns = len(fids)
    years = np.unique(case["year"])
    nm = years.size * 12
    ym = np.repeat(years, 12) * 100 + np.tile(np.arange(1, 13), years.size)
    out = {}
    for v, mean, seed, skip in (("tmin", mean_tmin, 1, (7,)), ("tmax", mean_tmax, 2, (8, 20))):
        rs = np.random.RandomState(4200 + seed)
        with np.errstate(invalid="ignore"):
            base = np.where(np.isnan(mean), 1000.0 + np.arange(nm)[None, :], np.rint(RH.round2(mean.astype(np.float64)) * 100.0))
        pha = base.astype(np.int32)
        lines = []
        for s in range(ns):
            a1, a2 = np.round(rs.randn(2) * 0.6, 2)
            if s == 3:
                a2 = 0.0
            if s % 3 == 0:                                               # the others: PHA changed nothing
                pha[s, (ym >= 198001) & (ym <= 198106)] += int(round(a1 * 100))
                pha[s, (ym >= 198107) & (ym <= 198312)] += int(round(a2 * 100))
            pha[s, rs.rand(nm) < 0.03] = RH.PHA_MISSING
            ent = [adj_line(fids[s], 198107, 198312, a2), adj_line(fids[s], 198001, 198106, a1)]
            lines.extend(ent if s % 2 else ent[::-1])
        for s in (2, 3):
            for m in (197903, 198001, 198106, 198203, 198405):
                pha[s, ym == m] = 1234
        pha[1, ym == 198206] = 1500                                      # h present on the month without a finite day
        out[v] = dict(pha=pha, fls_text=[fls_text(fids[s], years, pha[s]) for s in range(ns)], adj_log="".join(lines),
                      not_stnlist="".join("%s  45.0000 -110.0000\n" % fids[s] for s in skip))
    return out


def adj_csr(fids, adj_ids, start, end, adj):
    """The parsed adjustment table as the CSR ``twxhm_homog_daily`` takes, each station's entries sorted by start."""
    off, order = [0], []
    for f in fids:
        idx = np.nonzero(adj_ids == f)[0]
        order.extend(idx[np.argsort(start[idx], kind="stable")])
        off.append(len(order))
    order = np.array(order, np.int64)
    return (np.array(off, np.int64), np.asarray(start, np.int32)[order], np.asarray(end, np.int32)[order],
            np.asarray(adj, np.float64)[order])


def random_case(seed, ns, start, end, bad=()):
    """A seeded case of ``ns`` stations over ``start`` .. ``end``: everything the four entries take.  ``bad`` is a list of
    (station, "noadj" | "overlap")."""
    rs = np.random.RandomState(seed)
    year, month, day = day_axis(start, end)
    nd = year.size
    mf, mn, mymd = RH.month_groups(year, month)
    nm = mf.size
    obs = np.round(rs.randn(ns, nd) * 9, 1).astype(np.float32)
    obs[rs.rand(ns, nd) < 0.15] = np.nan
    obs[rs.rand(ns, nd) < 0.01] = -0.0
    for g in range(nm):                                                  # some months mostly or wholly missing
        r = rs.rand(ns)
        obs[r < 0.10, mf[g]:mf[g] + mn[g] - 1] = np.nan
        obs[r < 0.04, mf[g]:mf[g] + mn[g]] = np.nan
    tobs = rs.choice(np.array([np.nan, 0, 700, 1099, 1100, 1700, -1], np.float32), size=(ns, nd),
                     p=[0.2, 0.05, 0.3, 0.05, 0.05, 0.3, 0.05]).astype(np.float32)
    tobs[::4] = np.nan
    if ns > 1:
        tobs[1, :] = np.nan
        tobs[1, nd // 2] = 700
        obs[1, nd // 2 - 1] = np.nan                                      # exactly one member of S
    mean, miss = RH.monthly_means(obs, mf, mn, 9)
    with np.errstate(invalid="ignore"):
        pha = np.where(np.isnan(mean), 500.0, np.rint(RH.round2(mean.astype(np.float64)) * 100.0)).astype(np.int32)
    pha[rs.rand(ns, nm) < 0.5] += rs.randint(-90, 90)
    pha[rs.rand(ns, nm) < 0.1] = RH.PHA_MISSING
    off, st, en, ad = [0], [], [], []
    lo, hi = int(mymd[0]), int(mymd[-1])
    cut = int(mymd[nm // 2])
    kinds = dict(bad)
    for s in range(ns):
        if s % 5 == 4 or kinds.get(s) == "noadj":
            needs = ((np.isnan(mean[s])) & (pha[s] != RH.PHA_MISSING) & (miss[s] < mn)).any()
            if kinds.get(s) == "noadj":
                assert needs, "the case must make station %d need its list" % s
                off.append(len(st))
                continue
            if not needs:                                                # an empty list that is never needed: fine
                off.append(len(st))
                continue
        ent = [(lo if s % 2 else cut, cut - 1 if s % 2 else hi, np.round(rs.randn(), 2))]
        if s % 3 == 0 and nm > 2:
            ent = [(int(mymd[1]), cut, np.round(rs.randn(), 2)), (cut + 1, hi - 1, 0.0 if s % 2 else np.round(rs.randn(), 2))]
        if kinds.get(s) == "overlap":
            ent = [(lo, hi, 0.25), (lo + 1, hi, -0.5)]
        for a, b, c in ent:
            st.append(a); en.append(b); ad.append(c)
        off.append(len(st))
    return dict(year=year, month=month, obs=obs, tobs=tobs, mth_first=mf, mth_ndays=mn, mth_ymd=mymd, mth_mean=mean,
                mth_miss=miss, pha=pha, adj_off=np.array(off, np.int64), adj_start=np.array(st, np.int32),
                adj_end=np.array(en, np.int32), adj=np.array(ad, np.float64))
