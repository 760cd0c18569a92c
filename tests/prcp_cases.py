"""Synthetic inputs of the precipitation QA tests: the main case of the executed-reference golden
(tests/golden/make_golden_prcp.py), its short-record case, and the random pool the GPU test compares with the numpy
restatement (tests/restate_prcp.py).  Everything is regenerated from a seed and pinned by ``input_hash``.

Main case: 16 stations, 1990-2005 (the leap years 1992, 1996, 2000, 2004), hundredths of a centimetre, about 30 % wet
days, 3 % missing, a seasonal Tavg with 3 % missing, and the planted ingredients listed at ``PLANTS``."""
import hashlib
from datetime import date

import numpy as np

from topowx_amd.dates import YMD, get_days_metadata

SEED = 9029
NSTN = 16
FIRST, LAST = date(1990, 1, 1), date(2005, 12, 31)
(S_DUPYEAR, S_DUPNAN, S_DUPMONTHS, S_DUPCAL, S_IMPOSS, S_GAP, S_CLIM, S_PLAIN7, S_STREAK, S_FREQ, S_SPARSE, S_SPARSE2,
 S_PLAIN12, S_DRY, S_PLAIN14, S_PLAIN15) = range(16)
PCT_STNS = (S_CLIM, S_SPARSE, S_PLAIN12)          # stations whose tables of check 15 are stored
FREQ_PLANTS = ((300, 9, 0.3), (600, 8, 0.65), (900, 7, 1.2), (1200, 5, 3.6))     # (start in the wet sequence, copies, value)
PLANTS = """station 0 duplicate years (1993 onto 1995, common to common; 1996 onto 1997, leap to common by position),
1 a copied year with one NaN in the copy, and two years that are equal but hold only 2 positive values, 2 duplicate months
of a year (March onto May; November onto December: the quirk, not flagged; October onto December of another year:
flagged; January onto February), 3 the same calendar month of two years (July; February leap / common; an August pair
with exactly 3 positive values: flagged; a September pair with exactly 2: not), 4 impossible values (negative; 200;
float32(182.88) and its successor), 5 gaps (August: a step of exactly 30.0 in float32; October: one float32 step less),
6 climatological outliers (18 cm with Tavg < 0: flagged, with Tavg >= 0 and with Tavg NaN: not; 28 cm with Tavg >= 0
and with Tavg NaN: flagged), 8 streaks (20 equal values with zeros and NaN days inside; 19; 25 that reach the end of the
series), 9 frequent values for each tier (9 of 10 above the 30th percentile, 8 above the 50th, 7 above the 70th, 5
above the 90th), 10 a sparse station whose rows hold 19, 20 and 21 values, with a large value on a day of a common
year after February whose own row is NaN while the row of its shifted day-of-year is not, 11 a station with 12 wet
values, 10 of them equal (every percentile NaN: no frequent value), 13 an all-dry station."""


def didx(days, y, m, d):
    return int(np.nonzero(days[YMD] == y * 10000 + m * 100 + d)[0][0])


def month_days(days, y, m):
    return np.nonzero((days.YEAR == y) & (days.MONTH == m))[0]


def year_days(days, y):
    return np.nonzero(days.YEAR == y)[0]


def _rain(rs, shape):
    wet = rs.rand(*shape) < 0.30
    amt = np.round(rs.gamma(0.8, 0.9, shape) + 0.01, 2)
    return np.where(wet, amt, 0.0)


def _tavg(rs, nd, n):
    t = np.arange(nd)
    out = 8.0 - 12.0 * np.cos(2 * np.pi * (t - 15) / 365.25)[:, None] + rs.randn(nd, n) * 3.0
    out = np.round(out, 2)
    out[np.abs(out) < 0.05] = 0.5                                       # no Tavg on the edge of the m = 5 / m = 9 choice
    return out


def case_inputs(seed=SEED):
    """(prcp [ndays, n], tavg [ndays, n] float32, days, plants: dict of day indices the assertions use)."""
    rs = np.random.RandomState(seed)
    days = get_days_metadata(FIRST, LAST)
    nd, n = days.size, NSTN
    p = _rain(rs, (nd, n))
    full = p.copy()                                                     # before the missing days
    p[rs.rand(nd, n) < 0.03] = np.nan
    tv = _tavg(rs, nd, n)
    tv[rs.rand(nd, n) < 0.03] = np.nan
    P = {}
    # 0: duplicate years
    y93, y95, y96, y97 = (year_days(days, y) for y in (1993, 1995, 1996, 1997))
    p[y93, 0] = full[y93, 0]
    p[y95, 0] = p[y93, 0]
    p[y96, 0] = full[y96, 0]
    p[y97, 0] = p[y96[:365], 0]
    P["dupyear"] = np.r_[y93, y95, y96, y97]
    # 1: a copied year with one NaN in the copy; two equal years with only 2 positive values
    p[y93, 1] = full[y93, 1]
    p[y95, 1] = p[y93, 1]
    p[y95[200], 1] = np.nan
    P["dupnan_years"], P["dupnan_day"] = np.r_[y93, y95], int(y95[200])
    y99, y01 = year_days(days, 1999), year_days(days, 2001)
    p[y99, 1], p[y01, 1] = 0.0, 0.0
    p[y99[[40, 250]], 1] = (1.25, 0.75)
    p[y01[[40, 250]], 1] = (1.25, 0.75)
    P["two_values"] = np.r_[y99, y01]
    # 2: duplicate months of one year
    m3, m5 = month_days(days, 1994, 3), month_days(days, 1994, 5)
    p[m3, 2] = full[m3, 2]
    p[m5, 2] = p[m3, 2]
    m11, m12 = month_days(days, 1998, 11), month_days(days, 1998, 12)
    p[m11, 2] = full[m11, 2]
    p[m12, 2] = full[m12, 2]
    p[m12[:30], 2] = p[m11, 2]
    o10, o12 = month_days(days, 1996, 10), month_days(days, 1996, 12)
    p[o10, 2] = full[o10, 2]
    p[o12, 2] = p[o10, 2]
    m1, m2 = month_days(days, 2001, 1), month_days(days, 2001, 2)
    p[m1, 2] = full[m1, 2]
    p[m2, 2] = p[m1[:28], 2]
    P["dupmonths"], P["dupmonths_quirk"] = np.r_[m3, m5, o10, o12, m1, m2], np.r_[m11, m12]
    # 3: the same calendar month of two years; pairs with exactly 3 and exactly 2 positive values
    j91, j99 = month_days(days, 1991, 7), month_days(days, 1999, 7)
    p[j91, 3] = full[j91, 3]
    p[j99, 3] = p[j91, 3]
    f96, f97 = month_days(days, 1996, 2), month_days(days, 1997, 2)
    p[f96, 3] = full[f96, 3]
    p[f97, 3] = p[f96[:28], 3]
    a92, a00 = month_days(days, 1992, 8), month_days(days, 2000, 8)
    s92, s00 = month_days(days, 1992, 9), month_days(days, 2000, 9)
    for m in (a92, a00, s92, s00):
        p[m, 3] = 0.0
    for m in (a92, a00):
        p[m[[3, 11, 25]], 3] = (0.4, 1.7, 0.9)
    for m in (s92, s00):
        p[m[[5, 19]], 3] = (0.6, 2.2)
    P["dupcal"], P["dupcal_three"], P["dupcal_two"] = np.r_[j91, j99, f96, f97], np.r_[a92, a00], np.r_[s92, s00]
    # 4: impossible values
    d = [didx(days, 1991, 4, 9), didx(days, 1997, 7, 20), didx(days, 2002, 5, 11), didx(days, 2003, 6, 2)]
    edge = np.float32(182.88)
    p[d[0], 4], p[d[1], 4] = -0.5, 200.0
    P["imposs"], P["imposs_edge"], P["imposs_next"] = d[:2], d[2], d[3]
    # 5: gaps.  August and October hold nothing above 5.0 but the planted value
    for mth, key, top in ((8, "gap30", np.float32(35.0)), (10, "gap_below", np.nextafter(np.float32(35.0), np.float32(0.0)))):
        md = np.nonzero(days.MONTH == mth)[0]
        col = p[md, 5]
        col[col > 5.0] = 5.0
        p[md, 5] = col
        p[md[17], 5], p[md[140], 5] = 5.0, 0.0
        P[key] = int(md[140])
        P[key + "_value"] = np.float32(top)
    # 6: climatological outliers
    cd = [didx(days, 1993, 1, 16), didx(days, 1996, 7, 5), didx(days, 1999, 7, 21), didx(days, 2002, 7, 9),
          didx(days, 2004, 8, 3)]
    p[cd, 6] = (18.0, 18.0, 18.0, 28.0, 28.0)
    tv[cd, 6] = (-3.0, 14.0, np.nan, 15.0, np.nan)
    P["clim_m5"], P["clim_not"], P["clim_m9"] = cd[0], cd[1:3], cd[3:]
    # 8: streaks
    a = didx(days, 1995, 5, 1)
    run = np.arange(a, a + 26)
    p[a - 1, 8] = 1.11
    p[run, 8] = 0.77
    p[run[[4, 9, 15]], 8] = np.nan
    p[run[[6, 12, 20]], 8] = 0.0                                        # 20 equal values, three NaN and three dry days inside
    p[a + 26, 8] = 1.11
    b = didx(days, 1998, 9, 1)
    p[b - 1, 8], p[b:b + 19, 8], p[b + 19, 8] = 1.11, 0.66, 1.11
    p[nd - 26, 8], p[nd - 25:, 8] = 1.11, 0.55
    P["streak20"] = run[np.isfinite(p[run, 8]) & (p[run, 8] > 0)]
    P["streak19"], P["streak_end"] = np.arange(b, b + 19), np.arange(nd - 25, nd)
    # 9: frequent values: c copies of v among 10 consecutive wet values, the others distinct small values
    wet = np.nonzero(np.isfinite(p[:, 9]) & (p[:, 9] > 0))[0]
    for t, (start, c, v) in enumerate(FREQ_PLANTS):
        w = wet[start:start + 10]
        p[w, 9] = np.round(0.02 + 0.01 * np.arange(10), 2)
        p[w[:c], 9] = v
        p[wet[start - 1], 9], p[wet[start + 10], 9] = 0.01, 0.01
        P["freq%d" % t] = w[:c]
    # 10: a sparse station: dry but for 19 values on 10-12 June of 1990-1996, one on 28 June 1997 and a large one on
    # 25 June 1995 (a common year)
    p[:, 10] = 0.0
    k = 0
    for y in range(1990, 1997):
        for dd in (10, 11, 12):
            if k < 19:
                p[didx(days, y, 6, dd), 10] = 0.5 + 0.01 * k
                k += 1
    p[didx(days, 1997, 6, 28), 10] = 0.95
    big = didx(days, 1995, 6, 25)
    p[big, 10], tv[big, 10] = 12.0, 15.0
    P["shift_day"] = big
    # 11: 12 wet values in one October, 10 of them equal
    p[:, 11] = 0.0
    o = month_days(days, 1994, 10)
    p[o[2:14], 11] = 3.33
    p[o[[5, 9]], 11] = (0.4, 0.7)
    P["freq_nan"] = o[2:14]
    # 13: all dry
    p[:, 13] = 0.0
    p = p.astype(np.float32)
    p[P["imposs_edge"], 4] = edge
    p[P["imposs_next"], 4] = np.nextafter(edge, np.float32(1e9))
    p[P["gap30"], 5] = P["gap30_value"]
    p[P["gap_below"], 5] = P["gap_below_value"]
    return p, tv.astype(np.float32), days, P


def short_inputs(seed=SEED + 1):
    """The short record: 1 March - 30 September 1991.  (The library takes consecutive days only, so an axis with fewer than
    12 distinct months cannot span several years.)  Seven distinct months, ``max(mth_nums)`` = 6: June is never the first
    month of a pair.  4 stations: June copied onto August (not flagged: the quirk), May copied onto July (flagged),
    March copied onto June (flagged: June is the second month), an ordinary one."""
    rs = np.random.RandomState(seed)
    days = get_days_metadata(date(1991, 3, 1), date(1991, 9, 30))
    nd = days.size
    p = _rain(rs, (nd, 4))
    tv = _tavg(rs, nd, 4)
    m = {k: np.nonzero(days.MONTH == k)[0] for k in range(3, 10)}
    for s, k in ((0, 6), (1, 5), (2, 3)):                               # at least three positive values on each side
        p[m[k][[1, 8, 20]], s] = (0.31, 1.42, 0.53)
    p[m[8][:30], 0] = p[m[6], 0]
    p[m[7], 1] = p[m[5], 1]
    p[m[6], 2] = p[m[3][:30], 2]
    return p.astype(np.float32), tv.astype(np.float32), days


def input_hash(prcp, tavg, days):
    h = hashlib.sha256()
    for a in (np.ascontiguousarray(prcp).tobytes(), np.ascontiguousarray(tavg).tobytes(),
              np.asarray(days[YMD], np.int32).tobytes()):
        h.update(a)
    return h.hexdigest()[:16]


# ---- the random pool of the GPU test: 24 stations x 6 years, dense enough for finite rows, with repeats, gaps and outliers
RANDOM_SEED = 77
RANDOM_NSTN = 24
RANDOM_MAX_KNIFE = 1


def random_inputs(seed=RANDOM_SEED):
    rs = np.random.RandomState(seed)
    days = get_days_metadata(date(1999, 3, 7), date(2005, 3, 6))       # starts and ends mid-year
    nd, n = days.size, RANDOM_NSTN
    p = _rain(rs, (nd, n))
    p[:, ::3] = np.round(p[:, ::3], 1)                                  # coarse values: frequent repeats
    p[rs.rand(nd, n) < 0.04] = np.nan
    tv = _tavg(rs, nd, n)
    tv[rs.rand(nd, n) < 0.1] = np.nan
    for s in range(n):                                                  # large and impossible values, copies, repeats
        d = rs.randint(0, nd, 8)
        p[d, s] = np.r_[np.round(rs.uniform(8.0, 60.0, 6), 2), -0.3, 190.0]
        if s % 4 == 0:                                                  # a calendar month copied onto the next year's
            y, m = 2000 + s % 3, 1 + s % 12
            p[month_days(days, y + 1, m)[:28], s] = p[month_days(days, y, m)[:28], s]
        if s % 4 == 1:                                                  # a month copied onto a later one of its year
            y, m = 2001 + s % 3, 1 + s % 9
            p[month_days(days, y, m + 2)[:28], s] = p[month_days(days, y, m)[:28], s]
        if s % 6 == 2:                                                  # a whole year copied
            p[year_days(days, 2001), s] = np.nan_to_num(p[year_days(days, 2001), s])
            p[year_days(days, 2003)[:365], s] = p[year_days(days, 2001)[:365], s]
        if s % 5 == 0:                                                  # a run of one value with dry days inside
            c = rs.randint(0, nd - 40)
            p[c:c + 30, s] = np.where(rs.rand(30) < 0.8, 0.3, 0.0)
        if s % 5 == 1:                                                  # a frequent large value among others
            c = rs.randint(0, nd - 40)
            p[c:c + 30, s] = np.where(rs.rand(30) < 0.6, 2.5, np.round(rs.uniform(0.1, 3.0, 30), 2))
    ids = np.array(["R%02d" % i for i in range(n)])
    return p.astype(np.float32), tv.astype(np.float32), days, ids


_RESTATED = {}


def restated(name, streak, frequent):
    """The restatement of a named case, computed once per process and left unchanged."""
    import restate_prcp as RP
    key = (name, bool(streak), bool(frequent))
    if key not in _RESTATED:
        p, tv, days = {"main": lambda: case_inputs()[:3], "short": short_inputs, "random": lambda: random_inputs()[:3]}[name]()
        _RESTATED[key] = RP.run(p, tv, days[YMD], streak=streak, frequent=frequent)
    return _RESTATED[key]


def write_db(path, ids, lon, lat, prcp, tmin, tmax, days, fmt, qflags=("qflag_tmin", "qflag_tmax"), prev=()):
    """An all-stations database in the reference's layout with ``prcp`` (cm), ``tmin`` and ``tmax``; ``qflags``: the
    quality-flag variables to create (``"S1"``, empty); ``prev``: ``(variable, day, station, character)`` entries set
    beforehand."""
    from topowx_amd import ncio
    from topowx_amd import stationdb as sdb
    n = ids.size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = ids, lon, lat, 100.0
    variables = [("prcp", "f4", ncio.FILL_F4, "precipitation", "cm"), ("tmin", "f4", ncio.FILL_F4, "minimum air temperature", "C"),
                 ("tmax", "f4", ncio.FILL_F4, "maximum air temperature", "C")]
    variables += [(name, "S1", "", "quality assurance flag " + name[6:], "") for name in qflags]
    ncio.create_quick_db(path, stns, days, variables, format=fmt)
    ds = ncio.open_dataset(path, "a")
    try:
        for name, a in (("prcp", prcp), ("tmin", tmin), ("tmax", tmax)):
            v = ds.variables[name]
            v.missing_value = np.float32(ncio.FILL_F4)
            v[:] = np.where(np.isnan(a), np.float32(ncio.FILL_F4), a)
        for name in sorted(set(p[0] for p in prev)):
            q = np.zeros((days.size, n), "S1")
            for _, d, s, ch in (p for p in prev if p[0] == name):
                q[d, s] = ch
            ds.variables[name][:] = q
    finally:
        ds.close()
    return path
