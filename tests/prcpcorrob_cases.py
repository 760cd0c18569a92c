"""Synthetic inputs of the tests of the precipitation QA's spatial corroboration check (flag 17): the case of the
executed-reference golden (tests/golden/make_golden_prcpcorrob.py) and the random pool the GPU test compares with the numpy
restatement (tests/restate_prcpcorrob.py).  Everything is regenerated from a seed and pinned by ``input_hash``.

Main case: 28 stations, 2000-2005 (the leap years 2000 and 2004), hundredths of a centimetre, about 30 % wet days, 3 %
missing, five clusters more than 75 km apart, and the planted ingredients listed at ``PLANTS``."""
import hashlib
from datetime import date

import numpy as np

from topowx_amd.dates import YMD, get_days_metadata

SEED = 4117
NSTN = 28
FIRST, LAST = date(2000, 1, 1), date(2005, 12, 31)
A = tuple(range(0, 9))            # a line of 9: 8 neighbours each; station k's 8th neighbour is the other end of the line
B = tuple(range(9, 17))           # 8 stations: 7 neighbours each
C1 = (17, 18, 19, 20)             # 3 neighbours each; 17 is a sparse TARGET (S_SPARSE)
C2 = (21, 22, 23, 24)             # 3 neighbours each; 22 is a sparse NEIGHBOUR (S_SPARSE_NGH) of the target 21
D = (25, 26, 27)                  # 2 neighbours each: never tested
CLUSTERS = (A, B, C1, C2, D)
S_SPARSE, S_TWO_FINITE, S_BASIS_TARGET, S_SPARSE_NGH, S_FEW = 17, 18, 21, 22, 25
PLANTS = """cluster A (a line; all values of the cluster set on the three days of each plant): station 0 with 30.0 where its
first 7 neighbours are small and the 8th holds 31.0 (eighth); 0.0 where the first 7 hold 28.0 on all three days and the
8th 0.5 (dry_wet: pctile_dif 0.5, a threshold above 26.924, not flagged); 0.0 where the first 7 hold 0.3 and the 8th 0.0
(dif_zero: pctile_dif == 0); station 2 with 16.0 where every neighbour holds 8.0 (quirk: flagged against the observations
in cm, not flagged had the neighbours' percentiles been used); station 1 with 29.0 and, on the same day, its 8th neighbour
station 8 with 28.5, whose 7th neighbour is station 1 (raw_ngh: 1 is flagged, 8 is corroborated by 1's flagged value; under
run_qa_all station 1's day is removed earlier: chain15).  Cluster B: 12.0 on days 63, 64, 65 of the axis (lane_edge), on
29 February 2004, on 31 December 2002, on 1 January 2004; 40.0 on the second and second-to-last day (flagged; on the first
and last day, never tested, in cluster A).  Cluster C1: the sparse station 17 with 10.0 on 1 June 2001 where its row holds
exactly 20 values (no basis: not flagged), 10.0 on 20 June 2002 where it holds 21 (flagged through the lowered threshold), 40.0 on
10 November 2003 (no basis, flagged), 10.0 on 1 March 2001 where row 59 (yday - 1) holds 21 values and the calendar row 60
holds 20 (flagged through the row quirk); station 18 with 40.0 where only 2 neighbours are finite on the next day (not
flagged).  Cluster C2: station 21 with 10.0 on 1 June 2001, where the rows of the sparse neighbour 22 hold exactly 20
values (2 neighbours with a basis: not flagged), and on 20 June 2002, where they hold 21 (flagged).  Cluster D: 40.0 on a
station with 2 neighbours."""


def didx(days, y, m, d):
    return int(np.nonzero(days[YMD] == y * 10000 + m * 100 + d)[0][0])


def _rain(rs, shape):
    wet = rs.rand(*shape) < 0.30
    amt = np.round(rs.gamma(0.8, 0.9, shape) + 0.01, 2)
    return np.where(wet, amt, 0.0)


def _coords(rs):
    lon, lat = np.zeros(NSTN), np.zeros(NSTN)
    for k, s in enumerate(A):                                           # a line, 0.05 degrees apart, jittered
        lon[s], lat[s] = -110.0 + 0.05 * k + rs.uniform(-0.008, 0.008), 45.0 + rs.uniform(-0.008, 0.008)
    for c, (x0, y0) in zip((B, C1, C2, D), ((-107.0, 45.0), (-104.0, 45.0), (-101.0, 45.0), (-98.0, 45.0))):
        for s in c:
            lon[s], lat[s] = x0 + rs.uniform(0, 0.2), y0 + rs.uniform(0, 0.2)
    return lon, lat


def case_inputs(seed=SEED):
    """(ids, lon, lat, prcp [ndays, n], tavg [ndays, n] float32, days, plants: dict name -> (station, day) or days)."""
    rs = np.random.RandomState(seed)
    days = get_days_metadata(FIRST, LAST)
    nd, n = days.size, NSTN
    lon, lat = _coords(rs)
    p = _rain(rs, (nd, n))
    p[rs.rand(nd, n) < 0.03] = np.nan
    tv = np.round(12.0 + rs.randn(nd, n) * 2.0, 2)
    cluster_of = {s: c for c in CLUSTERS for s in c}
    P = {}

    def quiet(s, d, others=None):
        """The days d - 1 .. d + 1 of the other stations of s's cluster: small values, all finite."""
        for o in (cluster_of[s] if others is None else others):
            if o == s:
                continue
            for e in range(max(d - 1, 0), min(d + 2, nd)):
                p[e, o] = 0.0 if o in (S_SPARSE, S_SPARSE_NGH) else rs.choice([0.0, 0.1, 0.2, 0.3])

    def plant(name, s, d, v):
        quiet(s, d)
        p[d, s] = v
        P[name] = (s, d)

    # ---- the sparse stations: dry but for what is planted ------------------------------------------------------------
    p[:, S_SPARSE], p[:, S_SPARSE_NGH] = 0.0, 0.0
    k = 0
    for y in range(2000, 2006):
        for dd in (10, 11, 12):
            p[didx(days, y, 6, dd), S_SPARSE] = p[didx(days, y, 6, dd), S_SPARSE_NGH] = 0.5 + 0.01 * k
            k += 1
        for dd in (5, 6, 7):
            p[didx(days, y, 3, dd), S_SPARSE] = 0.4 + 0.01 * k
            k += 1
    for y, m, d in ((2003, 6, 2), (2003, 6, 25), (2004, 6, 26), (2000, 3, 8), (2002, 2, 15)):
        p[didx(days, y, m, d), S_SPARSE] = 0.3
    for y, m, d in ((2003, 5, 20), (2004, 5, 21), (2003, 6, 25), (2004, 6, 26), (2005, 6, 27)):
        p[didx(days, y, m, d), S_SPARSE_NGH] = 0.3
    # ---- cluster A ----------------------------------------------------------------------------------------------------
    d = didx(days, 2001, 7, 10)
    plant("eighth", 0, d, 30.0)
    p[d, 8] = 31.0
    d = didx(days, 2002, 4, 10)
    plant("dry_wet", 0, d, 0.0)
    p[d - 1:d + 2, 1:8] = 28.0
    p[d - 1:d + 2, 8] = 0.5
    d = didx(days, 2003, 5, 15)
    plant("dif_zero", 0, d, 0.0)
    p[d - 1:d + 2, 1:9] = 0.3
    p[d, 8] = 0.0
    d = didx(days, 2003, 8, 20)
    plant("quirk", 2, d, 16.0)
    p[d, [0, 1, 3, 4, 5, 6, 7, 8]] = 8.0
    d = didx(days, 2004, 6, 15)
    plant("raw_ngh_flagged", 1, d, 29.0)
    p[d - 1:d + 2, 1] = (0.1, 29.0, 0.2)
    p[d, 8] = 28.5
    P["raw_ngh_kept"] = (8, d)
    P["chain15"] = (1, d)
    # ---- cluster B ----------------------------------------------------------------------------------------------------
    for e in (62, 63, 64, 65, 66):
        quiet(9, e)
    p[63:66, 9] = 12.0
    P["lane_edge"] = (9, np.array([63, 64, 65]))
    plant("feb29", 10, didx(days, 2004, 2, 29), 12.0)
    plant("dec31", 11, didx(days, 2002, 12, 31), 12.0)
    plant("jan1", 12, didx(days, 2004, 1, 1), 12.0)
    plant("first", 4, 0, 40.0)                                         # (cluster A: away from the second day's neighbours)
    plant("last", 4, nd - 1, 40.0)
    plant("second", 14, 1, 40.0)
    plant("second_last", 15, nd - 2, 40.0)
    # ---- cluster C1: the sparse target ----------------------------------------------------------------------------------
    plant("row20", S_SPARSE, didx(days, 2001, 6, 1), 10.0)
    plant("row21", S_SPARSE, didx(days, 2002, 6, 20), 10.0)
    plant("no_basis", S_SPARSE, didx(days, 2003, 11, 10), 40.0)
    plant("mar1", S_SPARSE, didx(days, 2001, 3, 1), 10.0)
    d = didx(days, 2004, 9, 10)
    plant("two_finite", S_TWO_FINITE, d, 40.0)
    p[d + 1, 19] = np.nan
    # ---- cluster C2: the sparse neighbour ---------------------------------------------------------------------------------
    plant("ngh20", S_BASIS_TARGET, didx(days, 2001, 6, 1), 10.0)
    plant("ngh21", S_BASIS_TARGET, didx(days, 2002, 6, 20), 10.0)
    # ---- cluster D ------------------------------------------------------------------------------------------------------
    plant("few", S_FEW, didx(days, 2003, 3, 3), 40.0)
    ids = np.array(["PC%03d" % i for i in range(n)])
    return ids, lon, lat, p.astype(np.float32), tv.astype(np.float32), days, P


def input_hash(lon, lat, prcp, tavg, days):
    h = hashlib.sha256()
    for a in (np.asarray(lon, np.float64).tobytes(), np.asarray(lat, np.float64).tobytes(),
              np.ascontiguousarray(prcp).tobytes(), np.ascontiguousarray(tavg).tobytes(),
              np.asarray(days[YMD], np.int32).tobytes()):
        h.update(a)
    return h.hexdigest()[:16]


# ---- the random pool of the GPU test: 40 stations x 4 years in a 1.2 x 0.8 degree box, a record that starts and ends
# mid-year, regional wet spells so that neighbours corroborate, 4 % missing, a gap of months, planted large values
RANDOM_SEED = 52
RANDOM_NSTN = 40
RANDOM_MARGIN = 1e-5


def random_inputs(seed=RANDOM_SEED):
    """(ids, lon, lat, prcp [ndays, n], tavg [ndays, n] float32, days)."""
    rs = np.random.RandomState(seed)
    days = get_days_metadata(date(2001, 3, 7), date(2005, 3, 6))
    nd, n = days.size, RANDOM_NSTN
    lon, lat = -110.0 + 1.2 * rs.rand(n), 45.0 + 0.8 * rs.rand(n)
    lon[-1], lat[-1] = -104.0, 47.0                                     # one station alone
    regional = rs.rand(nd, 1) < 0.35
    wet = regional & (rs.rand(nd, n) < 0.8) | (rs.rand(nd, n) < 0.04)
    p = np.where(wet, np.round(rs.gamma(0.8, 0.9, (nd, n)) + 0.01, 2), 0.0)
    p[rs.rand(nd, n) < 0.04] = np.nan
    for s in range(0, n, 7):                                            # a gap of months
        g0 = int(rs.randint(30, nd - 200))
        p[g0:g0 + int(rs.randint(60, 150)), s] = np.nan
    p[:, 5] = np.where(rs.rand(nd) < 0.02, p[:, 5], 0.0)                # a sparse station: rows without a basis
    for s in range(n):                                                  # large values, a few of them impossible
        dd = rs.randint(0, nd, 12)
        p[dd, s] = np.r_[np.round(rs.uniform(4.0, 60.0, 10), 2), -0.3, 190.0]
    p[0, 3], p[nd - 1, 4], p[1, 6], p[nd - 2, 7] = 45.0, 45.0, 45.0, 45.0
    tv = np.round(8.0 - 12.0 * np.cos(2 * np.pi * (np.arange(nd) - 15) / 365.25)[:, None] + rs.randn(nd, n) * 3.0, 2)
    tv[np.abs(tv) < 0.05] = 0.5
    tv[rs.rand(nd, n) < 0.1] = np.nan
    ids = np.array(["RC%02d" % i for i in range(n)])
    return ids, lon, lat, p.astype(np.float32), tv.astype(np.float32), days


_RESTATED = {}


def restated(name, chain):
    """The restatement of a named case (``"main"`` / ``"random"``) after ``chain`` (``"spatial"``: the flags of the missing
    check; ``"all"``: those of the restated non-spatial chain), computed once per process and left unchanged."""
    import restate_prcp as RP
    import restate_prcpcorrob as RC
    key = (name, chain)
    if key not in _RESTATED:
        if name == "main":
            _, lon, lat, p, tv, days, _ = case_inputs()
        else:
            _, lon, lat, p, tv, days = random_inputs()
        if chain == "spatial":
            fl = np.where(np.isnan(p), 2, 1).astype(np.uint8)
        else:
            fl = RP.run(p, tv, days[YMD])["flags"]
        _RESTATED[key] = RC.run(lon, lat, p, days[YMD], np.arange(p.shape[1]), fl)
        _RESTATED[key]["flags_in"] = fl
    return _RESTATED[key]
