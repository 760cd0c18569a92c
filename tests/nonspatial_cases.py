"""Random inputs for the non-spatial checks (tests/test_nonspatial_host.py, tests/test_gpu_nonspatial.py,
tests/tools/gpu_nonspatial_timing.py): ``spatial_cases.synthetic_pool`` plus, per station and at random, the
ingredients the golden case plants by hand (tests/golden/make_golden_nonspatial.py) -- so that every check of the chain
fires somewhere and the later checks see series the earlier ones have thinned.  The restatement of a case is computed
once per process and shared."""
import datetime as dt
import functools

import numpy as np

import spatial_cases
from topowx_amd.dates import YMD

# name -> (stations, first day, last day, seed): the three random cases of the GPU test
CASES = {"64x12": (64, dt.date(1990, 1, 1), dt.date(2001, 12, 31), 101),
         "5x8_mid_year": (5, dt.date(1993, 3, 15), dt.date(2001, 10, 2), 102),
         "130x7_near_100": (130, dt.date(1994, 1, 1), dt.date(2001, 1, 5), 103)}
MAX_KNIFE = 0.01            # share of the series the restatement may mark as knife-edge


def plant(tmin, tmax, days, rs):
    """Plants in place.  Every ingredient goes to a random subset of the stations."""
    nd, n = tmin.shape
    years = np.unique(days.YEAR)

    def seg(y, m=None):
        return np.nonzero((days.YEAR == y) & ((days.MONTH == m) if m else True))[0]

    for s in range(n):
        v = (tmin, tmax)[rs.randint(2)]
        if s % 8 == 7:                                                   # a sparse station: two short blocks, wide swings
            keep = np.zeros(nd, bool)
            for _ in range(2):
                a = rs.randint(0, max(1, nd - 45))
                keep[a:a + 45] = True
            tmin[~keep, s], tmax[~keep, s] = np.nan, np.nan
            k = np.nonzero(keep)[0]
            tmin[k, s] = np.round(np.cumsum(rs.uniform(-9, 9, k.size)) * 0.5, 1)
            tmax[k, s] = np.round(tmin[k, s] + rs.uniform(-2, 50, k.size), 1)
            continue
        if rs.rand() < 0.3:
            d = rs.randint(nd)
            tmin[d, s] = tmax[d, s] = (-17.8, 0.0)[rs.randint(2)]
        if rs.rand() < 0.15 and years.size > 1:
            y1, y2 = rs.choice(years, 2, replace=False)
            a, b = seg(y1), seg(y2)
            k = min(a.size, b.size)
            v[b[:k], s] = v[a[:k], s]
            if rs.rand() < 0.5:
                v[a[:k], s] = np.where(np.isnan(v[a[:k], s]), 1.5, v[a[:k], s])
                v[b[:k], s] = v[a[:k], s]
        if rs.rand() < 0.3:
            y = rs.choice(years)
            m1, m2 = rs.choice(np.arange(1, 13), 2, replace=False)
            a, b = seg(y, m1), seg(y, m2)
            k = min(a.size, b.size)
            if k:
                v[a[:k], s] = np.where(np.isnan(v[a[:k], s]), 2.5, v[a[:k], s])
                v[b[:k], s] = v[a[:k], s]
        if rs.rand() < 0.3 and years.size > 1:
            y1, y2 = rs.choice(years, 2, replace=False)
            m = rs.randint(1, 13)
            a, b = seg(y1, m), seg(y2, m)
            k = min(a.size, b.size)
            if k:
                v[a[:k], s] = np.where(np.isnan(v[a[:k], s]), 3.5, v[a[:k], s])
                v[b[:k], s] = v[a[:k], s]
        if rs.rand() < 0.3:
            a = seg(rs.choice(years), rs.randint(1, 13))
            if a.size > 12:
                k = rs.choice(a, rs.randint(9, 12), replace=False)
                tmin[k, s] = np.where(np.isnan(tmin[k, s]), 0.5, tmin[k, s])
                tmax[k, s] = tmin[k, s]
        if rs.rand() < 0.2:
            tmax[rs.randint(nd), s], tmin[rs.randint(nd), s] = 60.0, -95.0
        if rs.rand() < 0.4:
            L = (19, 20, 21, 40)[rs.randint(4)]
            a = rs.randint(0, nd - L - 3) if rs.rand() < 0.8 else nd - L - 3       # some reach the end of the series
            run = np.arange(a, a + L + 3)
            val = np.round(rs.uniform(-5, 15), 1)
            v[run, s] = val
            v[run[rs.choice(run.size - 2, 3, replace=False) + 1], s] = np.nan
            if a + L + 3 < nd and rs.rand() < 0.7:
                v[a + L + 3, s] = val + 1.0
        if rs.rand() < 0.4:
            for d in rs.choice(nd, 3, replace=False):
                v[d, s] = np.round(np.nan_to_num(v[d, s], nan=0.0) + rs.choice([-1, 1]) * rs.uniform(20, 35), 1)
        if rs.rand() < 0.3:
            d = rs.randint(nd)
            tmin[d, s] = np.round(np.nan_to_num(tmax[d, s], nan=5.0) + rs.uniform(0.1, 3), 1)
        if rs.rand() < 0.3:
            d = rs.randint(1, nd - 1)
            v[d - 1:d + 2, s] = np.round(np.nan_to_num(v[d, s], nan=0.0) + np.array([0.0, 25.0, 0.0]) * rs.choice([-1, 1]), 1)


@functools.lru_cache(maxsize=None)
def random_case(name):
    """(tmin [ndays, n], tmax [ndays, n] float32, days) of ``CASES[name]``."""
    n, first, last, seed = CASES[name]
    _, _, _, tmin, tmax, days, _ = spatial_cases.synthetic_pool(n, first, last, (44.0, 46.0, -111.0, -108.0), seed,
                                                                spikes_per_stn=2, miss=0.05, gap_every=5)
    plant(tmin, tmax, days, np.random.RandomState(seed + 5000))
    tmin.setflags(write=False)
    tmax.setflags(write=False)
    return tmin, tmax, days


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's result of ``random_case(name)`` (tests/restate_nonspatial.py), computed once and left alone."""
    import restate_nonspatial as RN
    tmin, tmax, days = random_case(name)
    return RN.run(tmin, tmax, days[YMD])


def timing_case(n, years, seed=7, year0=1948):
    """``n`` stations over ``years`` whole years with the planted ingredients, for the timing tool."""
    _, _, _, tmin, tmax, days, _ = spatial_cases.synthetic_pool(n, dt.date(year0, 1, 1), dt.date(year0 + years - 1, 12, 31),
                                                                (40.0, 50.0, -115.0, -100.0), seed, spikes_per_stn=2)
    plant(tmin, tmax, days, np.random.RandomState(seed + 5000))
    return tmin, tmax, days
