"""Synthetic raw-observation pools for the spatial regression check: the inputs of tests/test_gpu_spatial.py and
tests/tools/gpu_spatial_timing.py (the golden case has its own generator in tests/golden/make_golden_spatial.py).

A pool is a seasonal cycle + a regional AR(1) signal that varies smoothly over the box (four corner series blended
bilinearly) + a station offset + noise, rounded to 0.1 degC, as float32 with NaN for missing; Tmax = Tmin + a noisy
diurnal range.  The station noise is UNIFORM (standard deviation 1.2 and 1.5 degC), not normal: the tests compare
flags exactly and therefore first assert that no tested quantity lies within 1e-5 of its threshold; with bounded noise
the standardised residuals of ordinary days stay below the 4.0 cutoff, so that among the 1.4e7 tested days of the
2 000-station case only planted spikes come anywhere near it (normal tails put about one day within 1e-5 of 4.0 at
that size, whatever the seed).  Built station block by station block so that a 12 000-station, 69-year pool needs
no float64 copy of the whole matrix.
"""
import datetime as dt

import numpy as np
import pytest

from topowx_amd import h5nc
from topowx_amd.dates import get_days_metadata

TOL = 1e-7          # degC and r: TOL of test_gpu_outlier.py, the bar for two fp64 formulations that differ in their
#                     rounding order only (expected ~1e-12: sums of <= 62 terms of magnitude <= 1e2)
FORMATS = [pytest.param("NETCDF4", marks=pytest.mark.skipif(not h5nc.available(), reason="libhdf5 not loadable")),
           "NETCDF3_64BIT"]

NOISE_TMIN, NOISE_TMAX = 1.2 * 12 ** 0.5, 1.5 * 12 ** 0.5          # widths of the uniform station noise


def synthetic_pool(n, first, last, bbox, seed, spikes_per_stn=3, miss=0.05, gap_every=5, block=500):
    """(ids, lon, lat, tmin [ndays, n], tmax [ndays, n] float32, days, spikes [k, 2] = (station, day)).
    bbox = (lat_s, lat_n, lon_w, lon_e).  ``spikes_per_stn`` +-9..25 degC spikes are planted in Tmin; ``miss`` of the
    days are missing at random; every ``gap_every``-th station has a gap of 70-200 days in both variables."""
    rs = np.random.RandomState(seed)
    days = get_days_metadata(first, last)
    nd = days.size
    lat_s, lat_n, lon_w, lon_e = bbox
    u, v = rs.rand(n), rs.rand(n)
    lon, lat = lon_w + (lon_e - lon_w) * u, lat_s + (lat_n - lat_s) * v
    ids = np.array(["SYN%06d" % i for i in range(n)])
    t = np.arange(nd)
    season = -12.0 * np.cos(2 * np.pi * (t - 15) / 365.25)
    corner = np.zeros((4, nd))
    e = rs.randn(4, nd) * 3.0
    for i in range(1, nd):
        corner[:, i] = 0.7 * corner[:, i - 1] + e[:, i]
    off = rs.randn(n) * 2.0
    tmin, tmax = np.empty((nd, n), np.float32), np.empty((nd, n), np.float32)
    spikes = []
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        k = b1 - b0
        ub, vb = u[b0:b1], v[b0:b1]
        wgt = np.stack([(1 - ub) * (1 - vb), ub * (1 - vb), (1 - ub) * vb, ub * vb])          # [4, k]
        lo = 2.0 + season[:, None] + corner.T @ wgt + off[None, b0:b1] + (rs.rand(nd, k) - 0.5) * NOISE_TMIN
        hi = lo + 11.0 + (rs.rand(nd, k) - 0.5) * NOISE_TMAX
        lo, hi = np.round(lo, 1), np.round(hi, 1)
        for s in range(k):
            for d in rs.choice(nd, spikes_per_stn, replace=False):
                lo[d, s] = np.round(lo[d, s] + rs.choice([-1, 1]) * rs.randint(90, 251) / 10.0, 1)
                spikes.append((b0 + s, int(d)))
        keep = np.zeros((nd, k), bool)
        for s, d in spikes[len(spikes) - k * spikes_per_stn:]:
            keep[d, s - b0] = True
        lo[(rs.rand(nd, k) < miss) & ~keep] = np.nan
        hi[rs.rand(nd, k) < miss] = np.nan
        for s in range(b0, b1):
            if gap_every and s % gap_every == gap_every - 1 and nd > 400:
                g0 = int(rs.randint(60, nd - 300))
                g1 = g0 + int(rs.randint(70, 200))
                lo[g0:g1, s - b0] = np.nan
                hi[g0:g1, s - b0] = np.nan
        tmin[:, b0:b1], tmax[:, b0:b1] = lo, hi
    return ids, lon, lat, tmin, tmax, days, np.array(spikes, np.int64).reshape(-1, 2)


def big_case(n=2000, years=10, seed=8, year0=1991):
    """About 25 stations within 75 km of a station: ``n`` = 2 000 over a 12 x 13.5 degree box centred on 45 N (the
    box grows with ``n``); one planted spike per station."""
    f = (n / 2000.0) ** 0.5
    return synthetic_pool(n, dt.date(year0, 1, 1), dt.date(year0 + years - 1, 12, 31),
                          (45.0 - 6.0 * f, 45.0 + 6.0 * f, -112.0, -112.0 + 13.5 * f), seed, spikes_per_stn=1)
