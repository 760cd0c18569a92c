"""Seeded inputs of the reanalysis tests (tests/test_nnr_host.py, tests/test_gpu_nnr.py, tests/golden/make_golden_nnr.py).

A 6 x 5 grid at 2.5 degrees, three time slots, the reference's seven variables as eight variable / level columns (hgt has
two levels; tair, rhum, uwnd and vwnd one level on a ``level`` dimension; thick and slp none), nine calendar years of days
(1981-1989: a 31-day month has 279 rows, February 254).  Every column is an offset plus a mix of six latent series of
geometrically falling variance plus small noise: collinear, as neighbouring cells are, with separated eigenvalues.  Twelve
stations, none equidistant from two cells; S01 and S02 share cells and slot; S03 has offset -7 (24z for Tmax).
"""
import datetime as dt
import hashlib
import os

import numpy as np

from topowx_amd.dates import MONTH, get_days_metadata

NNR_VARS = ("tair", "hgt", "thick", "rhum", "uwnd", "vwnd", "slp")
NNR_TIMES = ("24z", "18z", "12z")
LEVELS = {"tair": (850.0,), "hgt": (500.0, 700.0), "thick": None, "rhum": (700.0,), "uwnd": (700.0,), "vwnd": (700.0,),
          "slp": None}
OFFSET = {"tair": 275.0, "hgt": 5500.0, "thick": 5400.0, "rhum": 55.0, "uwnd": 4.0, "vwnd": -1.0, "slp": 101000.0}
SCALE = {"tair": 8.0, "hgt": 100.0, "thick": 90.0, "rhum": 18.0, "uwnd": 6.0, "vwnd": 5.0, "slp": 700.0}
LONS = np.array([-115.0, -112.5, -110.0, -107.5, -105.0, -102.5])
LATS = np.array([47.5, 45.0, 42.5, 40.0, 37.5])                     # north to south, as the reanalysis files are
START, END = dt.date(1981, 1, 1), dt.date(1989, 12, 31)
NLATENT = 6
CUTS = (0.99, 0.90)
NNGH = 4
MIN_REL_GAP, MIN_CUT_MARGIN = 1e-2, 1e-6

STN_IDS = np.array(["S%02d" % i for i in range(1, 13)])
STN_LON = np.array([-111.13, -111.05, -108.52, -113.91, -106.07, -103.44, -109.03, -112.02, -104.61, -107.77, -110.49, -105.58])
STN_LAT = np.array([44.02, 44.10, 41.21, 46.33, 39.14, 38.66, 45.91, 40.37, 43.08, 46.72, 38.93, 41.88])
STN_UTC = np.array([-6, -6, -7, -8, -5, -5, -7, -8, -6, -7, -4, -6], np.int16)


class NnrCase(object):
    """``days``; ``data[(var, time)]``: float32 [ndays, nlev, nlat, nlon] or [ndays, nlat, nlon]; the stations."""

    def __init__(self, start=START, end=END, lons=LONS, lats=LATS, seed=20240519):
        rng = np.random.default_rng(seed)
        self.days = get_days_metadata(start, end)
        self.start, self.lons, self.lats = start, np.asarray(lons), np.asarray(lats)
        LONS, LATS = self.lons, self.lats
        nd = self.days.size
        sd = 0.5 ** np.arange(NLATENT)
        self.data = {}
        yy, xx = np.meshgrid(np.arange(LATS.size), np.arange(LONS.size), indexing="ij")
        for slot in NNR_TIMES:
            lat = rng.standard_normal((nd, NLATENT)) * sd
            for var in NNR_VARS:
                nlev = 1 if LEVELS[var] is None else len(LEVELS[var])
                w0 = rng.standard_normal((nlev, NLATENT))
                # the weights change smoothly over the grid: neighbouring cells are nearly collinear
                grad = 0.35 * rng.standard_normal((nlev, 2, NLATENT))
                w = w0[:, None, None, :] + grad[:, 0, None, None, :] * yy[None, :, :, None] / 4.0 + \
                    grad[:, 1, None, None, :] * xx[None, :, :, None] / 5.0
                a = np.einsum("dl,vyxl->dvyx", lat, w) + 0.03 * rng.standard_normal((nd, nlev, LATS.size, LONS.size))
                a = (OFFSET[var] + SCALE[var] * a).astype(np.float32)
                self.data[(var, slot)] = a if LEVELS[var] is not None else a[:, 0]
        self.ids, self.lon, self.lat, self.utc = STN_IDS, STN_LON, STN_LAT, STN_UTC
        self.group = (np.asarray(self.days[MONTH], np.int64) - 1).astype(np.int8)
        self.day_idx = [np.nonzero(self.group == g)[0] for g in range(12)]

    def checksum(self):
        h = hashlib.sha256()
        for var in NNR_VARS:
            for slot in NNR_TIMES:
                h.update(np.ascontiguousarray(self.data[(var, slot)]).tobytes())
        for a in (self.lon, self.lat, self.utc, self.lons, self.lats):
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    def write(self, path, fmt=None):
        """The files ``nnr_<var>_<time>.nc`` as ``create_nnr_subset*`` lay them out, through ``ncio``."""
        from topowx_amd import ncio
        os.makedirs(path, exist_ok=True)
        LONS, LATS, START = self.lons, self.lats, self.start
        for (var, slot), a in self.data.items():
            ds = ncio.open_dataset(os.path.join(path, "nnr_%s_%s.nc" % (var, slot)), "w", fmt)
            try:
                ds.createDimension("time", int(self.days.size))
                dims = ["time"]
                if LEVELS[var] is not None:
                    ds.createDimension("level", len(LEVELS[var]))
                    dims.append("level")
                ds.createDimension("lat", LATS.size)
                ds.createDimension("lon", LONS.size)
                tv = ds.createVariable("time", "f8", ("time",))
                tv.units, tv.calendar, tv.standard_name = ncio._units(START), "standard", "time"
                tv[:] = np.arange(self.days.size, dtype=np.float64)
                if LEVELS[var] is not None:
                    ds.createVariable("level", "f8", ("level",))[:] = np.array(LEVELS[var])
                ds.createVariable("lat", "f8", ("lat",))[:] = LATS
                ds.createVariable("lon", "f8", ("lon",))[:] = LONS
                v = ds.createVariable(var, "f4", tuple(dims + ["lat", "lon"]), fill_value=ncio.FILL_F4)
                v[:] = a
            finally:
                ds.close()
        return path


    def reader(self):
        """An in-memory ``NNRNghData`` over the case."""
        from topowx_amd.reanalysis import NNRNghData
        return NNRNghData.from_arrays(self.days, self.lons, self.lats, self.data)


class OnlyMatrix(object):
    """A reader that exposes nothing but ``get_nngh_matrix``: the per-target host route of the infill calls."""

    def __init__(self, reader):
        self._r = reader

    def get_nngh_matrix(self, lon, lat, tair_var, utc_offset, nngh=4):
        return self._r.get_nngh_matrix(lon, lat, tair_var, utc_offset, nngh)


def case_over(pool, seed=77):
    """A case on the days of ``pool`` whose grid (2.5 degrees) covers its stations, and the stations' UTC offsets by
    longitude (-7 west of -106, else -6)."""
    import datetime as _dt
    from topowx_amd.dates import DAY, YEAR
    d = pool.days
    first = _dt.date(int(d[YEAR][0]), int(d[MONTH][0]), int(d[DAY][0]))
    last = _dt.date(int(d[YEAR][-1]), int(d[MONTH][-1]), int(d[DAY][-1]))
    lon0, lon1 = 2.5 * np.floor(pool.lon.min() / 2.5) - 2.5, 2.5 * np.ceil(pool.lon.max() / 2.5) + 2.5
    lat0, lat1 = 2.5 * np.floor(pool.lat.min() / 2.5) - 2.5, 2.5 * np.ceil(pool.lat.max() / 2.5) + 2.5
    c = NnrCase(first, last, np.arange(lon0, lon1 + 1.0, 2.5), np.arange(lat1, lat0 - 1.0, -2.5), seed)
    return c, np.where(pool.lon < -106.0, -7, -6).astype(np.int16)


_CASE = []


def case():
    if not _CASE:
        _CASE.append(NnrCase())
    return _CASE[0]


def slot_of(tair_var, utc):
    from topowx_amd.reanalysis import NNRNghData
    return NNRNghData.UTC_OFFSET_TIMES[tair_var][int(utc)]


def check_separation(var_explain, ncomp):
    """Refuse a case on which the comparison would be ill-posed: the eigenvalues up to the largest cut must have a relative
    gap of ``MIN_REL_GAP`` and the cumulative variance must stay ``MIN_CUT_MARGIN`` away from every cut."""
    ve = np.asarray(var_explain, np.float64)
    k = int(max(ncomp))
    gap = (ve[:k] - ve[1:k + 1]) / ve[:k]
    if gap.min() < MIN_REL_GAP:
        raise AssertionError("retained eigenvalues closer than %g (relative): %r" % (MIN_REL_GAP, gap))
    cum = np.cumsum(ve)
    for c in CUTS:
        if np.abs(cum - c).min() < MIN_CUT_MARGIN:
            raise AssertionError("the cumulative variance comes within %g of the cut %g" % (MIN_CUT_MARGIN, c))
