"""Seeded inputs of the step12 tests (the reanalysis subsets): raw yearly files of the six variables on a small grid at real
coordinates, so that the reference's bounds (60 .. 10 N, -135 .. -55 E) apply.  Generated, never stored.

Grid: lats 90 .. -90 by 10 (6 rows inside, raw 3 .. 8), lons 0 .. 348 by 12 (7 columns inside, raw 19 .. 25: the subset is
6 x 7, a partial chunk on both axes), levels 1000, 850, 700, 500.  Years 2000 (a leap year) and 2001, four records a day;
the period is 20000101 .. 20011231.  Planted: both kinds of mark, marks on one level only of the thickness pair, a
float32 variable (rhum) with a negative zero, a variable without any mark (slp), ``valid_range`` in unpacked units (air:
ignored).  Packed values stay inside -32000 .. 32000 apart from the planted marks."""
import datetime as dt
import functools
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LATS = np.arange(90, -91, -10).astype(np.float32)
LONS = np.arange(0, 360, 12).astype(np.float32)
LEVELS = np.array([1000, 850, 700, 500], np.float32)
YEARS = (2000, 2001)
START, END = dt.date(2000, 1, 1), dt.date(2001, 12, 31)
UNITS = "hours since 1800-01-01 00:00:0.0"
EPOCH = dt.datetime(1800, 1, 1)
FILL_F4 = np.float32(9.969209968386869e36)
F4_MARK = np.float32(-9.96921e36)
# representative pack pairs of the NCEP files: air, hgt, the winds, slp
PACKS = ((0.01, 477.65), (1.0, 32066.0), (0.01, 202.65), (1.0, 119765.0))
# raw variable -> dtype, (scale_factor, add_offset) or None, missing_value, _FillValue, has a level axis, deflated in NetCDF-4
VARS = {"air": ("i2", PACKS[0], 32766, -32767, True, True),
        "hgt": ("i2", PACKS[1], 32766, None, True, False),
        "rhum": ("f4", None, F4_MARK, None, True, True),
        "vwnd": ("i2", PACKS[2], 32766, 32766, True, False),
        "uwnd": ("i2", PACKS[2], None, -32767, True, False),
        "slp": ("i2", PACKS[3], None, None, False, False)}
UTC = (12, 18, 24)


def _each(stem, **kw):
    return [dict(fname="nnr_%s_%dz.nc" % (stem, u), utc_time=u, **kw) for u in UTC]


# the 21 products of scripts/step12_process_reanalysis_data.py:43-146, by raw variable
PRODUCTS = (("air", _each("tair", varname_out="tair", levels=(850,), conv="k_to_c")),
            ("hgt", _each("thick", varname_out="thick", thick=(500, 1000)) + _each("hgt", varname_out="hgt", levels=(500, 700))),
            ("rhum", _each("rhum", varname_out="rhum", levels=(850,))),
            ("vwnd", _each("vwnd", varname_out="vwnd", levels=(850,))),
            ("uwnd", _each("uwnd", varname_out="uwnd", levels=(850,))),
            ("slp", _each("slp", varname_out="slp")))


def days():
    from topowx_amd.dates import get_days_metadata
    return get_days_metadata(START, END)


def year_times(year, nrec=None):
    """The file's ``time``: hours since the epoch, every six hours of the year."""
    h0 = (dt.datetime(year, 1, 1) - EPOCH).days * 24
    n = (dt.date(year + 1, 1, 1) - dt.date(year, 1, 1)).days * 4 if nrec is None else nrec
    return h0 + 6.0 * np.arange(n, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def year_raw(var, year):
    """The stored values of a yearly file: [nrec, 4, 19, 30] (slp: [nrec, 19, 30]); read-only."""
    dtype, _, mv, fv, has_level, _ = VARS[var]
    rng = np.random.default_rng([20, sorted(VARS).index(var), year])
    nrec = year_times(year).size
    shape = (nrec, LEVELS.size, LATS.size, LONS.size) if has_level else (nrec, LATS.size, LONS.size)
    if dtype == "i2":
        a = rng.integers(-32000, 32001, shape, dtype=np.int16)
    else:
        a = rng.uniform(0.0, 100.0, shape).astype(np.float32)
    # marks: all over the slab, and thickly inside the subset (rows 3 .. 8, columns 19 .. 25)
    for k, m in enumerate((mv, fv)):
        if m is None:
            continue
        for _ in range(2):
            n = 400
            idx = [rng.integers(0, s, n) for s in shape]
            if _ == 1:
                idx[-2], idx[-1] = rng.integers(3, 9, n), rng.integers(19, 26, n)
            a[tuple(idx)] = m
    if dtype == "f4":
        a[7, 1, 4, 20] = np.float32(-0.0)                        # 18z of 2 January, 850 hPa, output cell (1, 1)
    if var == "hgt":                                             # one level of the thickness pair, the other, and both
        a[7, 3, 4, 21], a[11, 0, 5, 22] = mv, mv
        a[15, 0, 6, 23] = a[15, 3, 6, 23] = mv
    a.setflags(write=False)
    return a


def checksum():
    h = hashlib.sha256()
    for var in sorted(VARS):
        for y in YEARS:
            h.update(year_raw(var, y).tobytes())
            h.update(year_times(y).tobytes())
    h.update(repr((VARS, UNITS, LATS.tolist(), LONS.tolist(), LEVELS.tolist())).encode())
    return h.hexdigest()


def write_raw_file(path, var, year, fmt, raw=None, times=None, units=UNITS):
    """One yearly file as NCEP lays it out, in the container ``fmt``."""
    from topowx_amd import ncio
    dtype, pack, mv, fv, has_level, deflate = VARS[var]
    raw = year_raw(var, year) if raw is None else raw
    times = year_times(year) if times is None else times
    ds = ncio.open_dataset(path, "w", fmt)
    try:
        ds.title = "generated %s" % var
        for name, vals in (("lon", LONS), ("lat", LATS)) + ((("level", LEVELS),) if has_level else ()):
            ds.createDimension(name, vals.size)
        ds.createDimension("time", times.size)
        for name, vals in ((("level", LEVELS),) if has_level else ()) + (("lat", LATS), ("lon", LONS)):
            ds.createVariable(name, "f4", (name,))[:] = vals
        tv = ds.createVariable("time", "f8", ("time",))
        tv.units = units
        tv[:] = times
        dims = ("time", "level", "lat", "lon") if has_level else ("time", "lat", "lon")
        kw = dict(zlib=True, complevel=1, chunksizes=(1,) * (len(dims) - 2) + (LATS.size, LONS.size)) if deflate and fmt == "NETCDF4" else {}
        v = ds.createVariable(var, dtype, dims, fill_value=None if fv is None else np.dtype(dtype).type(fv), **kw)
        if pack is not None:
            v.scale_factor, v.add_offset = np.float32(pack[0]), np.float32(pack[1])
        if mv is not None:
            v.missing_value = np.dtype(dtype).type(mv)
        if var == "air":
            v.valid_range = np.array([137.5, 362.5], np.float32)
        v[:] = raw
    finally:
        ds.close()


def write_raw_files(dirpath, fmt):
    for var in VARS:
        for y in YEARS:
            write_raw_file(os.path.join(dirpath, "%s.%d.nc" % (var, y)), var, y, fmt)
    return dirpath
