"""Period-of-record bookkeeping of a station database and its monthly means, on the GPU (``twxhm_obs_cnt`` /
``twxhm_monthly_means`` of include/twx_qa.h): ``add_obs_cnt`` (create_db_all_stations.py:1383-1450), ``build_por_mask``
(obs_por.py:41-84) and ``add_monthly_means`` (create_db_all_stations.py:1230-1331).  Every station of a variable goes
through one batched call; the files are read and written through ``ncio`` in either container.

Differences from the reference, all of the container: the counts and ``mth`` are int32 (classic netCDF has no 64-bit
integer), and ``add_monthly_means`` needs a day axis of whole calendar years, which is what the reference's databases have
and what PHA's yearly lines assume.
"""
import datetime as _dt

import numpy as np

from . import _qalib, ncio
from .dates import DAY, MONTH, YEAR

__all__ = ["add_obs_cnt", "build_por_mask", "add_monthly_means", "obs_cnt_name", "read_rows", "month_axis"]

DAYS_IN_MTH = np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])        # of 2015, as _build_a_por_mask takes them


def _ymd(d):
    """yyyymmdd of a date, a datetime, an integer or a string of that form."""
    if hasattr(d, "year"):
        return d.year * 10000 + d.month * 100 + d.day
    v = int(str(d).replace("-", ""))
    _dt.date(v // 10000, v // 100 % 100, v % 100)
    return v


def obs_cnt_name(elem, start_date, end_date):
    return "obs_cnt_%s_%d_%d" % (elem, _ymd(start_date), _ymd(end_date))


def read_rows(ds, name, qflags=False):
    """The variable ``name`` on (time, station_id) as station-major float32 rows with NaN for its fill / missing value; with
    ``qflags`` the days that carry a flag in ``qflag_<name>`` (if the database has it) are NaN too."""
    v = ds.variables[name]
    a = v[:]
    if np.ma.isMaskedArray(a):
        a = np.ma.filled(a.astype(np.float32), np.nan)
    a = np.array(a, np.float32)
    marks = [v.getncattr(att) for att in ("missing_value", "_FillValue") if att in v.ncattrs()]
    for m in marks or [ncio.FILL_F4]:
        a[a == np.float32(m)] = np.nan
    if qflags and "qflag_" + name in ds.variables:
        from .qa.qa_temp import read_qflags
        a[read_qflags(ds.variables["qflag_" + name]) != b""] = np.nan
    return np.ascontiguousarray(a.T)


def _day_ymd(days):
    return np.asarray(days[YEAR], np.int64) * 10000 + np.asarray(days[MONTH], np.int64) * 100 + np.asarray(days[DAY], np.int64)


def add_obs_cnt(path, elem, start_date, end_date, device=0, timing=None):
    """``add_obs_cnt``: the variable ``obs_cnt_<elem>_<start>_<end>`` on ``(mth, station_id)``, the number of observations
    of ``elem`` per calendar month inside the period.  It counts the variable as stored: quality flags are NOT applied,
    as the reference counts ``ds[elem]``.  Returns the counts [nstn, 12]."""
    ds = ncio.open_dataset(path, "r+")
    try:
        days = ncio.days_of(ds)
        ymd = _day_ymd(days)
        inside = np.nonzero((ymd >= _ymd(start_date)) & (ymd <= _ymd(end_date)))[0]
        if inside.size == 0:
            raise ValueError("no day of the database lies in %d .. %d" % (_ymd(start_date), _ymd(end_date)))
        rows = read_rows(ds, elem)
        cnt = _qalib.obs_cnt(rows, np.asarray(days[MONTH], np.int8), int(inside[0]), int(inside[-1]), device=device,
                             timing=timing) if rows.shape[0] else np.zeros((0, 12), np.int32)
        if "mth" not in ds.dimensions:
            ds.createDimension("mth", 12)
            ds.createVariable("mth", "i4", ("mth",))[:] = np.arange(1, 13, dtype=np.int32)
        name = obs_cnt_name(elem, start_date, end_date)
        if name in ds.variables:
            v = ds.variables[name]
        else:
            v = ds.createVariable(name, "i4", ("mth", "station_id"))
            v.comments = "Number of observations per calendar month"
        v[:] = np.ascontiguousarray(cnt.T)
    finally:
        ds.close()
    return cnt


def _build_a_por_mask(obs_cnts, min_por_yrs):
    """[12, nstn] counts -> the stations with at least ``min_por_yrs`` years of days in every calendar month."""
    nmin = (DAYS_IN_MTH * min_por_yrs)[:, None]
    return np.sum(np.asarray(obs_cnts) >= nmin, axis=0) == 12


def build_por_mask(ds, elems, start_date, end_date, min_por_yrs):
    """``build_por_mask``: the stations with a long enough record for one or more of ``elems``; ``ds`` is an open dataset
    or a path.  Needs the counts of ``add_obs_cnt`` for that period (``KeyError`` otherwise)."""
    if isinstance(ds, (str, bytes)) or hasattr(ds, "__fspath__"):
        with ncio.open_dataset(ds, "r") as opened:
            return build_por_mask(opened, elems, start_date, end_date, min_por_yrs)
    masks = []
    for elem in elems:
        name = obs_cnt_name(elem, start_date, end_date)
        if name not in ds.variables:
            raise KeyError("no variable %s: run add_obs_cnt (python -m topowx_amd.step05) first" % name)
        masks.append(_build_a_por_mask(np.asarray(ds.variables[name][:]), min_por_yrs))
    return np.sum(np.array(masks), axis=0) >= 1


def month_axis(days):
    """(mth_first, mth_ndays, mth_ymd) of a day axis of whole calendar years; ``ValueError`` otherwise."""
    if (int(days[MONTH][0]), int(days[DAY][0])) != (1, 1) or (int(days[MONTH][-1]), int(days[DAY][-1])) != (12, 31):
        raise ValueError("the day axis must run from a 1 January to a 31 December")
    return _qalib.month_groups(days[YEAR], days[MONTH])


def add_monthly_means(path, var_name, max_miss=_qalib.HM_MAX_MISS, device=0, timing=None):
    """``add_monthly_means``: ``time_mth``, ``<var>_mth`` (f4, masked where a month has more than ``max_miss`` missing
    days) and ``<var>_mthmiss`` (i2, the missing days of each month) on ``(time_mth, station_id)``.  Days with a quality
    flag count as missing.  Returns (mth_mean [nstn, nmth] with NaN where masked, mth_miss)."""
    ds = ncio.open_dataset(path, "r+")
    try:
        days = ncio.days_of(ds)
        mf, mn, _ = month_axis(days)
        nm = mf.size
        rows = read_rows(ds, var_name, qflags=True)
        if rows.shape[0]:
            mean, miss = _qalib.monthly_means(rows, mf, mn, max_miss, device=device, timing=timing)
        else:
            mean, miss = np.zeros((0, nm), np.float32), np.zeros((0, nm), np.int16)
        if "time_mth" not in ds.variables:
            ds.createDimension("time_mth", nm)
            tv = ds.createVariable("time_mth", "f8", ("time_mth",))
            tv.units, tv.standard_name, tv.calendar = ds.variables["time"].units, "time", "standard"
            tv[:] = np.asarray(ds.variables["time"][:], np.float64)[mf]
        names = (var_name + "_mth", var_name + "_mthmiss")
        kw = dict(zlib=True, chunksizes=(nm, 1)) if ncio._is_nc4(ds) and rows.shape[0] else {}
        vm = ds.variables[names[0]] if names[0] in ds.variables else \
            ds.createVariable(names[0], "f4", ("time_mth", "station_id"), fill_value=ncio.FILL_F4, **kw)
        vs = ds.variables[names[1]] if names[1] in ds.variables else \
            ds.createVariable(names[1], "i2", ("time_mth", "station_id"), fill_value=ncio.DEFAULT_FILLS["i2"], **kw)
        vm[:] = np.ascontiguousarray(np.where(np.isnan(mean), ncio.FILL_F4, mean).T)
        vs[:] = np.ascontiguousarray(miss.T)
    finally:
        ds.close()
    return mean, miss
