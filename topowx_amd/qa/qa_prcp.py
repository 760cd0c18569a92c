"""The quality assurance of daily precipitation (twx/qa/qa_prcp.py; Durre et al. 2010) on the GPU: the flag and threshold
constants of the reference, ``run_qa_non_spatial`` (qa_prcp.py:135-176: missing, the three duplicate checks, impossible
values, gaps, climatological outliers; every station on its own, all stations in one call of libtwxqa's
``twxpq_non_spatial``), the two checks the reference defines but leaves commented out of its chain (``_qa_streak``,
``_qa_frequent``; off by default), ``build_percentiles`` (``_build_percentiles``, :790-812, ``twxpq_percentiles``),
``load_prcp_pool``, and the spatial corroboration check ``qa_spatial_corrob`` (``_qa_spatial_corrob``, :614-664, flag 17;
libtwxqa's ``twxpc_spatial_corrob``, every target in one call) with the two chains that end in it, ``run_qa_spatial_only``
(:178-215) and ``run_qa_all`` (:87-133).  There is no CPU fallback: without the library the calls raise.

Out of scope here: ``_qa_yr_clim_outlier`` (20), which the reference defines and never calls.

    python -m topowx_amd.qa.qa_prcp --db all.nc --out report.npz [--streak] [--frequent] [--write] [--targets ids.txt]
                                    [--spatial | --all]

runs the chain on every station of an all-stations database (``prcp`` in cm, ``tmin`` / ``tmax`` for Tavg; observations
of Tmin / Tmax that carry a quality flag do not enter Tavg), prints one JSON line (stations, days, the count of every
flag number, seconds, kernel milliseconds) and writes ``report.npz``: ``ids``, ``ymd``, ``flags_prcp`` [ndays, nstn].  It
is a report by default; ``--write`` puts the flags into ``qflag_prcp`` as the characters of ``TWX_TO_GHCN_FLAGS_MAP``, keeps
a flag that is already there wherever the new one is 1 or 2, and creates ``qflag_prcp`` if the database lacks it.  Exits
with 1 if the database cannot be opened or a target is unknown.  ``--spatial`` runs ``run_qa_spatial_only`` instead and
``--all`` ``run_qa_all`` (the two exclude each other): the neighbours of a target are all stations of the database, the
JSON line also counts the targets of every ``status``, and ``report.npz`` also holds ``status``.
"""
import argparse
import json
import sys
import time

import numpy as np

from .. import _qalib, ncio
from ..dates import YMD
from .qa_temp import read_qflags

__all__ = ["run_qa_non_spatial", "build_percentiles", "load_prcp_pool", "PrcpObsPool", "PRCP_NON_SPATIAL_FLAGS",
           "qa_spatial_corrob", "run_qa_spatial_only", "run_qa_all", "pors_counts", "PRCP_SPATIAL_FLAGS",
           "QA_FREQUENT", "QA_YR_CLIM_OUTLIER", "PRCP_MIN_VALUE", "PRCP_MAX_VALUE", "STREAK_LEN", "GAP_THRES",
           "MIN_PERCENTILE_VALUES", "PERCENTILES", "MAX_SPATIAL_COLLAB_THRES", "PRCP_TWX_TO_GHCN_FLAGS_MAP",
           "PRCP_GHCN_TO_TWX_FLAGS_MAP"]

# flag numbers (qa_prcp.py:37-57)
QA_OK = 1
QA_MISSING = 2
QA_NAUGHT = 3
DUP = 25
QA_DUP_YEAR = 4
QA_DUP_MONTH = 5
QA_DUP_YEAR_MONTH = 6
QA_DUP_WITHIN_MONTH = 7
QA_IMPOSS_VALUE = 8
QA_STREAK = 9
QA_GAP = 10
QA_INTERNAL_INCONSIST = 11
QA_LAGRANGE_INCONSIST = 12
QA_SPIKE_DIP = 13
QA_CLIM_OUTLIER = 15
QA_SPATIAL_REGRESS = 16
QA_SPATIAL_CORROB = 17
QA_MEGA_INCONSIST = 18    # (the reference assigns 14, then 18: 18 is what its module holds)
QA_FREQUENT = 19
QA_YR_CLIM_OUTLIER = 20

# the numbers the non-spatial chain can produce, in the order its checks run (qa_prcp.py:168-174, 232-234); 9 and 19 only
# with ``streak`` / ``frequent``
PRCP_NON_SPATIAL_FLAGS = (QA_MISSING, QA_DUP_YEAR, QA_DUP_YEAR_MONTH, QA_DUP_MONTH, QA_IMPOSS_VALUE, QA_STREAK, QA_FREQUENT,
                          QA_GAP, QA_CLIM_OUTLIER)

# the numbers the spatial-only chain can produce (qa_prcp.py:210-212); run_qa_all: PRCP_NON_SPATIAL_FLAGS and 17
PRCP_SPATIAL_FLAGS = (QA_MISSING, QA_SPATIAL_CORROB)

PRCP_MIN_VALUE = 0.0
PRCP_MAX_VALUE = 182.88               # world record daily precipitation, cm (qa_prcp.py:61)
MAX_SPATIAL_COLLAB_THRES = 26.924     # qa_prcp.py:64-70: the constants of the spatial check (the library holds its own)
MAX_SPATIAL_COLLAB_THRES_MM = MAX_SPATIAL_COLLAB_THRES * 10.0
NGH_RADIUS = 75.0
ANOMALY_CUTOFF = 10.0
MIN_DAYS_MTH_WINDOW = 40
MIN_NGHS = 3
MAX_NGHS = 7
STREAK_LEN = 20
GAP_THRES = 30.0                      # cm
MIN_PERCENTILE_VALUES = 20
PERCENTILES = (30, 50, 70, 90, 95)    # the columns of the table (qa_prcp.py:796)
MIN_YR_DAYS_PRCP_OBS = 245            # qa_prcp.py:81-84: the constants of _qa_yr_clim_outlier, not used here
MIN_NUM_YRS_PRCP = 7
NGH_RESID_CUTOFF = 1000
NGH_RESID_STD_CUTOFF = 0.0

# the temperature maps (qa_temp.py), with 19 -> "K" and 20 -> "O": the reference maps neither; a frequent value is a kind
# of streak and the yearly outlier a kind of outlier
PRCP_TWX_TO_GHCN_FLAGS_MAP = {QA_OK: "", QA_MISSING: "", DUP: "D", QA_DUP_YEAR: "D", QA_DUP_MONTH: "D", QA_DUP_YEAR_MONTH: "D",
                              QA_DUP_WITHIN_MONTH: "D", QA_GAP: "G", QA_INTERNAL_INCONSIST: "I", QA_STREAK: "K",
                              QA_MEGA_INCONSIST: "M", QA_NAUGHT: "N", QA_CLIM_OUTLIER: "O", QA_LAGRANGE_INCONSIST: "R",
                              QA_SPATIAL_REGRESS: "S", QA_SPATIAL_CORROB: "S", QA_SPIKE_DIP: "T", QA_IMPOSS_VALUE: "X",
                              QA_FREQUENT: "K", QA_YR_CLIM_OUTLIER: "O"}

PRCP_GHCN_TO_TWX_FLAGS_MAP = {"": QA_OK, "D": DUP, "G": QA_GAP, "I": QA_INTERNAL_INCONSIST, "K": QA_STREAK,
                              "M": QA_MEGA_INCONSIST, "N": QA_NAUGHT, "O": QA_CLIM_OUTLIER, "R": QA_LAGRANGE_INCONSIST,
                              "S": QA_SPATIAL_REGRESS, "T": QA_SPIKE_DIP, "X": QA_IMPOSS_VALUE}

QFLAG_VAR = "qflag_prcp"


def run_qa_non_spatial(prcp, tavg, days, device=0, streak=False, frequent=False, details=False, timing=None):
    """``run_qa_non_spatial`` (qa_prcp.py:135-176) on the GPU: ``prcp`` (cm) and ``tavg`` (degC; may be all NaN) [ndays]
    (the reference's signature) or [ndays, n], NaN = missing, ``days`` from ``get_days_metadata``; every column is a
    station checked on its own, all in one call.  The checks in order: missing, duplicate years / months of a year /
    calendar months, impossible values, (``streak``: runs of 20 equal values,) (``frequent``: frequent values,) gaps,
    climatological outliers; each sees the series without what the earlier ones flagged.  Returns the flags as uint8 of
    the input's shape in the reference's numbering (``PRCP_NON_SPATIAL_FLAGS`` and ``QA_OK``).  With ``details=True`` a
    dict: ``flags`` and ``pctiles`` [366, 5, n] ([366, 5] for a 1-d series), the percentile table as the outlier check used
    it.  ``timing`` (a dict) receives the device time of each kernel group.  The inputs are not modified."""
    a, b = np.asarray(prcp, np.float32), np.asarray(tavg, np.float32)
    if a.shape != b.shape or a.ndim not in (1, 2) or a.shape[0] != days.size:
        raise ValueError("prcp / tavg must be [ndays] or [ndays, n], with the days of ``days``")
    one = a.ndim == 1
    a2, b2 = (np.ascontiguousarray(np.atleast_2d(x) if one else x.T) for x in (a, b))
    res = _qalib.prcp_non_spatial(a2, b2, days[YMD], streak=streak, frequent=frequent, device=device, details=details,
                                  timing=timing)
    flag = res[0] if details else res
    flags = flag[0].copy() if one else np.ascontiguousarray(flag.T)
    if not details:
        return flags
    return {"flags": flags, "pctiles": res[1][0] if one else np.ascontiguousarray(np.moveaxis(res[1], 0, 2))}


def build_percentiles(vals, days, device=0):
    """``_build_percentiles(vals, days, DATES_366)`` (qa_prcp.py:790-812) of each column of ``vals`` [ndays] or [ndays, n]
    (NaN = missing) on the GPU: row r holds the 30th / 50th / 70th / 90th / 95th percentile of all finite values > 0 whose
    month-day lies within 14 days of the r-th date of 2004; NaN below ``MIN_PERCENTILE_VALUES``.  Returns [366, 5] or
    [366, 5, n] float64."""
    a = np.asarray(vals, np.float32)
    if a.ndim not in (1, 2) or a.shape[0] != days.size:
        raise ValueError("vals must be [ndays] or [ndays, n], with the days of ``days``")
    one = a.ndim == 1
    out = _qalib.prcp_percentiles(np.ascontiguousarray(np.atleast_2d(a) if one else a.T), days[YMD], device=device)
    return out[0] if one else np.ascontiguousarray(np.moveaxis(out, 0, 2))


class PrcpObsPool(object):
    """Daily precipitation of a set of stations, in memory: ``ids``, ``lon``, ``lat`` [n], ``prcp`` (cm), ``tmin``, ``tmax``
    and ``tavg`` [ndays, n] float32 with NaN for missing, ``days``, and ``qflag_prcp`` (``"S1"`` [ndays, n], or None)."""

    def __init__(self, ids, lon, lat, prcp, tmin, tmax, days, qflag_prcp=None):
        self.ids = np.asarray(ids).astype(str)
        self.lon, self.lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
        self.prcp, self.tmin, self.tmax = (np.asarray(x, np.float32) for x in (prcp, tmin, tmax))
        self.days, self.qflag_prcp = days, qflag_prcp
        n, nd = self.ids.size, days.size
        if self.lon.shape != (n,) or self.lat.shape != (n,) or any(x.shape != (nd, n) for x in (self.prcp, self.tmin, self.tmax)):
            raise ValueError("lon / lat must be [n] and prcp / tmin / tmax [ndays, n]")
        both = np.isfinite(self.tmin) & np.isfinite(self.tmax)
        self.tavg = np.full((nd, n), np.nan, np.float32)
        self.tavg[both] = (self.tmin[both] + self.tmax[both]) / np.float32(2.0)
        self.idxs = {s: i for i, s in enumerate(self.ids)}
        if len(self.idxs) != n:
            raise ValueError("station ids must be unique")


def load_prcp_pool(path, qflags=False):
    """The reference's all-stations database (create_db_all_stations.py:233-316): ``prcp``, ``tmin`` and ``tmax`` on
    ``(time, station_id)``, ``longitude``, ``latitude``, the ids and the daily time axis; ``missing_value`` / ``_FillValue``
    entries read as NaN.  ``tavg`` is ``(tmin + tmax) / 2`` where both are finite and NaN elsewhere.  With ``qflags=True``
    the observations flagged in ``qflag_tmin`` / ``qflag_tmax`` are NaN before the mean (a database without these two
    raises ``KeyError``); ``qflag_prcp`` is kept on the pool when the database has it, and never masks ``prcp``."""
    ds = ncio.open_dataset(path, "r")
    try:
        days = ncio.days_of(ds)
        ids = ncio._read_ids(ds.variables["station_id"])
        col = {}
        for name in ("longitude", "latitude", "prcp", "tmin", "tmax"):
            if name not in ds.variables:
                raise KeyError("%s has no variable %s" % (path, name))
            v = ds.variables[name]
            col[name] = ncio._masked_to_nan(v, v[:])
        if qflags:
            for name in ("qflag_tmin", "qflag_tmax"):
                if name not in ds.variables:
                    raise KeyError("%s has no variable %s" % (path, name))
                col[name[6:]][read_qflags(ds.variables[name]) != b""] = np.nan
        qf = read_qflags(ds.variables[QFLAG_VAR]) if QFLAG_VAR in ds.variables else None
    finally:
        ds.close()
    return PrcpObsPool(ids, col["longitude"], col["latitude"], col["prcp"], col["tmin"], col["tmax"], days, qf)


def pors_counts(vals, days, device=0):
    """The sizes of the rows of ``_build_pors(vals, _get_pctiles_md_masks(days, DATES_366))`` (qa_prcp.py:675-681, 814-832)
    of each column of ``vals`` [ndays] or [ndays, n] (NaN = missing) on the GPU: row r counts the finite values > 0 whose
    month-day lies within 14 days of the r-th date of 2004.  The spatial check takes a row as a percentile basis when it
    holds MORE than ``MIN_PERCENTILE_VALUES`` values.  Returns [366] or [366, n] uint16."""
    a = np.asarray(vals, np.float32)
    if a.ndim not in (1, 2) or a.shape[0] != days.size:
        raise ValueError("vals must be [ndays] or [ndays, n], with the days of ``days``")
    one = a.ndim == 1
    out = _qalib.prcp_pors_counts(np.ascontiguousarray(np.atleast_2d(a) if one else a.T), days[YMD], device=device)
    return out[0].copy() if one else np.ascontiguousarray(out.T)


def _target_cols(pool, targets):
    if targets is None:
        return np.arange(pool.ids.size, dtype=np.int64)
    t = np.atleast_1d(np.asarray(targets))
    if t.ndim != 1 or t.size < 1:
        raise ValueError("targets must be a non-empty list of station ids or of columns of the pool")
    if np.issubdtype(t.dtype, np.integer):
        if t.min() < 0 or t.max() >= pool.ids.size:
            raise ValueError("a target column lies outside the pool")
        return t.astype(np.int64)
    missing = [s for s in t.astype(str) if s not in pool.idxs]
    if missing:
        raise ValueError("%d target ids are not in the pool (first: %s)" % (len(missing), missing[0]))
    return np.array([pool.idxs[s] for s in t.astype(str)], np.int64)


def qa_spatial_corrob(pool, targets=None, flags=None, device=0, details=False, timing=None):
    """``_qa_spatial_corrob`` (qa_prcp.py:614-664, 683-782) of the stations ``targets`` (ids or columns of ``pool``, a
    ``PrcpObsPool``; default: every station) on the GPU, all in one call.  ``flags`` [ndays, ntarget] are the flags of the
    checks that ran before: a target's series is its pool value where its flag is 1 (default: the flags of ``_qa_missing``,
    2 where the value is NaN).  The neighbours of a target are all other stations of the pool within 75 km, with their
    observations as they are.  Returns the flags with ``QA_SPATIAL_CORROB`` (17) where a day is not corroborated and its
    flag was 1; the given array is not modified.  With ``details=True`` a dict: ``flags``, ``status`` [ntarget]
    (``_qalib.SP_OK``, ``SP_FEW_NGHS``: fewer than 3 neighbours, ``SP_NGH_CAP``: more than ``_qalib.MAX_RADIUS_NGH``; no flag
    in either case), ``abs_dif``, ``pctile`` and ``thres`` [ndays, ntarget] float64, NaN where the check did not get that far
    on the day.  ``timing`` (a dict) receives the device time of each kernel group."""
    cols = _target_cols(pool, targets)
    nd = pool.days.size
    if flags is None:
        fl = np.where(np.isnan(pool.prcp[:, cols]), QA_MISSING, QA_OK).astype(np.uint8)
    else:
        fl = np.asarray(flags)
        if fl.shape != (nd, cols.size):
            raise ValueError("flags must be [ndays, ntarget]")
    res = _qalib.prcp_spatial_corrob(pool.lon, pool.lat, np.ascontiguousarray(pool.prcp.T), pool.days[YMD], cols,
                                     np.ascontiguousarray(fl.T), device=device, details=details, timing=timing)
    out = np.ascontiguousarray(res[0].T)
    if not details:
        return out
    return {"flags": out, "status": res[1], "abs_dif": np.ascontiguousarray(res[2].T),
            "pctile": np.ascontiguousarray(res[3].T), "thres": np.ascontiguousarray(res[4].T)}


def run_qa_spatial_only(pool, targets=None, device=0, details=False, timing=None):
    """``run_qa_spatial_only`` (qa_prcp.py:178-215) of the stations ``targets`` of ``pool``: ``_qa_missing``, then the
    spatial corroboration check.  Returns flags [ndays, ntarget] (``QA_OK`` and ``PRCP_SPATIAL_FLAGS``), or the dict of
    ``qa_spatial_corrob`` with ``details=True``."""
    return qa_spatial_corrob(pool, targets, None, device=device, details=details, timing=timing)


def run_qa_all(pool, targets=None, streak=False, frequent=False, device=0, details=False, timing=None):
    """``run_qa_all`` (qa_prcp.py:87-133) of the stations ``targets`` of ``pool``: the non-spatial chain
    (``run_qa_non_spatial``; ``streak`` / ``frequent`` as there), then the spatial corroboration check on what it left.
    Returns flags [ndays, ntarget] (``QA_OK``, ``PRCP_NON_SPATIAL_FLAGS`` and 17), or the dict of ``qa_spatial_corrob`` with
    ``details=True``."""
    cols = _target_cols(pool, targets)
    fl = run_qa_non_spatial(pool.prcp[:, cols], pool.tavg[:, cols], pool.days, device=device, streak=streak,
                            frequent=frequent, timing=timing)
    return qa_spatial_corrob(pool, cols, fl, device=device, details=details, timing=timing)


def merge_qflags(flags, prev):
    """The rule of step08's ``merge_qflags`` for one variable: ``(rows, chars)``, the entries to write (a flag other than
    1 / 2) and the character for each entry -- the new flag's, or the previous one where the new flag is 1 / 2."""
    flags, prev = np.asarray(flags), np.asarray(prev, "S1")
    if flags.shape != prev.shape:
        raise ValueError("flags and previous flags must have one shape")
    known = np.isin(flags, list(PRCP_TWX_TO_GHCN_FLAGS_MAP))
    if not known.all():
        raise ValueError("flag number %d has no character" % int(flags[~known].ravel()[0]))
    lut = np.zeros(256, "S1")
    for num, ch in PRCP_TWX_TO_GHCN_FLAGS_MAP.items():
        lut[num] = ch.encode()
    plain = (flags == QA_OK) | (flags == QA_MISSING)
    chars = lut[flags.astype(np.int64)]
    keep = plain & (prev != b"")
    chars[keep] = prev[keep]
    return ~plain, chars


def write_qflags(path, cols, flags):
    """Put ``flags`` [ndays, ntarget] of the station columns ``cols`` into ``qflag_prcp`` of the database at ``path``; the
    variable is created (``"S1"`` on ``(time, station_id)``, empty) if the database lacks it.  Only the entries
    ``merge_qflags`` names are changed.  Returns the number of entries written."""
    ds = ncio.open_dataset(path, "a")
    try:
        if QFLAG_VAR in ds.variables:
            v = ds.variables[QFLAG_VAR]
            prev = read_qflags(v)
        else:
            nd, n = (int(k) for k in ds.variables["prcp"].shape)
            kw = dict(chunksizes=(int(nd), 1), zlib=True) if ncio._is_nc4(ds) and n else {}
            v = ds.createVariable(QFLAG_VAR, "S1", ("time", "station_id"), fill_value="", **kw)
            v.long_name, v.units = "quality assurance flag prcp", ""
            prev = np.zeros((nd, n), "S1")
            v[:] = prev
        nw = 0
        for k, j in enumerate(cols):
            rows, c = merge_qflags(flags[:, k], prev[:, j])
            if not rows.any():
                continue
            col = prev[:, j].copy()
            col[rows] = c[rows]
            v[:, int(j)] = col
            nw += int(rows.sum())
    finally:
        ds.close()
    return nw


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.qa.qa_prcp",
                                 description="the non-spatial quality assurance of daily precipitation: a report of its "
                                             "flags; --write puts them into qflag_prcp of the database")
    ap.add_argument("--db", required=True, help="all-stations database (netCDF): prcp, tmin, tmax on (time, station_id)")
    ap.add_argument("--out", required=True, help="report to write (.npz)")
    ap.add_argument("--targets", help="text file of station ids to check, one per line (default: every station)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--streak", action="store_true", help="also run the reference's _qa_streak (flag 9)")
    ap.add_argument("--frequent", action="store_true", help="also run the reference's _qa_frequent (flag 19)")
    ap.add_argument("--write", action="store_true", help="update qflag_prcp in the database (created if it is not there)")
    chain = ap.add_mutually_exclusive_group()
    chain.add_argument("--spatial", action="store_true", help="run_qa_spatial_only: missing values, then the spatial "
                       "corroboration check (flag 17) against every station of the database")
    chain.add_argument("--all", action="store_true", help="run_qa_all: the non-spatial chain, then the spatial corroboration check")
    a = ap.parse_args(argv)
    try:
        ds = ncio.open_dataset(a.db, "r")
        try:
            qflags = all(name in ds.variables for name in ("qflag_tmin", "qflag_tmax"))
        finally:
            ds.close()
        pool = load_prcp_pool(a.db, qflags=qflags)
        ids = pool.ids
        if a.targets:
            with open(a.targets) as fh:
                ids = np.array([ln.strip() for ln in fh if ln.strip()], dtype=str)
            missing = [s for s in ids if s not in pool.idxs]
            if missing:
                raise ValueError("%d target ids are not in the database (first: %s)" % (len(missing), missing[0]))
    except (IOError, OSError, ValueError, KeyError) as e:
        print("qa_prcp: cannot open %s: %s" % (a.db, e), file=sys.stderr)
        return 1
    cols = [pool.idxs[s] for s in ids]
    tm = {}
    t0 = time.perf_counter()
    extra, numbers = {}, (QA_OK,) + PRCP_NON_SPATIAL_FLAGS
    if a.spatial or a.all:
        if a.spatial:
            res = run_qa_spatial_only(pool, cols, device=a.device, details=True, timing=tm)
            numbers = (QA_OK,) + PRCP_SPATIAL_FLAGS
        else:
            res = run_qa_all(pool, cols, streak=a.streak, frequent=a.frequent, device=a.device, details=True, timing=tm)
            numbers += (QA_SPATIAL_CORROB,)
        flags, extra = res["flags"], {"status": res["status"]}
    else:
        flags = run_qa_non_spatial(pool.prcp[:, cols], pool.tavg[:, cols], pool.days, device=a.device, streak=a.streak,
                                   frequent=a.frequent, timing=tm)
    sec = time.perf_counter() - t0
    np.savez_compressed(a.out, ids=ids, ymd=np.asarray(pool.days[YMD], np.int32), flags_prcp=flags, **extra)
    line = {"stations": int(ids.size), "pool": int(pool.ids.size), "days": int(pool.days.size),
            "flags_prcp": {str(k): int((flags == k).sum()) for k in numbers},
            "seconds": round(sec, 3)}
    if extra:
        line["chain"] = "spatial_only" if a.spatial else "all"
        line["status"] = {str(int(k)): int((extra["status"] == k).sum()) for k in np.unique(extra["status"])}
    for k in sorted(tm):
        line[k] = round(tm[k], 3)
    if a.write:
        line["rows_written"] = write_qflags(a.db, cols, flags)
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
