"""step08's checks of the daily Tmin / Tmax observations on the GPU: the flag and threshold constants of the
reference, a small in-memory pool of raw observations, ``qa_spatial_regress`` (``_qa_spatial_regress``,
twx/qa/qa_temp.py:688-738, 858-1015: one batched call of libtwxqa's ``twxqa_spatial_regress`` over all target stations),
``run_qa_spatial_only`` (qa_temp.py:218-258: the regression check, the corroboration check and the mega-inconsistency
check, ``twxqa_spatial_only``), ``doy_norms`` (the day-of-year normals the corroboration check compares against) and
``run_qa_non_spatial`` (qa_temp.py:172-216: the fourteen checks of step08's first run, every station on its own,
``twxqa_non_spatial``).  There is no CPU fallback: without the library the calls raise.

Out of scope here: ``run_qa_all`` (step08 never calls it).  Writing flags into a database is ``topowx_amd.step08``.
"""
import numpy as np

from .. import _qalib, ncio
from ..dates import YMD

__all__ = ["StationObsPool", "qa_spatial_regress", "run_qa_spatial_only", "run_qa_non_spatial", "doy_norms", "ITEM_STATUS",
           "QA_NAUGHT", "QA_DUP_YEAR", "QA_DUP_MONTH", "QA_DUP_YEAR_MONTH", "QA_DUP_WITHIN_MONTH", "QA_IMPOSS_VALUE",
           "QA_STREAK", "QA_GAP", "QA_INTERNAL_INCONSIST", "QA_LAGRANGE_INCONSIST", "QA_SPIKE_DIP", "QA_CLIM_OUTLIER",
           "NON_SPATIAL_FLAGS", "QA_SPATIAL_CORROB",
           "QA_MEGA_INCONSIST", "ANOMALY_CUTOFF", "MIN_NORM_VALUES", "GHCN_TO_TWX_FLAGS_MAP", "QA_OK", "QA_MISSING", "QA_SPATIAL_REGRESS", "NGH_RADIUS",
           "NGH_CORR", "NGH_RESID_CUTOFF", "NGH_RESID_STD_CUTOFF", "MIN_DAYS_MTH_WINDOW", "MIN_NGHS", "MAX_NGHS",
           "TWX_TO_GHCN_FLAGS_MAP"]

# flag numbers (qa_temp.py:41-59) -- the ones a spatial-only run can produce or map
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

# the numbers a non-spatial run can produce, in the order its checks run (qa_temp.py:202-214, 288-291)
NON_SPATIAL_FLAGS = (QA_MISSING, QA_NAUGHT, QA_DUP_YEAR, QA_DUP_YEAR_MONTH, QA_DUP_MONTH, QA_DUP_WITHIN_MONTH, QA_IMPOSS_VALUE,
                     QA_STREAK, QA_GAP, QA_CLIM_OUTLIER, QA_INTERNAL_INCONSIST, QA_SPIKE_DIP, QA_LAGRANGE_INCONSIST,
                     QA_MEGA_INCONSIST)

# thresholds of the spatial checks (qa_temp.py:65-73)
NGH_RADIUS = 75.0
NGH_CORR = 0.8
NGH_RESID_CUTOFF = 8.0
NGH_RESID_STD_CUTOFF = 4.0
MIN_DAYS_MTH_WINDOW = 40
MIN_NGHS = 3
MAX_NGHS = 7
ANOMALY_CUTOFF = 10.0     # qa_temp.py:70
MIN_NORM_VALUES = 100     # qa_temp.py:84

TWX_TO_GHCN_FLAGS_MAP = {QA_OK: "", QA_MISSING: "", DUP: "D", QA_DUP_YEAR: "D", QA_DUP_MONTH: "D", QA_DUP_YEAR_MONTH: "D",
                         QA_DUP_WITHIN_MONTH: "D", QA_GAP: "G", QA_INTERNAL_INCONSIST: "I", QA_STREAK: "K",
                         QA_MEGA_INCONSIST: "M", QA_NAUGHT: "N", QA_CLIM_OUTLIER: "O", QA_LAGRANGE_INCONSIST: "R",
                         QA_SPATIAL_REGRESS: "S", QA_SPATIAL_CORROB: "S", QA_SPIKE_DIP: "T", QA_IMPOSS_VALUE: "X"}

GHCN_TO_TWX_FLAGS_MAP = {"": QA_OK, "D": DUP, "G": QA_GAP, "I": QA_INTERNAL_INCONSIST, "K": QA_STREAK, "M": QA_MEGA_INCONSIST,
                         "N": QA_NAUGHT, "O": QA_CLIM_OUTLIER, "R": QA_LAGRANGE_INCONSIST, "S": QA_SPATIAL_REGRESS,
                         "T": QA_SPIKE_DIP, "X": QA_IMPOSS_VALUE}

# per-item status of the check (TWXQA_SP_* of include/twx_qa.h)
ITEM_STATUS = {_qalib.SP_OK: "ok", _qalib.SP_FEW_DAYS: "too few window days", _qalib.SP_FEW_NGHS: "too few neighbours",
               _qalib.SP_FEW_VALID: "too few valid neighbours", _qalib.SP_DEGENERATE: "degenerate",
               _qalib.SP_NGH_CAP: "more neighbours than TWXQA_MAX_RADIUS_NGH"}


class StationObsPool(object):
    """Raw daily observations of a set of stations, in memory: ``ids``, ``lon``, ``lat`` [n], ``tmin`` / ``tmax``
    [ndays, n] float32 with NaN for missing (the reference's ``(time, station_id)`` layout) and ``days``
    (``topowx_amd.dates.get_days_metadata``)."""

    def __init__(self, ids, lon, lat, tmin, tmax, days, qflag_tmin=None, qflag_tmax=None):
        self.qflag_tmin, self.qflag_tmax = qflag_tmin, qflag_tmax          # "S1" [ndays, n], or None: not read
        self.ids = np.asarray(ids).astype(str)
        self.lon, self.lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
        self.tmin, self.tmax = np.asarray(tmin, np.float32), np.asarray(tmax, np.float32)
        self.days = days
        n, nd = self.ids.size, days.size
        if self.lon.shape != (n,) or self.lat.shape != (n,) or self.tmin.shape != (nd, n) or self.tmax.shape != (nd, n):
            raise ValueError("lon / lat must be [n] and tmin / tmax [ndays, n]")
        self.idxs = {s: i for i, s in enumerate(self.ids)}
        if len(self.idxs) != n:
            raise ValueError("station ids must be unique")

    @classmethod
    def from_netcdf(cls, path, qflags=False):
        """The reference's all-stations database (create_db_all_stations.py:233-316): ``tmin`` and ``tmax`` on
        ``(time, station_id)``, ``longitude``, ``latitude``, the ids and the daily time axis; ``missing_value`` /
        ``_FillValue`` entries read as NaN.  With ``qflags=True`` the quality-flag character variables ``qflag_tmin`` /
        ``qflag_tmax`` are read too and kept on the pool (``"S1"`` [ndays, n], ``b""`` = no flag), and every observation
        with a non-empty flag is set to NaN, as ``load_all_stn_obs(set_flagged_nan=True)`` does
        (station_data.py:517-522); a database without them raises ``KeyError``."""
        ds = ncio.open_dataset(path, "r")
        try:
            days = ncio.days_of(ds)
            ids = ncio._read_ids(ds.variables["station_id"])
            col = {}
            for name in ("longitude", "latitude", "tmin", "tmax"):
                v = ds.variables[name]
                col[name] = ncio._masked_to_nan(v, v[:])
            qf = [None, None]
            if qflags:
                for k, name in enumerate(("qflag_tmin", "qflag_tmax")):
                    if name not in ds.variables:
                        raise KeyError("%s has no variable %s" % (path, name))
                    qf[k] = read_qflags(ds.variables[name])
                    col[name[6:]][qf[k] != b""] = np.nan
        finally:
            ds.close()
        return cls(ids, col["longitude"], col["latitude"], col["tmin"], col["tmax"], days, qf[0], qf[1])

    def qa_spatial_regress(self, targets=None, device=0, details=False):
        return qa_spatial_regress(self, targets, device, details)

    def run_qa_spatial_only(self, targets=None, device=0, details=False, timing=None):
        return run_qa_spatial_only(self, targets, device, details, timing)

    def run_qa_non_spatial(self, targets=None, device=0, details=False, timing=None):
        """``run_qa_non_spatial`` of the columns of ``targets`` (station ids; default: every station): ``(flags_tmin,
        flags_tmax)`` [ndays, ntarget], with ``details=True`` also the dict of ``norms`` [ntarget, 2, 731, 2]."""
        cols = _target_rows(self, targets)
        return run_qa_non_spatial(self.tmin[:, cols], self.tmax[:, cols], self.days, device, details, timing)


def read_qflags(var):
    """A quality-flag variable as ``"S1"`` [ndays, n]: ``b""`` where no flag is set (a NUL or blank character, a
    masked or fill entry)."""
    a = var[:]
    if np.ma.isMaskedArray(a):
        a = np.ma.filled(a, b"")
    a = np.asarray(a)
    if a.dtype.kind in "UO":
        a = np.array([str(x).encode("ascii", "replace")[:1] for x in a.ravel()], "S1").reshape(a.shape)
    a = a.astype("S1")
    a[(a == b" ") | (a == b"\0")] = b""
    return a


def _target_rows(pool, targets):
    if targets is None:
        return np.arange(pool.ids.size, dtype=np.int32)
    try:
        return np.array([pool.idxs[str(s)] for s in np.atleast_1d(np.asarray(targets))], np.int32)
    except KeyError as e:
        raise KeyError("target station %s is not in the pool" % e)


def doy_norms(series, days, device=0):
    """The day-of-year normals of ``_build_mean_norms`` (qa_temp.py:1111-1130, 1171-1184, 1215-1228) of each column of
    ``series`` [ndays] or [ndays, k] (NaN = missing) on the GPU: biweight means over the finite days within 7 calendar
    days of a row's date, NaN below ``MIN_NORM_VALUES``.  Returns ``(norms_365, norms_366)``, [365, k] from the dates
    of 2003 and [366, k] from those of 2004 ([365] and [366] for a 1-d series)."""
    a = np.asarray(series, np.float32)
    one = a.ndim == 1
    out = _qalib.doy_norms(np.ascontiguousarray(np.atleast_2d(a.T if not one else a)), days[YMD], device=device)
    n365, n366 = np.ascontiguousarray(out[:, :365].T), np.ascontiguousarray(out[:, 365:].T)
    return (n365[:, 0], n366[:, 0]) if one else (n365, n366)


def run_qa_non_spatial(tmin, tmax, days, device=0, details=False, timing=None):
    """``run_qa_non_spatial`` (qa_temp.py:172-216) on the GPU: ``tmin`` / ``tmax`` [ndays] (the reference's signature) or
    [ndays, n], NaN = missing, ``days`` from ``get_days_metadata``; every column is a station checked on its own, all
    in one call.  The checks in order: missing, naught, duplicate years / months of a year / calendar months / Tmin ==
    Tmax months, impossible values, streaks, gaps, climatological outliers, Tmin > Tmax, spikes, lagged range,
    mega-inconsistency; each sees the series without what the earlier ones flagged.  Returns ``(flags_tmin,
    flags_tmax)`` as uint8 of the inputs' shape in the reference's numbering (``NON_SPATIAL_FLAGS`` and ``QA_OK``).  With
    ``details=True`` a third value: a dict of ``norms`` [n, 2, 731, 2] ([2, 731, 2] for a 1-d series): mean and
    standard deviation of the day-of-year rows (variable 0 = tmin, the 365-row table then the 366-row table) as the
    outlier check used them.  ``timing`` (a dict) receives the device time of each kernel group.  The inputs are not
    modified."""
    a, b = np.asarray(tmin, np.float32), np.asarray(tmax, np.float32)
    if a.shape != b.shape or a.ndim not in (1, 2) or a.shape[0] != days.size:
        raise ValueError("tmin / tmax must be [ndays] or [ndays, n], with the days of ``days``")
    one = a.ndim == 1
    a2, b2 = (np.ascontiguousarray(np.atleast_2d(x) if one else x.T) for x in (a, b))
    res = _qalib.non_spatial(a2, b2, days[YMD], device=device, details=details, timing=timing)
    out = [res[0][0].copy(), res[1][0].copy()] if one else [np.ascontiguousarray(res[0].T), np.ascontiguousarray(res[1].T)]
    if details:
        out.append({"norms": res[2][0] if one else res[2]})
    return tuple(out)


def run_qa_spatial_only(pool, targets=None, device=0, details=False, timing=None):
    """``run_qa_spatial_only`` (qa_temp.py:218-258) of ``targets`` (station ids; default: every station of the pool)
    against the pool, all targets in one call: missing -> the spatial regression check -> the corroboration check (on
    the series without the days the regression check flagged) -> the mega-inconsistency check (without the days of
    both).  Returns ``(flags_tmin, flags_tmax)``, each uint8 ``[ndays, ntarget]`` in the reference's numbering: ``QA_OK``
    (1), ``QA_MISSING`` (2), ``QA_SPATIAL_REGRESS`` (16), ``QA_SPATIAL_CORROB`` (17), ``QA_MEGA_INCONSIST`` (18).  With
    ``details=True`` a third value: a dict of ``norms`` [ntarget, 2, 731] (the target's normals, variable 0 = tmin, the
    365-row table then the 366-row table) and ``status`` [ntarget] (``ITEM_STATUS``: ok, too few neighbours, or more
    than the cap -- the last two get no spatial flags).  ``timing`` (a dict) receives the device time of each kernel."""
    tidx = _target_rows(pool, targets)
    tmin_s, tmax_s = np.ascontiguousarray(pool.tmin.T), np.ascontiguousarray(pool.tmax.T)
    fmin, fmax, norms, status = _qalib.spatial_only(pool.lon, pool.lat, tmin_s, tmax_s, pool.days[YMD], tidx, device=device,
                                                    timing=timing)
    out = [np.ascontiguousarray(fmin.T), np.ascontiguousarray(fmax.T)]
    if details:
        out.append({"norms": norms, "status": status})
    return tuple(out)


def qa_spatial_regress(pool, targets=None, device=0, details=False, timing=None):
    """The spatial regression check of ``targets`` (station ids; default: every station of the pool) against the pool,
    all targets in one call.  Returns ``(flags_tmin, flags_tmax)``, each uint8 ``[ndays, ntarget]`` in the reference's
    numbering: ``QA_OK`` (1), ``QA_MISSING`` (2, the observation is NaN) or ``QA_SPATIAL_REGRESS`` (16).  With
    ``details=True`` a third value: a dict of ``est`` [ntarget, 2, ndays] (variable 0 = tmin, 1 = tmax; the estimate of
    each day within its own month's item, NaN if none), ``r``, ``nvalid`` and ``status`` [ntarget, 2, nmonths]
    (``ITEM_STATUS``) and ``nmonths``.  ``timing`` (a dict) receives the device time of the two kernels."""
    if targets is None:
        tidx = np.arange(pool.ids.size, dtype=np.int32)
    else:
        try:
            tidx = np.array([pool.idxs[str(s)] for s in np.atleast_1d(np.asarray(targets))], np.int32)
        except KeyError as e:
            raise KeyError("target station %s is not in the pool" % e)
    # station-major: a wavefront reads a window as one contiguous run
    tmin_s, tmax_s = np.ascontiguousarray(pool.tmin.T), np.ascontiguousarray(pool.tmax.T)
    res = _qalib.spatial_regress(pool.lon, pool.lat, tmin_s, tmax_s, pool.days[YMD], tidx, device=device, details=details,
                                 timing=timing)
    out = []
    for flagged, obs in ((res[0], tmin_s), (res[1], tmax_s)):
        f = np.where(np.isnan(obs[tidx]), QA_MISSING, QA_OK).astype(np.uint8)
        f[flagged != 0] = QA_SPATIAL_REGRESS           # (only finite days are ever flagged)
        out.append(np.ascontiguousarray(f.T))
    if details:
        det = dict(res[2])
        det["nmonths"] = det["r"].shape[2]
        out.append(det)
    return tuple(out)
