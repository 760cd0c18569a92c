"""step09: the time-of-observation adjustment of Tmax (twx/homog/tobs.py) for every station in one ``twxhm_tobs_shift`` call,
and the adjusted database ``InsertTobs`` builds."""
import numpy as np

from .. import _qalib, ncio
from .. import stationdb as sdb
from ..obs_por import build_por_mask, read_rows

__all__ = ["tobs_shift_tmax", "create_tobs_adjusted_db", "MISSING", "write_tair_db"]

MISSING = -9999.0         # create_db_all_stations.py:46


def tobs_shift_tmax(tmax, tobs, device=0, timing=None, counts=False):
    """``_tobs_shift_tmax`` (tobs.py:243-264), batched: ``tmax`` / ``tobs`` [ndays] or station-major [nstn, ndays], NaN =
    none.  A morning observation (0 < tobs < 1100) whose previous day holds no afternoon value moves back a day.  THE
    REFERENCE'S QUIRK IS KEPT: a station with fewer than two such days is returned unchanged.  With ``counts`` also the
    number of such days per station."""
    a, t = np.asarray(tmax, np.float32), np.asarray(tobs, np.float32)
    one = a.ndim == 1
    out, nshift = _qalib.tobs_shift(np.atleast_2d(a), np.atleast_2d(t), device=device, timing=timing)
    if one:
        out, nshift = out[0], nshift[0]
    return (out, nshift) if counts else out


def write_tair_db(path, stns, days, tmin, tmax, format=None):
    """A database of ``tmin`` / ``tmax`` (station-major, NaN = none, stored as ``MISSING``) with empty quality flags."""
    ncio.create_quick_db(path, stns, days, [("tmin", "f4", MISSING, "minimum air temperature", "C"),
                                           ("tmax", "f4", MISSING, "maximum air temperature", "C"),
                                           ("qflag_tmin", "S1", "", "quality assurance flag tmin", ""),
                                           ("qflag_tmax", "S1", "", "quality assurance flag tmax", "")], format=format)
    with ncio.open_dataset(path, "r+") as ds:
        for name, rows in (("tmin", tmin), ("tmax", tmax)):
            if stns.size:
                ds.variables[name][:] = np.ascontiguousarray(np.where(np.isnan(rows), np.float32(MISSING), rows).T)
    return path


def create_tobs_adjusted_db(path_all, path_out, start_date, end_date, min_por_yrs=1, format=None, device=0, timing=None):
    """``scripts/step09``: the stations with ``min_por_yrs`` years of Tmin or of Tmax (``build_por_mask`` per variable, their
    union, sorted by id), Tmin as it is and Tmax shifted from ``tobs_tmax``, flagged observations removed, the flags of the
    new database empty.  Returns a dict of ``ids``, ``mask_tmin``, ``mask_tmax`` (over the input's stations) and
    ``nshift`` (per output station)."""
    stns, _, days, _ = ncio.read_station_db_arrays(path_all, "")
    with ncio.open_dataset(path_all, "r") as ds:
        mask_tmin = build_por_mask(ds, ["tmin"], start_date, end_date, min_por_yrs)
        mask_tmax = build_por_mask(ds, ["tmax"], start_date, end_date, min_por_yrs)
        if "tobs_tmax" not in ds.variables:
            raise KeyError("%s has no variable tobs_tmax" % path_all)
        keep = np.nonzero(mask_tmin | mask_tmax)[0]
        keep = keep[np.argsort(stns[sdb.STN_ID][keep], kind="stable")]
        tmin, tmax, tobs = (read_rows(ds, n, qflags=True)[keep] for n in ("tmin", "tmax", "tobs_tmax"))
    tmin[~mask_tmin[keep]] = np.nan
    nshift = np.zeros(keep.size, np.int32)
    if keep.size:
        tmax, nshift = tobs_shift_tmax(tmax, tobs, device=device, timing=timing, counts=True)
    tmax[~mask_tmax[keep]] = np.nan
    nshift[~mask_tmax[keep]] = 0
    write_tair_db(path_out, stns[keep], days, tmin, tmax, format=format)
    return dict(ids=stns[sdb.STN_ID][keep], mask_tmin=mask_tmin, mask_tmax=mask_tmax, nshift=nshift)
