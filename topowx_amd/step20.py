"""The last stage of ``scripts/step20_add_bad_stn_flag.py`` (:70-97): the leave-one-out outlier screen.

The Tmin and Tmax databases are each screened over their good stations with ``XvalOutlier`` (optimize.py:84-207); the
union of the outliers is flagged bad in both files.  Both screens see the flags as they were before this stage: the
reference loads both tables before the first pass (step20:80-81), so what the Tmin pass writes is not seen by the Tmax
pass.  Here both screens run first and the union is written once -- the same files.

The earlier checks of step20 (duplicate stations, stations without TDI or climate division) need the infilled
database and are not part of this module.

    python -m topowx_amd.step20 --tmin serial_tmin.nc --tmax serial_tmax.nc [--nnghs 100] [--zscore 6] [--dry-run]

prints one JSON line per variable (stations screened, outlier ids, seconds) and exits with 1 if a database cannot be
opened or its station table is not sorted by id.
"""
import argparse
import json
import sys
import time

import numpy as np

from . import ncio
from .stationdb import BAD, STN_ID, StationSerialDataDb

__all__ = ["set_bad_stations", "screen", "main"]


def _fill_of(v, default):
    return v.getncattr("_FillValue") if "_FillValue" in v.ncattrs() else default


def set_bad_stations(stn_da_or_ds, bad_ids, reset=True):
    """``set_bad_stations`` (twx/infill/post_infill.py:158-191): flag ``bad_ids`` bad (1).  ``reset``: every station is
    first set back to okay.  Ids that are not in the database are ignored, as the reference's docstring says (its
    code re-flags the previous index instead; post_infill.py:181-189).

    Takes a ``StationSerialDataDb`` -- through ``add_stn_variable(BAD, 'bad station flag', '', 'i1', fill_value=0,
    reset=False)``, so the in-memory table follows and a database opened with ``mode='r+'`` is written through -- or an
    open dataset (``ncio.open_dataset(path, 'a')``).  "Okay" is the flag variable's fill value: 0 for the ``i1``
    variable the reference creates, the ``f8`` fill of a table written by ``ncio.write_station_db``; both read back as
    NaN (``isnan(stns[BAD])``)."""
    bad_ids = [str(s) for s in np.atleast_1d(np.asarray(bad_ids))]
    if hasattr(stn_da_or_ds, "add_stn_variable"):
        da = stn_da_or_ds
        ds = da.ds if da.ds is not None and getattr(da.ds, "mode", "r") != "r" else None
        fill = _fill_of(ds.variables[BAD], 0) if ds is not None and BAD in ds.variables else 0
        v = da.add_stn_variable(BAD, "bad station flag", "", "i1", fill_value=fill, reset=False)
        if reset:
            v[:] = np.nan
        for sid in bad_ids:
            i = da.stn_idxs.get(sid)
            if i is not None:
                v[int(i)] = 1
        if ds is not None:
            ds.sync()
        return
    ds = stn_da_or_ds
    db_ids = ncio._read_ids(ds.variables[STN_ID])
    if BAD not in ds.variables:
        v = ds.createVariable(BAD, "i1", (STN_ID,), fill_value=0)
        v.long_name, v.units = "bad station flag", ""
        if db_ids.size:
            v[:] = np.zeros(db_ids.size, np.int8)
    v = ds.variables[BAD]
    if reset and db_ids.size:
        v[:] = np.full(db_ids.size, _fill_of(v, 0), np.dtype(v.dtype))
    pos = {s: i for i, s in enumerate(db_ids)}
    for sid in bad_ids:
        i = pos.get(sid)
        if i is not None:
            v[int(i)] = 1
    ds.sync()


def screen(stn_da, bw_nngh=100, zscore_threshold=6, device=0):
    """Outlier ids of one database over its good stations (step20:84-93) and the seconds it took."""
    from .interp.optimize import XvalOutlier
    t0 = time.perf_counter()
    xo = XvalOutlier(stn_da, device=device)
    try:
        ids = stn_da.stn_ids[np.isnan(stn_da.stns[BAD])] if BAD in stn_da.stns.dtype.names else stn_da.stn_ids
        out = xo.find_xval_outliers(ids, bw_nngh, zscore_threshold)
    finally:
        xo.close()
    return ids.size, out, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step20",
                                 description="step20's leave-one-out outlier screen: flag the union of the Tmin and "
                                             "Tmax outliers bad in both station databases")
    ap.add_argument("--tmin", required=True, help="serially-complete Tmin station database (netCDF)")
    ap.add_argument("--tmax", required=True, help="serially-complete Tmax station database (netCDF)")
    ap.add_argument("--nnghs", type=int, default=100, help="neighbours of each leave-one-out fit (default 100)")
    ap.add_argument("--zscore", type=float, default=6.0, help="z-score above which a station is an outlier (default 6)")
    ap.add_argument("--dry-run", action="store_true", help="report the outliers, write nothing")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    mode = "r" if a.dry_run else "r+"
    dbs = []
    try:
        for path, var in ((a.tmin, "tmin"), (a.tmax, "tmax")):
            try:
                dbs.append(StationSerialDataDb(path, var, mode=mode))
            except (IOError, OSError, ValueError) as e:
                print("step20: cannot open %s: %s" % (path, e), file=sys.stderr)
                return 1
        union = []
        for da in dbs:
            n, out, sec = screen(da, a.nnghs, a.zscore, a.device)
            print(json.dumps({"var": da.var_name, "stations": int(n), "outliers": [str(s) for s in out],
                              "seconds": round(sec, 3)}), flush=True)
            union.extend(str(s) for s in out)
        if not a.dry_run:
            union = np.unique(np.array(union, dtype=str)) if union else np.array([], str)
            for da in dbs:
                set_bad_stations(da, union, reset=False)
    finally:
        for da in dbs:
            da.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
