"""``scripts/step20_add_bad_stn_flag.py``: the leave-one-out outlier screen (:70-97) and, on request, what comes before and
after it (:28-68, :102-112).

The Tmin and Tmax databases are each screened over their good stations with ``XvalOutlier`` (optimize.py:84-207); the
union of the outliers is flagged bad in both files.  Both screens see the flags as they were before this stage: the
reference loads both tables before the first pass (step20:80-81), so what the Tmin pass writes is not seen by the Tmax
pass.  Here both screens run first and the union is written once -- the same files.

    python -m topowx_amd.step20 --tmin serial_tmin.nc --tmax serial_tmax.nc [--nnghs 100] [--zscore 6] [--dry-run]
                                [--infill-tmin infill_tmin.nc --infill-tmax infill_tmax.nc --flagged-bad flagged_bad.csv]

prints one JSON line per variable (stations screened, outlier ids, seconds) and exits with 1 if a database cannot be
opened or its station table is not sorted by id.

The earlier checks of step20 need the infilled databases and step17's ``flagged_bad.csv``.  With ``--infill-tmin``,
``--infill-tmax`` and ``--flagged-bad`` all given, ``front`` runs first: per variable the union of the flagged ids, the
stations without a TDI value, the stations inside the mask without a climate division (the variables step19 writes) and the
duplicate stations (``topowx_amd.infill.find_dup_stns``) is flagged with ``reset=True`` and the counts are printed as the
reference prints them; the outlier screen then sees those flags, and after the write ``final_check`` counts the missing
days of every good station (``twxrv_col_count`` on the file's layout) and exits with 1, naming the file, if there is one.
Without the three arguments none of this runs: the output and the written files are what they were.
"""
import argparse
import json
import sys
import time

import numpy as np

from . import ncio
from .stationdb import BAD, CLIMDIV, MASK, STN_ID, TDI, StationSerialDataDb

__all__ = ["set_bad_stations", "screen", "front", "final_check", "read_flagged_bad", "main"]


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


def read_flagged_bad(path):
    """The unique ids of step17's ``flagged_bad.csv`` (first column, one header row; step20:34-36)."""
    ids = []
    with open(path) as fh:
        for k, line in enumerate(fh):
            if k and line.strip():
                ids.append(line.split(",")[0].strip())
    return np.unique(np.array(ids, dtype=str)) if ids else np.array([], str)


def front(stn_da, stn_da_infill, bad_stnids, device=0, out=None):
    """step20:43-68 for one variable: flag (``reset=True``) the union of ``bad_stnids``, the stations without TDI, the
    stations in the mask without a climate division and the duplicates of the infilled database; print the reference's
    lines.  Returns the four id arrays and the union."""
    out = sys.stdout if out is None else out
    for name in (TDI, CLIMDIV, MASK):
        if name not in stn_da.stns.dtype.names:
            raise KeyError("the database has no %r: run python -m topowx_amd.step19 first" % name)
    stn_da.add_stn_variable(BAD, "bad station flag", "", "i1", fill_value=0)
    no_tdi = stn_da.stn_ids[np.isnan(stn_da.stns[TDI])]
    no_climdiv = stn_da.stn_ids[np.logical_and(np.isnan(stn_da.stns[CLIMDIV]), np.isfinite(stn_da.stns[MASK]))]
    print("Finding duplicate stations for %s..." % (stn_da.var_name,), file=out)
    dup = find_dup_stns(stn_da_infill, device=device)
    all_rm = np.unique(np.concatenate([np.asarray(a, dtype=str) for a in (bad_stnids, no_tdi, no_climdiv, dup)]))
    set_bad_stations(stn_da, all_rm)
    print("%d total stations removed for %s:" % (all_rm.size, stn_da.var_name), file=out)
    print("%d stations removed due to infilling issues" % (len(bad_stnids),), file=out)
    print("%d stations removed due to no TDI values" % (no_tdi.size,), file=out)
    print("%d stations removed due no climate division value, but within domain mask" % (no_climdiv.size,), file=out)
    print("%d stations removed due to being duplicates" % (dup.size,), file=out, flush=True)
    return dict(bad=np.asarray(bad_stnids, dtype=str), no_tdi=no_tdi, no_climdiv=no_climdiv, dup=dup, all=all_rm)


def final_check(stn_da, device=0):
    """step20:102-112: the number of good stations (``bad`` not set) with a day that is non-finite or the fill value."""
    from . import _qalib
    good = np.nonzero(np.isnan(stn_da.stns[BAD]))[0] if BAD in stn_da.stns.dtype.names else np.arange(stn_da.stns.size)
    if good.size == 0 or stn_da.var is None:
        return 0
    return int((_qalib.col_count(stn_da.var, good, fill=float(ncio.FILL_F4), device=device) > 0).sum())


def find_dup_stns(stn_da_infill, device=0):
    from .infill import find_dup_stns as _find
    return _find(stn_da_infill, device=device)


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
    ap.add_argument("--infill-tmin", help="infilled Tmin database: with --infill-tmax and --flagged-bad, run step20's front")
    ap.add_argument("--infill-tmax", help="infilled Tmax database")
    ap.add_argument("--flagged-bad", help="step17's flagged_bad.csv")
    a = ap.parse_args(argv)
    extra = (a.infill_tmin, a.infill_tmax, a.flagged_bad)
    if any(extra) and not all(extra):
        ap.error("--infill-tmin, --infill-tmax and --flagged-bad are given together or not at all")
    mode = "r" if a.dry_run else "r+"
    dbs, infill = [], []
    try:
        for path, var in ((a.tmin, "tmin"), (a.tmax, "tmax")):
            try:
                dbs.append(StationSerialDataDb(path, var, mode=mode))
            except (IOError, OSError, ValueError) as e:
                print("step20: cannot open %s: %s" % (path, e), file=sys.stderr)
                return 1
        if all(extra):
            try:
                for path, var in ((a.infill_tmin, "tmin"), (a.infill_tmax, "tmax")):
                    infill.append(StationSerialDataDb(path, var))
                path = a.flagged_bad
                bad_stnids = read_flagged_bad(path)
                for da, ida in zip(dbs, infill):
                    front(da, ida, bad_stnids, device=a.device)
            except (IOError, OSError, ValueError, KeyError) as e:
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
        if all(extra):
            print("Performing final checks to ensure all 'good' stations have no missing values...", flush=True)
            for da, path in zip(dbs, (a.tmin, a.tmax)):
                if final_check(da, device=a.device):
                    print("step20: Missing values found in %s" % path, file=sys.stderr)
                    return 1
    finally:
        for da in dbs + infill:
            da.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
