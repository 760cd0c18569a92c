"""The quality checks of ``scripts/step08_mpi_qa_stn_obs.py``: its first run with ``--nonspatial``, its second with
``--spatial``, the ``qflag_*`` update of either with ``--write``, and a report of the regression check alone by default.

Every station of an all-stations database (or the ``--targets`` subset) is checked against the stations within 75 km
in one batched GPU call instead of the reference's MPI farm over stations.

Default: the spatial regression check alone (``topowx_amd.qa.qa_spatial_regress``), as a report; nothing is written into
the database.

    python -m topowx_amd.step08 --db all.nc --out report.npz [--targets ids.txt] [--device N]

prints one JSON line (stations, items, flags per variable, seconds, kernel milliseconds) and writes ``report.npz``:
``ids`` [ntarget], ``ymd`` [ndays], ``flags_tmin`` / ``flags_tmax`` [ndays, ntarget] (1 ok, 2 missing, 16 flagged) and
the per-item ``status`` [ntarget, 2, nmonths].

``--spatial``: the reference's ``run_qa_spatial_only`` (qa_temp.py:218-258; ``topowx_amd.qa.run_qa_spatial_only``): the
regression check, the corroboration check on what it left, the mega-inconsistency check on what both left.  If the
database has ``qflag_tmin`` / ``qflag_tmax`` the observations that already carry a flag are set to NaN first, as the
reference's ``load_all_stn_obs`` does.  The report holds ``flags_tmin`` / ``flags_tmax`` in the reference's numbering
(1 ok, 2 missing, 16 regression, 17 corroboration, 18 mega-inconsistency) and the per-target ``status`` [ntarget]; the
JSON line counts each flag per variable.  The database is left alone.

``--spatial --write`` then updates ``qflag_tmin`` / ``qflag_tmax`` as the reference's ``create_update_iter`` /
``set_prev_flags`` / ``update_flags`` do (step08_mpi_qa_stn_obs.py:58-95, 160-213): the rows are the days on which either
variable carries a flag other than 1 or 2; both variables are written on every such row, as the characters of
``TWX_TO_GHCN_FLAGS_MAP``; a previous non-empty flag is kept wherever the new flag is 1 or 2.  A database without the
``qflag_*`` variables gives exit 1 and a message.

``--nonspatial``: the reference's ``run_qa_non_spatial`` (qa_temp.py:172-216; ``topowx_amd.qa.run_qa_non_spatial``),
the run that comes first: missing, naught, the duplicate checks, impossible values, streaks, gaps, climatological
outliers, Tmin > Tmax, spikes, lagged range and mega-inconsistency of every station on its own.  Observations that
already carry a flag are set to NaN first, as above.  The report holds ``flags_tmin`` / ``flags_tmax`` (1 .. 13, 15, 18);
the JSON line counts every flag number per variable.  ``--nonspatial --write`` updates the ``qflag_*`` variables by the
same rules as ``--spatial --write``; a later ``--spatial`` run then reads those observations as NaN.

    python -m topowx_amd.step08 --db all.nc --out report.npz --nonspatial [--write] [--targets ids.txt]
    python -m topowx_amd.step08 --db all.nc --out report.npz --spatial [--write] [--targets ids.txt]

Out of scope: the refresh of the observation counts after the write (the reference's ``add_obs_cnt``), the reference's
filter of stations by data provider (use ``--targets``), and ``run_qa_all``, which step08 never calls.

Exits with 1 if the database cannot be opened, a target is unknown, or ``--write`` has nothing to write into.
"""
import argparse
import json
import sys
import time

import numpy as np

from . import ncio
from .dates import YMD
from .qa import (NON_SPATIAL_FLAGS, QA_MEGA_INCONSIST, QA_MISSING, QA_OK, QA_SPATIAL_CORROB, QA_SPATIAL_REGRESS,
                 TWX_TO_GHCN_FLAGS_MAP, StationObsPool, qa_spatial_regress, run_qa_non_spatial, run_qa_spatial_only)
from .qa.qa_temp import read_qflags

__all__ = ["main", "merge_qflags", "write_qflags"]

QFLAG_VARS = ("qflag_tmin", "qflag_tmax")


def merge_qflags(flags_tmin, flags_tmax, prev_tmin, prev_tmax):
    """``create_update_iter`` + ``set_prev_flags`` (step08_mpi_qa_stn_obs.py:160-213) on whole arrays.  flags_* : the new
    flag numbers, prev_* : the characters the database holds (``"S1"``, ``b""`` = none), all of one shape.  Returns
    ``(rows, chars_tmin, chars_tmax)``: the boolean mask of the entries to write (either variable has a flag other than
    1 / 2) and the characters to write there for each variable -- the new flag's character, or the previous one where
    the new flag is 1 / 2 and a previous one exists.  (A previous character outside ``GHCN_TO_TWX_FLAGS_MAP`` is kept
    as it is; the reference raises a KeyError there.)"""
    flags = [np.asarray(flags_tmin), np.asarray(flags_tmax)]
    prev = [np.asarray(prev_tmin, "S1"), np.asarray(prev_tmax, "S1")]
    if not (flags[0].shape == flags[1].shape == prev[0].shape == prev[1].shape):
        raise ValueError("flags and previous flags must have one shape")
    plain = [(f == QA_OK) | (f == QA_MISSING) for f in flags]
    rows = ~plain[0] | ~plain[1]
    lut = np.zeros(256, "S1")
    for num, ch in TWX_TO_GHCN_FLAGS_MAP.items():
        lut[num] = ch.encode()
    chars = []
    for f, p, pl in zip(flags, prev, plain):
        known = np.isin(f, list(TWX_TO_GHCN_FLAGS_MAP))
        if not known.all():
            raise ValueError("flag number %d has no character" % int(f[~known].ravel()[0]))
        c = lut[f.astype(np.int64)]
        keep = pl & (p != b"")
        c[keep] = p[keep]
        chars.append(c)
    return rows, chars[0], chars[1]


def write_qflags(path, cols, flags_tmin, flags_tmax):
    """Apply ``merge_qflags`` to the database at ``path``: ``cols`` [ntarget] are the station columns of the flag arrays
    [ndays, ntarget].  Only the rows ``merge_qflags`` names are changed.  Returns the number of (day, station) rows
    written; raises ``KeyError`` if the database has no ``qflag_*`` variables."""
    ds = ncio.open_dataset(path, "a")
    try:
        for name in QFLAG_VARS:
            if name not in ds.variables:
                raise KeyError("%s has no variable %s to write into" % (path, name))
        v0, v1 = (ds.variables[name] for name in QFLAG_VARS)
        prev0, prev1 = read_qflags(v0), read_qflags(v1)
        n = 0
        for k, j in enumerate(cols):
            rows, c0, c1 = merge_qflags(flags_tmin[:, k], flags_tmax[:, k], prev0[:, j], prev1[:, j])
            if not rows.any():
                continue
            for v, prev, c in ((v0, prev0, c0), (v1, prev1, c1)):
                col = prev[:, j].copy()
                col[rows] = c[rows]
                v[:, int(j)] = col
            n += int(rows.sum())
    finally:
        ds.close()
    return n


def _spatial(a, pool, targets, ids):
    tm = {}
    t0 = time.perf_counter()
    f_tmin, f_tmax, det = run_qa_spatial_only(pool, targets, device=a.device, details=True, timing=tm)
    sec = time.perf_counter() - t0
    np.savez_compressed(a.out, ids=ids, ymd=np.asarray(pool.days[YMD], np.int32), flags_tmin=f_tmin, flags_tmax=f_tmax,
                        status=det["status"])
    line = {"stations": int(ids.size), "pool": int(pool.ids.size), "days": int(pool.days.size)}
    for name, f in (("flags_tmin", f_tmin), ("flags_tmax", f_tmax)):
        line[name] = {str(k): int((f == k).sum()) for k in (QA_OK, QA_MISSING, QA_SPATIAL_REGRESS, QA_SPATIAL_CORROB,
                                                             QA_MEGA_INCONSIST)}
    line["seconds"] = round(sec, 3)
    for k in sorted(tm):
        line[k] = round(tm[k], 3)
    if a.write:
        line["rows_written"] = write_qflags(a.db, [pool.idxs[s] for s in ids], f_tmin, f_tmax)
    print(json.dumps(line), flush=True)
    return 0


def _nonspatial(a, pool, targets, ids):
    tm = {}
    cols = [pool.idxs[s] for s in ids]
    t0 = time.perf_counter()
    f_tmin, f_tmax = run_qa_non_spatial(pool.tmin[:, cols], pool.tmax[:, cols], pool.days, device=a.device, timing=tm)
    sec = time.perf_counter() - t0
    np.savez_compressed(a.out, ids=ids, ymd=np.asarray(pool.days[YMD], np.int32), flags_tmin=f_tmin, flags_tmax=f_tmax)
    line = {"stations": int(ids.size), "pool": int(pool.ids.size), "days": int(pool.days.size)}
    for name, f in (("flags_tmin", f_tmin), ("flags_tmax", f_tmax)):
        line[name] = {str(k): int((f == k).sum()) for k in (QA_OK,) + NON_SPATIAL_FLAGS}
    line["seconds"] = round(sec, 3)
    for k in sorted(tm):
        line[k] = round(tm[k], 3)
    if a.write:
        line["rows_written"] = write_qflags(a.db, cols, f_tmin, f_tmax)
    print(json.dumps(line), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step08",
                                 description="step08's quality checks of daily Tmin / Tmax: by default a report of the "
                                             "spatial regression check's flags; --nonspatial and --spatial run the "
                                             "reference's two runs, --write puts their flags into the database")
    ap.add_argument("--db", required=True, help="all-stations database (netCDF): tmin / tmax on (time, station_id)")
    ap.add_argument("--out", required=True, help="report to write (.npz)")
    ap.add_argument("--targets", help="text file of station ids to check, one per line (default: every station)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--spatial", action="store_true",
                    help="run the whole spatial stage (regression, corroboration, mega-inconsistency) and report its flags")
    ap.add_argument("--nonspatial", action="store_true",
                    help="run the non-spatial checks of step08's first run and report their flags")
    ap.add_argument("--write", action="store_true",
                    help="with --spatial or --nonspatial: update qflag_tmin / qflag_tmax in the database")
    a = ap.parse_args(argv)
    if a.spatial and a.nonspatial:
        ap.error("--spatial and --nonspatial exclude each other")
    if a.write and not (a.spatial or a.nonspatial):
        ap.error("--write needs --spatial or --nonspatial")
    try:
        qflags = False
        if a.spatial or a.nonspatial:
            ds = ncio.open_dataset(a.db, "r")
            try:
                qflags = all(name in ds.variables for name in QFLAG_VARS)
            finally:
                ds.close()
            if a.write and not qflags:
                raise ValueError("no qflag_tmin / qflag_tmax variables to write into")
        pool = StationObsPool.from_netcdf(a.db, qflags=True) if qflags else StationObsPool.from_netcdf(a.db)
        targets = None
        if a.targets:
            with open(a.targets) as fh:
                targets = [ln.strip() for ln in fh if ln.strip()]
            missing = [s for s in targets if s not in pool.idxs]
            if missing:
                raise ValueError("%d target ids are not in the database (first: %s)" % (len(missing), missing[0]))
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step08: cannot open %s: %s" % (a.db, e), file=sys.stderr)
        return 1
    ids = pool.ids if targets is None else np.array(targets, dtype=str)
    if a.spatial:
        return _spatial(a, pool, targets, ids)
    if a.nonspatial:
        return _nonspatial(a, pool, targets, ids)
    tm = {}
    t0 = time.perf_counter()
    f_tmin, f_tmax, det = qa_spatial_regress(pool, targets, device=a.device, details=True, timing=tm)
    sec = time.perf_counter() - t0
    np.savez_compressed(a.out, ids=ids, ymd=np.asarray(pool.days[YMD], np.int32), flags_tmin=f_tmin, flags_tmax=f_tmax,
                        status=det["status"])
    print(json.dumps({"stations": int(ids.size), "pool": int(pool.ids.size), "items": int(det["status"].size),
                      "flags_tmin": int((f_tmin == QA_SPATIAL_REGRESS).sum()),
                      "flags_tmax": int((f_tmax == QA_SPATIAL_REGRESS).sum()), "seconds": round(sec, 3),
                      "radius_kernel_ms": round(tm["radius_kernel_ms"], 3),
                      "regress_kernel_ms": round(tm["regress_kernel_ms"], 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
