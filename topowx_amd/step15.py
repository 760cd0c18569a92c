"""``scripts/step15_mpi_xval_infill.py``: the cross-validation of the infill (``topowx_amd.infill.XvalInfill``).  Of every
cross-validation station all observations but the last ``--ntrain-yrs`` years are hidden; the infill chain (neighbour
matrices, mean / variance, daily PPCA with ``chk_perf``) runs on what is left, for all stations in batched GPU calls
instead of the reference's MPI farm; the model is compared with the hidden observations.  Both variables are run, with the
parameters of step15:204-211.

    python -m topowx_amd.step15 --db all.nc --normals step14_report.npz --xval-stnids ids.txt --out xval_infill.nc
                                [--report xval.npz] [--ntrain-yrs 5] [--device N] [--format NETCDF4|NETCDF3_64BIT]
                                [--nnr-dir DIR]

``--normals``: the monthly mean and variance of EVERY station of the database, which the reference reads from the station
table: one ``.npz`` with ``ids``, ``mean_tmin``, ``variance_tmin``, ``mean_tmax``, ``variance_tmax`` [n, 12], or a path with
``{var}`` in it that names the two reports of ``python -m topowx_amd.step14 --estimate`` (``ids``, ``mean``, ``variance``).
``--xval-stnids``: a text file of station ids, one per line; required (the reference's default lists are its data files and
are not shipped).  If the database has ``qflag_tmin`` / ``qflag_tmax`` the flagged observations are set to NaN first.

Writes the reference's file (``create_quick_db``): ``obs_tmin``, ``obs_tmax``, ``infilled_tmin``, ``infilled_tmax`` as f4 on
``(time, station_id)`` over the cross-validation stations, the hidden observation and the model on the scored days and
the fill value elsewhere.  Prints the writer's line per station and variable (``WRITER|id|var|MAE: x|BIAS: y``) and one
JSON line (stations, held days, items per status, seconds).  ``--report``: an ``.npz`` with ``ids``, ``ymd`` and per variable
``held_*``, ``n_*``, ``bias_*``, ``mae_*``, ``month_n_*``, ``month_bias_*``, ``month_mae_*``, ``em_status_*``, ``em_mean_*``,
``em_variance_*``, ``status_*``, ``matrix_status_*``, ``attempt_*``, ``npcs_*``.

Without ``--nnr-dir`` the values come from station columns only and the outputs are what they were before that flag
existed.  With ``--nnr-dir DIR`` (the subsets ``nnr_<var>_<time>.nc``, ``topowx_amd.NNRNghData``) the matrices of both stages
get the reference's reanalysis score columns; the station variable ``utc_offset`` (i2, what step13 writes) is read from the
database and the report gains ``ncomp_*``.  The estimators are restated ones (DESIGN.md sections 17 to 19): the values are
not what the reference would write.  ``--ppca-varyexplain`` (default 0.99, step15:209) is
there for pools whose noise is not the reference's.

Exits with 1 if a file cannot be opened, a station id is unknown, the normals do not cover the database's stations, or
``--nnr-dir`` is given and the database has no ``utc_offset`` or the subsets cannot be opened or do not cover its days.
"""
import argparse
import json
import sys
import time
import zipfile

import numpy as np

from . import _qalib, ncio
from . import stationdb as sdb
from ._cli import NNR_DIR_HELP, BadNormals, NnrInputError, UnknownIds, normals, open_nnr, read_ids
from .dates import YMD
from .infill import EM_STATUS, PP_STATUS, XvalInfill, XvalInfillParams
from .qa import StationObsPool
from .step14 import QFLAG_VARS

__all__ = ["main"]

VARS = ("tmin", "tmax")
OUT_VARIABLES = [("obs_tmin", "f4", ncio.FILL_F4, "observed minimum air temperature", "C"),
                 ("obs_tmax", "f4", ncio.FILL_F4, "observed maximum air temperature", "C"),
                 ("infilled_tmin", "f4", ncio.FILL_F4, "infilled minimum air temperature", "C"),
                 ("infilled_tmax", "f4", ncio.FILL_F4, "infilled maximum air temperature", "C")]      # step15:25-32
REPORT = ("held", "n", "bias", "mae", "month_n", "month_bias", "month_mae", "em_status", "em_mean", "em_variance")
REPORT_DAILY = ("status", "matrix_status", "attempt", "npcs")
REPORT_DAILY_NNR = ("ncomp",)             # with --nnr-dir


def _both_normals(path, pool):
    """{var: (mean, vari)} in the pool's station order."""
    if "{var}" in path:
        return {v: normals(path.replace("{var}", v), pool) for v in VARS}
    try:
        with np.load(path) as z:
            need = ["ids"] + ["%s_%s" % (k, v) for v in VARS for k in ("mean", "variance")]
            if not all(k in z.files for k in need):
                raise BadNormals("%s has no %s" % (path, " / ".join(need)))
            ids = [str(s) for s in z["ids"]]
            arr = {k: np.asarray(z[k], np.float64) for k in need[1:]}
    except (IOError, OSError, ValueError, KeyError, zipfile.BadZipFile) as e:
        raise BadNormals("cannot read the normals %s: %s" % (path, e))
    if any(a.shape != (len(ids), 12) for a in arr.values()):
        raise BadNormals("%s: mean / variance must be [%d, 12] over its ids" % (path, len(ids)))
    pos = {s: i for i, s in enumerate(ids)}
    missing = [s for s in pool.ids if str(s) not in pos]
    if missing:
        raise UnknownIds("%s: %d stations of the database have no normals (first: %s)" % (path, len(missing), missing[0]))
    order = [pos[str(s)] for s in pool.ids]
    return {v: (arr["mean_" + v][order], arr["variance_" + v][order]) for v in VARS}


def _elevation(path, n):
    ds = ncio.open_dataset(path, "r")
    try:
        if sdb.ELEV in ds.variables:
            v = ds.variables[sdb.ELEV]
            return ncio._masked_to_nan(v, v[:])
    finally:
        ds.close()
    return np.full(n, np.nan)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step15", description=__doc__.split("\n\n")[0])
    ap.add_argument("--db", required=True, help="all-stations database (netCDF): tmin / tmax on (time, station_id)")
    ap.add_argument("--normals", required=True, help="monthly mean / variance of every station (.npz; see above)")
    ap.add_argument("--xval-stnids", required=True, help="text file of cross-validation station ids, one per line")
    ap.add_argument("--out", required=True, help="cross-validation database to write (netCDF)")
    ap.add_argument("--report", help="report to write (.npz)")
    ap.add_argument("--ntrain-yrs", type=float, default=5, help="years of observations kept for training (step15:194)")
    ap.add_argument("--ppca-varyexplain", type=float, default=0.99)
    ap.add_argument("--format", choices=ncio.FORMATS, default=None, help="container of --out (default: the build's)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--nnr-dir", help=NNR_DIR_HELP)
    a = ap.parse_args(argv)
    nnr = utc = None
    try:
        ds = ncio.open_dataset(a.db, "r")
        try:
            qflags = all(name in ds.variables for name in QFLAG_VARS)
        finally:
            ds.close()
        pool = StationObsPool.from_netcdf(a.db, qflags=qflags)
        ids = read_ids(a.xval_stnids, pool, "cross-validation")
        if not ids or len(set(ids)) != len(ids):
            raise UnknownIds("%s: need at least one station id, each once" % a.xval_stnids)
        normals = _both_normals(a.normals, pool)
        elev = _elevation(a.db, pool.ids.size)
        if a.nnr_dir:
            nnr, utc = open_nnr(a.nnr_dir, a.db, pool)
    except (UnknownIds, BadNormals, NnrInputError) as e:
        print("step15: %s" % e, file=sys.stderr)
        return 1
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step15: cannot open %s: %s" % (getattr(e, "filename", None) or a.db, e), file=sys.stderr)
        return 1
    params = XvalInfillParams(nnr, 3, 4, 0.99, True, 0, 0.5, a.ppca_varyexplain, False)      # step15:204-211
    t0 = time.perf_counter()
    res, tms = {}, {}
    try:
        for v in VARS:
            tms[v] = {}
            xv = XvalInfill(pool, v, params, normals[v][0], normals[v][1], ids, a.ntrain_yrs, a.device, utc_offset=utc)
            res[v] = xv.run_all(tms[v])
    finally:
        if nnr is not None:
            nnr.close()
    sec = time.perf_counter() - t0
    cols = np.array([pool.idxs[s] for s in ids])
    stns = np.empty(len(ids), dtype=[(sdb.STN_ID, "U%d" % max(len(s) for s in ids)), (sdb.LON, np.float64),
                                     (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = ids, pool.lon[cols], pool.lat[cols], elev[cols]
    try:
        ncio.create_quick_db(a.out, stns, pool.days, OUT_VARIABLES, format=a.format)
        ds = ncio.open_dataset(a.out, "a")
        try:
            for x, sid in enumerate(ids):                            # the writer's loop (step15:127-143)
                for v in VARS:
                    print("|".join(["WRITER", sid, v, "MAE: %.2f" % res[v].mae[x], "BIAS: %.2f" % res[v].bias[x]]))
            for v in VARS:
                for name, rows in (("obs_" + v, res[v].obs_tair), ("infilled_" + v, res[v].infill_tair)):
                    ds.variables[name][:] = np.where(np.isnan(rows), ncio.FILL_F4, rows).T.astype(np.float32)
        finally:
            ds.close()
        if a.report:
            rep = dict(ids=np.array(ids), ymd=np.asarray(pool.days[YMD], np.int32))
            for v in VARS:
                rep.update({"%s_%s" % (k, v): getattr(res[v], k) for k in REPORT})
                rep.update({"%s_%s" % (k, v): getattr(res[v].daily, k)
                            for k in REPORT_DAILY + (REPORT_DAILY_NNR if nnr is not None else ())})
            np.savez_compressed(a.report, **rep)
    except (IOError, OSError) as e:
        print("step15: cannot write %s: %s" % (getattr(e, "filename", None) or a.out, e), file=sys.stderr)
        return 1
    line = {"step": "step15_xval_infill", "stations": len(ids), "pool": int(pool.ids.size), "days": int(pool.days.size),
            "nkeep": _qalib.xval_nkeep(a.ntrain_yrs), "seconds": round(sec, 3)}
    for v in VARS:
        r = res[v]
        line[v] = {"held": int(r.nheld.sum()), "scored": int(r.n.sum()),
                   "em_status": {EM_STATUS[k]: int((r.em_status == k).sum()) for k in sorted(EM_STATUS)
                                 if (r.em_status == k).any()},
                   "status": {PP_STATUS[k]: int((r.daily.status == k).sum()) for k in sorted(PP_STATUS)
                              if (r.daily.status == k).any()},
                   "nonoptimal": int(r.daily.nonoptimal.sum()), "calls": int(r.daily.calls),
                   "xv_holdout_kernel_ms": round(tms[v].get("xv_holdout_kernel_ms", 0.0), 3),
                   "xv_score_kernel_ms": round(tms[v].get("xv_score_kernel_ms", 0.0), 3)}
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
