"""``scripts/step16_mpi_infill_stn_daily.py``: the daily infill of every target station and calendar month
(``topowx_amd.infill.infill_daily``): neighbour matrices, then the PPCA with its search for the number of components, in
batched GPU calls instead of the reference's MPI farm over stations.  A report: nothing is written into the database.

    python -m topowx_amd.step16 --db all.nc --var tmin --normals step14_report.npz --out infilled.npz [--targets ids.txt]
                                [--device N] [--chk-perf [--cpt-sig X]]

``--normals``: the report of ``python -m topowx_amd.step14 --estimate`` run for EVERY station of the database (``ids``,
``mean``, ``variance`` [n, 12]); a station without a finite mean and variance in a month is no neighbour that month, as
the reference's ``stns_mask`` has it.  ``--targets``: a text file of station ids, one per line (default: every station).
If the database has ``qflag_tmin`` / ``qflag_tmax`` the flagged observations are set to NaN first.

Prints one JSON line (stations, items, items per status, fits, calls, seconds, kernel milliseconds) and writes
``infilled.npz``: ``ids`` [ntarget], ``ymd`` [ndays], ``fnl_tair``, ``mask_infill``, ``infill_tair`` [ntarget, ndays], ``mae``,
``bias`` [ntarget], and per item [ntarget, 12] ``status`` (``topowx_amd.infill.PP_STATUS``), ``matrix_status``, ``npcs``,
``nfits``, ``iters``, ``r2_not_reached``, ``ncols``, ``item_mae``, ``item_r2``, ``item_impossible``.

``--chk-perf``: judge every fit as the reference's ``_is_nonoptimal_infill`` does (MAE, r2, impossible values, a variance
change point at the level ``--cpt-sig``, default 1e-10) and refit the non-optimal ones up its retry ladder
(``infill_daily(chk_perf=True)``).  The report then also holds ``attempt``, ``nattempts``,
``nonoptimal``, ``retry_fixed``, ``cpt_stat``, ``cpt_tau``, ``cpt_pen`` [ntarget, 12] and ``reasons``, ``attempt_mae``,
``attempt_r2`` [ntarget, 12, 4], and the JSON line ``attempt_items`` (items per attempt), ``nonoptimal``, ``retry_fixed`` and
the check's ``ck_check_kernel_ms``.  Without the flag the report and the JSON line are what they were.

Without ``--nnr-dir`` the values come from station columns only and the report is what it was before that flag existed.
With ``--nnr-dir DIR`` (the subsets ``nnr_<var>_<time>.nc``, ``topowx_amd.NNRNghData``) every matrix gets the reference's
reanalysis score columns, and the ladder's 0.90 attempt takes the leading columns of the same decomposition; the station
variable ``utc_offset`` (i2, what step13 writes) is read from the database, and the report gains ``ncomp`` [ntarget, 12].  The
estimator is a restated one whose start is not R's, so there is no ``--write``.

Out of scope: ``tair_mask`` (step15's cross-validation is ``python -m topowx_amd.step15``), step12's subsetting of the raw
yearly reanalysis files and step13's time-zone lookup.  The
infilled database is written from this report by ``python -m topowx_amd.step17 --report-*``.  The variance change-point check is restated, not R's ``changepoint`` executed.

Exits with 1 if a file cannot be opened, a station id is unknown, the normals do not cover the database's stations, or
``--nnr-dir`` is given and the database has no ``utc_offset`` or the subsets cannot be opened or do not cover its days.
"""
import argparse
import json
import sys
import time

import numpy as np

from . import ncio
from ._cli import (NNR_DIR_HELP, BadNormals as _BadNormals, NnrInputError as _NnrInputError, UnknownIds as _UnknownIds,
                   normals as _normals, open_nnr as _open_nnr, read_ids as _read_ids)
from .dates import YMD
from .infill import PP_STATUS, infill_daily
from .qa import StationObsPool
from .step14 import QFLAG_VARS

__all__ = ["main"]

ITEM_COLUMNS = ("status", "matrix_status", "npcs", "nfits", "iters", "r2_not_reached", "ncols", "item_mae", "item_r2",
                "item_impossible")
CHK_COLUMNS = ("attempt", "nattempts", "nonoptimal", "retry_fixed", "cpt_stat", "cpt_tau", "cpt_pen", "reasons", "attempt_mae",
               "attempt_r2")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step16", description=__doc__.split("\n\n")[0])
    ap.add_argument("--db", required=True, help="all-stations database (netCDF): tmin / tmax on (time, station_id)")
    ap.add_argument("--var", required=True, choices=("tmin", "tmax"))
    ap.add_argument("--normals", required=True, help="report of step14 --estimate over every station (.npz)")
    ap.add_argument("--out", required=True, help="report to write (.npz)")
    ap.add_argument("--targets", help="text file of target station ids, one per line (default: every station)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--chk-perf", action="store_true", help="judge every fit and refit the non-optimal ones up the retry ladder")
    ap.add_argument("--cpt-sig", type=float, default=1e-10, help="level of the variance change-point check (with --chk-perf)")
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
        targets = _read_ids(a.targets, pool, "target") if a.targets else list(pool.ids)
        mean, vari = _normals(a.normals, pool)
        if a.nnr_dir:
            nnr, utc = _open_nnr(a.nnr_dir, a.db, pool)
            utc = utc[[pool.idxs[str(s)] for s in targets]]
    except (_UnknownIds, _BadNormals, _NnrInputError) as e:
        print("step16: %s" % e, file=sys.stderr)
        return 1
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step16: cannot open %s: %s" % (getattr(e, "filename", None) or a.db, e), file=sys.stderr)
        return 1
    tm = {}
    t0 = time.perf_counter()
    if nnr is not None:
        try:
            r = infill_daily(pool, a.var, targets, mean, vari, nnr, utc, device=a.device, timing=tm, chk_perf=a.chk_perf,
                             cpt_sig=a.cpt_sig)
        finally:
            nnr.close()
    elif a.chk_perf:
        r = infill_daily(pool, a.var, targets, mean, vari, device=a.device, timing=tm, chk_perf=True, cpt_sig=a.cpt_sig)
    else:
        r = infill_daily(pool, a.var, targets, mean, vari, device=a.device, timing=tm)
    sec = time.perf_counter() - t0
    np.savez_compressed(a.out, ids=r.target_ids, ymd=np.asarray(pool.days[YMD], np.int32), fnl_tair=r.fnl_tair,
                        mask_infill=r.mask_infill, infill_tair=r.infill_tair, mae=r.mae, bias=r.bias,
                        **{k: getattr(r, k) for k in ITEM_COLUMNS + (CHK_COLUMNS if a.chk_perf else ()) +
                           (("ncomp",) if nnr is not None else ())})
    line = {"var": a.var, "stations": int(r.target_ids.size), "pool": int(pool.ids.size), "days": int(pool.days.size),
            "items": int((r.status >= 0).sum()),
            "status": {PP_STATUS[k]: int((r.status == k).sum()) for k in sorted(PP_STATUS) if (r.status == k).any()},
            "fits": int(r.nfits.sum()), "calls": int(r.calls), "r2_not_reached": int(r.r2_not_reached.sum()),
            "seconds": round(sec, 3)}
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
