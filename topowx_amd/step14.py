"""``scripts/step14_mpi_infill_stn_normals.py``: the infill neighbour matrices of every target station and calendar
month (``topowx_amd.infill.build_infill_matrices``) and, with ``--estimate``, the mean and variance of every item from
them (``topowx_amd.infill.estimate_mean_variance``), each in one batched GPU call instead of the reference's MPI farm
over stations.  A report: nothing is written into the database.

    python -m topowx_amd.step14 --db all.nc --var tmin --out matrices.npz [--targets ids.txt] [--neighbours ids.txt]
                                [--device N] [--estimate [--nnr-dir DIR]]

``--targets``: the stations to build matrices for (default: every station); ``--neighbours``: the stations that may serve
as neighbours, the reference's ``stns_mask`` (default: every station; a target is never its own neighbour).  Both are
text files of station ids, one per line; they stand in for the reference's ``build_por_mask``.  If the database has
``qflag_tmin`` / ``qflag_tmax`` the observations that carry a flag are set to NaN first, as the reference's
``load_all_stn_obs_var(set_flagged_nan=True)`` does.

Prints one JSON line (stations, items, items per status, rounds, seconds, kernel milliseconds) and writes
``matrices.npz``: ``ids`` [ntarget], ``pool_ids`` [n], ``ymd`` [ndays], ``group`` [ndays] (month - 1), ``status``, ``nnghs``,
``max_dist``, ``nthres_target_por`` [ntarget, 12], ``nthres_all`` [12], and the ranked lists as CSR columns over ``off``
[ntarget * 12 + 1] (item = target * 12 + month - 1): ``idx`` (row of ``pool_ids``), ``ioa``, ``dist``, ``nlap``, ``nlap_stn``,
``keep``.  The observation matrix of an item is the target's column and the columns ``idx[keep == 1][:30]`` of the
database on the item's days (``InfillMatrices.matrix``).

``--estimate`` adds ``mean``, ``variance``, ``em_iters``, ``em_status`` [ntarget, 12] (``topowx_amd.infill.EM_STATUS``) to the
report, and the items per estimator status (``em_status``), the launches and the kernel milliseconds to the JSON line.
Without ``--nnr-dir`` the values are estimated from station columns only and the output is what it was before that flag
existed.  With ``--nnr-dir DIR`` (the subsets ``nnr_<var>_<time>.nc``, ``topowx_amd.NNRNghData``) every matrix gets the
reference's reanalysis score columns, all items decomposed in one ``twxnr_components`` call; the station variable
``utc_offset`` (i2, what step13 writes) is read from the database, and the report gains ``ncols`` / ``ncomp`` [ntarget, 12].
The estimator is the restated one, so there is still no ``--write``.

Out of scope: ``build_por_mask``, writing the estimates into the database, step12's subsetting of the raw yearly reanalysis
files and step13's time-zone lookup.

Exits with 1 if the database cannot be opened, a station id is unknown, or ``--nnr-dir`` is given and the database has no
``utc_offset`` or the subsets cannot be opened or do not cover the database's days.  ``--nnr-dir`` without ``--estimate`` is a
usage error.
"""
import argparse
import json
import sys
import time

import numpy as np

from . import ncio
from ._cli import NNR_DIR_HELP, NnrInputError as _NnrInputError, UnknownIds as _UnknownIds, open_nnr as _open_nnr, read_ids as _read_ids
from .dates import YMD
from .infill import EM_STATUS, ITEM_STATUS, build_infill_matrices, estimate_mean_variance
from .qa import StationObsPool

__all__ = ["main"]

QFLAG_VARS = ("qflag_tmin", "qflag_tmax")
COLUMNS = ("status", "nnghs", "max_dist", "nthres_all", "nthres_target_por", "off", "idx", "ioa", "dist", "nlap", "nlap_stn",
           "keep")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step14", description=__doc__.split("\n\n")[0])
    ap.add_argument("--db", required=True, help="all-stations database (netCDF): tmin / tmax on (time, station_id)")
    ap.add_argument("--var", required=True, choices=("tmin", "tmax"))
    ap.add_argument("--out", required=True, help="report to write (.npz)")
    ap.add_argument("--targets", help="text file of target station ids, one per line (default: every station)")
    ap.add_argument("--neighbours", help="text file of the station ids that may be neighbours (default: every station)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--estimate", action="store_true",
                    help="also estimate the mean and variance of every item (station columns only unless --nnr-dir is given)")
    ap.add_argument("--nnr-dir", help=NNR_DIR_HELP + " (with --estimate)")
    a = ap.parse_args(argv)
    if a.nnr_dir and not a.estimate:
        ap.error("--nnr-dir needs --estimate: the matrices themselves hold no reanalysis column")
    nnr = utc = None
    try:
        ds = ncio.open_dataset(a.db, "r")
        try:
            qflags = all(name in ds.variables for name in QFLAG_VARS)
        finally:
            ds.close()
        pool = StationObsPool.from_netcdf(a.db, qflags=qflags)
        targets = _read_ids(a.targets, pool, "target") if a.targets else None
        mask = None
        if a.neighbours:
            mask = np.zeros(pool.ids.size, bool)
            mask[[pool.idxs[s] for s in _read_ids(a.neighbours, pool, "neighbour")]] = True
        if a.nnr_dir:
            nnr, utc = _open_nnr(a.nnr_dir, a.db, pool)
    except (_UnknownIds, _NnrInputError) as e:
        print("step14: %s" % e, file=sys.stderr)
        return 1
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step14: cannot open %s: %s" % (getattr(e, "filename", None) or a.db, e), file=sys.stderr)
        return 1
    tm = {}
    t0 = time.perf_counter()
    m = build_infill_matrices(pool, a.var, targets, mask, device=a.device, timing=tm)
    extra = {}
    if a.estimate:
        if nnr is None:
            e = estimate_mean_variance(m, device=a.device, timing=tm)
        else:
            try:
                e = estimate_mean_variance(m, nnr, utc[m.target_cols], device=a.device, timing=tm)
            finally:
                nnr.close()
        extra = dict(mean=e.mean, variance=e.variance, em_iters=e.iters, em_status=e.status)
        if nnr is not None:
            extra.update(ncols=e.ncols, ncomp=e.ncomp)
    sec = time.perf_counter() - t0
    np.savez_compressed(a.out, ids=m.target_ids, pool_ids=pool.ids, ymd=np.asarray(pool.days[YMD], np.int32), group=m.group,
                        **dict({k: getattr(m, k) for k in COLUMNS}, **extra))
    line = {"var": a.var, "stations": int(m.target_ids.size), "pool": int(pool.ids.size), "days": int(pool.days.size),
            "eligible": int(pool.ids.size if mask is None else mask.sum()), "items": int(m.status.size),
            "status": {ITEM_STATUS[k]: int((m.status == k).sum()) for k in sorted(ITEM_STATUS) if (m.status == k).any()},
            "ranked": int(m.idx.size), "kept": int(m.keep.sum()), "seconds": round(sec, 3)}
    if a.estimate:
        line["em_status"] = {EM_STATUS[k]: int((e.status == k).sum()) for k in sorted(EM_STATUS) if (e.status == k).any()}
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
