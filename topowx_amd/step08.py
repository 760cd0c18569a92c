"""The spatial regression check of ``scripts/step08_mpi_qa_temp.py --spatial`` as a report.

Every station of an all-stations database (or the ``--targets`` subset) is checked against the stations within 75 km
(``topowx_amd.qa.qa_spatial_regress``: one batched GPU call instead of the reference's MPI farm over stations).

Nothing is written into the database.  The reference's ``run_qa_spatial_only`` (qa_temp.py:218-240) goes on from this
check to the corroboration check -- which sees the observations this check removed -- and to ``_qa_mega_inconsist``;
only the three together decide the ``qflag_*`` that step08 writes.  The corroboration check is not built yet, so the
flags of this check alone go into a report:

    python -m topowx_amd.step08 --db all.nc --out report.npz [--targets ids.txt] [--device N]

prints one JSON line (stations, items, flags per variable, seconds, kernel milliseconds) and writes ``report.npz``:
``ids`` [ntarget], ``ymd`` [ndays], ``flags_tmin`` / ``flags_tmax`` [ndays, ntarget] (1 ok, 2 missing, 16 flagged) and
the per-item ``status`` [ntarget, 2, nmonths].  Exits with 1 if the database cannot be opened or a target is unknown.
"""
import argparse
import json
import sys
import time

import numpy as np

from .dates import YMD
from .qa import QA_SPATIAL_REGRESS, StationObsPool, qa_spatial_regress

__all__ = ["main"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step08",
                                 description="step08's spatial regression check of daily Tmin / Tmax: a report of the "
                                             "flags, nothing is written into the database")
    ap.add_argument("--db", required=True, help="all-stations database (netCDF): tmin / tmax on (time, station_id)")
    ap.add_argument("--out", required=True, help="report to write (.npz)")
    ap.add_argument("--targets", help="text file of station ids to check, one per line (default: every station)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        pool = StationObsPool.from_netcdf(a.db)
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
    tm = {}
    t0 = time.perf_counter()
    f_tmin, f_tmax, det = qa_spatial_regress(pool, targets, device=a.device, details=True, timing=tm)
    sec = time.perf_counter() - t0
    ids = pool.ids if targets is None else np.array(targets, dtype=str)
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
