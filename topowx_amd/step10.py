"""``add_monthly_means`` of the reference's step10: ``time_mth``, ``<var>_mth`` and ``<var>_mthmiss`` of Tmin and Tmax (monthly
means with at most 9 missing days, and the missing days of every month), the input of PHA, every station in one
``twxhm_monthly_means`` call per variable.

    python -m topowx_amd.step10 --db tobs_adj.nc [--max-miss 9] [--device N]

The database is updated in place; its day axis must cover whole calendar years.

Prints one JSON line (per variable the stations, months, masked means; seconds, kernel milliseconds).  Exits with 1 if the
database cannot be opened or its axis is not whole years.
"""
import argparse
import json
import sys
import time

import numpy as np

from . import ncio
from .obs_por import add_monthly_means

__all__ = ["main"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step10", description=__doc__.split("\n\n")[0])
    ap.add_argument("--db", required=True, help="time-of-observation adjusted database (netCDF), updated in place")
    ap.add_argument("--max-miss", type=int, default=9, help="missing days a month may have (negative: no threshold)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    tm, line = {}, {}
    t0 = time.perf_counter()
    try:
        ncio.file_format(a.db)
        for var in ("tmin", "tmax"):
            mean, _ = add_monthly_means(a.db, var, max_miss=a.max_miss, device=a.device, timing=tm)
            line[var] = {"stations": int(mean.shape[0]), "months": int(mean.shape[1]), "masked": int(np.isnan(mean).sum())}
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step10: %s: %s" % (getattr(e, "filename", None) or a.db, e), file=sys.stderr)
        return 1
    line["seconds"] = round(time.perf_counter() - t0, 3)
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
