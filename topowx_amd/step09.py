"""``scripts/step09_tobs_adj.py``: the time-of-observation adjusted database.  The stations with one year of Tmin or of
Tmax (``build_por_mask``, ``min_por_yrs`` = 1), flagged observations removed, Tmax of the morning observers moved back a
day (``_tobs_shift_tmax``), every station in one ``twxhm_tobs_shift`` call.

    python -m topowx_amd.step09 --db all.nc --out tobs_adj.nc --start YMD --end YMD [--format NETCDF4|NETCDF3_64BIT] [--device N]

``--db``: the database ``python -m topowx_amd.step08 --write`` has flagged, with ``tobs_tmax`` (the time of observation of
Tmax on every day, hhmm) and the counts of ``python -m topowx_amd.step05`` for the same ``--start`` / ``--end``.  An
existing output file is not overwritten.

Prints one JSON line (stations kept, per variable the stations with a record, stations whose Tmax moved; seconds, kernel
milliseconds).  Exits with 1 if a file cannot be opened or written or a variable is missing.

``tobs_tmax`` is what ``python -m topowx_amd.step04 --by-year DIR`` writes (``create_tobs_file`` / ``create_tobs_db``: the
search of GHCN-D's yearly files).
"""
import argparse
import json
import os
import sys
import time

from . import ncio
from .homog import create_tobs_adjusted_db

__all__ = ["main"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step09", description=__doc__.split("\n\n")[0])
    ap.add_argument("--db", required=True, help="flagged all-stations database (netCDF) with tobs_tmax and the counts")
    ap.add_argument("--out", required=True, help="time-of-observation adjusted database to write")
    ap.add_argument("--start", required=True, help="first day of the period of the counts, yyyymmdd")
    ap.add_argument("--end", required=True, help="last day of the period of the counts, yyyymmdd")
    ap.add_argument("--format", choices=ncio.FORMATS, help="container of the output (default: ncio.default_format())")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    tm = {}
    t0 = time.perf_counter()
    try:
        ncio.file_format(a.db)
        if os.path.exists(a.out):
            raise IOError("%s exists: not overwritten" % a.out)
        r = create_tobs_adjusted_db(a.db, a.out, a.start, a.end, format=a.format, device=a.device, timing=tm)
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step09: %s: %s" % (getattr(e, "filename", None) or a.db, e), file=sys.stderr)
        return 1
    line = {"stations": int(r["ids"].size), "tmin": int(r["mask_tmin"].sum()), "tmax": int(r["mask_tmax"].sum()),
            "shifted": int((r["nshift"] > 1).sum()), "seconds": round(time.perf_counter() - t0, 3)}
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
