"""``scripts/step11_homog_tair.py`` on either side of the external PHA program.  ``--setup`` writes PHA's input tree for Tmin
and Tmax from the monthly means of ``python -m topowx_amd.step10``; PHA is then unpacked, built and run by hand;
``--apply`` reads its adjustment logs and homogenised monthly files, homogenises every station's daily series in one
``twxhm_homog_daily`` call per variable, writes the homogenised database and adds its observation counts.

    python -m topowx_amd.step11 --db tobs_adj.nc --pha-dir DIR --setup [--stnhist FILE.csv]
    python -m topowx_amd.step11 --db tobs_adj.nc --pha-dir DIR --apply --out homog.nc --start YMD --end YMD
                                [--format NETCDF4|NETCDF3_64BIT] [--device N]

``--pha-dir``: the run directories are ``DIR/tmin`` and ``DIR/tmax``; below each, ``data/benchmark/world1/`` holds
``meta/world1_stnlist.<var>``, ``meta/world1_metadata_file.txt``, ``monthly/raw/<id>.raw.<var>`` (written by ``--setup``) and
``monthly/FLs.r00/<id>.FLs.r00.<var>``, ``output/pha_adj_<var>.log``, ``corr/*input_not_stnlist`` (PHA's, read by
``--apply``).  ``--stnhist``: a CSV of ``station_id,yyyymm`` lines (documented station changes) for the metadata file.
``--start`` / ``--end``: the period of the observation counts of the new database.  An existing ``--out`` is not overwritten.

Prints one JSON line.  Exits with 1 if a file cannot be opened or written, or a station's adjustment list is missing or
overlapping (the message names the station).

Out of scope: unpacking, building and running PHA (``setup_pha``'s first half, ``run_pha``); the USHCN reference series and
the SNOTEL sensor history the reference adds to PHA's input (``--stnhist`` takes such a history from a file).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

from . import ncio
from .homog import create_homog_db, write_input_station_data
from .obs_por import add_obs_cnt, month_axis, read_rows

__all__ = ["main", "setup"]


def setup(path_db, pha_dir, stnhist=()):
    """PHA's input tree for both variables; returns per variable the number of stations written."""
    stns, _, days, _ = ncio.read_station_db_arrays(path_db, "")
    _, _, mth_ymd = month_axis(days)
    yrs = np.unique(mth_ymd // 10000)
    n = {}
    with ncio.open_dataset(path_db, "r") as ds:
        for var in ("tmin", "tmax"):
            if var + "_mth" not in ds.variables:
                raise KeyError("%s has no variable %s_mth (python -m topowx_amd.step10 writes it)" % (path_db, var))
            mean = read_rows(ds, var + "_mth")
            write_input_station_data(os.path.join(pha_dir, var), var, stns, np.ma.masked_invalid(mean.T), yrs, stnhist)
            n[var] = int(stns.size)
    return n


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step11", description=__doc__.split("\n\n")[0])
    ap.add_argument("--db", required=True, help="time-of-observation adjusted database with the monthly means (netCDF)")
    ap.add_argument("--pha-dir", required=True, help="directory of the two PHA run directories, tmin/ and tmax/")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--setup", action="store_true", help="write PHA's input tree")
    g.add_argument("--apply", action="store_true", help="read PHA's output and write the homogenised database")
    ap.add_argument("--stnhist", help="with --setup: CSV of station_id,yyyymm lines for PHA's metadata file")
    ap.add_argument("--out", help="with --apply: homogenised database to write")
    ap.add_argument("--start", help="with --apply: first day of the period of the observation counts, yyyymmdd")
    ap.add_argument("--end", help="with --apply: last day of that period, yyyymmdd")
    ap.add_argument("--format", choices=ncio.FORMATS, help="container of the output (default: ncio.default_format())")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.apply and not (a.out and a.start and a.end):
        ap.error("--apply needs --out, --start and --end")
    tm, line = {}, {}
    t0 = time.perf_counter()
    cur = a.db
    try:
        ncio.file_format(a.db)
        if a.setup:
            hist = []
            if a.stnhist:
                cur = a.stnhist
                with open(a.stnhist, newline="") as f:
                    hist = [(r[0].strip(), r[1].strip()) for r in csv.reader(f) if len(r) >= 2 and r[1].strip().isdigit()]
                cur = a.db
            line["written"] = setup(a.db, a.pha_dir, hist)
            line["stnhist"] = len(hist)
        else:
            if os.path.exists(a.out):
                raise IOError("%s exists: not overwritten" % a.out)
            cur = a.pha_dir
            r = create_homog_db(a.db, a.out, os.path.join(a.pha_dir, "tmin"), os.path.join(a.pha_dir, "tmax"),
                                format=a.format, device=a.device, timing=tm)
            cur = a.out
            line["stations"] = int(r["ids"].size)
            for var in ("tmin", "tmax"):
                cnt = add_obs_cnt(a.out, var, a.start, a.end, device=a.device, timing=tm)
                line[var] = {"homogenised": int(r["used"][var].sum()), "months_changed": int(r["nchanged"][var].sum()),
                             "obs": int(cnt.sum())}
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step11: %s: %s" % (getattr(e, "filename", None) or cur, e), file=sys.stderr)
        return 1
    line["seconds"] = round(time.perf_counter() - t0, 3)
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
