"""``add_obs_cnt`` / ``build_por_mask`` (the reference's step05 and the period-of-record masks of step09, step14 and
step16): the observation counts per calendar month of Tmin and Tmax over a period, written into the database as
``obs_cnt_<elem>_<start>_<end>``, every station in one ``twxhm_obs_cnt`` call per variable.

    python -m topowx_amd.step05 --db DB --start YMD --end YMD [--min-por-yrs N --ids-out FILE] [--device N]

``--start`` / ``--end``: ``yyyymmdd`` or ``yyyy-mm-dd``, inclusive.  The counts are of the variables as stored: quality
flags are not applied, as in the reference.  With ``--min-por-yrs N --ids-out FILE`` the ids of the stations with N years of
observations in every calendar month for Tmin or for Tmax are written one per line: the file
``python -m topowx_amd.step14 --targets / --neighbours`` takes.

Prints one JSON line (stations, days in the period, per variable the stations with any observation, with the mask the
stations that pass; seconds, kernel milliseconds).  Exits with 1 if the database cannot be opened or a date is bad.
"""
import argparse
import json
import sys
import time

from . import ncio
from .obs_por import add_obs_cnt, build_por_mask

__all__ = ["main"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step05", description=__doc__.split("\n\n")[0])
    ap.add_argument("--db", required=True, help="station database (netCDF), updated in place")
    ap.add_argument("--start", required=True, help="first day of the period, yyyymmdd")
    ap.add_argument("--end", required=True, help="last day of the period, yyyymmdd")
    ap.add_argument("--min-por-yrs", type=int, help="with --ids-out: years of observations needed in every calendar month")
    ap.add_argument("--ids-out", help="text file of the ids of the stations that pass, one per line")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if (a.min_por_yrs is None) != (a.ids_out is None):
        ap.error("--min-por-yrs and --ids-out go together")
    tm, line = {}, {}
    t0 = time.perf_counter()
    try:
        ncio.file_format(a.db)
        for elem in ("tmin", "tmax"):
            cnt = add_obs_cnt(a.db, elem, a.start, a.end, device=a.device, timing=tm)
            line[elem] = {"stations": int(cnt.shape[0]), "with_obs": int((cnt.sum(axis=1) > 0).sum()), "obs": int(cnt.sum())}
        if a.ids_out:
            with ncio.open_dataset(a.db, "r") as ds:
                mask = build_por_mask(ds, ["tmin", "tmax"], a.start, a.end, a.min_por_yrs)
                ids = ncio._read_ids(ds.variables["station_id"])
            with open(a.ids_out, "w") as f:
                f.writelines("%s\n" % s for s in ids[mask])
            line["passed"] = int(mask.sum())
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step05: %s: %s" % (getattr(e, "filename", None) or a.db, e), file=sys.stderr)
        return 1
    line["seconds"] = round(time.perf_counter() - t0, 3)
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
