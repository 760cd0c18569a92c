"""``create_netcdf_db`` / ``insert_data_netcdf_db`` with ``InsertGhcn`` (the reference's step04): the all-stations database
from GHCN-Daily's ``ghcnd-stations.txt`` and ``.dly`` files, parsed on the GPU (``twxgh_parse_dly``), and with ``--by-year``
the times of observation of Tmax from the by-year CSV files (``twxgh_parse_tobs``) as ``tobs_tmax``: the file every command
from step05 on takes as ``--db``.  With the three ``--raws-*`` arguments ``InsertRaws`` adds the RAWS sites from their WRCC
daily listings (``twxrw_parse``).

    python -m topowx_amd.step04 --stations ghcnd-stations.txt --dly-dir DIR --out all.nc --start YMD --end YMD
                                [--by-year DIR] [--check-obs-exist] [--format NETCDF4|NETCDF3_64BIT] [--device N]
                                [--raws-stations FILE --raws-ids FILE --raws-obs DIR] [--deflate gpu|host]

``--start`` / ``--end``: ``yyyymmdd`` or ``yyyy-mm-dd``, inclusive.  US / CA / MX stations outside HI and AK that are not
SNOTEL or RAWS sites are inserted; a station without a ``.dly`` file is an error unless ``--check-obs-exist`` drops it.
``--by-year DIR`` holds ``<year>.csv.gz`` (or ``<year>.csv``) for every year of the period.  The station variables are not
compressed unless ``--deflate`` asks for it: ``gpu`` creates them with ``zlib=True`` as the reference does and shuffles and
deflates every batch's rows on the GPU (``twxsd_deflate``), ``host`` leaves that to libhdf5.  ``--raws-stations`` (the metadata file), ``--raws-ids`` (the id file with the states) and ``--raws-obs`` (the
directory of the ``<id>.txt`` daily listings) go together, all three or none: the RAWS sites with a listing join the table,
with empty flags and no time of observation.  Where several lines of a listing give one day the last one wins (the
reference fails there) and the report counts them; a station name keeps its ASCII bytes; ``prcp`` is written.  Out of
scope: the SNOTEL insert, downloading (``add_utc_offset`` is step13: ``python -m topowx_amd.step13``).

Prints one JSON line (stations, days, bytes, lines, values, fallback fields, the RAWS counts as ``raws_*``, seconds, kernel
milliseconds).  Exits with 1 if a file is missing, a date is bad, a line's header is not a number or a RAWS line is one the
reference raises on.
"""
import argparse
import json
import sys
import time

from . import ghcn, ncio

__all__ = ["main"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step04", description=__doc__.split("\n\n")[0])
    ap.add_argument("--stations", required=True, help="ghcnd-stations.txt")
    ap.add_argument("--dly-dir", required=True, help="directory of the <id>.dly files")
    ap.add_argument("--out", required=True, help="the all-stations database to write (netCDF)")
    ap.add_argument("--start", required=True, help="first day of the period, yyyymmdd")
    ap.add_argument("--end", required=True, help="last day of the period, yyyymmdd")
    ap.add_argument("--by-year", help="directory of the by-year files <year>.csv.gz: writes tobs_tmax")
    ap.add_argument("--check-obs-exist", action="store_true", help="drop the stations without a .dly file")
    ap.add_argument("--format", choices=ncio.FORMATS, help="container (default: NETCDF4 when libhdf5 loads)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--raws-stations", help="the RAWS station metadata file")
    ap.add_argument("--raws-ids", help="the RAWS station id file (state and id)")
    ap.add_argument("--raws-obs", help="directory of the RAWS daily listings <id>.txt")
    ap.add_argument("--deflate", choices=("gpu", "host"), help="compress the station variables (default: not compressed)")
    a = ap.parse_args(argv)
    raws = (a.raws_stations, a.raws_ids, a.raws_obs)
    if any(r is not None for r in raws) and not all(r is not None for r in raws):
        ap.error("--raws-stations, --raws-ids and --raws-obs go together: all three or none")
    tm, st = {}, {}
    t0 = time.perf_counter()
    try:
        stns = ghcn.create_all_stations_db(a.out, a.stations, a.dly_dir, a.start, a.end, path_by_year=a.by_year,
                                           check_obs_exist=a.check_obs_exist, format=a.format, device=a.device, timing=tm,
                                           stats=st, raws=raws if raws[0] is not None else None, deflate=a.deflate)
    except (IOError, OSError, ValueError, KeyError, IndexError) as e:
        print("step04: %s" % e, file=sys.stderr)
        return 1
    line = {"stations": int(stns.size), "days": ghcn._period(a.start, a.end)[3], "seconds": round(time.perf_counter() - t0, 3)}
    for src in (st, tm):
        for k in sorted(src):
            line[k] = round(src[k], 3) if isinstance(src[k], float) else src[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
