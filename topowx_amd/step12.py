"""The reference's step12 (scripts/step12_process_reanalysis_data.py:31-146) without its downloads: the 21 North American
subsets ``nnr_<var>_<12z|18z|24z>.nc`` of the NCEP/NCAR reanalysis that ``--nnr-dir`` of step14, step15 and step16 names,
from the raw yearly files ``<var>.<year>.nc`` (air, hgt, rhum, vwnd, uwnd on pressure levels; slp).  The yearly files of a
raw variable are read once and every product of it is formed in one call of libtwxqa's ``twxns_subset``
(``reanalysis.create_nnr_subsets``): hgt gives six files from one reading.

    python -m topowx_amd.step12 --nnr-raw DIR --out DIR --start-year Y --end-year Y [--format NETCDF4|NETCDF3_64BIT]
                                [--device N]

The period runs from 1 January of ``--start-year`` to 31 December of ``--end-year`` PLUS ONE, as the script's lines 35-36
have it, and a yearly file of every year of it must exist.  Products: tair (air at 850 hPa, Kelvin to Celsius), thick
(hgt 500 - hgt 1000), hgt (500 and 700), rhum, vwnd, uwnd (850) and slp, each at 12z, 18z and 24z.  Nothing is downloaded.

Prints one JSON line (days, years, files, seconds, the stages' seconds and milliseconds, the counts of every file: days
with a record, values filled for a mark, days unwritten).  Exits with 1 if a file is missing or cannot be dated.
"""
import argparse
import datetime as _dt
import json
import os
import sys
import time

import numpy as np

from . import _qalib, ncio, reanalysis
from .dates import YEAR, get_days_metadata

__all__ = ["main", "PRODUCTS", "period"]

UTC = (12, 18, 24)


def _each(stem, **kw):
    return [dict(fname="nnr_%s_%dz.nc" % (stem, u), utc_time=u, **kw) for u in UTC]


# raw variable -> its products, in the script's order (:43-146)
PRODUCTS = (("air", _each("tair", varname_out="tair", levels=(850,), conv="k_to_c")),
            ("hgt", _each("thick", varname_out="thick", thick=(500, 1000)) + _each("hgt", varname_out="hgt", levels=(500, 700))),
            ("rhum", _each("rhum", varname_out="rhum", levels=(850,))),
            ("vwnd", _each("vwnd", varname_out="vwnd", levels=(850,))),
            ("uwnd", _each("uwnd", varname_out="uwnd", levels=(850,))),
            ("slp", _each("slp", varname_out="slp")))


def period(start_year, end_year):
    """The days of step12 (:35-37): 1 January of the start year to 31 December of the end year + 1."""
    return get_days_metadata(_dt.date(int(start_year), 1, 1), _dt.date(int(end_year) + 1, 12, 31))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step12", description=__doc__.split("\n\n")[0])
    ap.add_argument("--nnr-raw", required=True, help="directory of the raw yearly files <var>.<year>.nc")
    ap.add_argument("--out", required=True, help="directory of the subsets to write")
    ap.add_argument("--start-year", required=True, type=int, help="first year of the interpolation period")
    ap.add_argument("--end-year", required=True, type=int, help="last year of the interpolation period (the subsets run a year on)")
    ap.add_argument("--format", choices=ncio.FORMATS, help="container (default: NETCDF4 when libhdf5 loads)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    tm = {}
    t0 = time.perf_counter()
    try:
        if a.end_year < a.start_year:
            raise ValueError("the period ends before it starts")
        days = period(a.start_year, a.end_year)
        yrs = np.unique(days[YEAR])
        os.makedirs(a.out, exist_ok=True)
        files = []
        for raw_var, products in PRODUCTS:
            files += reanalysis.create_nnr_subsets(a.nnr_raw, a.out, yrs, days, raw_var, products, format=a.format,
                                                   device=a.device, timing=tm)
    except (IOError, OSError, ValueError, KeyError, _qalib.QaError) as e:
        print("step12: %s" % e, file=sys.stderr)
        return 1
    line = {"days": int(days.size), "years": int(yrs.size), "files": len(files), "seconds": round(time.perf_counter() - t0, 3)}
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
