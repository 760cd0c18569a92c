"""``scripts/step18_create_final_stn_nc.py``: the serially-complete station databases ``serial_tmin.nc`` /
``serial_tmax.nc`` from the two infilled databases (``topowx_amd.infill.create_serially_complete_db``: per station
"observations + infill" or, after 5 years of consecutive infilled days, "all model"; values still missing become the fill
value) with the monthly normals ``norm01 .. norm12`` (``add_monthly_normals``: monthly means with at most 9 missing days).
Every station of a variable goes through one batched ``twxsc_serial_complete`` call, where the reference loops over the
stations through netCDF.

    python -m topowx_amd.step18 --infill-tmin A.nc --infill-tmax B.nc --serial-tmin C.nc --serial-tmax D.nc
                                [--start-norm-yr 1981] [--end-norm-yr 2010] [--format NETCDF4|NETCDF3_64BIT] [--device N]
                                [--deflate gpu|host]

The infilled databases are what ``python -m topowx_amd.step17 --report-*`` (``write_infill_db``) or the reference's step16
wrote.  An existing output file is not overwritten.  The outputs are what ``python -m topowx_amd.step20``,
``topowx_amd.xval`` and the interpolation read (``ncio.read_station_db``).

Prints one JSON line (per variable the stations, days, stations with all infilled values and with missing values, months
with a normal; seconds, kernel milliseconds).  Exits with 1 if a file cannot be opened or written.

What follows: ``python -m topowx_amd.step19`` (``add_stn_raster_values``) and ``python -m topowx_amd.step20`` with its
``--infill-*`` arguments (``find_dup_stns``, the TDI and climate-division checks).
"""
import argparse
import contextlib
import json
import sys
import time

import numpy as np

from . import ncio
from .infill import add_monthly_normals, create_serially_complete_db
from .stationdb import StationSerialDataDb

__all__ = ["main"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step18", description=__doc__.split("\n\n")[0])
    ap.add_argument("--infill-tmin", required=True, help="infilled Tmin database (netCDF)")
    ap.add_argument("--infill-tmax", required=True, help="infilled Tmax database (netCDF)")
    ap.add_argument("--serial-tmin", required=True, help="serially-complete Tmin database to write")
    ap.add_argument("--serial-tmax", required=True, help="serially-complete Tmax database to write")
    ap.add_argument("--start-norm-yr", type=int, default=1981)
    ap.add_argument("--end-norm-yr", type=int, default=2010)
    ap.add_argument("--format", choices=ncio.FORMATS, help="container of the outputs (default: ncio.default_format())")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--deflate", choices=("gpu", "host"),
                    help="write the series station-major, their chunks deflated on the GPU (gpu) or by libhdf5 (host); default: the "
                         "transposed assignment")
    a = ap.parse_args(argv)
    tm, line = {}, {}
    t0 = time.perf_counter()
    cur = a.infill_tmin
    try:
        for var, src, dst in (("tmin", a.infill_tmin, a.serial_tmin), ("tmax", a.infill_tmax, a.serial_tmax)):
            cur = src
            ncio.file_format(src)
            with contextlib.redirect_stdout(sys.stderr):             # the reference's warnings: not on the JSON line's stream
                rec = create_serially_complete_db(src, var, dst, device=a.device, format=a.format, timing=tm, deflate=a.deflate)
            cur = dst
            stnda = StationSerialDataDb(dst, var, mode="r+")
            try:
                norm, nmths = add_monthly_normals(stnda, a.start_norm_yr, a.end_norm_yr, device=a.device, timing=tm)
            finally:
                stnda.close()
            line[var] = {"stations": int(rec.all_infill.size), "days": int(stnda.days.size),
                         "all_infill": int(rec.all_infill.sum()), "with_missing": int((rec.nmissing > 0).sum()),
                         "normals": int(np.isfinite(norm).sum()), "no_normal": int(np.isnan(norm).sum())}
    except (IOError, OSError, ValueError, KeyError) as e:
        print("step18: cannot open %s: %s" % (getattr(e, "filename", None) or cur, e), file=sys.stderr)
        return 1
    line["seconds"] = round(time.perf_counter() - t0, 3)
    for k in sorted(tm):
        line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
