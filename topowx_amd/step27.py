"""The reference's step27 (scripts/step27_create_monthly.py): the monthly files of daily mosaics that already exist.

    python -m topowx_amd.step27 --daily DIR --out DIR --start-year Y --end-year Y --version S [--vars tmin tmax]
                                [--deflate gpu|host] [--format NETCDF4|NETCDF3_64BIT] [--device N]

Reads ``<daily>/<var>/<var>_<year>.nc`` and writes ``<out>/<var>/<var>_<year>.nc`` (``write_ds_mthly``).  The monthly means
are formed on the GPU either way.  ``--deflate gpu``: each daily file is read through libhdf5 in bands of chunk rows, the
twelve layers are deflated on the device and appended to the file as they are; ``host``: libhdf5 deflates them.  The default
is ``gpu`` when libtwxqa loads and a device is present, ``host`` otherwise; the command prints which one runs.  (step26 with
``--out-monthly`` writes the same files from the year it holds on the device, without reading the daily files back.)

Prints one JSON line per (variable, year).  Exits with 1 and a message that names the offending thing.
"""
import argparse
import json
import os
import sys
import time

from . import _lib, _qalib
from .step26 import FORMATS, check_years, pick_deflate

__all__ = ["main"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step27", description=__doc__.split("\n\n")[0])
    ap.add_argument("--daily", required=True, help="directory of the daily mosaics: <daily>/<var>/<var>_<year>.nc")
    ap.add_argument("--out", required=True)
    ap.add_argument("--start-year", type=int, required=True)
    ap.add_argument("--end-year", type=int, required=True)
    ap.add_argument("--version", required=True)
    ap.add_argument("--vars", nargs="+", default=["tmin", "tmax"], choices=["tmin", "tmax"])
    ap.add_argument("--deflate", choices=["gpu", "host"], help="where the monthly chunks are deflated")
    ap.add_argument("--format", choices=FORMATS, help="container of the monthly files (default: NETCDF4 when libhdf5 loads)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from . import ncio
    from .interp.aggregate import write_ds_mthly, write_ds_mthly_gpu
    try:
        check_years(a.start_year, a.end_year)
        deflate = pick_deflate(a.deflate, a.device)
        fmt = a.format or ncio.default_format()
        if deflate == "gpu" and fmt != "NETCDF4":
            raise ValueError("--deflate gpu appends HDF5 chunks: the monthly files must be NETCDF4, a %s file has no chunks "
                             "(use --deflate host)" % fmt)
        print("step27: chunks deflated on the %s" % deflate, flush=True)
        for var in a.vars:
            os.makedirs(os.path.join(a.out, var), exist_ok=True)
            for yr in range(a.start_year, a.end_year + 1):
                fp_in = os.path.join(a.daily, var, "%s_%d.nc" % (var, yr))
                if not os.path.exists(fp_in):
                    raise IOError("no daily mosaic %s" % fp_in)
                fp_out = os.path.join(a.out, var, "%s_%d.nc" % (var, yr))
                t0 = time.perf_counter()
                line = {"step": "step27", "var": var, "year": yr, "deflate": deflate}
                with ncio.open_dataset(fp_in) as ds:
                    if deflate == "gpu":
                        timings = []
                        write_ds_mthly_gpu(ds, fp_out, var, yr, a.version, format=fmt, device=a.device, timings=timings)
                        line.update({k: (round(v, 4) if isinstance(v, float) else v) for k, v in timings[0].items()})
                    else:
                        write_ds_mthly(ds, fp_out, var, yr, a.version, format=fmt, device=a.device)
                line["seconds"] = round(time.perf_counter() - t0, 3)
                print(json.dumps(line), flush=True)
    except (IOError, OSError, ValueError, KeyError, _lib.TwxError, _qalib.QaError) as e:
        print("step27: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
