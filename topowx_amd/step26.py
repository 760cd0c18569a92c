"""The reference's step26 (scripts/step26_mosaic_tiles.py): the tile files of step25 mosaicked into the normals files and the
yearly daily files of the product, and -- with ``--out-monthly`` -- step27's monthly files in the same pass.

    python -m topowx_amd.step26 --mask mask.nc --tiles DIR --out-normals DIR --out-daily DIR --start-year Y --end-year Y
                                --version S [--out-monthly DIR] [--vars tmin tmax] [--tile 250] [--chunk 50]
                                [--deflate gpu|host] [--batch-days N] [--format NETCDF4|NETCDF3_64BIT] [--device N]

Tile names are the folders ``h[0-9][0-9]v[0-9][0-9]`` under ``--tiles``.  Writes ``<out-normals>/normals_<var>.nc``, then
``<out-daily>/<var>/<var>_<year>.nc`` (and ``<out-monthly>/<var>/<var>_<year>.nc``).

``--deflate gpu``: a year of the mosaic is assembled in device memory, its ``(1, 325, 700)`` chunks are deflated there and
appended to the file as they are (``TileMosaic.create_dly_ann_mosaics(..., deflate="gpu")``); ``host``: libhdf5 deflates them
on this core.  The default is ``gpu`` when libtwxqa loads and a device is present, ``host`` otherwise; the command prints which
one runs.  The normals mosaics (24 layers per variable) are always deflated on the host.  Tile files whose daily variable is
itself deflated (``driver --deflate``) are read through libhdf5, which inflates them on one core: slow.

Prints one JSON line per (variable, year) with the seconds of read, upload + place, deflate (kernels + download), write and
the device's kernel times by group.  Exits with 1 and a message that names the offending thing when the years, the tile
directory or a tile file cannot be used.
"""
import argparse
import fnmatch
import json
import os
import sys
import time

from . import _lib, _qalib

__all__ = ["main", "pick_deflate", "tile_names"]

FORMATS = ("NETCDF4", "NETCDF3_64BIT")


def pick_deflate(asked, device=0):
    """'gpu' or 'host' for ``--deflate``: what was asked for, else 'gpu' when the library loads and a device is present."""
    if asked is not None:
        return asked
    try:
        _qalib.load()
        _lib.Context(device).close()
        return "gpu"
    except (_lib.TwxError, _qalib.QaError, OSError):
        return "host"


def tile_names(path_tiles):
    if not os.path.isdir(path_tiles):
        raise IOError("--tiles %s is not a directory" % path_tiles)
    names = sorted(fnmatch.filter(os.listdir(path_tiles), "h[0-9][0-9]v[0-9][0-9]"))
    if not names:
        raise IOError("--tiles %s holds no tile folder h[0-9][0-9]v[0-9][0-9]" % path_tiles)
    return names


def check_years(start, end):
    if start > end:
        raise ValueError("--start-year %d is after --end-year %d" % (start, end))


def report(step, var, timings):
    for t in timings:
        line = {"step": step, "var": var}
        line.update({k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()})
        print(json.dumps(line), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step26", description=__doc__.split("\n\n")[0])
    ap.add_argument("--mask", required=True, help="the mask raster the tile grid was cut from")
    ap.add_argument("--tiles", required=True, help="directory of the tile folders hXXvYY written by step25")
    ap.add_argument("--out-normals", required=True)
    ap.add_argument("--out-daily", required=True)
    ap.add_argument("--out-monthly", help="also write step27's monthly files here")
    ap.add_argument("--start-year", type=int, required=True)
    ap.add_argument("--end-year", type=int, required=True)
    ap.add_argument("--version", required=True, help="dataset version string of the files' history attribute")
    ap.add_argument("--vars", nargs="+", default=["tmin", "tmax"], choices=["tmin", "tmax"])
    ap.add_argument("--tile", type=int, default=250, help="tile edge in cells (step26:30)")
    ap.add_argument("--chunk", type=int, default=50, help="chunk edge of the tile files in cells")
    ap.add_argument("--deflate", choices=["gpu", "host"], help="where the daily and monthly chunks are deflated")
    ap.add_argument("--batch-days", type=int, help="days of a year resident on the device at a time (default: as many as fit)")
    ap.add_argument("--format", choices=FORMATS, help="container of the mosaics (default: NETCDF4 when libhdf5 loads)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from . import ncio
    from .interp import TileMosaic
    try:
        check_years(a.start_year, a.end_year)
        deflate = pick_deflate(a.deflate, a.device)
        fmt = a.format or ncio.default_format()
        if deflate == "gpu" and fmt != "NETCDF4":
            raise ValueError("--deflate gpu appends HDF5 chunks: the mosaics must be NETCDF4, a %s file has no chunks "
                             "(use --deflate host)" % fmt)
        names = tile_names(a.tiles)
        print("step26: %d tiles, chunks deflated on the %s" % (len(names), deflate), flush=True)
        mtwx = TileMosaic(a.mask, a.tile, a.tile, a.chunk, a.chunk, device=a.device)
        os.makedirs(a.out_normals, exist_ok=True)
        for var in a.vars:
            t0 = time.perf_counter()
            fp = os.path.join(a.out_normals, "normals_%s.nc" % var)
            mtwx.create_normals_mosaic(names, var, a.tiles, fp, a.version, format=fmt)
            print(json.dumps({"step": "step26", "var": var, "normals": fp, "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
        for var in a.vars:
            timings = []
            t0 = time.perf_counter()
            paths = mtwx.create_dly_ann_mosaics(names, var, a.tiles, os.path.join(a.out_daily, var), a.start_year, a.end_year, a.version,
                                                chunk_cache_size=250000000, format=fmt, deflate=deflate, batch_days=a.batch_days,
                                                path_out_mthly=os.path.join(a.out_monthly, var) if a.out_monthly else None,
                                                timings=timings)
            report("step26", var, timings)
            print(json.dumps({"step": "step26", "var": var, "files": len(paths), "deflate": deflate,
                              "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    except (IOError, OSError, ValueError, KeyError, _lib.TwxError, _qalib.QaError) as e:
        print("step26: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
