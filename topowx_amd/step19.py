"""``scripts/step19_add_raster_predictors.py``: the raster predictors at the stations of the two serially-complete databases
-- ``lst01 .. lst12`` (night-time LST for Tmin, day-time LST for Tmax), ``tdi``, ``mask`` and ``climdiv`` -- through
``topowx_amd.infill.add_stn_raster_values``: one ``twxrv_sample`` call per raster over all stations and one
``twxrv_nearest_data`` call over those that need a forced value, where the reference calls ``basemap.interp`` per station.

    python -m topowx_amd.step19 --serial-tmin F --serial-tmax F --rasters DIR [--dry-run] [--device N]

DIR holds the reference's file names: ``lst/LST_Night.MM.tif``, ``lst/LST_Day.MM.tif``, ``tdi.tif``, ``mask.tif``,
``climdiv.tif`` (``topowx_amd.raster.from_geotiff``); a ``.nc`` file of the same stem is accepted in a GeoTIFF's place.  The
options per raster are step19's: LST bilinear with ``revert_nn`` and ``force_data_value`` (every station gets a value);
TDI bilinear with ``revert_nn``; mask and climate division the nearest cell, the mask raster with ``ndata = 0``.

Prints one JSON line per variable and database (the counts of bilinear / nearest / forced / no-data stations, the forced
stations decided again on the host, seconds).  ``--dry-run`` writes nothing.  Exits with 1 if a file cannot be opened.
"""
import argparse
import json
import os
import sys
import time

from .infill import add_stn_raster_values
from .raster import open_raster
from .stationdb import CLIMDIV, MASK, TDI, StationSerialDataDb, get_lst_varname

__all__ = ["raster_jobs", "find_raster", "main"]


def find_raster(root, stem):
    """``root/stem.tif`` or, in its place, ``root/stem.nc``."""
    for ext in (".tif", ".nc"):
        p = os.path.join(root, stem + ext)
        if os.path.exists(p):
            return p
    raise IOError("no such raster: %s(.tif|.nc)" % os.path.join(root, stem))


def raster_jobs():
    """step19's calls in its order: (database, variable, long name, units, raster stem, ndata override, keywords)."""
    jobs = []
    lst = dict(revert_nn=True, force_data_value=True)
    for var, stem in (("tmin", "LST_Night"), ("tmax", "LST_Day")):
        for mth in range(1, 13):
            jobs.append((var, get_lst_varname(mth), "land skin temperature", "C", os.path.join("lst", "%s.%.2d" % (stem, mth)),
                         None, lst))
    for name, long_name, units, stem, ndata, kw in (
            (TDI, "topographic dissection index", "[3,6,9,12,15] km radius", "tdi", None, dict(revert_nn=True)),
            (MASK, "Interpolation Mask", "0 or 1", "mask", 0, dict(extract_method=0)),
            (CLIMDIV, "U.S. Climate Division", "", "climdiv", None, dict(extract_method=0))):
        for var in ("tmin", "tmax"):
            jobs.append((var, name, long_name, units, stem, ndata, kw))
    return jobs


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step19", description=__doc__.split("\n\n")[0])
    ap.add_argument("--serial-tmin", required=True, help="serially-complete Tmin station database (netCDF)")
    ap.add_argument("--serial-tmax", required=True, help="serially-complete Tmax station database (netCDF)")
    ap.add_argument("--rasters", required=True, help="directory of the predictor rasters")
    ap.add_argument("--dry-run", action="store_true", help="report the counts, write nothing")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    mode = "r" if a.dry_run else "r+"
    dbs, cur = {}, a.serial_tmin
    try:
        for var, path in (("tmin", a.serial_tmin), ("tmax", a.serial_tmax)):
            cur = path
            dbs[var] = StationSerialDataDb(path, var, mode=mode)
        last = (None, None)
        for var, name, long_name, units, stem, ndata, kw in raster_jobs():
            t0 = time.perf_counter()
            cur = os.path.join(a.rasters, stem)
            path = find_raster(a.rasters, stem)
            rast = last[1] if last[0] == path else open_raster(path)    # TDI, mask and climdiv serve both databases
            last = (path, rast)
            if ndata is not None:
                rast.ndata = ndata
            rep, tm = {}, {}
            left = add_stn_raster_values(dbs[var], name, long_name, units, rast, device=a.device, timing=tm, report=rep, **kw)
            line = {"db": var, "var": name, "raster": os.path.relpath(path, a.rasters), "rows": rast.rows, "cols": rast.cols}
            line.update(rep)
            line["left_at_ndata"] = int(left.size)
            line["seconds"] = round(time.perf_counter() - t0, 3)
            for k in sorted(tm):
                line[k] = round(tm[k], 3) if isinstance(tm[k], float) else tm[k]
            print(json.dumps(line), flush=True)
    except (IOError, OSError, ValueError, KeyError, NotImplementedError) as e:
        print("step19: cannot open %s: %s" % (getattr(e, "filename", None) or cur, e), file=sys.stderr)
        return 1
    finally:
        for da in dbs.values():
            da.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
