"""The reference's step13 (scripts/step13_add_utc_offset.py; ``add_utc_offset``, create_db_all_stations.py:1333-1383): the
station variable ``utc_offset`` (i2) that ``--nnr-dir`` of step14, step15 and step16 reads, from a point-in-polygon lookup
of time-zone polygons in one call of libtwxqa's ``twxtz_locate`` (``utc_offsets.add_utc_offset``).

    python -m topowx_amd.step13 --db all.nc --tz-polygons FILE [--max-force-deg X] [--no-holes] [--dry-run]
                                [--report out.npz] [--device N]

``--tz-polygons``: a GeoJSON FeatureCollection, tzwhere's ``tz_world.json`` or timezone-boundary-builder's
``combined.json``; nothing is downloaded.  ``--max-force-deg`` (default 1.0; a negative number: no limit): how far the
nearest polygon of a station that no polygon contains may lie.  ``--no-holes`` drops interior rings.  ``--dry-run`` looks
up and reports but leaves the database as it is.

Prints the reference's line for every station without an offset, then one JSON line (stations, inside / forced / none,
pairs, items settled on the host, the phases' milliseconds).  Exits with 1 if the database or the polygon file cannot be
read.
"""
import argparse
import json
import sys
import time

import numpy as np

from . import _qalib
from .utc_offsets import add_utc_offset

__all__ = ["main"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m topowx_amd.step13", description=__doc__.split("\n\n")[0])
    ap.add_argument("--db", required=True, help="the station database (NetCDF-4 or classic), changed in place")
    ap.add_argument("--tz-polygons", required=True, help="GeoJSON FeatureCollection of time-zone polygons")
    ap.add_argument("--max-force-deg", type=float, default=1.0, help="reach of the nearest-polygon search in degrees (< 0: no limit)")
    ap.add_argument("--no-holes", action="store_true", help="ignore interior rings")
    ap.add_argument("--dry-run", action="store_true", help="look up and report, write nothing")
    ap.add_argument("--report", help="write the per-station results to this .npz")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    t0 = time.perf_counter()
    try:
        rep = add_utc_offset(a.db, a.tz_polygons, max_force_deg=None if a.max_force_deg < 0 else a.max_force_deg,
                             holes=not a.no_holes, device=a.device, dry_run=a.dry_run)
    except (IOError, OSError, ValueError, KeyError, _qalib.QaError) as e:
        print("step13: %s" % e, file=sys.stderr)
        return 1
    arrays = {k: v for k, v in rep.items() if isinstance(v, np.ndarray)}
    if a.report:
        np.savez(a.report, **arrays)
    line = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rep.items() if k not in arrays}
    line["seconds"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
