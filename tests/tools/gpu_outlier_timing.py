#!/usr/bin/env python3
"""Time step20's outlier screen once on a C3-shaped station database (12 000 stations over the CONUS-sized box of
synth config C3): ``XvalOutlier.find_xval_outliers()`` over every station, split into neighbour selection (twx_knn),
the WLS call of libtwxqa (and its kernel alone) and host time.  Prints one JSON line.

    python tests/tools/gpu_outlier_timing.py [--nstns 12000] [--nnghs 100]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from topowx_amd import stationdb as sdb, synth  # noqa: E402
from topowx_amd.interp.optimize import XvalOutlier  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstns", type=int, default=12000)
    ap.add_argument("--nnghs", type=int, default=100)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    nrows, ncols, lat_n, lon_w, _, seed = synth.CONFIGS["C3"]
    bbox = (lat_n - nrows * synth.CELL, lat_n, lon_w, lon_w + ncols * synth.CELL)
    db = synth.make_stations(bbox, a.nstns, seed, "tmin", expand_deg=0.0)
    for i in np.linspace(0, db.stns.size - 1, 8).astype(int):     # a few planted outliers
        db.stns[sdb.get_norm_varname(1 + i % 12)][i] += 12.0
    t0 = time.perf_counter()
    xo = XvalOutlier(db, device=a.device)
    t1 = time.perf_counter()
    xo.find_xval_outliers(None, a.nnghs)                           # warm-up (module load, first launches)
    t2 = time.perf_counter()
    out = xo.find_xval_outliers(None, a.nnghs)
    t3 = time.perf_counter()
    tm = dict(xo.last_timing)
    xo.close()
    rec = dict(tool="gpu_outlier_timing", stations=int(db.stns.size), nnghs=a.nnghs, fits=int(db.stns.size) * 13,
               outliers=int(out.size), setup_s=round(t1 - t0, 4), first_call_s=round(t2 - t1, 4),
               total_s=round(t3 - t2, 4), knn_s=round(tm["knn_s"], 4), wls_call_s=round(tm["wls_s"], 4),
               wls_kernel_ms=round(tm["wls_kernel_ms"], 3),
               host_s=round(t3 - t2 - tm["knn_s"] - tm["wls_s"], 4))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
