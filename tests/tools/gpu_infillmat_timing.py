#!/usr/bin/env python3
"""Time the infill neighbour matrices (``topowx_amd.infill.build_infill_matrices``, twelve calendar-month groups) once on
two synthetic pools at the station density of a 12 000-station CONUS database (about 26 stations within 75 km):

    small   2 000 stations x 10 years, every station a target
    full    12 000 stations x 69 years (1948-2016), 2 000 targets

Per case: the HIP-event milliseconds of each kernel group summed over the rounds, the number of rounds, the seconds of
the first call (module load, first launches) and of a second, warm call, and the host share of the warm call (what is
not kernel time), and the parts of the warm call on the host clock: the transposed copy of the observations, the
thresholds, the library call and, inside it, the allocations and copies to the device and the copies back.  Writes one
JSON document with the device name as the runtime reports it.

    python tests/tools/gpu_infillmat_timing.py --out profiles/infill_matrix_timing.json [--cases small,full]
"""
import argparse
import datetime as dt
import json
import os
import sys
import time

import torch  # noqa: F401  -- first: its bundled HIP runtime must be the one the process loads

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from topowx_amd.dates import get_days_metadata  # noqa: E402
from topowx_amd.infill import build_infill_matrices  # noqa: E402
from topowx_amd.qa import StationObsPool  # noqa: E402

CASES = {"small": (2000, dt.date(2001, 1, 1), dt.date(2010, 12, 31), None),
         "full": (12000, dt.date(1948, 1, 1), dt.date(2016, 12, 31), 2000)}
KM2_PER_STATION = 58.0 * 25.0 * 111.0 * 85.0 / 12000.0            # the C3-sized box shared among 12 000 stations


def make_pool(n, first, last, seed=5):
    rng = np.random.default_rng(seed)
    days = get_days_metadata(first, last)
    nd = days.size
    side_km = np.sqrt(n * KM2_PER_STATION)
    lon = -100.0 + (rng.random(n) - 0.5) * side_km / 85.0
    lat = 40.0 + (rng.random(n) - 0.5) * side_km / 111.0
    t = np.arange(nd)
    reg, e = np.zeros(nd), rng.standard_normal(nd) * 3.0
    for i in range(1, nd):
        reg[i] = 0.7 * reg[i - 1] + e[i]
    base = (-12.0 * np.cos(2 * np.pi * (t - 15) / 365.25) + reg).astype(np.float32)
    tmin = np.empty((nd, n), np.float32)
    for a in range(0, n, 500):                                     # by blocks of stations: the whole array is 1.2 GB
        b = min(n, a + 500)
        blk = base[:, None] + rng.standard_normal((nd, b - a), dtype=np.float32) * 1.5 + \
            (rng.standard_normal(b - a) * 2.0).astype(np.float32)[None, :]
        blk = np.round(blk, 1)
        blk[rng.random((nd, b - a), dtype=np.float32) < 0.06] = np.nan
        for s in range(0, b - a, 4):                               # a quarter of the stations: a partial record
            k = int(rng.integers(0, nd))
            blk[k:k + int(rng.integers(nd // 10, nd // 2)), s] = np.nan
        tmin[:, a:b] = blk
    ids = np.array(["T%06d" % i for i in range(n)])
    return StationObsPool(ids, lon, lat, tmin, tmin, days)


def run_case(name, device):
    n, first, last, ntarget = CASES[name]
    t0 = time.perf_counter()
    pool = make_pool(n, first, last)
    targets = None if ntarget is None else pool.ids[np.sort(np.random.default_rng(9).choice(n, ntarget, replace=False))]
    t1 = time.perf_counter()
    build_infill_matrices(pool, "tmin", targets, device=device)
    t2 = time.perf_counter()
    tm = {}
    m = build_infill_matrices(pool, "tmin", targets, device=device, timing=tm)
    t3 = time.perf_counter()
    kernel_s = sum(v for k, v in tm.items() if k.endswith("_kernel_ms")) / 1000.0
    status, count = np.unique(m.status, return_counts=True)
    return dict(case=name, stations=n, days=int(pool.days.size), targets=int(m.target_ids.size), items=int(m.status.size),
                status={str(int(s)): int(c) for s, c in zip(status, count)}, ranked=int(m.idx.size), kept=int(m.keep.sum()),
                nnghs_max=int(m.nnghs.max()), max_dist_max=float(np.nanmax(m.max_dist)), rounds=int(tm["rounds"]),
                kernel_ms={k[:-10]: round(v, 3) for k, v in tm.items() if k.endswith("_kernel_ms")},
                make_pool_s=round(t1 - t0, 3), first_call_s=round(t2 - t1, 3), warm_call_s=round(t3 - t2, 3),
                warm_call_parts_s=dict(transpose=round(tm["transpose_s"], 4), thresholds=round(tm["thresholds_s"], 4),
                                       library=round(tm["library_s"], 4), upload=round(tm["upload_ms"] / 1000.0, 4),
                                       download=round(tm["download_ms"] / 1000.0, 4)),
                obs_layout="%s-contiguous [ndays, n]" % ("C" if pool.tmin.flags.c_contiguous else "F"),
                obs_bytes=int(pool.tmin.nbytes),
                host_share=round(1.0 - kernel_s / (t3 - t2), 4), items_per_second=round(m.status.size / (t3 - t2), 1))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default="small,full")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    doc = dict(tool="gpu_infillmat_timing", device_name=torch.cuda.get_device_name(a.device), cases=[])
    for name in a.cases.split(","):
        doc["cases"].append(run_case(name, a.device))
        print(json.dumps(doc["cases"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
