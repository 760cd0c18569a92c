#!/usr/bin/env python3
"""Timing of step12's reanalysis subsets on generated raw ``hgt`` files at the real shape; not a test.

    python tests/tools/gpu_nnrsub_timing.py [--years 4] [--repeats 5] [--out profiles/nnrsub_timing.json]

The input: ``hgt.<year>.nc`` for ``--years`` years from 2000, 17 levels x 73 x 144, four records a day, packed int16
(scale 1, offset 32066, missing_value 32766), classic container, written by this tool; the count of years and the bytes
are stated in the output.  The files are read once before anything is timed (page cache warm: a memory rate, not a disk
rate).  All six hgt products of step12 (thickness 500 - 1000 and hgt at 500 / 700 hPa, at 12z, 18z, 24z) are written as
NetCDF-4.  After one warm-up call, medians of ``--repeats`` calls of ``reanalysis.create_nnr_subsets``, by stage: reading
(the years on threads into the page-locked buffer), upload, the subset kernels, download (HIP events inside the library
call), and writing the six files.  The kernels' bytes moved (values gathered plus bytes stored) per second are set against
the float4 copy rate measured on this part, 6.29 TB/s.

The baseline is ``restate_nnrsub.reference_way``: the reference's schedule -- a pass of its own over the yearly files for
every product, six in all -- in numpy, on the same machine and the same files, median of ``--baseline-repeats`` runs
after one warm-up.  It is never the code under test.  The executed reference itself cannot be timed: its container
library (netCDF4-python) is not installed here.  The one condition recorded: the one-read GPU route takes no longer end
to end than the six-pass numpy route.
"""
import argparse
import datetime as dt
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_RATE = 6.29e12                      # bytes/s, the float4 copy of DESIGN section 21
LEVELS = np.array([1000, 925, 850, 700, 600, 500, 400, 300, 250, 200, 150, 100, 70, 50, 30, 20, 10], np.float32)


def write_year(path, year, rng):
    from topowx_amd import ncio
    nrec = (dt.date(year + 1, 1, 1) - dt.date(year, 1, 1)).days * 4
    ds = ncio.open_dataset(path, "w", "NETCDF3_64BIT")
    try:
        for name, vals in (("lon", np.arange(0, 360, 2.5)), ("lat", np.arange(90, -90.1, -2.5)), ("level", LEVELS)):
            ds.createDimension(name, len(vals))
            ds.createVariable(name, "f4", (name,))[:] = vals.astype(np.float32)
        ds.createDimension("time", nrec)
        tv = ds.createVariable("time", "f8", ("time",))
        tv.units = "hours since 1800-01-01 00:00:0.0"
        tv[:] = (dt.datetime(year, 1, 1) - dt.datetime(1800, 1, 1)).days * 24 + 6.0 * np.arange(nrec)
        v = ds.createVariable("hgt", "i2", ("time", "level", "lat", "lon"))
        v.scale_factor, v.add_offset, v.missing_value = np.float32(1), np.float32(32066), np.int16(32766)
        a = rng.integers(-32000, 32001, (nrec, 17, 73, 144), dtype=np.int16)
        a[rng.integers(0, nrec, 2000), rng.integers(0, 17, 2000), rng.integers(12, 33, 2000), rng.integers(90, 123, 2000)] = 32766
        v[:] = a
    finally:
        ds.close()
    return os.path.getsize(path)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--years", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnrsub_timing.json"))
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    import restate_nnrsub as RN
    from topowx_amd import ncio, reanalysis, step12
    from topowx_amd.dates import YEAR, get_days_metadata

    products = dict(step12.PRODUCTS)["hgt"]
    yrs = list(range(2000, 2000 + a.years))
    days = get_days_metadata(dt.date(yrs[0], 1, 1), dt.date(yrs[-1], 12, 31))
    assert list(np.unique(days[YEAR])) == yrs
    tmp = tempfile.mkdtemp(prefix="nnrsub_timing_")
    try:
        raw_dir, out_gpu, out_base = (os.path.join(tmp, d) for d in ("raw", "gpu", "base"))
        for d in (raw_dir, out_gpu, out_base):
            os.mkdir(d)
        rng = np.random.default_rng(7)
        raw_bytes = 0
        for y in yrs:
            raw_bytes += write_year(os.path.join(raw_dir, "hgt.%d.nc" % y), y, rng)
            print("wrote hgt.%d.nc" % y, file=sys.stderr, flush=True)
        for y in yrs:                                                # page cache warm
            with open(os.path.join(raw_dir, "hgt.%d.nc" % y), "rb") as fh:
                while fh.read(1 << 26):
                    pass
        rec = []
        for rep in range(a.repeats + 1):
            tm = {}
            t0 = time.perf_counter()
            reanalysis.create_nnr_subsets(raw_dir, out_gpu, yrs, days, "hgt", products, format="NETCDF4", timing=tm)
            total = time.perf_counter() - t0
            print("one-read route %.0f ms" % (total * 1e3), file=sys.stderr, flush=True)
            if rep:
                rec.append({"total_ms": total * 1e3, "read_ms": tm["nsub_read_s"] * 1e3, "library_call_ms": tm["nsub_library_s"] * 1e3,
                            "upload_ms": tm["nsub_upload_ms"], "kernels_ms": tm["nsub_kernels_ms"],
                            "download_ms": tm["nsub_download_ms"], "write_ms": tm["nsub_write_s"] * 1e3})
        med = {k: round(float(np.median([r[k] for r in rec])), 3) for k in rec[0]}
        base = []
        for rep in range(a.baseline_repeats + 1):
            t0 = time.perf_counter()
            for p in products:                                       # a pass over the yearly files per product
                RN.reference_way(raw_dir, out_base, yrs, days, "hgt", [p], format="NETCDF4")
            print("six-pass route %.0f ms" % ((time.perf_counter() - t0) * 1e3), file=sys.stderr, flush=True)
            if rep:
                base.append((time.perf_counter() - t0) * 1e3)
        base_ms = round(float(np.median(base)), 3)
        # the two routes wrote the same arrays
        out_bytes = gathered = 0
        for p in products:
            with ncio.open_dataset(os.path.join(out_gpu, p["fname"])) as d1, ncio.open_dataset(os.path.join(out_base, p["fname"])) as d2:
                x, y = np.asarray(d1.variables[p["varname_out"]][:]), np.asarray(d2.variables[p["varname_out"]][:])
                assert x.tobytes() == y.tobytes(), p["fname"]
                nlat, nlon = x.shape[-2:]
                nlev = x.shape[1] if x.ndim == 4 else 1
                out_bytes += days.size * nlev * ((nlat + 3) // 4) * ((nlon + 3) // 4) * 64
                gathered += int((tm["nsub_counts"][p["fname"]][0]) * nlev * nlat * nlon * 2 * (2 if p.get("thick") else 1))
        moved = out_bytes + gathered
        stages = {k[:-3]: med[k] for k in ("read_ms", "upload_ms", "kernels_ms", "download_ms", "write_ms")}
        out = {"tool": "gpu_nnrsub_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
               "raw_variable": "hgt", "years": a.years, "first_year": yrs[0], "raw_shape_per_record": [17, 73, 144],
               "records": int(sum((dt.date(y + 1, 1, 1) - dt.date(y, 1, 1)).days * 4 for y in yrs)), "raw_bytes": int(raw_bytes),
               "raw_container": "NETCDF3_64BIT", "raw_dtype": "int16", "days": int(days.size), "products": [p["fname"] for p in products],
               "subset_grid": [int(nlat), int(nlon)], "output_format": "NETCDF4", "repeats": a.repeats,
               "baseline_repeats": a.baseline_repeats,
               "note": "one run on one machine; medians of the repeats after one warm-up call; raw files read from a warm page "
                       "cache; upload, kernels and download are HIP-event times inside the one library call "
                       "(library_call_ms is its wall time, allocation included); the baseline is the six-pass numpy route of "
                       "tests/restate_nnrsub.py on the same files, not the executed reference (its container library is "
                       "not installed)",
               "median_ms": med, "stage_ms": {k: round(v, 2) for k, v in stages.items()},
               "limiting_stage": max(stages, key=stages.get),
               "kernel_bytes_stored": int(out_bytes), "kernel_bytes_gathered": int(gathered),
               "kernel_bytes_per_s": round(moved / (med["kernels_ms"] * 1e-3), 0),
               "copy_rate_bytes_per_s": COPY_RATE,
               "kernel_share_of_copy_rate": round(moved / (med["kernels_ms"] * 1e-3) / COPY_RATE, 5),
               "gpu_route_end_to_end_ms": med["total_ms"], "six_pass_numpy_route_ms": base_ms,
               "gpu_route_no_slower_than_six_pass": bool(med["total_ms"] <= base_ms)}
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
