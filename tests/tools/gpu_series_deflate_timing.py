#!/usr/bin/env python3
"""Time the series coder (topowx_amd/series_deflate.py, twxsd_deflate) on the GPU and write profiles/series_deflate_timing.json.

    python tests/tools/gpu_series_deflate_timing.py [--rows 12000] [--repeats 5] [--gpu-stations 2000] [--host-stations 200]
                                                    [--out profiles/series_deflate_timing.json]

One run.  ``--rows`` x 25 203 float32 rows -- the 16 rows of the seeded "observations in tenths" pool of
tests/series_deflate_cases.py, tiled -- go through ONE ``twxsd_deflate`` call from page-locked memory into page-locked
memory, ``--repeats`` times after a warm-up: the medians of upload, every kernel group, download and the whole call, the
packed size, the rate of the two passes (count + emit) against a device-to-device copy measured in the same run, and the
stage that limits the call.  Beside that, step18's write (``tmin`` f4 and ``flag_infilled`` i1 of a serial database through
``ncio.write_series_chunks``, file creation aside, flush included) with ``deflate="gpu"`` over ``--gpu-stations`` stations and
with ``deflate="host"`` over ``--host-stations`` stations, both SCALED to ``--rows`` stations by the station count; the file
says so.  No threshold is set anywhere."""
import argparse
import datetime as dt
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NDAYS = 25203


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=12000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gpu-stations", type=int, default=2000)
    ap.add_argument("--host-stations", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_deflate_timing.json"))
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    import series_deflate_cases as SC
    from topowx_amd import _qalib, ncio, series_deflate as SD
    from topowx_amd.dates import get_days_metadata
    from topowx_amd.infill.post_infill import SERIAL_DB_VARIABLES
    if not torch.cuda.is_available():
        print("gpu_series_deflate_timing: no GPU", file=sys.stderr)
        return 1
    pool = SC.pool("tenths")
    nbytes = a.rows * NDAYS * 4
    src, dst = _qalib.PinnedBuffer(nbytes), _qalib.PinnedBuffer(nbytes // 2)
    try:
        rows = np.frombuffer(src.view, np.float32).reshape(a.rows, NDAYS)
        for i in range(0, a.rows, pool.shape[0]):
            rows[i:i + pool.shape[0]] = pool[:min(pool.shape[0], a.rows - i)]
        runs = []
        for k in range(a.repeats + 1):
            t, t0 = {}, time.perf_counter()
            _, off, counts = SD.deflate_rows(rows, out=dst.view, timing=t)
            t["call_ms"] = (time.perf_counter() - t0) * 1e3
            if k:                                                    # (the first call is the warm-up)
                runs.append(t)
        med = {k: float(np.median([r[k] for r in runs])) for k in runs[0] if k.endswith("_ms")}
        packed = int(off[-1])
        # a device-to-device copy of the same bytes, this run
        dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dev2 = torch.empty_like(dev)
        cp = []
        for _ in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dev2.copy_(dev)
            e1.record()
            torch.cuda.synchronize()
            cp.append(e0.elapsed_time(e1))
        copy_ms = float(np.median(cp[1:]))
        del dev, dev2
        passes_ms = med["sd_count_kernel_ms"] + med["sd_emit_kernel_ms"]
        kernels_ms = sum(med[k + "_kernel_ms"] for k in SD.SD_KERNELS)
        stages = {"upload": med["sd_upload_ms"], "kernels": kernels_ms, "download": med["sd_download_ms"]}
        # step18's write, both routes
        days = get_days_metadata(dt.date(1948, 1, 1), dt.date(2016, 12, 31))
        assert days.size == NDAYS
        write = {}
        with tempfile.TemporaryDirectory() as tmp:
            for route, nstn in (("gpu", min(a.gpu_stations, a.rows)), ("host", min(a.host_stations, a.rows))):
                stns = np.zeros(nstn, dtype=[("station_id", "U16"), ("longitude", "f8"), ("latitude", "f8"), ("elevation", "f8")])
                stns["station_id"] = ["S%05d" % i for i in range(nstn)]
                path = os.path.join(tmp, "serial_%s.nc" % route)
                ncio.create_quick_db(path, stns, days, SERIAL_DB_VARIABLES["tmin"])
                flag = np.ascontiguousarray((rows[:nstn] == SC.MISSING).astype(np.int8))
                sub = np.ascontiguousarray(rows[:nstn])
                ds = ncio.open_dataset(path, "a")
                t0 = time.perf_counter()
                ncio.write_series_chunks(ds.variables["tmin"], sub, deflate=route)
                ncio.write_series_chunks(ds.variables["flag_infilled"], flag, deflate=route)
                ds.close()
                sec = time.perf_counter() - t0
                write[route] = {"stations_measured": nstn, "seconds_measured": round(sec, 4), "file_bytes": os.path.getsize(path),
                                "seconds_scaled_to_rows": round(sec * a.rows / nstn, 3)}
        out = {"tool": "gpu_series_deflate_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
               "rows": a.rows, "ndays": NDAYS, "element_bytes": 4, "input_bytes": nbytes, "packed_bytes": packed,
               "packed_share_of_input": round(packed / nbytes, 4), "repeats": a.repeats,
               "note": "medians of %d calls after a warm-up, one run; rows and streams in page-locked memory; the pool's 16 rows "
                       "tiled, so every 16th stream is the same; step18_write is measured on stations_measured stations per route "
                       "and SCALED to %d stations by the station count" % (a.repeats, a.rows),
               "median_ms": {k: round(v, 3) for k, v in sorted(med.items())},
               "counts": {k: int(v) for k, v in zip(SD.SD_COUNTS, counts)},
               "kernels_ms": round(kernels_ms, 3), "two_passes_ms": round(passes_ms, 3),
               "two_passes_input_bytes_per_s": round(2 * nbytes / (passes_ms * 1e-3), 0),
               "copy_ms_measured": round(copy_ms, 3), "copy_rate_measured_bytes_per_s": round(2 * nbytes / (copy_ms * 1e-3), 0),
               "two_passes_share_of_measured_copy_rate": round((2 * nbytes / passes_ms) / (2 * nbytes / copy_ms), 4),
               "input_bytes_per_s_whole_call": round(nbytes / (med["call_ms"] * 1e-3), 0),
               "limiting_stage": max(stages, key=stages.get), "stage_ms": {k: round(v, 3) for k, v in stages.items()},
               "step18_write": write,
               "step18_write_host_over_gpu": round(write["host"]["seconds_scaled_to_rows"] / write["gpu"]["seconds_scaled_to_rows"], 2)}
    finally:
        rows = sub = None                                            # (views of the page-locked memory)
        src.close()
        dst.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
