"""Timing of step19 and of the front of step20 on an MI355X: ``twxrv_sample`` and
``twxrv_nearest_data`` at 12 000 stations x 28 rasters of 3250 x 7000, ``twxrv_dup_classes`` on 12 000 stations and
``twxrv_col_count`` on 25 203 x 12 000 in both instances.  Synthetic inputs; one warm-up call, then the median of five calls,
HIP-event kernel milliseconds and host-clock milliseconds of the copies apart.  The baseline, in the same run, is the
per-station host route the reference takes (tests/restate_stnrast.py, one station at a time) on a stated subset.

    python tests/tools/stnrast_timing.py [--out profiles/stnrast_timing.json] [--small]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  -- first: its HIP runtime serves the process (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_stnrast as RR  # noqa: E402
from topowx_amd import _qalib  # noqa: E402

REPEATS = 5


def med(rows):
    keys = rows[0].keys()
    return {k: round(float(np.median([r[k] for r in rows])), 3) for k in keys}


def timed(fn):
    """One warm-up, then REPEATS calls: the medians of the timing dict's entries and of the host milliseconds of a call."""
    fn({})
    rows = []
    for _ in range(REPEATS):
        t = {}
        t0 = time.perf_counter()
        fn(t)
        t["host_ms"] = (time.perf_counter() - t0) * 1e3
        rows.append({k: v for k, v in t.items() if k.endswith("_ms")})
    return med(rows)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="a tenth of the workload (a check of the tool, not a measurement)")
    a = ap.parse_args(argv)
    rows, cols, nstn, ndays, nrast = (325, 700, 1200, 2520, 3) if a.small else (3250, 7000, 12000, 25203, 28)
    rs = np.random.RandomState(24)
    geo_t = (-125.0, 1.0 / 120 * (10 if a.small else 1), 0.0, 52.0, 0.0, -1.0 / 120 * (10 if a.small else 1))
    out = {"tool": "stnrast_timing", "device_name": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "repeats": REPEATS, "stations": nstn, "raster": [rows, cols], "rasters": nrast, "days": ndays, "cases": []}

    # ---- the rasters: a smooth field with a no-data coast band and scattered holes; float32, 91 MB each at full size ----
    yy = np.linspace(0, 1, rows, dtype=np.float32)[:, None]
    xx = np.linspace(0, 1, cols, dtype=np.float32)[None, :]
    base = (280 + 20 * yy - 10 * xx).astype(np.float32)
    base[:, :cols // 50] = -9999.0
    base[rs.randint(0, rows, 20000), rs.randint(0, cols, 20000)] = -9999.0
    rasters = [np.roll(base, 7 * k, axis=0) for k in range(min(nrast, 4))]      # four distinct arrays serve the 28 calls
    lon = rs.uniform(geo_t[0] - 0.05, geo_t[0] + cols * geo_t[1] + 0.05, nstn)
    lat = rs.uniform(geo_t[3] + rows * geo_t[5] - 0.05, geo_t[3] + 0.05, nstn)
    state = {}

    def sample_all(t):
        nforced = redecided = 0
        for k in range(nrast):
            r = _qalib.raster_sample(rasters[k % len(rasters)], geo_t, -9999.0, lon, lat, band_ndata=-9999.0, revert_nn=True,
                                     force_data_value=True, timing=t)
            f = np.nonzero(r["status"] == _qalib.RV_NEEDS_FORCE)[0]
            if f.size:
                nn = _qalib.raster_nearest_data(rasters[k % len(rasters)], geo_t, -9999.0, r["row"][f], r["col"][f], timing=t)
                redecided += nn["redecided"]
            nforced += f.size
        state.update(forced=nforced, redecided=redecided)

    m = timed(sample_all)
    case = {"case": "twxrv_sample + twxrv_nearest_data, %d rasters, LST options" % nrast, "median_ms": m,
            "forced_stations": state["forced"], "redecided_on_host": state["redecided"],
            "raster_bytes": int(rasters[0].nbytes), "upload_bytes_per_s": round(
                (nrast + (1 if state["forced"] else 0) * nrast) * rasters[0].nbytes / (m["rv_upload_ms"] * 1e-3))}
    # the baseline: the reference's route, one station at a time, on one raster and a subset of the stations
    nsub = min(nstn, 1000)
    g = RR.Grid(rasters[0], geo_t, -9999.0)
    t0 = time.perf_counter()
    RR.add_stn_raster_values(g, lon[:nsub], lat[:nsub], 1, True, True)
    sec = time.perf_counter() - t0
    case["baseline"] = {"what": "numpy restatement, one station at a time, 1 raster x %d stations" % nsub, "seconds": round(sec, 3),
                        "scaled_to_workload_seconds": round(sec * nrast * nstn / nsub, 1)}
    out["cases"].append(case)

    # ---- the duplicate search ----
    dlon, dlat = lon.copy(), lat.copy()
    k = rs.permutation(nstn)[:nstn // 50]
    dlon[k], dlat[k] = dlon[(k + 1) % nstn], dlat[(k + 1) % nstn]
    m = timed(lambda t: _qalib.dup_classes(dlon, dlat, timing=t))
    cls, size = _qalib.dup_classes(dlon, dlat)
    nsub = min(nstn, 500)
    t0 = time.perf_counter()
    for i in range(nsub):                                             # find_dup_stns' loop: one station against all others
        other = np.arange(nstn) != i
        (RR.grt_circle_dist(dlon[i], dlat[i], dlon[other], dlat[other]) == 0).any()
    sec = time.perf_counter() - t0
    out["cases"].append({"case": "twxrv_dup_classes", "median_ms": m, "stations_in_classes": int((size > 1).sum()),
                         "baseline": {"what": "grt_circle_dist of one station against all others, %d of %d stations" % (nsub, nstn),
                                      "seconds": round(sec, 3), "scaled_to_workload_seconds": round(sec * nstn / nsub, 1)}})

    # ---- the column counts ----
    flag = (rs.rand(ndays, nstn) < 0.3).astype(np.int8)
    members = np.nonzero(size > 1)[0].astype(np.int32)
    state = {}

    def count_flags(t):
        state["a"] = _qalib.col_count(flag, members, fill=-127, timing=t)

    m = timed(count_flags)
    t0 = time.perf_counter()
    want = flag[:, members].sum(axis=0)
    sec = time.perf_counter() - t0
    assert np.array_equal(state["a"], want)
    out["cases"].append({"case": "twxrv_col_count int8, %d listed columns" % members.size, "median_ms": m, "bytes": int(flag.nbytes),
                         "kernel_bytes_per_s": round(members.size * ndays / (m["rv_colcount_kernel_ms"] * 1e-3)),
                         "baseline": {"what": "numpy: flag[:, members].sum(axis=0)", "seconds": round(sec, 4)}})
    del flag
    x = np.random.default_rng(7).standard_normal((ndays, nstn), dtype=np.float32)
    x[rs.randint(0, ndays, 1000), rs.randint(0, nstn, 1000)] = np.float32(_qalib.SC_FILL_F4)
    good = np.nonzero(rs.rand(nstn) < 0.95)[0].astype(np.int32)

    def count_missing(t):
        state["b"] = _qalib.col_count(x, good, timing=t)

    m = timed(count_missing)
    t0 = time.perf_counter()
    sel = x[:, good]
    want = (~np.isfinite(sel) | (sel == np.float32(_qalib.SC_FILL_F4))).sum(axis=0)
    sec = time.perf_counter() - t0
    assert np.array_equal(state["b"], want)
    out["cases"].append({"case": "twxrv_col_count float32, %d good columns" % good.size, "median_ms": m, "bytes": int(x.nbytes),
                         "kernel_bytes_per_s": round(4.0 * good.size * ndays / (m["rv_colcount_kernel_ms"] * 1e-3)),
                         "baseline": {"what": "numpy: non-finite or fill over x[:, good]", "seconds": round(sec, 3)}})
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
