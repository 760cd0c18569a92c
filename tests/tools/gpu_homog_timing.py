"""Timing of the four ``twxhm_`` entries (step05, step09-11) on synthetic rows (needs an MI355X and a build):
``twxhm_obs_cnt``, ``twxhm_monthly_means``, ``twxhm_tobs_shift`` and ``twxhm_homog_daily`` at 12 000 stations x 25 203 days
(1948-2016, 828 months).

    python tests/tools/gpu_homog_timing.py [--out profiles/homog_timing.json] [--stations 12000] [--repeats 5] [--host-stations 240]

One warm-up call, then the MEDIAN of ``--repeats`` calls: HIP-event milliseconds per kernel, host-clock milliseconds of the
copies in and out and of the whole call, the bytes a kernel has to move (per day: counts 4 read; means 4 read, plus 6 per
month written; shift 8 read and 4 written; homogenisation 4 read and 4 written, its month table and deltas stay in L2) and
that rate as a share of the 6.29 TB/s a float4 copy reaches on the MI355X.  Next to each entry the host time of the numpy
restatement (tests/restate_homog.py) on the first ``--host-stations`` stations of the same arrays, on the same machine: the
restatement loops in Python over stations and months, so it is timed on a slice and the slice is named, not scaled up.
The rows are a block of 500 random series repeated: the kernels do not care, and the host stays out of the generator.
"""
import argparse
import datetime as dt
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_MEASURED_TBS = 6.29


def median_call(fn, repeats):
    fn({})                                                           # warm-up: code objects, allocator, page faults
    runs = []
    for _ in range(repeats):
        tm = {}
        t0 = time.perf_counter()
        fn(tm)
        tm["host_ms"] = (time.perf_counter() - t0) * 1e3
        runs.append(tm)
    return {k: round(float(np.median([r[k] for r in runs])), 3) for k in runs[0] if isinstance(runs[0][k], float)}, runs[0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homog_timing.json"))
    ap.add_argument("--stations", type=int, default=12000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-stations", type=int, default=240)
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    import restate_homog as RH
    from topowx_amd import _qalib
    from topowx_amd.dates import MONTH, YEAR, get_days_metadata
    days = get_days_metadata(dt.date(1948, 1, 1), dt.date(2016, 12, 31))
    nd = days.size
    mf, mn, mymd = _qalib.month_groups(days[YEAR], days[MONTH])
    nm = mf.size
    month = np.asarray(days[MONTH], np.int8)
    rs = np.random.RandomState(911)
    blk = 500
    doy = np.arange(nd) % 365.25
    base = np.round(5.0 - 12.0 * np.cos(2 * np.pi * doy / 365.25) + rs.randn(blk, nd) * 4, 1).astype(np.float32)
    base[rs.rand(blk, nd) < 0.1] = np.nan
    for s in range(0, blk, 5):                                       # a fifth of the stations have a gap of years
        a0 = int(rs.randint(nd - 4000))
        base[s, a0:a0 + 3650] = np.nan
    tobs_blk = np.where(rs.rand(blk, 1) < 0.5, 700.0, 1700.0).astype(np.float32) * np.ones((1, nd), np.float32)
    tobs_blk[rs.rand(blk, nd) < 0.02] = np.nan
    reps = -(-a.stations // blk)
    obs = np.ascontiguousarray(np.tile(base, (reps, 1))[:a.stations])
    tobs = np.ascontiguousarray(np.tile(tobs_blk, (reps, 1))[:a.stations])
    ns = obs.shape[0]
    mean, miss = _qalib.monthly_means(obs, mf, mn, 9)
    pha = np.where(np.isnan(mean), 500.0, np.rint(RH.round2(mean.astype(np.float64)) * 100.0)).astype(np.int32)
    pha[:, nm // 3: 2 * nm // 3] += 37                               # a third of the months homogenised by +0.37
    pha[rs.rand(ns, nm) < 0.02] = _qalib.HM_PHA_MISSING
    cut = int(mymd[nm // 2])
    off = np.arange(ns + 1, dtype=np.int64) * 2
    st = np.tile(np.array([mymd[0], cut + 1], np.int32), ns)
    en = np.tile(np.array([cut, mymd[-1]], np.int32), ns)
    ad = np.tile(np.array([-0.37, 0.0]), ns)
    h = min(a.host_stations, ns)
    out = {"tool": "gpu_homog_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
           "stations": int(ns), "days": int(nd), "months": int(nm), "repeats": a.repeats, "hbm_measured_tb_s": HBM_MEASURED_TBS,
           "host_stations": int(h), "note": "one run on one machine; medians of the repeats after one warm-up call", "cases": []}
    cases = (
        ("obs_cnt", ("hm_cnt",), ns * nd * 4,
         lambda tm: _qalib.obs_cnt(obs, month, 0, nd - 1, timing=tm), lambda: RH.obs_cnt(obs[:h], month, 0, nd - 1)),
        ("monthly_means", ("hm_means",), ns * nd * 4 + ns * nm * 6,
         lambda tm: _qalib.monthly_means(obs, mf, mn, 9, timing=tm), lambda: RH.monthly_means(obs[:h], mf, mn, 9)),
        ("tobs_shift", ("hm_tobs",), ns * nd * 12,
         lambda tm: _qalib.tobs_shift(obs, tobs, timing=tm), lambda: RH.tobs_shift(obs[:h], tobs[:h])),
        ("homog_daily", ("hm_delta", "hm_apply"), ns * nd * 8,
         lambda tm: _qalib.homog_daily(obs, mean, miss, pha, mymd, mf, mn, off, st, en, ad, timing=tm),
         lambda: RH.homog_daily(obs[:h], mean[:h], miss[:h], pha[:h], mymd, mf, mn, off[:h + 1], st[:2 * h], en[:2 * h], ad[:2 * h])))
    for name, kernels, nbytes, fn, host in cases:
        med, first = median_call(fn, a.repeats)
        t0 = time.perf_counter()
        host()
        host_ms = (time.perf_counter() - t0) * 1e3
        kms = med[kernels[-1] + "_kernel_ms"]                        # the kernel that streams the days
        rate = nbytes / (kms * 1e-3)
        stages = {"kernels": sum(med[k + "_kernel_ms"] for k in kernels), "copies in": med["hm_upload_ms"],
                  "copies out": med["hm_download_ms"]}
        out["cases"].append(dict(case=name, batches=first["hm_batches"], median_ms=med, bytes_moved=int(nbytes),
                                 bytes_per_s=round(rate, 0), share_of_measured_hbm=round(rate / (HBM_MEASURED_TBS * 1e12), 4),
                                 limited_by=max(stages, key=stages.get),
                                 restatement_host_ms=round(host_ms, 1), restatement_stations=int(h)))
        print(json.dumps(out["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
