"""Timing of ``twxpq_non_spatial`` on synthetic rows (needs an MI355X and a build): 12 000 stations x 25 203 days (1948-2016).

    python tests/tools/gpu_prcp_timing.py [--out profiles/prcp_qa_timing.json] [--stations 12000] [--repeats 5] [--host-stations 4]

One warm-up call, then the MEDIAN of ``--repeats`` calls of the default chain: HIP-event milliseconds per kernel group and
host-clock milliseconds of the whole call (copies included); one further call with the streak and frequent-value checks
on.  The table kernel's rate: the bytes it has to move once (5 per observation read: value and flag; 40 per row written)
over its time, as a share of the rate a device-to-device copy of the same series reaches in the same run (read + write
bytes over HIP-event time, median of five).  Next to it the host time of the numpy restatement (tests/restate_prcp.py)
on the first ``--host-stations`` stations, named, not scaled up.  The rows are a block of 400 random series repeated: 30 %
wet days, hundredths of a centimetre, 5 % missing, a few large values.
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prcp_qa_timing.json"))
    ap.add_argument("--stations", type=int, default=12000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-stations", type=int, default=4)
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    import restate_prcp as RP
    from topowx_amd import _qalib
    from topowx_amd.dates import YMD, get_days_metadata
    days = get_days_metadata(dt.date(1948, 1, 1), dt.date(2016, 12, 31))
    nd = days.size
    ymd = np.asarray(days[YMD], np.int32)
    rs = np.random.RandomState(912)
    blk = 400
    base = np.where(rs.rand(blk, nd) < 0.30, np.round(rs.gamma(0.8, 0.9, (blk, nd)) + 0.01, 2), 0.0).astype(np.float32)
    base[rs.rand(blk, nd) < 0.05] = np.nan
    for s in range(blk):
        base[s, rs.randint(0, nd, 5)] = np.round(rs.uniform(20.0, 70.0, 5), 2)
    tv = np.round(8.0 - 12.0 * np.cos(2 * np.pi * (np.arange(nd) % 365.25) / 365.25) + rs.randn(blk, nd) * 3, 1).astype(np.float32)
    reps = -(-a.stations // blk)
    prcp = np.ascontiguousarray(np.tile(base, (reps, 1))[:a.stations])
    tavg = np.ascontiguousarray(np.tile(tv, (reps, 1))[:a.stations])
    ns = prcp.shape[0]

    def call(tm, **kw):
        t0 = time.perf_counter()
        f = _qalib.prcp_non_spatial(prcp, tavg, ymd, timing=tm, **kw)
        tm["host_ms"] = (time.perf_counter() - t0) * 1e3
        return f

    flags = call({})                                                 # warm-up: code objects, allocator, page faults
    runs = []
    for _ in range(a.repeats):
        tm = {}
        call(tm)
        runs.append(tm)
        print(json.dumps({k: round(v, 3) for k, v in tm.items()}), flush=True)
    med = {k: round(float(np.median([r[k] for r in runs])), 3) for k in runs[0]}
    tm_all = {}
    flags_all = call(tm_all, streak=True, frequent=True)
    # the copy rate of this device, this run: a device-to-device copy of one series array
    src = torch.empty(ns * nd, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    rates = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        rates.append(2 * src.numel() * 4 / (e0.elapsed_time(e1) * 1e-3))
    copy_rate = float(np.median(rates))
    del src, dst
    table_bytes = ns * nd * 5 + ns * 366 * 40
    table_rate = table_bytes / (med["pq_pctiles_kernel_ms"] * 1e-3)
    h = min(a.host_stations, ns)
    t0 = time.perf_counter()
    want = RP.run(prcp[:h].T, tavg[:h].T, ymd)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(want["flags"].T, flags[:h]), "the timed call and the restatement differ on the host slice"
    kernels = sum(med[k + "_kernel_ms"] for k in _qalib.PQ_KERNELS)
    out = {"tool": "gpu_prcp_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
           "stations": int(ns), "days": int(nd), "years": 69, "repeats": a.repeats,
           "note": "one run on one machine; medians of the repeats after one warm-up call; default chain",
           "median_ms": med, "kernels_ms": round(kernels, 3),
           "streak_frequent_single_call_ms": {k: round(v, 3) for k, v in tm_all.items()},
           "flags": {str(k): int((flags == k).sum()) for k in (1, 2, 4, 5, 6, 8, 10, 15)},
           "flags_streak_frequent": {str(k): int((flags_all == k).sum()) for k in (9, 19)},
           "copy_rate_measured_bytes_per_s": round(copy_rate, 0), "table_bytes_moved_once": int(table_bytes),
           "table_bytes_per_s": round(table_rate, 0), "table_share_of_measured_copy_rate": round(table_rate / copy_rate, 4),
           "table_rows_per_s": round(ns * 366 / (med["pq_pctiles_kernel_ms"] * 1e-3), 0),
           "station_years_per_s_whole_call": round(ns * 69 / (med["host_ms"] * 1e-3), 0),
           "station_years_per_s_kernels": round(ns * 69 / (kernels * 1e-3), 0),
           "restatement_host_ms": round(host_ms, 1), "restatement_stations": int(h)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
