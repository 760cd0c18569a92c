"""Timing of step17 / step18's two library entries on synthetic rows (needs an MI355X and a build):

  * ``twxsc_serial_complete`` at 12 000 stations x 25 203 days, in its full form (choice, scrub, flags and the 1981-2010
    normals) and in its normals-only form;
  * ``twxsc_series_check`` at 500 series x 25 203 days.

    python tests/tools/serial_timing.py [--out profiles/serial_complete_timing.json] [--stations 12000] [--series 500] [--repeats 5]

One warm-up call, then the MEDIAN of ``--repeats`` calls: HIP-event milliseconds per kernel, host milliseconds of the whole
call and of its copies, and for entry A the bytes its kernels move per second (per day k_sc_select reads the flag twice and
the chosen source once and writes the series and the flag: 11 bytes; normals only: 4; k_sc_norms reads the 4 bytes of every
day of the normals' years) against the HBM rate of the MI355X (8.0 TB/s specified, 6.29 TB/s measured with a float4 copy).
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

HBM_SPEC_TBS, HBM_MEASURED_TBS = 8.0, 6.29


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serial_complete_timing.json"))
    ap.add_argument("--stations", type=int, default=12000)
    ap.add_argument("--series", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args(argv)
    import torch                                                     # first: its HIP runtime serves the process
    from topowx_amd import _qalib
    from topowx_amd.dates import DAY, MONTH, YEAR, get_days_metadata
    days = get_days_metadata(dt.date(1948, 1, 1), dt.date(2016, 12, 31))
    nd = days.size
    gf, gn = _qalib.norm_groups(days[YEAR], days[MONTH], 1981, 2010, day=days[DAY])
    rs = np.random.RandomState(1718)
    blk = 500
    doy = np.arange(nd) % 365.25
    base = (5.0 - 12.0 * np.cos(2 * np.pi * doy / 365.25) + rs.randn(blk, nd) * 4).astype(np.float32)
    flag_blk = (rs.rand(blk, nd) < 0.3).astype(np.int8)
    for s in range(0, blk, 4):                                       # a quarter of the stations are all model
        a0 = int(rs.randint(nd - 2000))
        flag_blk[s, a0:a0 + 1900] = 1
    reps = -(-a.stations // blk)
    tair = np.ascontiguousarray(np.tile(base, (reps, 1))[:a.stations])
    tinf = tair + np.float32(0.5)
    flag = np.ascontiguousarray(np.tile(flag_blk, (reps, 1))[:a.stations])
    ns = tair.shape[0]
    out = {"tool": "serial_timing", "device_name": torch.cuda.get_device_name(0), "date": dt.date.today().isoformat(),
           "days": int(nd), "repeats": a.repeats, "hbm_spec_tb_s": HBM_SPEC_TBS, "hbm_measured_tb_s": HBM_MEASURED_TBS, "cases": []}
    norm_days = int(gn.sum())
    for name, bytes_a_day, fn in (
            ("serial_complete full", 11, lambda tm: _qalib.serial_complete(tair, tinf, flag, group_first=gf, group_ndays=gn, timing=tm)),
            ("serial_complete normals only", 4, lambda tm: _qalib.serial_complete(tair, group_first=gf, group_ndays=gn, timing=tm))):
        med, first = median_call(fn, a.repeats)
        sel = ns * nd * bytes_a_day / (med["sc_select_kernel_ms"] * 1e-3)
        nrm = ns * norm_days * 4 / (med["sc_norms_kernel_ms"] * 1e-3)
        out["cases"].append(dict(case=name, series=ns, batches=first["sc_batches"], median_ms=med,
                                 select_bytes_per_s=round(sel, 0), select_share_of_measured_hbm=round(sel / (HBM_MEASURED_TBS * 1e12), 4),
                                 norms_bytes_per_s=round(nrm, 0), norms_share_of_measured_hbm=round(nrm / (HBM_MEASURED_TBS * 1e12), 4)))
        print(json.dumps(out["cases"][-1]), flush=True)
    series = np.ascontiguousarray(base[:a.series] if a.series <= blk else np.tile(base, (-(-a.series // blk), 1))[:a.series])
    med, first = median_call(lambda tm: _qalib.series_check(series, timing=tm), a.repeats)
    rate = series.size * 4 * 3 / (med["sc_series_kernel_ms"] * 1e-3)               # three passes over the rows
    out["cases"].append(dict(case="series_check", series=int(series.shape[0]), batches=first["sc_series_batches"], median_ms=med,
                             bytes_read_per_s=round(rate, 0)))
    print(json.dumps(out["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
