#!/usr/bin/env python3
"""Time step15's cross-validation of the infill (``topowx_amd.infill.XvalInfill.run_all``) once: a synthetic pool at the
density of DESIGN.md section 16 (tests/tools/gpu_infillmat_timing.py, case ``small``: 2 000 stations x 10 years), ``--xval``
cross-validation stations (default 200), one variable, ``chk_perf`` on.  Recorded: host seconds and kernel milliseconds of
every stage (hold-out, matrices, EM, daily with the ladder, score).

There is no speed bar.  The only comparison figure is the same stations done ONE AT A TIME through the functions the
package had before ``XvalInfill`` (``build_infill_matrices`` / ``estimate_mean_variance`` / ``infill_daily`` on a pool copy
with the station's held observations masked): the only way to do step15 without the batched chain.  ``--serial-budget-s``
ends that loop early; the number of stations it did is written next to its seconds, and nothing is extrapolated.
Writes one JSON document with the device name as the runtime reports it.

    python tests/tools/gpu_xvalinfill_timing.py --out profiles/xval_infill_timing.json
"""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  -- first: its bundled HIP runtime must be the one the process loads

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import numpy as np  # noqa: E402

from topowx_amd.infill import (XvalInfill, XvalInfillParams, build_infill_matrices, estimate_mean_variance,  # noqa: E402
                               infill_daily)
from topowx_amd.qa import StationObsPool  # noqa: E402


def _round(d):
    return {k: (_round(v) if isinstance(v, dict) else round(v, 4) if isinstance(v, float) else v) for k, v in d.items()}


def main(argv=None):
    from gpu_infillmat_timing import CASES, make_pool
    from gpu_ppca_timing import normals
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--case", default="small")
    ap.add_argument("--xval", type=int, default=200)
    ap.add_argument("--ntrain-yrs", type=float, default=5)
    ap.add_argument("--serial-budget-s", type=float, default=0.0, help="end the one-at-a-time loop after this many seconds")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    n, first, last, _ = CASES[a.case]
    pool = make_pool(n, first, last)
    mean, vari = normals(pool)
    ids = pool.ids[np.sort(np.random.default_rng(15).choice(n, a.xval, replace=False))]
    params = XvalInfillParams(None, 3, 4, 0.99, True, 0, 0.5, 0.99, False)
    doc = dict(tool="gpu_xvalinfill_timing", device_name=torch.cuda.get_device_name(a.device), case=a.case, stations=n,
               days=int(pool.days.size), xval_stations=int(a.xval), ntrain_yrs=a.ntrain_yrs, runs=1)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")

    XvalInfill(pool, "tmin", params, mean, vari, ids[:2], a.ntrain_yrs, a.device).run_all()      # module load, first launches
    xv = XvalInfill(pool, "tmin", params, mean, vari, ids, a.ntrain_yrs, a.device)
    tm = {}
    t0 = time.perf_counter()
    res = xv.run_all(tm)
    sec = time.perf_counter() - t0
    day = tm["daily"]
    kernel_ms = dict(holdout=tm.get("xv_holdout_kernel_ms", 0.0), score=tm.get("xv_score_kernel_ms", 0.0),
                     matrices=sum(v for k, v in tm["matrices"].items() if k.endswith("_kernel_ms")),
                     em=sum(v for k, v in tm["em"].items() if k.endswith("_kernel_ms")),
                     daily=sum(v for k, v in day.items() if k.endswith("_kernel_ms")))
    host_s = {k[:-2]: tm[k] for k in ("holdout_s", "matrices_s", "em_s", "daily_s", "score_s")}
    doc["batched"] = _round(dict(seconds=sec, host_seconds=host_s, kernel_ms=kernel_ms,
                                 kernel_share_of_wall=sum(kernel_ms.values()) / 1e3 / sec, nkeep=xv.nkeep,
                                 held=int(res.nheld.sum()), scored=int(res.n.sum()),
                                 items_fitted=int(np.isin(res.daily.status, (0, 20)).sum()),
                                 nonoptimal=int(res.daily.nonoptimal.sum()), stage_timing=dict(matrices=tm["matrices"],
                                                                                                em=tm["em"], daily=day)))
    print(json.dumps(doc["batched"]["host_seconds"]), json.dumps(doc["batched"]["kernel_ms"]), flush=True)
    save()
    # the same stations one at a time, through the functions the package had before
    held = xv.stn_xval_masks
    done, same, s0 = 0, 0, time.perf_counter()
    for t, sid in enumerate(ids):
        c = pool.idxs[sid]
        tmin = pool.tmin.copy()
        tmin[held[t], c] = np.nan
        cp = StationObsPool(pool.ids, pool.lon, pool.lat, tmin, pool.tmax, pool.days)
        est = estimate_mean_variance(build_infill_matrices(cp, "tmin", [sid], np.isfinite(mean[:, 0]), None, 3, a.device),
                                     device=a.device)
        m2, v2 = mean.copy(), vari.copy()
        m2[c], v2[c] = est.mean[0], est.variance[0]
        d = infill_daily(cp, "tmin", [sid], m2, v2, device=a.device, chk_perf=True)
        same += d.infill_tair[0].tobytes() == res.daily.infill_tair[t].tobytes()
        done += 1
        if done % 10 == 0:
            print("one at a time: %d stations, %.1f s" % (done, time.perf_counter() - s0), flush=True)
        if a.serial_budget_s > 0 and time.perf_counter() - s0 > a.serial_budget_s:
            break
    ssec = time.perf_counter() - s0
    doc["one_at_a_time"] = _round(dict(stations_done=done, seconds=ssec, seconds_per_station=ssec / done,
                                       same_bytes_as_the_batched_row=int(same)))
    print(json.dumps(doc["one_at_a_time"]), flush=True)
    save()


if __name__ == "__main__":
    main()
