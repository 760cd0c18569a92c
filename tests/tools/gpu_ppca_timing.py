#!/usr/bin/env python3
"""Time step16's daily infill (``topowx_amd.infill.infill_daily``, station columns only) once on the two synthetic pools
of tests/tools/gpu_infillmat_timing.py (``small``: 2 000 stations x 10 years, every station a target; ``full``: 12 000
stations x 69 years, 2 000 targets; 24 000 items each).  The monthly mean and variance of every station are its own moments
over its finite values (a stand-in for step14's report).

Per case: the HIP-event milliseconds of k_pp_prep and of k_pp_iter summed over the launches, the launches and library
calls (rounds of the component search), the fits per item, the iterations of the accepted fits, the seconds of a first and
of a second, warm call, the parts of the warm call on the host clock and its host share (what is not kernel time).
There is no speed bar: the reference's estimator (R's ``pcaMethods``) cannot be run here.  The only comparison figure is the
numpy restatement (tests/restate_ppca.py) on ONE CPU core of the machine this runs on, timed on ``--restate`` items of the
case and named as that.  Not measured: occupancy, counters, the cost of the repeated column gather.  Writes one JSON
document with the device name as the runtime reports it.

    python tests/tools/gpu_ppca_timing.py --out profiles/ppca_timing.json [--cases small,full] [--restate 24]
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

import restate_ppca as RP  # noqa: E402
from gpu_infillmat_timing import CASES, make_pool  # noqa: E402
from topowx_amd.dates import MONTH  # noqa: E402
from topowx_amd.infill import infill_daily, item_matrix  # noqa: E402
from topowx_amd.infill.infill_daily import daily_items  # noqa: E402


def normals(pool):
    n = pool.ids.size
    mean, vari = np.full((n, 12), np.nan), np.full((n, 12), np.nan)
    with np.errstate(all="ignore"):
        for g in range(12):
            rows = pool.tmin[pool.days[MONTH] == g + 1].astype(np.float64)
            mean[:, g], vari[:, g] = np.nanmean(rows, axis=0), np.nanvar(rows, axis=0)
    vari[~(vari > 0)] = np.nan
    mean[~np.isfinite(vari)] = np.nan
    return mean, vari


def run_case(name, device, nrestate):
    n, first, last, ntarget = CASES[name]
    pool = make_pool(n, first, last)
    targets = pool.ids if ntarget is None else pool.ids[np.sort(np.random.default_rng(9).choice(n, ntarget, replace=False))]
    mean, vari = normals(pool)
    t1 = time.perf_counter()
    infill_daily(pool, "tmin", targets, mean, vari, device=device)
    t2 = time.perf_counter()
    tm = {}
    r = infill_daily(pool, "tmin", targets, mean, vari, device=device, timing=tm)
    t3 = time.perf_counter()
    kernel_s = (tm["pp_prep_kernel_ms"] + tm["pp_iter_kernel_ms"]) / 1000.0
    status, count = np.unique(r.status, return_counts=True)
    ok = np.isin(r.status, (0, 20))
    pick_t = np.random.default_rng(3).choice(len(targets), min(max(1, nrestate // 12), len(targets)), replace=False)
    items, obs = daily_items(pool, "tmin", targets[np.sort(pick_t)], mean, vari, device=device)
    group = (np.asarray(pool.days[MONTH], np.int64) - 1).astype(np.int8)
    sub = infill_daily(pool, "tmin", targets[np.sort(pick_t)], mean, vari, device=device)
    same = done = skipped = 0
    r0 = time.perf_counter()
    for it in items[:nrestate]:
        if it["matrix_status"] != 0:                                # nothing to restate: counted, not hidden
            skipped += 1
            continue
        with np.errstate(all="ignore"):
            w = RP.search(item_matrix(obs, np.nonzero(group == it["g"])[0], it))
        done += 1
        same += (w["npcs"], w["nfits"], w["iters"]) == (sub.npcs[it["t"], it["g"]], sub.nfits[it["t"], it["g"]], sub.iters[it["t"], it["g"]])
    restate_s = (time.perf_counter() - r0) / max(1, done)
    return dict(case=name, stations=n, days=int(pool.days.size), targets=int(len(targets)), items=int((r.status >= 0).sum()),
                status={str(int(s)): int(c) for s, c in zip(status, count)},
                columns={"min": int(r.ncols[ok].min()), "median": float(np.median(r.ncols[ok])), "max": int(r.ncols[ok].max())},
                npcs={"min": int(r.npcs[ok].min()), "median": float(np.median(r.npcs[ok])), "max": int(r.npcs[ok].max())},
                fits_per_item={"min": int(r.nfits[ok].min()), "median": float(np.median(r.nfits[ok])), "max": int(r.nfits[ok].max()),
                               "sum": int(r.nfits.sum())},
                iterations_of_the_accepted_fit={"min": int(r.iters[ok].min()), "median": float(np.median(r.iters[ok])),
                                                "max": int(r.iters[ok].max())},
                r2_not_reached=int(r.r2_not_reached.sum()), library_calls=int(r.calls), launches=int(tm["pp_rounds"]),
                batches=int(tm["pp_batches"]),
                kernel_ms=dict(prep=round(tm["pp_prep_kernel_ms"], 3), iter=round(tm["pp_iter_kernel_ms"], 3)),
                first_call_s=round(t2 - t1, 3), warm_call_s=round(t3 - t2, 3),
                warm_call_parts_s=dict(assemble=round(tm["assemble_s"], 4), search=round(tm["search_s"], 4),
                                       writeback=round(tm["writeback_s"], 4), upload=round(tm["pp_upload_ms"] / 1000.0, 4),
                                       download=round(tm["pp_download_ms"] / 1000.0, 4)),
                host_share=round(1.0 - kernel_s / (t3 - t2), 4), items_per_second=round(int((r.status >= 0).sum()) / (t3 - t2), 1),
                numpy_restatement_one_cpu_core=dict(items=int(done), items_without_a_matrix=int(skipped), seconds_per_item=round(restate_s, 4),
                                                    same_npcs_fits_iterations=int(same)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default="small,full")
    ap.add_argument("--restate", type=int, default=24)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    doc = dict(tool="gpu_ppca_timing", device_name=torch.cuda.get_device_name(a.device), cases=[])
    for name in a.cases.split(","):
        doc["cases"].append(run_case(name, a.device, a.restate))
        print(json.dumps(doc["cases"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
