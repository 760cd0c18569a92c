#!/usr/bin/env python3
"""Time the check of step16's fits (``twxck_infill_check``) once: on a synthetic batch of ``--items`` series of ``--rows``
rows (default 4096 x 2139: a 31-day month of 69 years), and, with ``--pool small`` or ``--pool full``, the whole
``infill_daily(chk_perf=True)`` on a synthetic pool of tests/tools/gpu_infillmat_timing.py (items per attempt, the check's
kernel milliseconds, ``pp_upload`` summed over the stages next to it).

There is no speed bar: the reference's check runs in R and cannot be run.  The only comparison figure is the numpy
restatement (tests/restate_chkperf.py, float64) on ONE CPU core of the machine this runs on, timed on ``--restate`` series
of the batch and named as that.  Writes one JSON document with the device name as the runtime reports it.

    python tests/tools/gpu_chkperf_timing.py --out profiles/chkperf_timing.json [--pool small]
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

import restate_chkperf as RC  # noqa: E402
from topowx_amd import _qalib  # noqa: E402


def run_batch(nitem, nrows, nrestate, device):
    rs = np.random.RandomState(11)
    fit = 5.0 + 4.0 * rs.randn(nitem * nrows)
    obs = fit + 0.6 * rs.randn(fit.size)
    obs[rs.rand(fit.size) < 0.3] = np.nan
    off = np.arange(nitem + 1, dtype=np.int64) * nrows
    _qalib.infill_check(off, fit, obs, device=device)               # first call: module load
    tm = {}
    t0 = time.perf_counter()
    res = _qalib.infill_check(off, fit, obs, device=device, timing=tm)
    call_s = time.perf_counter() - t0
    pen = RC.cpt_penalty(nrows)
    same = 0
    r0 = time.perf_counter()
    for i in range(nrestate):
        with np.errstate(all="ignore"):
            c = RC.check(fit[off[i]:off[i + 1]], obs[off[i]:off[i + 1]], pen)
        same += (c["reasons"], c["cpt_tau"], c["nobs"]) == (res["reasons"][i], res["cpt_tau"][i], res["nobs"][i])
    restate_s = (time.perf_counter() - r0) / max(1, nrestate)
    return dict(items=nitem, rows=nrows, kernel_ms=round(tm["ck_check_kernel_ms"], 3), upload_ms=round(tm["ck_upload_ms"], 3),
                download_ms=round(tm["ck_download_ms"], 3), call_s=round(call_s, 4), batches=int(tm["ck_batches"]),
                numpy_restatement_one_cpu_core=dict(items=nrestate, seconds_per_item=round(restate_s, 6),
                                                    seconds_for_the_batch_extrapolated=round(restate_s * nitem, 2),
                                                    same_reasons_tau_nobs=int(same)))


def run_pool(name, device):
    from gpu_infillmat_timing import CASES, make_pool
    from gpu_ppca_timing import normals
    from topowx_amd.infill import infill_daily
    n, first, last, ntarget = CASES[name]
    pool = make_pool(n, first, last)
    targets = pool.ids if ntarget is None else pool.ids[np.sort(np.random.default_rng(9).choice(n, ntarget, replace=False))]
    mean, vari = normals(pool)
    tm = {}
    t0 = time.perf_counter()
    r = infill_daily(pool, "tmin", targets, mean, vari, device=device, timing=tm, chk_perf=True)
    sec = time.perf_counter() - t0
    items = int((r.status >= 0).sum())
    return dict(case=name, stations=n, days=int(pool.days.size), targets=int(len(targets)), items=items, seconds=round(sec, 3),
                attempt_items=tm["attempt_items"], share_per_attempt=[round(k / max(1, items), 4) for k in tm["attempt_items"]],
                kept_attempt={str(a): int((r.attempt == a).sum()) for a in range(-1, 4)},
                nonoptimal=int(tm["nonoptimal"]), retry_fixed=int(tm["retry_fixed"]),
                reasons_of_attempt_0={str(b): int(((r.reasons[..., 0] >= 0) & (r.reasons[..., 0] & b > 0)).sum()) for b in (1, 2, 4, 8)},
                ck_check_kernel_ms=round(tm["ck_check_kernel_ms"], 3), ck_calls=int(tm["ck_calls"]),
                pp_upload_ms_over_the_stages=round(tm["pp_upload_ms"], 3), pp_calls=int(tm["pp_calls"]),
                pp_iter_kernel_ms=round(tm["pp_iter_kernel_ms"], 3))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=2139)
    ap.add_argument("--restate", type=int, default=64)
    ap.add_argument("--pool", default="", help="comma-separated cases of gpu_infillmat_timing (small, full)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    doc = dict(tool="gpu_chkperf_timing", device_name=torch.cuda.get_device_name(a.device), pools=[])

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")

    doc["batch"] = run_batch(a.items, a.rows, a.restate, a.device)
    print(json.dumps(doc["batch"]), flush=True)
    save()
    for name in [p for p in a.pool.split(",") if p]:
        doc["pools"].append(run_pool(name, a.device))
        print(json.dumps(doc["pools"][-1]), flush=True)
        save()


if __name__ == "__main__":
    main()
