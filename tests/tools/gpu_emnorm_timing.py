#!/usr/bin/env python3
"""Time step14's mean / variance estimate (``topowx_amd.infill.estimate_mean_variance``, station columns only) once on
the two synthetic pools of tests/tools/gpu_infillmat_timing.py (``small``: 2 000 stations x 10 years, every station a
target; ``full``: 12 000 stations x 69 years, 2 000 targets; 24 000 items each).

Per case: the HIP-event milliseconds of k_em_prep and of k_em_iter summed over the launches, the launches (rounds) and
workspace batches, the iterations per item, the seconds of a first and of a second, warm call, the parts of the warm
call on the host clock (column assembly, library call, copies in and out) and its host share (what is not kernel time).
There is no speed bar: the reference's estimator (R's ``norm``) cannot be run here.  The only comparison figure is the
numpy restatement (tests/restate_emnorm.py) on ONE CPU core of the machine this runs on, timed on ``--restate`` items
of the case and named as that.  Writes one JSON document with the device name as the runtime reports it.

    python tests/tools/gpu_emnorm_timing.py --out profiles/emnorm_timing.json [--cases small,full] [--restate 24]
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

import restate_emnorm as RE  # noqa: E402
from gpu_infillmat_timing import CASES, make_pool  # noqa: E402
from topowx_amd.infill import build_infill_matrices, estimate_mean_variance  # noqa: E402


def run_case(name, device, nrestate):
    n, first, last, ntarget = CASES[name]
    pool = make_pool(n, first, last)
    targets = None if ntarget is None else pool.ids[np.sort(np.random.default_rng(9).choice(n, ntarget, replace=False))]
    m = build_infill_matrices(pool, "tmin", targets, device=device)
    t1 = time.perf_counter()
    estimate_mean_variance(m, device=device)
    t2 = time.perf_counter()
    tm = {}
    e = estimate_mean_variance(m, device=device, timing=tm)
    t3 = time.perf_counter()
    kernel_s = (tm["em_prep_kernel_ms"] + tm["em_iter_kernel_ms"]) / 1000.0
    status, count = np.unique(e.status, return_counts=True)
    ok = e.status == 0
    rows = np.bincount(m.group[m.group >= 0].astype(np.int64), minlength=m.ngroups)
    pick = np.random.default_rng(3).choice(np.nonzero(ok.ravel())[0], min(nrestate, int(ok.sum())), replace=False)
    r0 = time.perf_counter()
    same = 0
    for i in pick:
        t, g = divmod(int(i), m.ngroups)
        with np.errstate(all="ignore"):
            same += RE.run(m.matrix(t, g))["iters"] == e.iters[t, g]
    restate_s = (time.perf_counter() - r0) / max(1, pick.size)
    return dict(case=name, stations=n, days=int(pool.days.size), targets=int(len(m.target_ids)), items=int(e.status.size),
                status={str(int(s)): int(c) for s, c in zip(status, count)}, rows_per_item=[int(rows.min()), int(rows.max())],
                columns={"min": int(e.ncols[ok].min()), "median": float(np.median(e.ncols[ok])), "max": int(e.ncols[ok].max())},
                iterations={"min": int(e.iters[ok].min()), "median": float(np.median(e.iters[ok])), "max": int(e.iters[ok].max()),
                            "sum": int(e.iters[ok].sum())},
                rounds=int(tm["em_rounds"]), batches=int(tm["em_batches"]),
                kernel_ms=dict(prep=round(tm["em_prep_kernel_ms"], 3), iter=round(tm["em_iter_kernel_ms"], 3)),
                first_call_s=round(t2 - t1, 3), warm_call_s=round(t3 - t2, 3),
                warm_call_parts_s=dict(assemble=round(tm["assemble_s"], 4), library=round(tm["em_library_s"], 4),
                                       upload=round(tm["em_upload_ms"] / 1000.0, 4), download=round(tm["em_download_ms"] / 1000.0, 4)),
                host_share=round(1.0 - kernel_s / (t3 - t2), 4), items_per_second=round(e.status.size / (t3 - t2), 1),
                numpy_restatement_one_cpu_core=dict(items=int(pick.size), seconds_per_item=round(restate_s, 4),
                                                    same_iterations=int(same)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default="small,full")
    ap.add_argument("--restate", type=int, default=24)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    doc = dict(tool="gpu_emnorm_timing", device_name=torch.cuda.get_device_name(a.device), cases=[])
    for name in a.cases.split(","):
        doc["cases"].append(run_case(name, a.device, a.restate))
        print(json.dumps(doc["cases"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
