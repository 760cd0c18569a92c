#!/usr/bin/env python3
"""Time step08's whole spatial stage (``topowx_amd.qa.run_qa_spatial_only``: regression check, day-of-year normals,
corroboration check, mega-inconsistency check) on two synthetic pools (tests/corrob_cases.py): 2 000 stations x 10 years
with every station a target, and a 12 000-station pool x 69 years (1948-2016) with 2 000 targets.  Per case one JSON
line: the device time of each kernel (HIP events inside the call; ``_qalib.SPATIAL_ONLY_KERNELS``), the seconds of the
first and of a second, warm call, what is left of the warm call beside the kernels (``host_and_copies_s``) and its share
of the warm call (``host_share``), the flag counts, and ``measured_on``: the device name the runtime reports.

``--ref-station-years-per-s`` is the executed reference's rate (tests/golden/make_golden_corrob.py prints it: one CPU
core of the build machine, not an MI355X figure); it is only carried into the line, next to the station-years of the
targets, so that the two can be read together.

    python tests/tools/gpu_corrob_timing.py [--case small|large|both] [--out profiles/qa_corrob_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import corrob_cases  # noqa: E402
from topowx_amd import _qalib  # noqa: E402
from topowx_amd.qa import StationObsPool, run_qa_spatial_only  # noqa: E402

CASES = {"small": dict(n=2000, years=10, ntarget=None), "large": dict(n=12000, years=69, ntarget=2000)}


def device_name(device):
    """What the runtime calls the device the figures come from."""
    import torch
    p = torch.cuda.get_device_properties(device)
    return "%s (%s)" % (p.name, getattr(p, "gcnArchName", "?"))


def run_case(name, device, ref_rate):
    c = CASES[name]
    t0 = time.perf_counter()
    if name == "small":
        ids, lon, lat, tmin, tmax, days, _ = corrob_cases.big_case(c["n"], c["years"])
    else:
        ids, lon, lat, tmin, tmax, days, _ = corrob_cases.big_case(c["n"], c["years"], seed=12, year0=1948)
    pool = StationObsPool(ids, lon, lat, tmin, tmax, days)
    targets = None if c["ntarget"] is None else ids[np.linspace(0, ids.size - 1, c["ntarget"]).astype(int)]
    t1 = time.perf_counter()
    run_qa_spatial_only(pool, targets, device=device)                      # first call: module load, first launches
    t2 = time.perf_counter()
    tm = {}
    f_tmin, f_tmax, det = run_qa_spatial_only(pool, targets, device=device, details=True, timing=tm)
    t3 = time.perf_counter()
    nt = ids.size if targets is None else len(targets)
    kern_ms = {k: round(tm[k + "_kernel_ms"], 3) for k in _qalib.SPATIAL_ONLY_KERNELS}
    kern_s = sum(kern_ms.values()) / 1e3
    warm = t3 - t2
    st, cnt = np.unique(det["status"], return_counts=True)
    rec = dict(tool="gpu_corrob_timing", case=name, measured_on=device_name(device),
               measured_how="HIP events inside the call (kernel ms), time.perf_counter around the call (seconds); one "
                            "warm call, no repeats",
               pool_stations=int(ids.size), targets=int(nt), days=int(days.size),
               status_counts={str(int(a)): int(b) for a, b in zip(st, cnt)},
               flags={str(k): int((f_tmin == k).sum() + (f_tmax == k).sum()) for k in (1, 2, 16, 17, 18)},
               setup_s=round(t1 - t0, 2), first_call_s=round(t2 - t1, 3), warm_call_s=round(warm, 3), kernel_ms=kern_ms,
               host_and_copies_s=round(warm - kern_s, 3), host_share=round((warm - kern_s) / warm, 3),
               target_station_years=int(nt * c["years"]), reference_station_years_per_s=ref_rate,
               reference_note="executed reference slice, one CPU core of the build machine (make_golden_corrob.py); "
                              "not run on the MI355X host and not at this size")
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("small", "large", "both"), default="both")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ref-station-years-per-s", type=float, default=None)
    ap.add_argument("--out", help="also write the records to this JSON file")
    a = ap.parse_args(argv)
    recs = [run_case(n, a.device, a.ref_station_years_per_s) for n in (("small", "large") if a.case == "both" else (a.case,))]
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
