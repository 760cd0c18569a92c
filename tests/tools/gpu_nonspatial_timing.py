#!/usr/bin/env python3
"""Time step08's non-spatial checks (``topowx_amd.qa.run_qa_non_spatial``) on two synthetic sets of stations
(tests/nonspatial_cases.py): 2 000 stations x 10 years, and 2 000 stations x 69 years (1948-2016), about the number of
SNOTEL / RAWS stations the reference runs this for.  Per case one JSON line: the device time of each kernel group (HIP
events inside the call; ``_qalib.NON_SPATIAL_KERNELS``), the seconds of the first and of a second, warm call, what is
left of the warm call beside the kernels (``host_and_copies_s``) and its share of the warm call (``host_share``), the
flag counts, and ``measured_on``: the device name the runtime reports.

``--ref-station-years-per-s`` is the executed reference's rate (tests/golden/make_golden_nonspatial.py prints it: one
CPU core of the build machine, not an MI355X figure); it is only carried into the line, next to the station-years of
the case, so that the two can be read together.

    python tests/tools/gpu_nonspatial_timing.py [--case small|large|both] [--out profiles/qa_nonspatial_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  -- before libtwxqa.so: whichever HIP runtime is loaded first serves the process
import numpy as np  # noqa: E402

import nonspatial_cases  # noqa: E402
from topowx_amd import _qalib  # noqa: E402
from topowx_amd.qa import NON_SPATIAL_FLAGS, run_qa_non_spatial  # noqa: E402

CASES = {"small": dict(n=2000, years=10, year0=1991), "large": dict(n=2000, years=69, year0=1948)}


def device_name(device):
    """What the runtime calls the device the figures come from."""
    p = torch.cuda.get_device_properties(device)
    return "%s (%s)" % (p.name, getattr(p, "gcnArchName", "?"))


def run_case(name, device, ref_rate):
    c = CASES[name]
    t0 = time.perf_counter()
    tmin, tmax, days = nonspatial_cases.timing_case(c["n"], c["years"], year0=c["year0"])
    t1 = time.perf_counter()
    run_qa_non_spatial(tmin, tmax, days, device=device)                    # first call: module load, first launches
    t2 = time.perf_counter()
    tm = {}
    f_tmin, f_tmax = run_qa_non_spatial(tmin, tmax, days, device=device, timing=tm)
    t3 = time.perf_counter()
    kern_ms = {k: round(tm[k + "_kernel_ms"], 3) for k in _qalib.NON_SPATIAL_KERNELS}
    kern_s = sum(kern_ms.values()) / 1e3
    warm = t3 - t2
    rec = dict(tool="gpu_nonspatial_timing", case=name, measured_on=device_name(device),
               measured_how="HIP events inside the call (kernel ms per group), time.perf_counter around the call (seconds, "
                            "transposes to station-major included); one warm call, no repeats",
               stations=int(c["n"]), days=int(days.size),
               flags={str(k): int((f_tmin == k).sum() + (f_tmax == k).sum()) for k in (1,) + NON_SPATIAL_FLAGS},
               setup_s=round(t1 - t0, 2), first_call_s=round(t2 - t1, 3), warm_call_s=round(warm, 3), kernel_ms=kern_ms,
               kernel_total_ms=round(kern_s * 1e3, 3), host_and_copies_s=round(warm - kern_s, 3),
               host_share=round((warm - kern_s) / warm, 3), station_years=int(c["n"] * c["years"]),
               station_years_per_s_warm=round(c["n"] * c["years"] / warm, 1), reference_station_years_per_s=ref_rate,
               reference_note="executed reference slice, one CPU core of the build machine (make_golden_nonspatial.py, 16 "
                              "stations x 16 years); not run on the MI355X host and not at this size")
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
