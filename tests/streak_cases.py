"""The series of the two streak tests (tests/test_gpu_nonspatial.py, tests/test_gpu_prcp.py): runs of equal values planted at
the seams of the 64-day blocks in which the shared streak walk (qa_streak_walk of topowx_amd/qa/twx_qa_series.h) reads a
series.  4 stations x 320 days (5 blocks) from 1990-01-01, every other value distinct."""
import datetime as dt

import numpy as np

from topowx_amd.dates import get_days_metadata

NDAYS, NSTN = 320, 4
# (station, first day, last day, flagged): a run of >= 20 values is flagged once a different value ends it
RUNS = (
    (0, 40, 70, True),        # 31 values over the seam 63 | 64
    (0, 100, 118, False),     # 19 values
    (0, 295, 319, False),     # 25 values up to the last day: nothing ends it
    (1, 60, 205, True),       # from block 0 into block 3: the blocks before the one that ends it are flagged by the carry loop
    (2, 44, 63, True),        # exactly 20, the last one closes block 0; the run that ends it opens block 1 ...
    (2, 64, 83, True),        # ... and is itself exactly 20 from the first lane of a block
    (3, 128, 147, True),      # exactly 20 from the first lane of a block, after distinct values
    (3, 236, 255, True),      # exactly 20 up to the last lane of a block, before distinct values
    (3, 300, 318, False),     # 19 values, then one distinct last day
)
HOLES = (95, 96, 125, 160, 191)       # days of station 1's run that are taken out of it: they break no run and count for none


def days():
    return get_days_metadata(dt.date(1990, 1, 1), dt.date(1990, 1, 1) + dt.timedelta(days=NDAYS - 1))


def build(base, run_values, hole_values):
    """base [NDAYS, NSTN] of distinct values; run k holds run_values[k]; HOLES[j] of station 1 holds hole_values[j].
    Returns the series (float32) and the mask of the values a streak check flags."""
    x = np.array(base, np.float32)
    want = np.zeros(x.shape, bool)
    for (s, a, b, hit), v in zip(RUNS, run_values):
        x[a:b + 1, s] = v
        want[a:b + 1, s] = hit
    for d, v in zip(HOLES, hole_values):
        x[d, 1] = v
        want[d, 1] = False
    return x, want
