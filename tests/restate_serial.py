"""step17 / step18 in numpy, the same text as include/twx_qa.h (``twxsc_serial_complete``, ``twxsc_series_check``): what the
GPU kernels are compared with.  The sums of the normals are sequential: a group's days in day order, a month's years in year
order.  The check of a whole series is tests/restate_chkperf.py's ``check`` with its cap of 8192 rows lifted (no new text:
the "impossible" and "change point" paragraphs are the ones the chk_perf kernel is tested against).
"""
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_chkperf as RC  # noqa: E402

FILL_F4 = np.float32(9.969209968386869e36)
RUN_THRESHOLD = 1826
MAX_MISS = 9
MAX_DAYS = 1 << 20
MAX_GROUPS = 1536


def runs_of_ones(bits):
    """The lengths of the runs of ones of a 0 / 1 vector (the reference's ``_runs_of_ones_array``, restated)."""
    b = np.concatenate([[0], np.asarray(bits, np.int64) != 0, [0]]).astype(np.int64)
    d = np.diff(b)
    return np.nonzero(d < 0)[0] - np.nonzero(d > 0)[0]


def max_run(bits):
    r = runs_of_ones(bits)
    return int(r.max()) if r.size else 0


def missing(a, fill=FILL_F4):
    a = np.asarray(a, np.float32)
    return ~np.isfinite(a) | (a == np.float32(fill))


def norm_groups(year, month, start_yr, end_yr):
    """(group_first, group_ndays) of a gap-free day axis: a loop over the groups, not the binding's vector form."""
    year, month = np.asarray(year), np.asarray(month)
    first, nd = [], []
    for y in range(start_yr, end_yr + 1):
        for m in range(1, 13):
            d = np.nonzero((year == y) & (month == m))[0]
            first.append(int(d[0]) if d.size else 0)
            nd.append(int(d.size))
            assert d.size == 0 or np.array_equal(d, np.arange(d[0], d[0] + d.size))
    return np.array(first, np.int32), np.array(nd, np.int32)


def normals(serial, fill, group_first, group_ndays, max_miss):
    """(norm [ns, 12] float64, norm_nmths [ns, 12] int32, mean [ns, ngroups] with NaN = masked) of ``serial`` [ns, ndays]."""
    serial = np.asarray(serial, np.float32)
    ns, ng = serial.shape[0], len(group_first)
    mean = np.full((ns, ng), np.nan)
    for g in range(ng):
        nd, d0 = int(group_ndays[g]), int(group_first[g])
        if nd == 0:
            continue
        x = serial[:, d0:d0 + nd]
        ok = ~missing(x, fill)
        s = np.zeros(ns)
        for j in range(nd):                                         # day order
            s = np.where(ok[:, j], s + x[:, j].astype(np.float64), s)
        n = ok.sum(axis=1)
        keep = n > 0
        if max_miss is not None and max_miss >= 0:
            keep &= (nd - n) <= max_miss
        with np.errstate(all="ignore"):
            mean[:, g] = np.where(keep, s / n, np.nan)
    norm, nm = np.full((ns, 12), np.nan), np.zeros((ns, 12), np.int32)
    for m in range(12):
        s, n = np.zeros(ns), np.zeros(ns, np.int64)
        for g in range(m, ng, 12):                                  # year order
            ok = ~np.isnan(mean[:, g])
            s = np.where(ok, s + np.where(ok, mean[:, g], 0.0), s)
            n += ok
        with np.errstate(all="ignore"):
            norm[:, m] = np.where(n > 0, s / n, np.nan)
        nm[:, m] = n
    return norm, nm, mean


def serial_complete(tair, tair_infilled=None, flag=None, run_threshold=RUN_THRESHOLD, fill=FILL_F4, group_first=None,
                    group_ndays=None, max_miss=MAX_MISS):
    """The outputs of ``twxsc_serial_complete``: a dict of max_run, nmissing, all_infill, ``miss`` [ns, ndays], and with
    flags serial / flag_infilled, with groups norm / norm_nmths."""
    tair = np.asarray(tair, np.float32)
    ns, nd = tair.shape
    fill = np.float32(fill)
    out = dict(max_run=np.zeros(ns, np.int32), all_infill=np.zeros(ns, bool))
    src = tair.copy()
    if flag is not None:
        flag, tinf = np.asarray(flag, np.int8), np.asarray(tair_infilled, np.float32)
        out["max_run"] = np.array([max_run(f) for f in flag], np.int32)
        out["all_infill"] = out["max_run"] >= run_threshold
        src[out["all_infill"]] = tinf[out["all_infill"]]
        out["flag_infilled"] = np.where(out["all_infill"][:, None], 1, flag != 0).astype(np.int8)
    miss = missing(src, fill)
    serial = src.copy()
    serial[miss] = fill
    out["miss"], out["nmissing"] = miss, miss.sum(axis=1).astype(np.int32)
    if flag is not None:
        out["serial"] = serial
    if group_first is not None:
        out["norm"], out["norm_nmths"], out["group_mean"] = normals(serial, fill, group_first, group_ndays, max_miss)
    return out


@contextlib.contextmanager
def _no_row_cap():
    old = RC.MAX_ROWS
    RC.MAX_ROWS = MAX_DAYS
    try:
        yield
    finally:
        RC.MAX_ROWS = old


def series_check(series, pen, fill=FILL_F4, impossible_high=RC.IMPOSSIBLE_HIGH, impossible_low=RC.IMPOSSIBLE_LOW):
    """``twxsc_series_check`` of ONE series: tests/restate_chkperf.py's ``check_pair`` record (float64 with its distances
    from longdouble) of the series widened to float64 with no observation and no row cap, plus ``nmissing`` and ``pen``.  A
    series with a missing value: status NOT_FITTED, reasons UNFITTED."""
    s = np.asarray(series, np.float32)
    miss = missing(s, fill)
    nmiss = int(miss.sum())
    f = s.astype(np.float64)
    if nmiss:
        f = np.where(miss, np.nan, f)                               # a fill value is as missing as a NaN
    with _no_row_cap(), np.errstate(all="ignore"):
        w = RC.check_pair(f, np.full(f.size, np.nan), pen, impossible_high=impossible_high, impossible_low=impossible_low)
    w["nmissing"], w["pen"] = nmiss, pen
    return w
