"""Shared by tests/test_serial_host.py and tests/test_gpu_serial.py: the golden of make_golden_serial.py, the rows of entry A
(``twxsc_serial_complete``), the series of entry B (``twxsc_series_check``) and the scripted step16 reports of the
end-to-end test (no GPU anywhere in this file)."""
import datetime as dt
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_chkperf as RC  # noqa: E402
import restate_serial as RS  # noqa: E402

FILL = RS.FILL_F4
THREADS, LANES = 256, 64
SELECT_NDAYS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 4097)
CHECK_N = (3, 4, 5, 255, 256, 257, 8192, 8193, 25203)
LONG_ND = 25203
STEP = 4.0                         # the factor of the standard deviation across a variance step (as chkperf_cases.STEP)
NORM_BOUND = 128 * 2.0 ** -53      # two orders of summing <= 31 + 30 terms plus two divisions, times max |x|


def load_gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_serial_v1.npz"))


# ---- entry A ----
FLAG_KINDS = ("none", "all", "all -127", "ends on the last day", "starts on day 0", "crosses a chunk boundary",
              "crosses a wavefront boundary", "two equal longest runs", "random 0.5", "random 0.9 with -127", "single day",
              "alternating")


def flag_row(kind, nd, rs):
    """One int8 flag row of ``nd`` days.  c = ceil(nd / 256) is the chunk of a thread, 64 c that of a wavefront."""
    c = -(-nd // THREADS)
    f = np.zeros(nd, np.int8)

    def put(a, b, v=1):
        f[max(a, 0):max(min(b, nd), 0)] = v

    if kind == "all":
        f[:] = 1
    elif kind == "all -127":
        f[:] = -127
    elif kind == "ends on the last day":
        put(nd - max(nd // 3, 1), nd)
    elif kind == "starts on day 0":
        put(0, max(nd // 4, 1))
    elif kind == "crosses a chunk boundary":
        put(c - 1, 3 * c + 1)                                        # all of two chunks and a day on either side
        put(7 * c - 1, 7 * c + 1)
    elif kind == "crosses a wavefront boundary":
        put(LANES * c - 2, LANES * c + 3, -127)
        put(2 * LANES * c - c - 1, 3 * LANES * c + 2)                # a whole wavefront's days and more
    elif kind == "two equal longest runs":
        n = max(nd // 5, 1)
        put(1, 1 + n)
        put(nd - 1 - n, nd - 1, 2)
        put(nd // 2, nd // 2 + max(n - 1, 0))
    elif kind == "random 0.5":
        f[:] = rs.rand(nd) < 0.5
    elif kind == "random 0.9 with -127":
        f[:] = np.where(rs.rand(nd) < 0.9, np.where(rs.rand(nd) < 0.2, -127, 1), 0)
    elif kind == "single day":
        put(nd // 2, nd // 2 + 1)
    elif kind == "alternating":
        f[::2] = 1
    return f


def select_case(nd, ns=None, seed=0, first_kind=0):
    """(tair, tinf, flag, kinds) of ``ns`` rows (default: one per kind) of ``nd`` days, the kinds in rotation from
    ``first_kind``; NaN / +-Inf / the fill value sit in both sources, so in the chosen and in the unchosen one."""
    rs = np.random.RandomState(1000 * nd + seed)
    ns = len(FLAG_KINDS) if ns is None else ns
    kinds = [FLAG_KINDS[(first_kind + i) % len(FLAG_KINDS)] for i in range(ns)]
    flag = np.array([flag_row(k, nd, rs) for k in kinds], np.int8)
    tair = (rs.randn(ns, nd) * 9).astype(np.float32)
    tinf = (tair + rs.randn(ns, nd).astype(np.float32)).astype(np.float32)
    bad = (np.nan, np.inf, -np.inf, FILL)
    for i in range(ns):
        for k, v in enumerate(bad):
            d = rs.randint(nd, size=2)
            (tair if (i + k) % 2 else tinf)[i, d[0]] = v
            if (i + k) % 3 == 0:
                tair[i, d[1]] = tinf[i, d[1]] = bad[(k + 1) % 4]
    tair[0, 0] = -0.0                                                # bit for bit: the sign of a zero survives
    return tair, tinf, flag, kinds


def thresholds_of(flag, row):
    """run_threshold in {1, 5, max_run, max_run + 1} of the designated row (0 is raised to 1: a threshold of 0 makes every
    row all model, which the first entry covers)."""
    m = RS.max_run(flag[row])
    return sorted({1, 5, max(m, 1), m + 1})


def simple_groups(nd, ngroups=12):
    """Synthetic contiguous groups on an axis of ``nd`` days: sizes 0 .. 31 in rotation, the first day skipped, one group
    without a day; the axis may end before the groups do (those have no day)."""
    first, n = np.zeros(ngroups, np.int32), np.zeros(ngroups, np.int32)
    at = 1
    for g in range(ngroups):
        size = 0 if g % 5 == 3 else (28 + (g * 7) % 4 if nd >= 400 else 1 + g % 3)
        if at + size > nd:
            size = 0
        first[g], n[g] = at if size else 0, size
        at += size + (g % 2)                                         # a gap after every second group
    return first, n


def long_case():
    """Three rows of 25 203 days with runs of 1825, 1826 and 1827 days (threshold 1826), each across chunk and wavefront
    boundaries (c = 99)."""
    rs = np.random.RandomState(25203)
    nd = LONG_ND
    flag = (rs.rand(3, nd) < 0.3).astype(np.int8)
    for i, (a, n) in enumerate(((6300, 1825), (99 * 64 - 900, 1826), (nd - 1827, 1827))):
        flag[i, a - 1:a + n + 1] = 0
        flag[i, a:a + n] = 1
    for i in range(3):                                               # no other run comes near
        assert RS.max_run(flag[i]) == 1825 + i
    tair = (rs.randn(3, nd) * 9).astype(np.float32)
    tinf = (tair + 1).astype(np.float32)
    tair[1, 5], tinf[1, 5], tinf[2, 9], tair[0, 11] = np.nan, FILL, np.inf, FILL
    return tair, tinf, flag


def calendar_case():
    """The normals on a real calendar: 1979 .. 1986, 14 stations, normals of 1981-1984.  Station 0 is complete; station 1
    has 0 .. 11 missing days in the months of 1981 and again, shifted, in 1983; station 2 misses all of June 1982; station 3
    has 12 missing days in every February (masked in every year at max_miss 9); station 4 is all fill; the rest are random
    with a tenth of the days NaN / fill."""
    from topowx_amd.dates import MONTH, YEAR, get_days_metadata
    days = get_days_metadata(dt.date(1979, 1, 1), dt.date(1986, 12, 31))
    rs = np.random.RandomState(8184)
    ns, nd = 14, days.size
    x = (rs.randn(ns, nd) * 10 + 5).astype(np.float32)

    def dof(y, m):
        return np.nonzero((days[YEAR] == y) & (days[MONTH] == m))[0]

    for m in range(1, 13):
        d = dof(1981, m)
        x[1, d[rs.permutation(d.size)[:m - 1]]] = FILL
        d = dof(1983, m)
        x[1, d[rs.permutation(d.size)[:(m + 5) % 12]]] = np.nan
    x[2, dof(1982, 6)] = FILL
    for y in range(1979, 1987):
        x[3, dof(y, 2)[:12]] = np.nan
    x[4] = FILL
    miss = rs.rand(ns - 5, nd)
    x[5:][miss < 0.05] = np.nan
    x[5:][miss > 0.95] = FILL
    return days, x


# ---- entry B ----
def check_series(n, seed=17):
    """(names, series [ns, n] float32) of the kinds of entry B at N = n."""
    rs = np.random.RandomState(seed * 100003 + n)
    names, rows = [], []

    def add(name, v):
        names.append(name)
        rows.append(np.asarray(v, np.float32))

    base = (3.0 + rs.randn(n)).astype(np.float32)
    add("iid", base)
    if n in (3, 4, 5):
        add("constant", np.full(n, 3.0))
    taus = []
    for t in (2, n // 2, n - 2):
        if 2 <= t <= n - 2 and t not in taus:
            taus.append(t)
    for t in taus:
        v = rs.randn(n)
        v *= np.where((np.arange(n) < t) == (t <= n // 2), STEP, 1.0)
        add("step at %d" % t, 3.0 + v)
    hi, lo = np.float32(57.7), np.float32(-89.4)                     # float32(57.7) widens to 57.700000762...: above the record
    for name, val in (("nearest float32 to 57.7", hi), ("just above 57.7", np.nextafter(hi, np.float32(np.inf))),
                      ("just below 57.7", np.nextafter(hi, np.float32(0))), ("nearest float32 to -89.4", lo),
                      ("just above -89.4", np.nextafter(lo, np.float32(0)))):
        v = base.copy()
        v[int(rs.randint(n))] = val
        add(name, v)
    for name, val in (("a NaN", np.nan), ("an infinity", np.inf), ("a fill", FILL)):
        v = base.copy()
        v[int(rs.randint(n))] = val
        add(name, v)
    return names, np.array(rows, np.float32)


CONSTANT_N = 186                   # chkperf_cases.degenerate_series: at this N the first tau is the smallest robustly


def expected_impossible(name):
    return {"nearest float32 to 57.7": 1, "just above 57.7": 1, "just below 57.7": 0, "nearest float32 to -89.4": 1,
            "just above -89.4": 0}.get(name)


# ---- the end-to-end pool ----
E2E_IDS = ("S000", "S001", "S002", "S003", "S004", "S005", "S006", "S007")
E2E_HOT, E2E_JUMP, E2E_GAP, E2E_FAILED = 2, 4, 5, 7


def e2e_pool(seed=5):
    """8 stations, 1979 .. 1986.  Returns (days, ids, lon, lat, obs [2, nd, ns] with NaN = missing, reports): ``reports`` is
    a dict var -> the arrays of a step16 ``--chk-perf`` report.  Station E2E_HOT has a planted 60 C model day (its January
    items are reported non-optimal with an impossible value); station E2E_JUMP has no observation in the second half, where its model is
    four times as noisy (its items are reported with a change point); station E2E_GAP has no observation for six years; station E2E_FAILED's June
    item has a status other than ok and NaN there."""
    from topowx_amd import _qalib
    from topowx_amd.dates import MONTH, YMD, get_days_metadata
    days = get_days_metadata(dt.date(1979, 1, 1), dt.date(1986, 12, 31))
    rs = np.random.RandomState(seed)
    ns, nd = len(E2E_IDS), days.size
    ids = np.array(E2E_IDS)
    lon, lat = -110.0 + 0.1 * np.arange(ns), 45.0 + 0.05 * np.arange(ns)
    doy = np.arange(nd) % 365.25
    obs, reports = np.zeros((2, nd, ns), np.float32), {}
    for v, var in enumerate(("tmin", "tmax")):
        truth = (8.0 * v + 2.0 - 11.0 * np.cos(2 * np.pi * doy / 365.25))[None, :] + rs.randn(ns, nd) * 3.0
        model = truth + rs.randn(ns, nd) * 0.7
        model[E2E_JUMP, nd // 2:] += rs.randn(nd - nd // 2) * 12.0
        mask = rs.rand(ns, nd) < 0.1
        mask[E2E_GAP, 300:300 + 6 * 365] = True
        mask[E2E_JUMP, nd // 2:] = True                              # no observation in the second half: the series IS the model there
        mask[E2E_JUMP, nd // 2 - 1] = False
        jan = np.nonzero(days[MONTH] == 1)[0]
        hot = jan[~mask[E2E_HOT, jan]][3]                            # an observed day: only the all-model series shows it...
        mask[E2E_HOT, hot] = True                                    # ...so make it an infilled one
        if var == "tmax":
            model[E2E_HOT, hot] = 60.0
        fnl = np.where(mask, model, truth)
        status = np.zeros((ns, 12), np.int32)
        nonopt, attempt = np.zeros((ns, 12), bool), np.zeros((ns, 12), np.int32)
        reasons = np.full((ns, 12, 4), -1, np.int32)
        reasons[:, :, 0] = 0
        if var == "tmax":
            nonopt[E2E_HOT, 0], attempt[E2E_HOT, 0] = True, 2
            reasons[E2E_HOT, 0, :3] = (_qalib.CK_IMPOSSIBLE, _qalib.CK_LOW_PERF, _qalib.CK_IMPOSSIBLE)
        nonopt[E2E_JUMP, :], attempt[E2E_JUMP, :] = True, 3
        reasons[E2E_JUMP] = _qalib.CK_VAR_CHGPT
        nonopt[1, 4] = True                                          # low performance alone: not suspect
        reasons[1, 4] = _qalib.CK_LOW_PERF
        attempt[1, 4] = 1
        if var == "tmin":
            status[E2E_FAILED, 5] = _qalib.PP_NUMERIC
            jun = days[MONTH] == 6
            model[E2E_FAILED, jun] = np.nan
            fnl[E2E_FAILED] = np.where(mask[E2E_FAILED] & jun, np.nan, fnl[E2E_FAILED])
        o = np.where(mask, np.nan, truth)
        obs[v] = o.T.astype(np.float32)
        dif = np.where(mask | np.isnan(model), np.nan, model - truth)
        reports[var] = dict(ids=ids, ymd=np.asarray(days[YMD], np.int32), fnl_tair=fnl, mask_infill=mask, infill_tair=model,
                            mae=np.nanmean(np.abs(dif), axis=1), bias=np.nanmean(dif, axis=1), status=status,
                            nonoptimal=nonopt, attempt=attempt, reasons=reasons)
    return days, ids, lon, lat, obs, reports
