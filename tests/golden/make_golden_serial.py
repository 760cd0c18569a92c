"""Generate tests/golden/golden_serial_v1.npz by EXECUTING the reference's step18 lines and its step16-log parser on scripted
inputs.  Needs the reference checkout (``make_golden.REF``); the tests only read the fixture.

    python tests/golden/make_golden_serial.py

Executed (read at run time, Python-2 ``print`` converted in memory by ``lib2to3``, ``np.bool`` / ``np.float`` aliased, nothing
of the text is stored):
  * twx/infill/post_infill.py:512-520 (``_runs_of_ones_array``);
  * twx/infill/post_infill.py:113-142, the decision and scrub lines of ``create_serially_complete_db``, placed under a
    function header of ours, on in-memory stand-ins of the netCDF variables that mask their fill value on reading as
    netCDF4 does; the threshold ``USE_ALL_INFILL_THRESHOLD`` is a name of the namespace, so short rows serve;
  * twx/utils/util_dates.py:19-203 and twx/utils/util_tair.py:26-158 (``TairAggregate.__init__``, ``daily_to_mthly``,
    ``daily_to_mthly_norms``) on [ndays, nstn] masked arrays, as ``add_monthly_normals`` (:395-396) calls them;
  * twx/infill/post_infill.py:404-441 (``get_bad_infill_stnids``) on a scripted log.
THE CHANGE-POINT DECISION OF STEP17 IS NOT EXECUTED REFERENCE: R's ``changepoint`` cannot be run; it is the restatement
tests/restate_chkperf.py, as in the chk_perf fixture, and is not part of this file.

The fixture holds two cases.  ``runs_*``: short rows at several thresholds.  ``db_*``: a database of 16 stations over
1979-01-01 .. 1986-12-31 at the reference's threshold of 1826 days, with the normals of 1981-1984 at ``max_miss`` 9 and None.
The maker compares the executed normals with tests/restate_serial.py bit for bit and records the number of entries that
differ (``norm_bits_differ``; the tests fall back to a bound only if it is not 0), and refuses a fixture in which an integer,
a mask or a byte of the serial series differs.
"""
import contextlib
import datetime as dt
import io
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_serial as RS  # noqa: E402

OUT = os.path.join(HERE, "golden_serial_v1.npz")
FILL = RS.FILL_F4
FILL_I1 = np.int8(-127)
RUN_ND = 420
RUN_THRESHOLDS = (1, 5, 30, 31, 420)
DB_NSTN, DB_START, DB_END, NORM_YRS = 16, dt.date(1979, 1, 1), dt.date(1986, 12, 31), (1981, 1984)

LOG = """\
WORKER 3: infilling USC00244558
ERROR: Could not infill USC00241044|array must not contain infs or NaNs
WRITER|USC00244558|tmin|0.8731|-0.0123
ERROR|USW00024033 had nonoptimal infill for tmin using norm07 as the mean even after retries. Reasons: low infill performance|variance change point. MAE:2.31, R2:0.64
ERROR|USC00245761 had nonoptimal infill for tmax using norm01 as the mean even after retries. Reasons: impossible infill values. MAE:0.91, R2:0.93
ERROR|USC00240364 had nonoptimal infill for tmax using norm02 as the mean even after retries. Reasons: low infill performance. MAE:2.20, R2:0.81
ERROR|USW00024033 had nonoptimal infill for tmax using norm08 as the mean even after retries. Reasons: variance change point. MAE:1.10, R2:0.90
ERROR: Could not infill SNOTEL_13C01S|SVD did not converge
Status: 40 of 120 (33.33 %)
"""


class _Var(object):
    """A netCDF4 variable on (time, station_id) with auto-masking: reading masks what equals the fill value."""

    def __init__(self, a, fill):
        self.a, self._FillValue = a, fill

    def __getitem__(self, key):
        return np.ma.masked_equal(self.a[key], self._FillValue)


class _Ds(object):
    def __init__(self, **v):
        self.variables = v


def load_reference():
    import make_golden as mg
    from lib2to3 import refactor
    for name, val in (("bool", bool), ("int", int), ("float", float), ("object", object)):
        if name not in vars(np):
            setattr(np, name, val)
    import builtins
    builtins.long = int
    warnings.filterwarnings("ignore", category=DeprecationWarning)
    tool = refactor.RefactoringTool(["lib2to3.fixes.fix_print"])
    post = dict(np=np, STN_ID="station_id", NONOPTIM_IMPOSS_VAL="impossible infill values",
                NONOPTIM_VARI_CHGPT="variance change point")
    exec(compile("\n" * 511 + mg._slice("twx/infill/post_infill.py", 512, 520), "post_infill.py", "exec"), post)
    exec(compile("\n" * 403 + mg._slice("twx/infill/post_infill.py", 404, 441), "post_infill.py", "exec"), post)
    head = "def _station(x, ds_infill, ds_out, tair_var, stns, all_infill_flags, all_infill_stns):\n    if True:\n"
    tail = "        return tair_stn, flag_stn, max_infill\n"
    src = str(tool.refactor_string(head + mg._slice("twx/infill/post_infill.py", 113, 142) + tail, "post_infill.py"))
    exec(compile(src, "post_infill.py", "exec"), post)
    dates = {}
    exec(compile(mg._slice("twx/utils/util_dates.py", 19, 203), "util_dates.py", "exec"), dates)
    til = dict(np=np, YEAR=dates["YEAR"], MONTH=dates["MONTH"], get_mth_metadata=dates["get_mth_metadata"])
    exec(compile("\n" * 25 + mg._slice("twx/utils/util_tair.py", 26, 158), "util_tair.py", "exec"), til)
    return post, dates, til["TairAggregate"]


def run_decision(post, tair, tinf, flag, threshold):
    """The executed lines on station-major inputs: (serial [ns, nd] f4, flag_out [ns, nd] i1, max_run, all_infill)."""
    ns, nd = tair.shape
    ds_infill = _Ds(tmin=_Var(np.ascontiguousarray(tair.T), FILL), tmin_infilled=_Var(np.ascontiguousarray(tinf.T), FILL),
                    flag_infilled=_Var(np.ascontiguousarray(flag.T), FILL_I1))
    ds_out = _Ds(tmin=_Var(np.zeros((nd, ns), np.float32), FILL))
    stns = {"station_id": np.array(["S%03d" % i for i in range(ns)])}
    post["USE_ALL_INFILL_THRESHOLD"] = threshold
    all_flags, all_stns = np.ones(nd, dtype=bool), np.zeros(ns, dtype=bool)
    serial, fout, runs = np.empty((ns, nd), np.float32), np.empty((ns, nd), np.int8), np.empty(ns, np.int32)
    for x in range(ns):
        tair_stn, flag_stn, runs[x] = post["_station"](x, ds_infill, ds_out, "tmin", stns, all_flags, all_stns)
        # what assigning to the output variables stores: masked values as the fill value; the flag as 0 / 1 of its DATA (a
        # masked -127 is an infilled day for the run and, per include/twx_qa.h, in flag_infilled too)
        serial[x] = np.ma.filled(tair_stn, FILL).astype(np.float32)
        fout[x] = np.asarray(np.ma.getdata(flag_stn)).astype(bool).astype(np.int8)
    return serial, fout, runs, all_stns


def runs_case():
    rs = np.random.RandomState(1718)
    nd = RUN_ND
    rows = []

    def row(flag):
        rows.append(np.asarray(flag, np.int8))

    z = np.zeros(nd, np.int8)
    row(z)                                                           # no infilled day
    row(np.ones(nd))                                                 # all infilled
    row(np.full(nd, -127))                                           # all -127
    for a, b in ((nd - 30, nd), (0, 30), (100, 131), (100, 130), (7, 12), (0, 1), (nd - 1, nd)):
        f = z.copy()
        f[a:b] = 1
        row(f)
    f = z.copy()
    f[10:40] = 1
    f[200:230] = 1                                                   # two equal longest runs
    f[300:310] = -127
    row(f)
    f = z.copy()
    f[50:70] = 1
    f[70:81] = -127                                                  # a run of 31 through the int8 fill
    row(f)
    for p in (0.3, 0.7, 0.95):
        row(rs.rand(nd) < p)
    flag = np.array(rows)
    ns = flag.shape[0]
    tair = np.round(rs.randn(ns, nd) * 8, 2).astype(np.float32)
    tinf = (tair + np.round(rs.randn(ns, nd), 2)).astype(np.float32)
    for a, vals in ((tair, (np.nan, np.inf, -np.inf, FILL)), (tinf, (np.nan, FILL, np.inf, -np.inf))):
        for k, v in enumerate(vals):                                 # in the chosen and in the unchosen source
            a[:, 3 + 5 * k] = v
            a[k::4, 200 + k] = v
    return tair, tinf, flag


def db_case(days_year, days_month):
    """16 stations x 1979-1986: fnl / model / flag as ``write_infill_db`` stores them (missing = the fill value)."""
    rs = np.random.RandomState(1819)
    ns, nd = DB_NSTN, days_year.size
    doy = np.arange(nd) % 365.25
    clim = (5.0 - 12.0 * np.cos(2 * np.pi * doy / 365.25))[None, :] + rs.randn(ns, 1) * 3
    truth = clim + rs.randn(ns, nd) * 4
    model = np.round(truth + rs.randn(ns, nd) * 0.8, 2).astype(np.float32)
    flag = (rs.rand(ns, nd) < 0.12).astype(np.int8)
    for s, (a, b) in {1: (400, 400 + 6 * 365), 2: (0, 1826), 4: (1000, 2825), 5: (1096, 2922), 6: (30, 1857)}.items():
        flag[s] = 0
        flag[s, a:b] = 1                                             # gaps of 2190, 1826, 1825, 1826, 1827 days
    fnl = np.where(flag != 0, model, np.round(truth, 2).astype(np.float32)).astype(np.float32)

    def days_of(y, m):
        return np.nonzero((days_year == y) & (days_month == m))[0]

    s = 3                                                            # months of 1981 with 0 .. 10 missing days, then 11
    for m in range(1, 13):
        d = days_of(1981, m)
        fnl[s, d[rs.permutation(d.size)[:m - 1]]] = FILL
        model[s, d[:2]] = FILL                                       # the unchosen source
    fnl[7, days_of(1982, 6)] = FILL                                  # a month that is wholly missing
    for y in range(1979, 1987):
        fnl[8, days_of(y, 2)[:12]] = FILL                            # February masked in every year
    flag[9] = FILL_I1                                                # a station that failed the infill: all model, all fill
    fnl[9], model[9] = FILL, FILL
    model[5, 17] = FILL                                              # an all-model station with a missing model day
    d = days_of(1983, 3)
    fnl[10, d[:9]] = FILL                                            # exactly max_miss, and one more the year after
    fnl[10, days_of(1984, 3)[:10]] = FILL
    return fnl, model, flag


def main():
    post, dates, TairAggregate = load_reference()
    rec = {}
    # ---- the runs, the decision, the scrub ----
    tair, tinf, flag = runs_case()
    rec.update(runs_tair=tair, runs_tinf=tinf, runs_flag=flag, runs_thresholds=np.array(RUN_THRESHOLDS, np.int32))
    ser, fo, ai = [], [], []
    for t in RUN_THRESHOLDS:
        with contextlib.redirect_stdout(io.StringIO()):
            serial, fout, runs, allst = run_decision(post, tair, tinf, flag, t)
        mine = RS.serial_complete(tair, tinf, flag, run_threshold=t, fill=FILL)
        for name, a, b in (("max_run", runs, mine["max_run"]), ("all_infill", allst, mine["all_infill"]),
                           ("flag_out", fout, mine["flag_infilled"]), ("serial", serial.view(np.uint32), mine["serial"].view(np.uint32))):
            if not np.array_equal(a, b):
                raise SystemExit("refused: the restatement's %s differs from the reference at threshold %d" % (name, t))
        ser.append(serial); fo.append(fout); ai.append(allst)
        rec["runs_max_run"] = runs
        print("threshold %4d: %2d of %d rows all model, longest runs %s" % (t, allst.sum(), allst.size, runs.tolist()))
    rec.update(runs_serial=np.array(ser), runs_flag_out=np.array(fo), runs_all_infill=np.array(ai))
    # ---- the database and its normals ----
    days = dates["get_days_metadata"](dt.datetime(DB_START.year, 1, 1), dt.datetime(DB_END.year, 12, 31))
    year, month = np.asarray(days[dates["YEAR"]], np.int32), np.asarray(days[dates["MONTH"]], np.int32)
    fnl, model, dflag = db_case(year, month)
    with contextlib.redirect_stdout(io.StringIO()):
        serial, fout, runs, allst = run_decision(post, fnl, model, dflag, RS.RUN_THRESHOLD)
    gf, gn = RS.norm_groups(year, month, *NORM_YRS)
    rec.update(db_fnl=fnl, db_model=model, db_flag=dflag, db_year=year, db_month=month, db_serial=serial, db_flag_out=fout,
               db_max_run=runs, db_all_infill=allst, db_norm_yrs=np.array(NORM_YRS, np.int32), db_group_first=gf, db_group_ndays=gn)
    tagg = TairAggregate(days)
    differ = 0
    for key, max_miss in (("9", 9), ("none", None)):
        mine = RS.serial_complete(fnl, model, dflag, fill=FILL, group_first=gf, group_ndays=gn, max_miss=max_miss)
        if key == "9":
            for name, a, b in (("max_run", runs, mine["max_run"]), ("all_infill", allst, mine["all_infill"]),
                               ("flag_out", fout, mine["flag_infilled"]),
                               ("serial", serial.view(np.uint32), mine["serial"].view(np.uint32))):
                if not np.array_equal(a, b):
                    raise SystemExit("refused: the restatement's %s differs from the reference on the database" % name)
        dly_vals = np.ma.masked_equal(np.ascontiguousarray(serial.T), FILL)      # add_monthly_normals:395
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            norm_vals = tagg.daily_to_mthly_norms(dly_vals, NORM_YRS[0], NORM_YRS[1], max_miss=max_miss)
            mthly = tagg.daily_to_mthly(dly_vals, max_miss=max_miss)[0]
        norm = np.ma.filled(np.ma.masked_invalid(np.ma.asarray(norm_vals, dtype=float)), np.nan).T
        sel = np.nonzero((tagg.yr_mths[dates["YEAR"]] >= NORM_YRS[0]) & (tagg.yr_mths[dates["YEAR"]] <= NORM_YRS[1]))[0]
        unmasked = ~np.ma.getmaskarray(mthly)[sel]                    # [48, nstn]
        nm = np.array([unmasked[m::12].sum(axis=0) for m in range(12)], np.int32).T
        if not np.array_equal(nm, mine["norm_nmths"]) or not np.array_equal(np.isnan(norm), np.isnan(mine["norm"])):
            raise SystemExit("refused: the restatement's masks of the normals differ from the reference (max_miss %s)" % key)
        d = int((norm.view(np.uint64) != mine["norm"].view(np.uint64))[~np.isnan(norm)].sum())
        differ += d
        print("max_miss %s: %d normals, %d masked, %d not bit-equal to the restatement, largest |difference| %.3g" % (
            key, norm.size, int(np.isnan(norm).sum()), d, float(np.nanmax(np.abs(norm - mine["norm"])))))
        rec["db_norm_" + key], rec["db_nmths_" + key] = norm, nm
    rec["norm_bits_differ"] = np.int32(differ)
    # ---- the log parser ----
    with tempfile.NamedTemporaryFile("w", suffix=".log", delete=False) as fh:
        fh.write(LOG)
    try:
        ids = post["get_bad_infill_stnids"](fh.name)
    finally:
        os.unlink(fh.name)
    rec.update(log=np.array(LOG), log_ids=np.array([str(s) for s in ids]))
    print("log: %s" % rec["log_ids"].tolist())
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
