"""Generate tests/golden/golden_homog_v1.npz by EXECUTING the reference's step09-11 lines on a scripted database.  Needs the
reference checkout (``make_golden.REF``) and pandas; the tests only read the fixture.

    python tests/golden/make_golden_homog.py

Executed (read at run time through ``make_golden._slice``, Python-2 ``print`` converted in memory, ``np.bool`` / ``np.float``
/ ``np.int`` aliased, nothing of the text is stored):
  * twx/homog/tobs.py:243-264 (``_tobs_shift_tmax``), a station at a time;
  * twx/utils/util_dates.py:19-203 and twx/utils/util_tair.py:26-158 (``TairAggregate``) through the chunk loop
    twx/db/create_db_all_stations.py:1305-1329 of ``add_monthly_means``, placed under a function header of ours, on
    in-memory stand-ins of the netCDF variables (time-major, masking their fill value on reading as netCDF4 does);
  * twx/db/obs_por.py:28-39 (``_build_a_por_mask``);
  * twx/homog/pha.py:208-290 (``HomogDaily.homog_stn``) as a method of a stand-in object whose attributes are built here as
    ``HomogDaily.__init__`` builds them.  ONE ADAPTATION: ``_parse_pha_adj`` returns the station id as bytes ("<S50"),
    which Python 3 never finds equal to a str, so the stand-in holds the parsed table with that field as str;
  * twx/homog/pha.py:468-593 (``_write_stn_list``, ``_format_stnid``, ``_write_stn_obs_files``, ``_parse_pha_adj``).
RESTATED, NOT EXECUTED: ``add_obs_cnt``'s group-by count (xarray is not available): ``restate_homog.obs_cnt``, an integer
count.  PHA CANNOT BE RUN: its output files (``FLs.r00/<id>.FLs.r00.<var>``, ``pha_adj_<var>.log``,
``corr/*input_not_stnlist``) are written here in the column layout the reference's parsers read; the layout is pinned by
the parsers, not by PHA.  The metadata file's line format is that of pha.py:455.

The inputs are those of tests/homog_cases.py (seeded; the fixture stores them too).  The maker refuses a fixture in which
tests/restate_homog.py differs from the executed reference in any bit.
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

import homog_cases as HC  # noqa: E402
import restate_homog as RH  # noqa: E402

OUT = os.path.join(HERE, "golden_homog_v1.npz")
FILL_F4 = np.float32(9.969209968386869e36)
FILL_I2 = np.int16(-32767)
STN_DTYPE = [("station_id", "U50"), ("latitude", np.float64), ("longitude", np.float64), ("elevation", np.float64),
             ("state", "U2"), ("station_name", "U30")]


class _Var(object):
    """A netCDF4 variable on (time, station_id) with auto-masking."""

    def __init__(self, a, fill):
        self.a, self._FillValue = a, fill

    def __getitem__(self, key):
        return np.ma.masked_equal(self.a[key], self._FillValue)

    def __setitem__(self, key, val):
        self.a[key] = np.ma.filled(val, self._FillValue) if np.ma.isMA(val) else val


class _Qa(object):
    """The qflag variable: masked where a day has NO flag (the empty string is the fill value)."""

    def __init__(self, flagged):
        self.f = flagged

    def __getitem__(self, key):
        f = self.f[key]
        return np.ma.masked_array(np.where(f, "X", ""), mask=~f)


class _Quiet(object):
    def sync(self):
        pass

    def increment(self, n=1):
        pass


def load_reference():
    import make_golden as mg
    from lib2to3 import refactor
    for name, val in (("bool", bool), ("int", int), ("float", float), ("object", object), ("str", str)):
        if name not in vars(np):
            setattr(np, name, val)
    import builtins
    builtins.long = int
    warnings.filterwarnings("ignore", category=DeprecationWarning)
    tool = refactor.RefactoringTool(["lib2to3.fixes.fix_print"])
    tobs = dict(np=np)
    exec(compile("\n" * 242 + mg._slice("twx/homog/tobs.py", 243, 264), "tobs.py", "exec"), tobs)
    dates = {}
    exec(compile(mg._slice("twx/utils/util_dates.py", 19, 203), "util_dates.py", "exec"), dates)
    til = dict(np=np, YEAR=dates["YEAR"], MONTH=dates["MONTH"], get_mth_metadata=dates["get_mth_metadata"])
    exec(compile("\n" * 25 + mg._slice("twx/utils/util_tair.py", 26, 158), "util_tair.py", "exec"), til)
    means = dict(np=np)
    head = "def _means(stns, var_dly, var_dly_qa, var_mthly, var_miss, tagg, max_miss, ds, stchk, chk_size):\n"
    src = str(tool.refactor_string(head + mg._slice("twx/db/create_db_all_stations.py", 1305, 1329), "create_db.py"))
    exec(compile(src, "create_db_all_stations.py", "exec"), means)
    import pandas as pd
    por = dict(np=np, pd=pd)
    exec(compile("\n" * 27 + mg._slice("twx/db/obs_por.py", 28, 39), "obs_por.py", "exec"), por)
    pha = dict(np=np, os=os, datetime=dt.datetime, STN_ID="station_id", LAT="latitude", LON="longitude", YMD=dates["YMD"])
    pha["DTYPE_PHA_ADJ"] = [("station_id", "<S50"), ("ymd_start", int), ("ymd_end", int), ("adj", np.float64)]
    exec(compile("\n" * 467 + mg._slice("twx/homog/pha.py", 468, 593), "pha.py", "exec"), pha)
    cls = "class HomogDaily(object):\n" + mg._slice("twx/homog/pha.py", 208, 290)
    exec(compile(str(tool.refactor_string(cls, "pha.py")), "pha.py", "exec"), pha)
    return tobs, dates, til["TairAggregate"], means["_means"], por, pha


class _Stnda(object):
    def __init__(self, ids, days, rows):
        self.stn_ids, self.days, self.rows = ids, days, rows
        self.stn_idxs = dict((s, i) for i, s in enumerate(ids))

    def load_all_stn_obs_var(self, stn_id, varname):
        return (self.rows[varname][self.stn_idxs[stn_id]].copy(),)


def nan_of(a, fill):
    a = np.array(a, np.float32)
    a[a == fill] = np.nan
    return a


def main():
    tobs_ns, dates, TairAggregate, ref_means, por, pha = load_reference()
    case = HC.db_case()
    ids, ns = case["ids"], case["ids"].size
    days = dates["get_days_metadata"](dt.datetime(HC.START.year, HC.START.month, HC.START.day),
                                      dt.datetime(HC.END.year, HC.END.month, HC.END.day))
    year, month, ymd = (np.asarray(days[dates[k]], np.int32) for k in ("YEAR", "MONTH", "YMD"))
    if not (np.array_equal(year, case["year"]) and np.array_equal(month, case["month"])):
        raise SystemExit("refused: the day axis of homog_cases differs from the reference's")
    rec = dict((k, case[k]) for k in ("ids", "lat", "lon", "elev", "name", "year", "month", "day", "raw_tmin", "raw_tmax",
                                      "flag_tmin", "flag_tmax", "tobs", "hist_ids", "hist_yyyymm"))
    nd = year.size
    # ---- counts (RESTATED) and the executed POR masks ----
    for v in ("tmin", "tmax"):
        cnt = RH.obs_cnt(case["raw_" + v], month, 0, nd - 1)
        rec["cnt_" + v] = cnt
        for yrs in (1, 5):
            rec["por_%s_%d" % (v, yrs)] = np.asarray(por["_build_a_por_mask"](np.ascontiguousarray(cnt.T), yrs), bool)
    # ---- step09: flags applied, Tmax shifted ----
    obs_tmin = np.where(case["flag_tmin"], np.float32(np.nan), case["raw_tmin"]).astype(np.float32)
    obs_tmax = np.where(case["flag_tmax"], np.float32(np.nan), case["raw_tmax"]).astype(np.float32)
    shifted = np.empty_like(obs_tmax)
    for s in range(ns):
        shifted[s] = np.asarray(tobs_ns["_tobs_shift_tmax"](obs_tmax[s].copy(), case["tobs"][s].copy()), np.float32)
    mine, nshift = RH.tobs_shift(obs_tmax, case["tobs"])
    if not np.array_equal(mine.view(np.uint32), shifted.view(np.uint32)):
        raise SystemExit("refused: the restatement's shifted Tmax differs from the reference")
    print("tobs: stations by |S|: %s" % np.bincount(np.minimum(nshift, 3)).tolist())
    rec.update(tobs_tmax=shifted, tobs_nshift=nshift)
    adj_db = dict(tmin=obs_tmin, tmax=shifted)
    # ---- step10: the monthly means through the reference's chunk loop ----
    tagg = TairAggregate(days)
    mths = dates["get_mth_metadata"](int(year[0]), int(year[-1]))
    nm = mths.size
    mf, mn, mymd = RH.month_groups(year, month)
    if not np.array_equal(mymd, np.asarray(mths[dates["YMD"]], np.int32)):
        raise SystemExit("refused: month_groups' ymd differs from get_mth_metadata")
    rec.update(mth_first=mf, mth_ndays=mn, mth_ymd=mymd)
    stns = np.zeros(ns, STN_DTYPE)
    stns["station_id"], stns["latitude"], stns["longitude"] = ids, case["lat"], case["lon"]
    stns["elevation"], stns["station_name"] = case["elev"], case["name"]
    mth = {}
    for v in ("tmin", "tmax"):
        dly = np.where(np.isnan(adj_db[v]), FILL_F4, adj_db[v]).astype(np.float32)
        var_dly = _Var(np.ascontiguousarray(dly.T), FILL_F4)
        var_m = _Var(np.full((nm, ns), FILL_F4, np.float32), FILL_F4)
        var_miss = _Var(np.full((nm, ns), FILL_I2, np.int16), FILL_I2)
        with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter("ignore")
            ref_means(stns, var_dly, _Qa(np.zeros((nd, ns), bool)), var_m, var_miss, tagg, 9, _Quiet(), _Quiet(), 50)
        mean, miss = nan_of(var_m.a.T, FILL_F4), np.ascontiguousarray(var_miss.a.T)
        m2, s2 = RH.monthly_means(adj_db[v], mf, mn, 9)
        if not np.array_equal(miss, s2) or not np.array_equal(mean.view(np.uint32), m2.view(np.uint32)):
            raise SystemExit("refused: the restatement's monthly means of %s differ from the reference (%d means, %d counts)"
                             % (v, int((mean.view(np.uint32) != m2.view(np.uint32)).sum()), int((miss != s2).sum())))
        print("%s: %d means, %d masked, %d ending in .xx5" % (
            v, mean.size, int(np.isnan(mean).sum()),
            int((np.abs(np.float64(mean) * 1000 % 10 - 5) < 1e-3)[~np.isnan(mean)].sum())))
        rec["mth_mean_" + v], rec["mth_miss_" + v] = mean, miss
        mth[v] = (mean, miss, var_m, var_miss)
    # ---- step11 --setup: PHA's input tree, written by the reference ----
    yrs = np.arange(int(year[0]), int(year[-1]) + 1)
    fids = np.array([pha["_format_stnid"](s) for s in ids])
    rec["fmt_ids"] = fids
    with tempfile.TemporaryDirectory() as tmp:
        for v in ("tmin", "tmax"):
            p_list = os.path.join(tmp, "world1_stnlist.%s" % v)
            pha["_write_stn_list"](stns, p_list)
            with open(p_list) as fh:
                rec["stnlist_" + v] = np.array(fh.read())
            p_raw = os.path.join(tmp, "raw_" + v)
            os.mkdir(p_raw)
            tair = np.ma.masked_equal(mth[v][2].a.copy(), FILL_F4)           # the writer scales its argument in place
            pha["_write_stn_obs_files"](stns, tair, yrs, v, p_raw)
            texts = []
            for f in fids:
                with open(os.path.join(p_raw, "%s.raw.%s" % (f, v))) as fh:
                    texts.append(fh.read())
            rec["raw_files_" + v] = np.array(texts)
        rec["metadata_file"] = np.array("".join("  %s %s 1\n" % (pha["_format_stnid"](s), m)
                                                for s, m in zip(case["hist_ids"], case["hist_yyyymm"])))
        # ---- PHA's output, scripted, in the parsers' layout; then step11 --apply ----
        out = HC.pha_output(case, fids, rec["mth_mean_tmin"], rec["mth_mean_tmax"], rec["mth_miss_tmin"],
                            rec["mth_miss_tmax"])
        for v in ("tmin", "tmax"):
            o = out[v]
            rec.update({"fls_files_" + v: np.array(o["fls_text"]), "adj_log_" + v: np.array(o["adj_log"]),
                        "not_stnlist_" + v: np.array(o["not_stnlist"]), "pha_" + v: o["pha"]})
            p_fls = os.path.join(tmp, "FLs_" + v)
            os.mkdir(p_fls)
            for f, text in zip(fids, o["fls_text"]):
                with open(os.path.join(p_fls, "%s.FLs.r00.%s" % (f, v)), "w") as fh:
                    fh.write(text)
            p_log = os.path.join(tmp, "pha_adj_%s.log" % v)
            with open(p_log, "w") as fh:
                fh.write(o["adj_log"])
            adjs = pha["_parse_pha_adj"](p_log)
            rec.update({"adj_ids_" + v: np.array([a.decode() for a in adjs["station_id"]]),
                        "adj_start_" + v: adjs["ymd_start"].astype(np.int32), "adj_end_" + v: adjs["ymd_end"].astype(np.int32),
                        "adj_" + v: adjs["adj"].astype(np.float64)})
            h = pha["HomogDaily"]()
            h.stnda, h.varname, h.path_FLs_data, h.mths = _Stnda(ids, days, adj_db), v, p_fls, mths
            h.mthly_data = np.ma.masked_invalid(np.ascontiguousarray(mth[v][0].T))
            h.miss_data = np.ma.masked_equal(mth[v][3].a, FILL_I2)
            h.pha_adjs = adjs.astype([("station_id", "U50"), ("ymd_start", int), ("ymd_end", int), ("adj", np.float64)])
            h.dly_yrmth_masks = [np.logical_and(days[dates["YEAR"]] == y, days[dates["MONTH"]] == m)
                                 for y in yrs for m in range(1, 13)]
            h.ndays_per_mth = np.array([np.sum(m) for m in h.dly_yrmth_masks], float)
            h.mthly_yr_masks = dict((y, mths[dates["YEAR"]] == y) for y in yrs)
            homog = np.empty((ns, nd), np.float32)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for s, sid in enumerate(ids):
                    homog[s] = np.ma.filled(h.homog_stn(sid), np.nan).astype(np.float32)
            off, st, en, ad = HC.adj_csr(fids, rec["adj_ids_" + v], rec["adj_start_" + v], rec["adj_end_" + v], rec["adj_" + v])
            mine = RH.homog_daily(adj_db[v], mth[v][0], mth[v][1], o["pha"], mymd, mf, mn, off, st, en, ad)
            if mine["status"].any():
                raise SystemExit("refused: the fixture's adjustment lists must be complete and disjoint")
            nbad = int((mine["out"].view(np.uint32) != homog.view(np.uint32)).sum())
            if nbad:
                raise SystemExit("refused: the restatement's homogenised %s differs from the reference on %d days" % (v, nbad))
            touched = ~np.isnan(mine["delta"])
            print("%s: %d months touched (%d by a difference, %d by the adjustment list, %d of those adding 0.0), %d days changed"
                  % (v, int(touched.sum()), int(mine["nchanged"].sum()), int(touched.sum() - mine["nchanged"].sum()),
                     int((touched & (mine["delta"] == 0)).sum()),
                     int((homog.view(np.uint32) != adj_db[v].view(np.uint32)).sum())))
            rec.update({"homog_" + v: homog, "delta_" + v: mine["delta"], "nchanged_" + v: mine["nchanged"]})
    # the raw values are tenths: stored as int16 tenths (NaN as TENTHS_NAN), which homog_cases.load_fixture widens again
    for v in ("tmin", "tmax"):
        raw = rec.pop("raw_" + v)
        rec["raw_tenths_" + v] = HC.to_tenths(raw)
        if not np.array_equal(HC.from_tenths(rec["raw_tenths_" + v]).view(np.uint32), raw.view(np.uint32)):
            raise SystemExit("refused: raw_%s does not survive the int16 tenths" % v)
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
