"""GPU: step17 / step18 -- the kernels of ``twxsc_serial_complete`` and ``twxsc_series_check`` against the numpy restatements
(tests/restate_serial.py, tests/restate_chkperf.py) and the executed-reference golden, through the bindings, the Python layer
and the two command lines.

Entry A: every integer, mask and byte of ``serial`` exact; the normals within 128 x 2^-53 x max |x| of the restatement (two
orders of summing <= 31 + 30 terms plus two divisions cannot differ by more) -- the kernel adds in the restatement's order
without contraction, so every test prints how many entries are not bit-equal and 0 is expected.  Entry B: tests/
test_gpu_chkperf.py's rules, imported: cpt_tau, nimpossible, reasons and status exact, cpt_stat
within 100 x the float64-to-longdouble distance of the restatement on that series with the floor N^2 2^-52, after the
series' runner-up tmp and its cpt_stat - pen margin were checked to lie above that tolerance.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chkperf_cases as CC  # noqa: E402
import restate_chkperf as RC  # noqa: E402
import restate_serial as RS  # noqa: E402
import serial_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu


def same_select(got, want, what, full=True):
    for name in ("max_run", "nmissing", "all_infill"):
        assert np.array_equal(got[name], want[name]), (what, name, got[name], want[name])
    if full:
        assert np.array_equal(got["flag_infilled"], want["flag_infilled"]), (what, "flag_infilled")
        assert got["serial"].tobytes() == want["serial"].tobytes(), (what, "serial")
        assert np.array_equal(got["serial"] == SC.FILL, want["miss"]), (what, "missing positions")


def same_norms(got, want, xmax, what):
    """The normals against the restatement: masks and counts exact, values within the bound; returns the number of entries
    that are not bit-equal."""
    assert np.array_equal(got["norm_nmths"], want["norm_nmths"]), (what, "norm_nmths")
    assert np.array_equal(np.isnan(got["norm"]), np.isnan(want["norm"])), (what, "masked normals")
    ok = ~np.isnan(want["norm"])
    dev = np.abs(np.where(ok, got["norm"] - want["norm"], 0.0))
    bound = SC.NORM_BOUND * np.asarray(xmax, np.float64)[:, None]
    assert (dev <= bound).all(), (what, float(dev.max()), float(bound.min()))
    nbits = int((got["norm"].view(np.uint64) != want["norm"].view(np.uint64))[ok].sum())
    print("%s: %d normals, %d not bit-equal to the restatement, largest deviation %.3g" % (what, int(ok.sum()), nbits, float(dev.max())))
    return nbits


def xmax_of(serial_rows, gf, gn, fill=SC.FILL):
    """max |x| over each station's non-missing days in its groups (0 if there is none)."""
    inside = np.zeros(serial_rows.shape[1], bool)
    for a, n in zip(gf, gn):
        inside[a:a + n] = True
    x = np.where(RS.missing(serial_rows, fill) | ~inside[None, :], 0.0, np.abs(serial_rows.astype(np.float64)))
    return x.max(axis=1)


@pytest.mark.parametrize("nd", SC.SELECT_NDAYS)
def test_select_against_the_restatement(nd):
    """Every kind of row at every length, run_threshold in {1, 5, max_run, max_run + 1} of the row whose run crosses a
    wavefront boundary (of the first row with a run where that one has none), with synthetic groups."""
    from topowx_amd import _qalib
    tair, tinf, flag, kinds = SC.select_case(nd)
    row = kinds.index("crosses a wavefront boundary")
    if RS.max_run(flag[row]) == 0:
        row = kinds.index("all")
    gf, gn = SC.simple_groups(nd)
    nbits = 0
    for t in SC.thresholds_of(flag, row):
        want = RS.serial_complete(tair, tinf, flag, run_threshold=t, group_first=gf, group_ndays=gn, max_miss=2)
        got = _qalib.serial_complete(tair, tinf, flag, run_threshold=t, group_first=gf, group_ndays=gn, max_miss=2)
        same_select(got, want, "ndays %d threshold %d" % (nd, t))
        nbits += same_norms(got, want, xmax_of(want["serial"], gf, gn), "ndays %d threshold %d" % (nd, t))
        assert got["batches"] == 1
    m = RS.max_run(flag[row])
    assert _qalib.serial_complete(tair, tinf, flag, run_threshold=m)["all_infill"][row]
    assert not _qalib.serial_complete(tair, tinf, flag, run_threshold=m + 1)["all_infill"][row]
    assert want["max_run"][kinds.index("none")] == 0 and want["max_run"][kinds.index("all -127")] == nd
    assert nbits == 0


@pytest.mark.parametrize("ns,first_kind", [(1, 5), (1, 6), (3, 2), (3, 6)])
def test_select_few_series(ns, first_kind):
    from topowx_amd import _qalib
    for nd in (257, 513):
        tair, tinf, flag, kinds = SC.select_case(nd, ns, seed=ns, first_kind=first_kind)
        for t in SC.thresholds_of(flag, 0):
            same_select(_qalib.serial_complete(tair, tinf, flag, run_threshold=t),
                        RS.serial_complete(tair, tinf, flag, run_threshold=t), "%d series of %d days from kind %d" % (ns, nd, first_kind))


def test_select_300_series_in_batches():
    """300 series in several workspace batches equal the one-batch bytes and the restatement; with normals."""
    from topowx_amd import _qalib
    nd = 513
    tair, tinf, flag, kinds = SC.select_case(nd, 300, seed=3)
    gf, gn = SC.simple_groups(nd)
    kw = dict(run_threshold=40, group_first=gf, group_ndays=gn, max_miss=3)
    one = _qalib.serial_complete(tair, tinf, flag, **kw)
    tm = {}
    many = _qalib.serial_complete(tair, tinf, flag, workspace_bytes=37 * nd * 14, timing=tm, **kw)
    assert one["batches"] == 1 and many["batches"] == 9
    times = [k + "_kernel_ms" for k in _qalib.SC_KERNELS] + [k + "_ms" for k in _qalib.SC_HOST_TIMES]
    assert tm["sc_batches"] == 9 and all(np.isfinite(tm[k]) and tm[k] >= 0 for k in times), tm
    want = RS.serial_complete(tair, tinf, flag, **kw)
    same_select(one, want, "300 series")
    for name in ("serial", "flag_infilled", "max_run", "nmissing", "all_infill", "norm", "norm_nmths"):
        assert one[name].tobytes() == many[name].tobytes(), name
    assert same_norms(one, want, xmax_of(want["serial"], gf, gn), "300 series") == 0
    assert 0 < want["all_infill"].sum() < 300


def test_select_long_rows():
    """25 203 days, run_threshold 1826: runs of 1825, 1826 and 1827 days."""
    from topowx_amd import _qalib
    tair, tinf, flag = SC.long_case()
    got = _qalib.serial_complete(tair, tinf, flag)
    same_select(got, RS.serial_complete(tair, tinf, flag), "25 203 days")
    assert got["max_run"].tolist() == [1825, 1826, 1827] and got["all_infill"].tolist() == [False, True, True]
    assert got["nmissing"].tolist() == [1, 1, 1]


def test_forms_without_flags_and_without_normals():
    """Normals only (no flag, no tair_infilled: the row is tair as it is) and no normals."""
    from topowx_amd import _qalib
    nd = 4097
    tair, tinf, flag, kinds = SC.select_case(nd)
    gf, gn = SC.simple_groups(nd)
    got = _qalib.serial_complete(tair, group_first=gf, group_ndays=gn, max_miss=1)
    want = RS.serial_complete(tair, group_first=gf, group_ndays=gn, max_miss=1)
    same_select(got, want, "normals only", full=False)
    assert "serial" not in got and not got["all_infill"].any() and (got["max_run"] == 0).all()
    src = np.where(want["miss"], SC.FILL, tair)
    assert same_norms(got, want, xmax_of(src, gf, gn), "normals only") == 0
    plain = _qalib.serial_complete(tair, tinf, flag, run_threshold=7)
    assert "norm" not in plain
    same_select(plain, RS.serial_complete(tair, tinf, flag, run_threshold=7), "no normals")


def test_normals_on_a_calendar():
    """Groups with 0 .. 11 missing days around max_miss = 9, max_miss = -1 / None, a month that is wholly missing, a month
    masked in every year, a station that is all fill; ngroups = 12, 48 and the cap (most of whose groups have no day)."""
    from topowx_amd import _qalib
    from topowx_amd.dates import DAY, MONTH, YEAR
    days, x = SC.calendar_case()
    nbits = 0
    for (y0, y1), max_miss in (((1981, 1984), 9), ((1981, 1984), None), ((1981, 1984), -1), ((1981, 1984), 0), ((1982, 1982), 9),
                               ((1960, 1960 + _qalib.SC_MAX_GROUPS // 12 - 1), 9)):
        gf, gn = _qalib.norm_groups(days[YEAR], days[MONTH], y0, y1, day=days[DAY])
        got = _qalib.serial_complete(x, group_first=gf, group_ndays=gn, max_miss=max_miss)
        want = RS.serial_complete(x, group_first=gf, group_ndays=gn, max_miss=max_miss)
        what = "normals %d-%d max_miss %s" % (y0, y1, max_miss)
        same_select(got, want, what, full=False)
        nbits += same_norms(got, want, xmax_of(np.where(want["miss"], SC.FILL, x), gf, gn), what)
        if (y0, y1) == (1981, 1984):
            nm = got["norm_nmths"]
            assert (nm[0] == 4).all() and (nm[4] == 0).all() and np.isnan(got["norm"][4]).all()
            if max_miss == 9:
                # 1981: m - 1 missing days in month m (10, 11 in m = 11, 12); 1983: (m + 5) % 12 (10, 11 in m = 5, 6)
                assert nm[1].tolist() == [4, 4, 4, 4, 3, 3, 4, 4, 4, 4, 3, 3] and nm[2, 5] == 3 and nm[3, 1] == 0
                assert np.isnan(got["norm"][3, 1]) and (nm[3, [0, 2, 5]] == 4).all()
            elif max_miss == 0:
                assert nm[1, 0] == 3 and nm[1, 1] == 2 and nm[1, 6] == 3
            else:
                assert (nm[1] == 4).all() and nm[2, 5] == 3 and nm[3, 1] == 4
        if y0 == 1960:
            assert gf.size == _qalib.SC_MAX_GROUPS and (gn > 0).sum() == 96 and (got["norm_nmths"][0] == 8).all()
        if y0 == 1982:
            assert gf.size == 12 and np.isnan(got["norm"][2, 5]) and got["norm_nmths"][2, 5] == 0
    assert nbits == 0


# ---- entry B ----
def compare_series(res, k, want, n, what, tie_ok=False):
    """Series ``k`` of a library result against its ``RS.series_check`` record, by test_gpu_chkperf.compare's rules."""
    assert np.isfinite(want["d_cpt"]), (what, "float64 and longdouble decide differently")
    tc = CC.tolerances(want, n)[2]
    assert want["tmp_gap"] > 2 * n * n * CC.U or (tie_ok and want["tmp_gap"] == 0.0), (what, want["tmp_gap"])
    assert not want["margins"].get("cpt", np.inf) <= tc / abs(want["pen"]), (what, want["margins"]["cpt"], tc)
    for name in ("nimpossible", "nmissing", "status", "cpt_tau"):
        assert res[name][k] == want[name], (what, name, res[name][k], want[name])
    assert res["reasons"][k] == want["reasons"] & ~RC.LOW_PERF, (what, res["reasons"][k], want["reasons"])
    got, ref = float(res["cpt_stat"][k]), float(want["cpt_stat"])
    if np.isnan(ref) or np.isinf(ref):
        assert (np.isnan(got) and np.isnan(ref)) or got == ref, (what, got, ref)
        return 0.0
    dev = abs(got - ref)
    print("%s cpt_stat: deviation %.3g, bound %.3g" % (what, dev, tc))
    assert dev <= tc, (what, got, ref, dev, tc)
    return dev / tc


@pytest.fixture(scope="module")
def checks():
    """Per N: (names, series, restatement records at the default penalty), computed once."""
    out = {}
    for n in SC.CHECK_N:
        names, series = SC.check_series(n)
        pen = RC.cpt_penalty(n)
        out[n] = (names, series, [RS.series_check(s, pen) for s in series])
    return out


@pytest.mark.parametrize("n", SC.CHECK_N)
def test_series_check_against_the_restatement(checks, n):
    from topowx_amd import _qalib
    names, series, wants = checks[n]
    tm = {}
    res = _qalib.series_check(series, timing=tm)
    assert (np.isnan(res["pen"]) and np.isnan(RC.cpt_penalty(n))) or res["pen"] == RC.cpt_penalty(n)
    assert tm["sc_series_kernel_ms"] > 0 and res["batches"] == 1
    worst = 0.0
    for k, name in enumerate(names):
        what = "N %d %s" % (n, name)
        worst = max(worst, compare_series(res, k, wants[k], n, what, tie_ok=name == "constant"))
        imp = SC.expected_impossible(name)
        if imp is not None:
            assert res["nimpossible"][k] == imp and bool(res["reasons"][k] & RC.IMPOSSIBLE) == bool(imp), what
        if name in ("a NaN", "an infinity", "a fill"):
            assert res["status"][k] == RC.NOT_FITTED and res["reasons"][k] == RC.UNFITTED and res["nmissing"][k] == 1, what
            assert np.isnan(res["cpt_stat"][k]) and res["cpt_tau"][k] == 0
        elif n < 4:
            assert res["status"][k] == RC.FEW_ROWS and np.isnan(res["cpt_stat"][k]), what
        else:
            assert res["status"][k] == RC.OK, what
        if name == "constant" and n >= 4:
            assert res["cpt_stat"][k] == -np.inf and res["cpt_tau"][k] == 2 and not res["reasons"][k] & RC.VAR_CHGPT
        if name.startswith("step at") and n >= 255:
            t = int(name.split()[-1])
            if 64 <= t <= n - 64:
                assert abs(int(res["cpt_tau"][k]) - t) <= 8, what     # found where it was put; at the level 1e-10 ...
                assert n < 8192 or res["reasons"][k] & RC.VAR_CHGPT, what     # ... a long series also passes the penalty
    print("N %d: %d series, largest deviation / bound %.3g, kernel %.3f ms" % (n, len(names), worst, tm["sc_series_kernel_ms"]))


def test_series_check_constant_and_penalties(checks):
    """A constant series at the N where the first tau wins robustly; a NaN penalty and a low one on the same rows."""
    from topowx_amd import _qalib
    n = SC.CONSTANT_N
    const = np.full((1, n), 3.0, np.float32)
    res = _qalib.series_check(const)
    w = RS.series_check(const[0], RC.cpt_penalty(n))
    compare_series(res, 0, w, n, "constant N %d" % n, tie_ok=True)
    assert res["cpt_stat"][0] == -np.inf and res["cpt_tau"][0] == 2 and res["reasons"][0] == 0
    names, series, wants = checks[8193]
    base = _qalib.series_check(series)
    nan = _qalib.series_check(series, pen=np.nan)
    low = _qalib.series_check(series, pen=1.0)
    assert not (nan["reasons"] & RC.VAR_CHGPT).any() and nan["cpt_stat"].tobytes() == base["cpt_stat"].tobytes()
    fitted = base["status"] == RC.OK
    assert (low["reasons"][fitted] & RC.VAR_CHGPT).all() and not (low["reasons"][~fitted] & RC.VAR_CHGPT).any()
    loose = _qalib.series_check(series, sig=0.5)
    assert loose["pen"] < base["pen"] and loose["cpt_tau"].tobytes() == base["cpt_tau"].tobytes()


@pytest.mark.parametrize("n", [k for k in SC.CHECK_N if k <= 8192])
def test_the_two_kernels_agree(checks, n):
    """``series_check`` and ``infill_check`` (the float32 series widened, no observation) on the same series: equal cpt_tau,
    nimpossible and change-point bit; cpt_stat within the sum of both tolerances."""
    from topowx_amd import _qalib
    names, series, wants = checks[n]
    a = _qalib.series_check(series)
    wide = series.astype(np.float64)
    off = np.arange(series.shape[0] + 1, dtype=np.int64) * n
    b = _qalib.infill_check(off, wide.ravel(), np.full(wide.size, np.nan))
    nbits = 0
    for k, name in enumerate(names):
        if name == "a fill":                                         # finite for infill_check, missing for series_check
            assert a["status"][k] == RC.NOT_FITTED and b["status"][k] in (RC.OK, RC.FEW_ROWS)
            continue
        assert a["status"][k] == b["status"][k] and a["cpt_tau"][k] == b["cpt_tau"][k], (n, name)
        assert a["nimpossible"][k] == b["nimpossible"][k], (n, name)
        assert (a["reasons"][k] & RC.VAR_CHGPT) == (b["reasons"][k] & RC.VAR_CHGPT), (n, name)
        x, y = a["cpt_stat"][k], b["cpt_stat"][k]
        if np.isnan(x) or np.isinf(x):
            assert (np.isnan(x) and np.isnan(y)) or x == y, (n, name)
            continue
        assert abs(x - y) <= 2 * CC.tolerances(wants[k], n)[2], (n, name, x, y)
        nbits += x.tobytes() != y.tobytes()
    print("N %d: %d of %d cpt_stat values not bit-equal between the two kernels" % (n, nbits, len(names)))


def test_both_entries_repeat_their_bytes(checks):
    from topowx_amd import _qalib
    names, series, wants = checks[25203]
    a, b = _qalib.series_check(series), _qalib.series_check(series)
    c = _qalib.series_check(series, workspace_bytes=3 * 25203 * 4)
    assert a["batches"] == 1 and c["batches"] == -(-len(names) // 3)
    for name in ("nimpossible", "nmissing", "cpt_stat", "cpt_tau", "reasons", "status"):
        assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes(), name
    tair, tinf, flag = SC.long_case()
    from topowx_amd.dates import DAY, MONTH, YEAR, get_days_metadata
    import datetime as dt
    days = get_days_metadata(dt.date(1948, 1, 1), dt.date(2016, 12, 31))
    assert days.size == SC.LONG_ND
    gf, gn = _qalib.norm_groups(days[YEAR], days[MONTH], 1981, 2010, day=days[DAY])
    r = [_qalib.serial_complete(tair, tinf, flag, group_first=gf, group_ndays=gn, workspace_bytes=w) for w in (0, 0, 1)]
    assert r[2]["batches"] == 3
    for name in ("serial", "flag_infilled", "max_run", "nmissing", "all_infill", "norm", "norm_nmths"):
        assert r[0][name].tobytes() == r[1][name].tobytes() == r[2][name].tobytes(), name
    want = RS.serial_complete(tair, tinf, flag, group_first=gf, group_ndays=gn)
    assert same_norms(r[0], want, xmax_of(want["serial"], gf, gn), "25 203 days, 1981-2010") == 0
    assert (r[0]["norm_nmths"] == 30).all()


# ---- the Python layer and the command lines ----
def _stns(ids, lon=-110.0, lat=45.0):
    from topowx_amd import stationdb as sdb
    stns = np.empty(len(ids), dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = ids, lon, lat, 100.0
    return stns


@pytest.mark.parametrize("fmt", ["NETCDF3_64BIT", None])
def test_executed_reference_golden_through_the_databases(tmp_path, capsys, fmt):
    """``write_infill_db`` -> ``create_serially_complete_db`` -> ``add_monthly_normals`` on the fixture's database: the
    serial file read back through ``ncio.read_station_db`` has <var>, flag_infilled and norm01 .. norm12 of the executed
    reference."""
    import datetime as dt
    from topowx_amd import ncio
    from topowx_amd.dates import get_days_metadata
    from topowx_amd.infill import add_monthly_normals, create_serially_complete_db, write_infill_db
    from topowx_amd.stationdb import StationSerialDataDb, get_norm_varname
    gold = SC.load_gold()
    days = get_days_metadata(dt.date(1979, 1, 1), dt.date(1986, 12, 31))
    assert np.array_equal(days["YEAR"], gold["db_year"]) and np.array_equal(days["MONTH"], gold["db_month"])
    ns = gold["db_fnl"].shape[0]
    ids = np.array(["G%03d" % i for i in range(ns)])
    unfill = lambda a: np.where(a == SC.FILL, np.nan, a.astype(np.float64))      # noqa: E731  (a step16 report holds NaN)
    rep = dict(ids=ids, fnl_tair=unfill(gold["db_fnl"]), infill_tair=unfill(gold["db_model"]), mask_infill=gold["db_flag"] != 0,
               mae=np.full(ns, 0.5), bias=np.zeros(ns))
    a, c = str(tmp_path / "infill_tmax.nc"), str(tmp_path / "serial_tmax.nc")
    write_infill_db(a, _stns(ids), days, "tmax", rep, format=fmt)
    rec = create_serially_complete_db(a, "tmax", c, format=fmt, norm_yrs=(1981, 1984))
    out = capsys.readouterr().out
    assert out.count("has missing values even after infill") == int((rec.nmissing > 0).sum()) == 6
    assert "Warning: Station G009 has missing values even after infill. Ensure station is flagged as bad." in out
    assert "% of stns with all infilled values: 31.25" in out
    assert np.array_equal(rec.all_infill, gold["db_all_infill"])
    # write_infill_db stores flags as 0 / 1: station 9's -127 became 1 and its run is the same
    assert np.array_equal(rec.max_run, gold["db_max_run"])
    stnda = StationSerialDataDb(c, "tmax", mode="r+")
    try:
        norm, nm = add_monthly_normals(stnda, 1981, 1984)
    finally:
        stnda.close()
    with pytest.raises(FileExistsError):
        create_serially_complete_db(a, "tmax", c)
    back = ncio.read_station_db(c, "tmax")
    assert back.stn_ids.tolist() == ids.tolist() and back.days.size == days.size
    got = np.ascontiguousarray(back.var.T)
    assert got.tobytes() == gold["db_serial"].tobytes()
    ds = ncio.open_dataset(c, "r")
    try:
        assert np.array_equal(np.asarray(ds.variables["flag_infilled"][:]).T, gold["db_flag_out"])
        assert ds.variables["flag_infilled"].dtype == np.int8 and ds.variables["tmax"].dtype == np.float32
        assert ds.variables["norm07"].long_name == "1981 - 1984 Monthly Normal" and ds.variables["norm07"].units == "C"
    finally:
        ds.close()
    table = np.array([back.stns[get_norm_varname(m)] for m in range(1, 13)]).T
    for got_norm in (norm, rec.norm, table):
        assert np.array_equal(np.isnan(got_norm), np.isnan(gold["db_norm_9"]))
        ok = ~np.isnan(got_norm)
        bound = SC.NORM_BOUND * xmax_of(gold["db_serial"], gold["db_group_first"], gold["db_group_ndays"])[:, None]
        assert (np.abs(np.where(ok, got_norm - gold["db_norm_9"], 0.0)) <= bound).all()
    nbits = int((norm.view(np.uint64) != gold["db_norm_9"].view(np.uint64))[~np.isnan(norm)].sum())
    print("golden database: %d normals not bit-equal to the executed reference" % nbits)
    assert nbits == 0 and np.array_equal(nm, gold["db_nmths_9"]) and np.array_equal(rec.norm_nmths, gold["db_nmths_9"])


def test_find_bad_infill_stns(tmp_path):
    """One call per variable; an id that a database lacks is not bad for that variable; the order of ``stnids`` is kept."""
    from topowx_amd.infill import find_bad_infill_stns, write_infill_db
    days, ids, lon, lat, obs, reports = SC.e2e_pool()
    a, b = str(tmp_path / "a.nc"), str(tmp_path / "b.nc")
    write_infill_db(a, _stns(ids), days, "tmin", reports["tmin"])
    sub = dict(reports["tmax"], **{k: reports["tmax"][k][:6] for k in ("ids", "fnl_tair", "mask_infill", "infill_tair", "mae", "bias")})
    write_infill_db(b, _stns(ids), days, "tmax", sub)               # S006, S007 have no Tmax
    order = ["S007", "S004", "S000", "S002", "S006"]
    tm = {}
    bad, det = find_bad_infill_stns(a, b, order, timing=tm)
    assert bad == ["S007", "S004", "S002"] and tm["sc_series_calls"] == 2
    assert det["tmax"]["present"].tolist() == [False, True, True, True, False] and det["tmin"]["present"].all()
    assert det["tmin"]["nmissing"][0] > 0 and det["tmin"]["status"][0] == RC.NOT_FITTED and not det["tmax"]["bad"][0]
    assert det["tmax"]["nimpossible"][3] == 1 and det["tmin"]["nimpossible"][3] == 0
    assert (det["tmin"]["reasons"][1] & RC.VAR_CHGPT) and (det["tmax"]["reasons"][1] & RC.VAR_CHGPT)
    assert 0.4 * days.size < det["tmin"]["cpt_tau"][1] < 0.6 * days.size
    assert det["tmin"]["pen"] == RC.cpt_penalty(days.size)
    series = reports["tmin"]["fnl_tair"][4].astype(np.float32)
    w = RS.series_check(series, RC.cpt_penalty(days.size))
    assert det["tmin"]["cpt_tau"][1] == w["cpt_tau"] and abs(det["tmin"]["cpt_stat"][1] - w["cpt_stat"]) <= CC.tolerances(w, days.size)[2]
    assert find_bad_infill_stns(a, b, ["S000", "S001"])[0] == []


def _run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (args, p.stdout, p.stderr)
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_end_to_end_command_lines(tmp_path):
    """Two scripted step16 reports -> ``step17 --report-*`` -> ``step18``, each a fresh child process: the planted 60 C day,
    the planted variance jump and the station whose infill failed land in the csv; the station with a six-year gap is all
    model; ``ncio.read_station_db`` opens the results."""
    import corrob_cases
    from topowx_amd import ncio
    from topowx_amd.stationdb import get_norm_varname
    days, ids, lon, lat, obs, reports = SC.e2e_pool()
    db = corrob_cases.write_db(str(tmp_path / "all.nc"), ids, lon, lat, obs[0], obs[1], days, "NETCDF3_64BIT", qflags=False)
    for var in ("tmin", "tmax"):
        np.savez_compressed(str(tmp_path / ("rep_%s.npz" % var)), **reports[var])
    p = {k: str(tmp_path / (k + ".nc")) for k in ("infill_tmin", "infill_tmax", "serial_tmin", "serial_tmax")}
    csv = str(tmp_path / "flagged_bad.csv")
    line, _ = _run(["topowx_amd.step17", "--infill-tmin", p["infill_tmin"], "--infill-tmax", p["infill_tmax"], "--out", csv,
                    "--db", db, "--report-tmin", str(tmp_path / "rep_tmin.npz"), "--report-tmax", str(tmp_path / "rep_tmax.npz")])
    assert open(csv).read() == "station_id,reason\nS002,infill issue\nS004,infill issue\nS007,infill issue\n"
    assert line["suspects"] == 3 and line["bad"] == 3 and line["tmin"]["checked"] == 3 and line["tmax"]["impossible"] == 1
    assert line["tmin"]["chgpt"] >= 1 and line["tmin"]["missing"] == 1 and line["sc_series_calls"] == 2
    line, err = _run(["topowx_amd.step18", "--infill-tmin", p["infill_tmin"], "--infill-tmax", p["infill_tmax"],
                      "--serial-tmin", p["serial_tmin"], "--serial-tmax", p["serial_tmax"], "--start-norm-yr", "1981",
                      "--end-norm-yr", "1984"])
    assert "Station S007 has missing values even after infill" in err and "% of stns with all infilled values: 12.5" in err
    assert line["tmin"] == {"stations": 8, "days": days.size, "all_infill": 1, "with_missing": 1, "normals": 96, "no_normal": 0}
    assert line["tmax"]["with_missing"] == 0 and line["sc_calls"] == 4
    for var in ("tmin", "tmax"):
        back = ncio.read_station_db(p["serial_" + var], var)
        assert back.stn_ids.tolist() == list(ids) and back.var.shape == (days.size, 8)
        ds, src = ncio.open_dataset(p["serial_" + var], "r"), ncio.open_dataset(p["infill_" + var], "r")
        try:
            flag = np.asarray(ds.variables["flag_infilled"][:])
            model, fnl = np.asarray(src.variables[var + "_infilled"][:]), np.asarray(src.variables[var][:])
            g = SC.E2E_GAP
            assert (flag[:, g] == 1).all() and back.var[:, g].tobytes() == model[:, g].tobytes()
            assert not np.array_equal(fnl[:, g], model[:, g])
            for s in range(8):
                if s != g:
                    assert back.var[:, s].tobytes() == fnl[:, s].tobytes(), (var, s)
                    assert np.array_equal(flag[:, s], np.asarray(src.variables["flag_infilled"][:])[:, s])
        finally:
            ds.close()
            src.close()
        norm = np.array([back.stns[get_norm_varname(m)] for m in range(1, 13)]).T
        want = RS.serial_complete(np.ascontiguousarray(back.var.T), group_first=RS.norm_groups(days["YEAR"], days["MONTH"], 1981, 1984)[0],
                                  group_ndays=RS.norm_groups(days["YEAR"], days["MONTH"], 1981, 1984)[1])
        assert np.isfinite(norm).all() and np.abs(norm - want["norm"]).max() <= SC.NORM_BOUND * 60.0
