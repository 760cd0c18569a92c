"""GPU: step08's spatial regression check (``twxqa_spatial_regress`` of libtwxqa, ``topowx_amd.qa``) against the
executed-reference golden (tests/golden/make_golden_spatial.py) and the numpy restatement (tests/restate_spatial.py),
its edge cases and per-item statuses, and the step08 driver end to end on NetCDF station databases.

Flags, NaN positions, valid-neighbour counts and statuses are compared exactly; that is fair because every comparison
first asserts, on the checker's own values, that r, the tested residuals and the tested standardised residuals stay
100 x TOL away from their thresholds (a failure there is a failure of the test's input, not of the GPU)."""
import datetime as dt
import json
import os
import sys

import numpy as np
import pytest

from topowx_amd import _qalib, ncio
from topowx_amd import stationdb as sdb
from topowx_amd.dates import YMD
from topowx_amd.qa import QA_MISSING, QA_OK, QA_SPATIAL_REGRESS, StationObsPool, qa_spatial_regress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from spatial_cases import FORMATS, TOL  # noqa: E402  (shared by both spatial test files)

pytestmark = pytest.mark.gpu


def _ymd(days, y, m, d):
    return int(np.nonzero(days[YMD] == y * 10000 + m * 100 + d)[0][0])


def _compare(pool, want, targets=None):
    """Run the pool through ``qa_spatial_regress`` and compare everything with a restatement result ``want``."""
    assert (want["margins"][:3] > 100 * TOL).all(), "input too close to a threshold: %r" % (want["margins"],)
    assert want["margins"][3] > 1e-6, "a station pair too close to the 75 km radius"
    f_tmin, f_tmax, det = qa_spatial_regress(pool, targets, details=True)
    for v, (got, obs) in enumerate(((f_tmin, pool.tmin), (f_tmax, pool.tmax))):
        cols = slice(None) if targets is None else [pool.idxs[s] for s in targets]
        assert got.shape == want["flags"][v].shape and got.dtype == np.uint8
        assert np.array_equal(got == QA_SPATIAL_REGRESS, want["flags"][v])
        assert np.array_equal(got == QA_MISSING, np.isnan(obs[:, cols]))
        assert np.isin(got, (QA_OK, QA_MISSING, QA_SPATIAL_REGRESS)).all()
    assert np.array_equal(np.isnan(det["est"]), np.isnan(want["est"]))
    d_est = float(np.nanmax(np.abs(det["est"] - want["est"]))) if np.isfinite(want["est"]).any() else 0.0
    assert np.array_equal(np.isnan(det["r"]), np.isnan(want["r"]))
    d_r = float(np.nanmax(np.abs(det["r"] - want["r"]))) if np.isfinite(want["r"]).any() else 0.0
    print("max |est - want| %.3g degC, max |r - want| %.3g" % (d_est, d_r))
    assert d_est < TOL and d_r < TOL
    assert np.array_equal(det["nvalid"], want["nvalid"])
    assert np.array_equal(det["status"], want["status"])
    return f_tmin, f_tmax, det


# ---- the executed reference -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_spatial_v1.npz"))


@pytest.fixture(scope="module")
def gold_pool(gold):
    import make_golden_spatial as mgs
    c = mgs.case_inputs()
    assert mgs.input_hash(*c[:6]) == str(gold["input_hash"])
    return StationObsPool(*c[:6])


def test_golden_through_the_c_abi(gold, gold_pool):
    p = gold_pool
    tm = {}
    fmin, fmax, det = _qalib.spatial_regress(p.lon, p.lat, p.tmin.T, p.tmax.T, p.days[YMD], np.arange(p.ids.size),
                                             details=True, timing=tm)
    assert tm["radius_kernel_ms"] > 0 and tm["regress_kernel_ms"] > 0
    # flags equal the executed reference's for every station, day and variable
    assert np.array_equal(fmin.T != 0, gold["flags_tmin"] == 16) and np.array_equal(fmax.T != 0, gold["flags_tmax"] == 16)
    assert (fmin != 0).sum() == (gold["flags_tmin"] == 16).sum() > 100
    # est on every day the reference estimated, identical NaN positions; per-item r; the valid-neighbour counts
    assert np.array_equal(np.isnan(det["est"]), np.isnan(gold["est"]))
    assert np.nanmax(np.abs(det["est"] - gold["est"])) < TOL
    assert np.array_equal(np.isnan(det["r"]), np.isnan(gold["r"]))
    assert np.nanmax(np.abs(det["r"] - gold["r"])) < TOL
    reached = gold["nvalid"] >= 0
    assert np.array_equal(det["nvalid"][reached], gold["nvalid"][reached])
    assert (det["nvalid"][~reached] == 0).all()
    assert set(np.unique(det["status"][~reached]).tolist()) == {_qalib.SP_FEW_NGHS, _qalib.SP_FEW_DAYS}
    assert (det["status"][np.isfinite(gold["r"])] == _qalib.SP_OK).all()
    assert (det["status"][p.ids.size - 1] == _qalib.SP_FEW_NGHS).all()
    # without details the flags are the same
    f2 = _qalib.spatial_regress(p.lon, p.lat, p.tmin.T, p.tmax.T, p.days[YMD], np.arange(p.ids.size))
    assert np.array_equal(f2[0], fmin) and np.array_equal(f2[1], fmax)


def test_golden_through_qa_spatial_regress(gold, gold_pool):
    f_tmin, f_tmax = gold_pool.qa_spatial_regress()
    assert np.array_equal(f_tmin, gold["flags_tmin"]) and np.array_equal(f_tmax, gold["flags_tmax"])
    # the spikes on the first and on the last day of the series
    assert f_tmin[0, 3] == QA_SPATIAL_REGRESS and f_tmin[-1, 11] == QA_SPATIAL_REGRESS


def test_target_subset_equals_rows_of_the_full_run(gold, gold_pool):
    p = gold_pool
    sub = [p.ids[i] for i in (31, 0, 39, 7, 12)]
    f_tmin, f_tmax, det = qa_spatial_regress(p, sub, details=True)
    cols = [p.idxs[s] for s in sub]
    assert np.array_equal(f_tmin, gold["flags_tmin"][:, cols]) and np.array_equal(f_tmax, gold["flags_tmax"][:, cols])
    full = qa_spatial_regress(p, details=True)[2]
    for k in ("est", "r", "nvalid", "status"):
        assert np.array_equal(det[k], full[k][cols], equal_nan=True), k


# ---- the large synthetic case against the restatement ---------------------------------------------------------------
def test_two_thousand_stations_ten_years_equal_the_restatement():
    import restate_spatial as R
    import spatial_cases
    ids, lon, lat, tmin, tmax, days, spikes = spatial_cases.big_case()
    assert ids.size == 2000 and days.size == 3653
    want = R.run(lon, lat, tmin, tmax, days[YMD], cap=_qalib.MAX_RADIUS_NGH)
    pool = StationObsPool(ids, lon, lat, tmin, tmax, days)
    f_tmin, _, det = _compare(pool, want)
    planted = np.zeros(f_tmin.shape, bool)
    planted[spikes[:, 1], spikes[:, 0]] = True
    flagged = f_tmin == QA_SPATIAL_REGRESS
    assert flagged.sum() > 1000 and (flagged & planted).sum() > 0.95 * flagged.sum()
    assert (det["status"] == _qalib.SP_OK).mean() > 0.8


# ---- edge cases -------------------------------------------------------------------------------------------------
N_CLUSTER = 20
TIE_TARGET, TIE_DAY = 8, (2000, 3, 15)
GAP_TARGET, CONST_TARGET = 2, 5


@pytest.fixture(scope="module")
def edge():
    """24 stations, 1999-12-20 .. 2001-02-10 (a series that starts and ends inside a month, a leap February, two year
    ends): 20 clustered, one alone, a far pair and one near the pair; a target with a four-month gap; every
    clustered station but one constant in Tmax over the October 2000 window; a day on which every clustered
    neighbour of one target is missing with its previous and next day equidistant from the target's observation."""
    import restate_spatial as R
    import spatial_cases
    ids, lon, lat, tmin, tmax, days, spikes = spatial_cases.synthetic_pool(
        24, dt.date(1999, 12, 20), dt.date(2001, 2, 10), (45.0, 45.4, -110.0, -109.5), 5, spikes_per_stn=4, gap_every=0)
    lon[20], lat[20] = -100.0, 47.0                            # alone
    lon[21:24], lat[21:24] = (-104.0, -103.9, -103.95), (41.0, 41.05, 41.1)      # two neighbours each
    tmin[_ymd(days, 2000, 5, 1):_ymd(days, 2000, 9, 1), GAP_TARGET] = np.nan
    a, b = _ymd(days, 2000, 9, 10), _ymd(days, 2000, 11, 20)
    for s in range(N_CLUSTER):
        if s != CONST_TARGET:
            tmax[a:b, s] = np.where(np.isnan(tmax[a:b, s]), np.nan, np.float32(12.5))
    x = _ymd(days, *TIE_DAY)
    tmin[x, TIE_TARGET] = 5.0
    for s in range(N_CLUSTER):
        if s != TIE_TARGET:
            tmin[x - 1, s], tmin[x, s], tmin[x + 1, s] = 4.0, np.nan, 6.0
    tmin[0, 1] += np.float32(15.0)                             # spikes on the first and the last day of the series
    tmin[-1, 4] -= np.float32(15.0)
    pool = StationObsPool(ids, lon, lat, tmin, tmax, days)
    want = R.run(lon, lat, tmin, tmax, days[YMD], cap=_qalib.MAX_RADIUS_NGH)
    f_tmin, f_tmax, det = _compare(pool, want)
    return dict(pool=pool, want=want, f_tmin=f_tmin, f_tmax=f_tmax, det=det, ws_we=R.month_table(days[YMD]))


def _month(days, y, m):
    return (y * 12 + m - 1) - (int(days.YEAR[0]) * 12 + int(days.MONTH[0]) - 1)


def test_edge_targets_with_fewer_than_three_neighbours(edge):
    det = edge["det"]
    for s in (20, 21, 22, 23):
        assert (det["status"][s] == _qalib.SP_FEW_NGHS).all() and (det["nvalid"][s] == 0).all()
        assert np.isnan(det["r"][s]).all() and np.isnan(det["est"][s]).all()
        assert not (edge["f_tmin"][:, s] == QA_SPATIAL_REGRESS).any()
    assert (det["status"][:N_CLUSTER] != _qalib.SP_FEW_NGHS).all()


def test_edge_item_with_fewer_than_forty_window_days(edge):
    det, days = edge["det"], edge["pool"].days
    for m in (6, 7):                                           # June, July 2000 lie inside the gap with their windows
        assert det["status"][GAP_TARGET, 0, _month(days, 2000, m)] == _qalib.SP_FEW_DAYS
    assert det["status"][GAP_TARGET, 1, _month(days, 2000, 6)] == _qalib.SP_OK          # Tmax has no gap
    assert det["status"][GAP_TARGET, 0, _month(days, 2000, 2)] == _qalib.SP_OK
    # the first and last month of the series: 12 + 15 and 10 + 15 days in the window
    assert (det["status"][:N_CLUSTER, :, 0] == _qalib.SP_FEW_DAYS).all()
    assert (det["status"][:N_CLUSTER, :, -1] == _qalib.SP_FEW_DAYS).all()


def test_edge_all_neighbours_constant(edge):
    det, days = edge["det"], edge["pool"].days
    m = _month(days, 2000, 10)
    assert det["status"][CONST_TARGET, 1, m] == _qalib.SP_FEW_VALID and det["nvalid"][CONST_TARGET, 1, m] == 0
    # a constant target has no valid neighbour either (its own overlap values are one value)
    others = [s for s in range(N_CLUSTER) if s != CONST_TARGET]
    assert (det["status"][others, 1, m] == _qalib.SP_FEW_VALID).all()
    assert (det["status"][:N_CLUSTER, 0, m] == _qalib.SP_OK).sum() >= N_CLUSTER - 1       # Tmin is untouched
    ms, me = edge["ws_we"][2][m], edge["ws_we"][3][m]
    assert np.isnan(det["est"][CONST_TARGET, 1, ms:me]).all()


def test_edge_argmin_tie_takes_the_previous_day(edge):
    """Every neighbour is missing on the day, its previous day lies 1.0 below and its next day 1.0 above the target's
    observation: np.argmin takes the first, the previous day (qa_temp.py:898-904)."""
    import restate_spatial as R
    p, det = edge["pool"], edge["det"]
    x, m = _ymd(p.days, *TIE_DAY), _month(p.days, *TIE_DAY[:2])
    o = R.check_station(p.tmin, p.days[YMD], TIE_TARGET, R.neighbours(p.lon, p.lat, TIE_TARGET))
    w, a, b = (o[k][:7, m] for k in ("w", "slope", "icpt"))
    assert np.isfinite(w).all()
    prev = float(np.sum((b + a * 4.0) * w) / np.sum(w))
    nxt = float(np.sum((b + a * 6.0) * w) / np.sum(w))
    assert abs(prev - nxt) > 1.0
    assert abs(det["est"][TIE_TARGET, 0, x] - prev) < TOL


def test_edge_first_and_last_day_of_the_series(edge):
    """Day 0 has no previous and the last day no next day; both lie in months with too few window days here, so the
    reference checks neither (the golden case holds flagged spikes on both ends)."""
    p, det = edge["pool"], edge["det"]
    assert edge["f_tmin"][0, 1] == QA_OK and edge["f_tmin"][-1, 4] == QA_OK
    # the January 2000 window starts on series day 0 and the January 2001 window ends on the last day
    ws, we = edge["ws_we"][0], edge["ws_we"][1]
    assert ws[1] == 0 and we[-2] == p.days.size
    for m in (1, ws.size - 2):
        assert (det["status"][:N_CLUSTER, 0, m] == _qalib.SP_OK).all()


def test_edge_leap_february_and_year_end_windows(edge):
    """February 2000 has 29 days; the December and January windows cross a year end: estimates on every day of
    those months (compared with the restatement in the fixture) and items that are ok."""
    p, det = edge["pool"], edge["det"]
    ws, we, ms, me = edge["ws_we"]
    feb = _month(p.days, 2000, 2)
    assert me[feb] - ms[feb] == 29 and we[feb] - ws[feb] == 59
    assert p.days[YMD][ws[feb]] == 20000117 and p.days[YMD][we[feb] - 1] == 20000315
    for y, mth in ((2000, 2), (2000, 12), (2000, 1), (2001, 1)):
        m = _month(p.days, y, mth)
        assert (det["status"][:N_CLUSTER, :, m] == _qalib.SP_OK).all()
        got = det["est"][0, 0, ms[m]:me[m]]
        assert np.isfinite(got).sum() >= 0.8 * (me[m] - ms[m])
    dec = _month(p.days, 2000, 12)
    assert p.days[YMD][ws[dec]] == 20001116 and p.days[YMD][we[dec] - 1] == 20010115


def test_neighbour_cap_status():
    """A target with more than TWXQA_MAX_RADIUS_NGH stations within 75 km says so on every item and flags nothing;
    a target below the cap in the same call is checked as usual."""
    import restate_spatial as R
    import spatial_cases
    n = _qalib.MAX_RADIUS_NGH + 10
    ids, lon, lat, tmin, tmax, days, _ = spatial_cases.synthetic_pool(
        n + 6, dt.date(2000, 1, 1), dt.date(2000, 4, 30), (45.0, 45.2, -110.0, -109.8), 9, spikes_per_stn=1)
    lon[n:], lat[n:] = -100.0 + 0.05 * np.arange(6), 40.0 + 0.03 * np.arange(6)      # six stations far away
    pool = StationObsPool(ids, lon, lat, tmin, tmax, days)
    want = R.run(lon, lat, tmin, tmax, days[YMD], cap=_qalib.MAX_RADIUS_NGH)
    f_tmin, f_tmax, det = _compare(pool, want)
    assert (det["status"][:n] == _qalib.SP_NGH_CAP).all() and (det["nvalid"][:n] == 0).all()
    assert not (f_tmin[:, :n] == QA_SPATIAL_REGRESS).any() and np.isnan(det["est"][:n]).all()
    assert (det["status"][n:, :, 1:3] == _qalib.SP_OK).all() and (det["nvalid"][n:, :, 1:3] == 5).all()
    # exactly at the cap the list is used
    keep = np.r_[0:_qalib.MAX_RADIUS_NGH + 1]
    sub = StationObsPool(ids[keep], lon[keep], lat[keep], tmin[:, keep], tmax[:, keep], days)
    st = qa_spatial_regress(sub, [ids[0]], details=True)[2]["status"]
    assert not (st == _qalib.SP_NGH_CAP).any() and (st == _qalib.SP_OK).any()


def test_degenerate_items_flag_nothing():
    """Identical neighbours: the estimate equals the observation, r is 1 and the window residuals have no spread --
    the reference divides by zero there (step08 runs under np.seterr(all='raise')); the item says degenerate."""
    import restate_spatial as R
    import spatial_cases
    ids, lon, lat, tmin, tmax, days, _ = spatial_cases.synthetic_pool(
        6, dt.date(2000, 1, 1), dt.date(2000, 6, 30), (45.0, 45.2, -110.0, -109.8), 11, spikes_per_stn=0, miss=0.0,
        gap_every=0)
    tmin[:], tmax[:] = tmin[:, :1], tmax[:, :1]
    pool = StationObsPool(ids, lon, lat, tmin, tmax, days)
    want = R.run(lon, lat, tmin, tmax, days[YMD])
    f_tmin, f_tmax, det = qa_spatial_regress(pool, details=True)
    assert np.array_equal(det["status"], want["status"])
    assert (det["status"][:, :, 1:5] == _qalib.SP_DEGENERATE).all()
    assert np.allclose(det["r"][:, :, 1:5], 1.0, atol=TOL, rtol=0)
    assert (f_tmin == QA_OK).all() and (f_tmax == QA_OK).all()


# ---- the driver -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_step08_driver_end_to_end(tmp_path, capsys, gold, gold_pool, fmt):
    from topowx_amd import step08
    p = gold_pool
    n = p.ids.size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = p.ids, p.lon, p.lat, 1000.0
    db = str(tmp_path / ("all_%s.nc" % fmt))
    ncio.create_quick_db(db, stns, p.days, [("tmin", "f4", ncio.FILL_F4, "minimum air temperature", "C"),
                                            ("tmax", "f4", ncio.FILL_F4, "maximum air temperature", "C")], format=fmt)
    ds = ncio.open_dataset(db, "a")
    for name, a in (("tmin", p.tmin), ("tmax", p.tmax)):
        v = ds.variables[name]
        v.missing_value = np.float32(ncio.FILL_F4)
        v[:] = np.where(np.isnan(a), np.float32(ncio.FILL_F4), a)
    ds.close()
    before = open(db, "rb").read()
    out = str(tmp_path / "report.npz")
    assert step08.main(["--db", db, "--out", out]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["stations"] == n and rec["items"] == n * 2 * 36
    assert rec["flags_tmin"] == int((gold["flags_tmin"] == 16).sum()) and rec["flags_tmax"] == int((gold["flags_tmax"] == 16).sum())
    assert rec["seconds"] > 0 and rec["regress_kernel_ms"] > 0 and rec["radius_kernel_ms"] > 0
    rep = np.load(out)
    assert np.array_equal(rep["flags_tmin"], gold["flags_tmin"]) and np.array_equal(rep["flags_tmax"], gold["flags_tmax"])
    assert np.array_equal(rep["ymd"], p.days[YMD]) and rep["ids"].tolist() == p.ids.tolist()
    assert open(db, "rb").read() == before                      # nothing is written into the database
    # a target list
    tfile = tmp_path / "targets.txt"
    tfile.write_text("%s\n%s\n\n" % (p.ids[11], p.ids[3]))
    assert step08.main(["--db", db, "--out", out, "--targets", str(tfile)]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    rep = np.load(out)
    assert rec["stations"] == 2 and rec["pool"] == n and rep["ids"].tolist() == [p.ids[11], p.ids[3]]
    assert np.array_equal(rep["flags_tmin"], gold["flags_tmin"][:, [11, 3]])
    tfile.write_text("NOT_AN_ID\n")
    assert step08.main(["--db", db, "--out", out, "--targets", str(tfile)]) == 1
    assert step08.main(["--db", str(tmp_path / "missing.nc"), "--out", out]) == 1
