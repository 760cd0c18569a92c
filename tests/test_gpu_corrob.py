"""GPU: the rest of step08's spatial stage (``twxqa_doy_norms`` and ``twxqa_spatial_only`` of libtwxqa,
``topowx_amd.qa.run_qa_spatial_only``) against the executed-reference golden (tests/golden/make_golden_corrob.py) and the
numpy restatement (tests/restate_corrob.py), its edge cases, and ``python -m topowx_amd.step08 --spatial [--write]`` end
to end on both containers.

Flags are compared exactly and normals to 1e-7 degC with identical NaN positions.  Exact flags are fair because the
checker's own margins are asserted first: the golden maker asserted that every dif the reference looked at lies more
than 1e-5 from the 10.0 cutoff; on the 2 000-station pool the days on which the restatement sees a dif within 1e-5 of
it are left out, and their share of the tested days is capped at 1e-4."""
import datetime as dt
import json
import os
import sys

import numpy as np
import pytest

from topowx_amd import _qalib
from topowx_amd.dates import YMD, get_days_metadata
from topowx_amd.qa import (QA_MEGA_INCONSIST, QA_MISSING, QA_OK, QA_SPATIAL_CORROB, QA_SPATIAL_REGRESS, StationObsPool,
                           doy_norms, qa_spatial_regress, run_qa_spatial_only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from spatial_cases import FORMATS, TOL  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1e-5               # flags are compared where no decision lies closer than this to its threshold
MAX_LEFT_OUT = 1e-4         # share of the tested days the restatement may leave out for that reason


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_corrob_v1.npz"))


@pytest.fixture(scope="module")
def gold_pool(gold):
    import make_golden_corrob as mk
    c = mk.case_inputs()
    assert mk.input_hash(*c[:6]) == str(gold["input_hash"])
    return StationObsPool(*c[:6])


def _close(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN positions"
    d = float(np.nanmax(np.abs(got - want))) if np.isfinite(want).any() else 0.0
    print("%s: max |got - want| %.3g degC over %d values" % (what, d, int(np.isfinite(want).sum())))
    assert d < TOL, what


# ---- the normals --------------------------------------------------------------------------------------------------
def test_doy_norms_equal_the_golden_tables(gold, gold_pool):
    p = gold_pool
    ymd = p.days[YMD]
    # the target tables: the series without the days the regression check flagged
    series = []
    for v, (obs, name) in enumerate(((p.tmin, "reg_tmin"), (p.tmax, "reg_tmax"))):
        a = obs.copy()
        a[gold[name] == 16] = np.nan
        series.append(a.T)
    tm = {}
    got = _qalib.doy_norms(np.concatenate(series), ymd, timing=tm)
    assert tm["kernel_ms"] > 0
    n = p.ids.size
    _close(got[:n], gold["tnorm"][:, 0], "target tables tmin")
    _close(got[n:], gold["tnorm"][:, 1], "target tables tmax")
    # the neighbour tables: the pool as it is; station 7 takes the MAD == 0 branch, station 26 has no normals
    stns = gold["nnorm_stns"]
    for v, obs in enumerate((p.tmin, p.tmax)):
        _close(_qalib.doy_norms(obs[:, stns].T, ymd), gold["nnorm"][:, v], "neighbour tables %d" % v)
    # the public function: [ndays, k] -> ([365, k], [366, k]); a 1-d series
    n365, n366 = doy_norms(p.tmin[:, stns], p.days)
    assert n365.shape == (365, stns.size) and n366.shape == (366, stns.size)
    assert np.array_equal(np.concatenate([n365, n366]).T, _qalib.doy_norms(p.tmin[:, stns].T, ymd), equal_nan=True)
    a365, a366 = doy_norms(p.tmin[:, 1], p.days)
    assert np.array_equal(a365, n365[:, 0], equal_nan=True) and np.array_equal(a366, n366[:, 0], equal_nan=True)


def test_doy_norms_random_series_equal_the_restatement():
    """Even and odd counts, ties (tenths of a degree, and a series of three distinct values), constant series (all
    rows MAD == 0), rows below, exactly at and above the 100-value minimum, a series with a leap-day-only record, +-inf
    read as missing, an all-NaN series."""
    import restate_corrob as RC
    days = get_days_metadata(dt.date(1995, 3, 10), dt.date(2006, 10, 20))
    ymd, nd = days[YMD], days.size
    rs = np.random.RandomState(77)
    t = np.arange(nd)
    base = 8.0 - 12.0 * np.cos(2 * np.pi * t / 365.25)
    S = []
    for k in range(12):                                           # random missing shares: counts of either parity
        a = np.round(base + rs.randn(nd) * (0.3 + k), 1)
        a[rs.rand(nd) < 0.03 * k] = np.nan
        S.append(a)
    S.append(np.full(nd, 3.5))                                    # constant
    c = np.full(nd, -2.0)
    c[rs.rand(nd) < 0.3] = 7.0                                    # two values, most of them equal: MAD == 0, mean != median
    S.append(c)
    S.append(rs.choice([1.0, 2.0, 4.0], nd))                      # heavy ties
    S.append(np.round(rs.randn(nd) * 30, 1))                      # wide
    w = RC.window_table(2003)
    md = np.asarray(ymd) % 10000
    for row, keep in ((181, 100), (181, 99), (181, 101), (40, 100), (59, 100)):      # exactly at / below / above the minimum
        a = np.full(nd, np.nan)
        inwin = np.nonzero(np.isin(md, w[row]))[0]
        a[rs.choice(inwin, keep, replace=False)] = np.round(rs.randn(keep) * 5, 1)
        S.append(a)
    e = np.round(base + rs.randn(nd), 1)
    e[md != 229] = np.nan                                         # Feb 29 only
    S.append(e)
    f = np.round(base + rs.randn(nd), 1)
    f[rs.rand(nd) < 0.1] = np.inf
    f[rs.rand(nd) < 0.1] = -np.inf
    S.append(f)
    S.append(np.full(nd, np.nan))
    S = np.array(S, np.float32)
    got = _qalib.doy_norms(S, ymd)
    want = np.array([RC.doy_norms(s, ymd) for s in S])
    _close(got, want, "random series")
    k0 = 16
    assert np.isfinite(want[k0]).sum() >= 1 and np.isnan(want[k0 + 1]).all() and np.isfinite(want[k0 + 2]).sum() >= 1
    assert np.isfinite(want[k0, 181]) and np.isfinite(want[k0 + 3, 40]) and np.isfinite(want[k0 + 4, 59])
    assert np.allclose(got[12][np.isfinite(got[12])], 3.5, atol=0, rtol=0) and np.isfinite(got[12]).all()
    assert np.isnan(got[-1]).all() and np.isnan(got[-3]).all()
    # a row of the 365 table and its twin of the 366 table: equal bits wherever Feb 29 is in neither window
    twin = np.r_[0:52, 67:366]
    assert np.array_equal(got[:, np.r_[0:52, 66:365]], got[:, 365 + twin], equal_nan=True)
    assert not np.array_equal(got[0, 52:66], got[0, 365 + 53:365 + 67])


# ---- the executed reference ---------------------------------------------------------------------------------------
def test_spatial_only_equals_the_golden_at_every_stage(gold, gold_pool):
    p = gold_pool
    tm = {}
    f_tmin, f_tmax, det = run_qa_spatial_only(p, details=True, timing=tm)
    for k in _qalib.SPATIAL_ONLY_KERNELS:
        assert tm[k + "_kernel_ms"] > 0, k
    r_tmin, r_tmax = qa_spatial_regress(p)
    for got, reg, name in ((f_tmin, r_tmin, "tmin"), (f_tmax, r_tmax, "tmax")):
        assert got.dtype == np.uint8 and got.shape == gold["flags_" + name].shape
        final = gold["flags_" + name]
        print(name, {k: int((got == k).sum()) for k in (1, 2, 16, 17, 18)})
        assert np.array_equal(got, final), name
        # the stages: after the regression check 17 / 18 are still 1, after the corroboration check 18 is
        assert np.array_equal(np.where(np.isin(got, (17, 18)), 1, got), gold["reg_" + name])
        assert np.array_equal(np.where(got == 18, 1, got), gold["cor_" + name])
        # the 16s are what the regression check gives alone
        assert np.array_equal(got == QA_SPATIAL_REGRESS, reg == QA_SPATIAL_REGRESS)
    _close(det["norms"], gold["tnorm"], "target normals")
    import make_golden_corrob as mk
    st = det["status"]
    assert st[mk.ALONE] == _qalib.SP_FEW_NGHS and (np.delete(st, mk.ALONE) == _qalib.SP_OK).all()
    # the empty-list quirk: the long-record target among short-record neighbours is flagged where the counts pass
    assert (f_tmin[:, mk.LONG_TARGET] == QA_SPATIAL_CORROB).sum() > 1000
    assert (f_tmin[:, mk.ALONE] == QA_MEGA_INCONSIST).sum() == 1 and (f_tmax[:, mk.ALONE] == QA_MEGA_INCONSIST).sum() == 1


def test_target_list_in_non_table_order(gold, gold_pool):
    p = gold_pool
    sub = [p.ids[i] for i in (25, 0, 29, 24, 7, 5)]
    cols = [p.idxs[s] for s in sub]
    f_tmin, f_tmax, det = p.run_qa_spatial_only(sub, details=True)
    assert np.array_equal(f_tmin, gold["flags_tmin"][:, cols]) and np.array_equal(f_tmax, gold["flags_tmax"][:, cols])
    _close(det["norms"], gold["tnorm"][cols], "target normals of a subset")
    with pytest.raises(KeyError):
        run_qa_spatial_only(p, ["NOT_AN_ID"])


# ---- the large synthetic case against the restatement ---------------------------------------------------------------
def test_two_thousand_stations_ten_years_equal_the_restatement():
    import corrob_cases
    import restate_corrob as RC
    ids, lon, lat, tmin, tmax, days, _ = corrob_cases.big_case()
    assert ids.size == 2000 and days.size == 3653
    want = RC.run(lon, lat, tmin, tmax, days[YMD], cap=_qalib.MAX_RADIUS_NGH)
    # the checker's own margins first: none of the regression check's decisions is near a threshold, and the days with
    # a corroboration dif near the cutoff are few
    assert (want["regress_margins"][:3] > MARGIN).all() and want["regress_margins"][3] > 1e-6, want["regress_margins"]
    near = want["near"]
    ntested = int(want["tested"].sum())
    print("tested days %d, left out %d, smallest |dif - 10| %.3g" % (ntested, int(near.sum()), want["cutoff_margin"]))
    assert ntested > 1e7 and near.sum() <= MAX_LEFT_OUT * ntested
    pool = StationObsPool(ids, lon, lat, tmin, tmax, days)
    f_tmin, f_tmax, det = run_qa_spatial_only(pool, details=True)
    # a day left out of the corroboration comparison also drops out of the month extremes: compare such a target's 18s
    # only if it has no such day
    clean = ~near.any(axis=(0, 1))
    for v, (got, name) in enumerate(((f_tmin, "flags_tmin"), (f_tmax, "flags_tmax"))):
        w = want[name]
        print(name, {k: int((got == k).sum()) for k in (1, 2, 16, 17, 18)})
        assert np.array_equal(got == QA_SPATIAL_REGRESS, w == QA_SPATIAL_REGRESS)
        assert np.array_equal(got == QA_MISSING, w == QA_MISSING)
        assert np.array_equal(got[:, clean], w[:, clean])
        same = ~near[v] & ~np.isin(w, (QA_OK, QA_MEGA_INCONSIST))
        assert np.array_equal(got[same], w[same])
        assert np.array_equal((got == QA_SPATIAL_CORROB)[~near[v]], (w == QA_SPATIAL_CORROB)[~near[v]])
    assert clean.sum() >= 0.99 * ids.size
    _close(det["norms"], want["norms"], "target normals")
    assert np.array_equal(det["status"], want["status"])
    assert (det["status"][-corrob_cases.N_FAR:] == _qalib.SP_FEW_NGHS).all()
    n17 = int((want["flags_tmin"] == 17).sum() + (want["flags_tmax"] == 17).sum())
    n18 = int((want["flags_tmin"] == 18).sum() + (want["flags_tmax"] == 18).sum())
    assert n17 > 50 and n18 >= 2 * corrob_cases.N_FAR and int(want["empty"].sum()) >= 0


# ---- edge cases ---------------------------------------------------------------------------------------------------
def _check(ids, lon, lat, tmin, tmax, days, targets=None, cap=None):
    import restate_corrob as RC
    pool = StationObsPool(ids, lon, lat, tmin, tmax, days)
    tidx = None if targets is None else np.array([pool.idxs[s] for s in targets])
    want = RC.run(lon, lat, tmin, tmax, days[YMD], targets=tidx, cap=cap)
    assert want["cutoff_margin"] > MARGIN
    f_tmin, f_tmax, det = run_qa_spatial_only(pool, targets, details=True)
    assert np.array_equal(f_tmin, want["flags_tmin"]) and np.array_equal(f_tmax, want["flags_tmax"])
    assert np.array_equal(det["status"], want["status"])
    _close(det["norms"], want["norms"], "target normals")
    return f_tmin, f_tmax, det, want


@pytest.mark.parametrize("ndays", [1, 2, 3])
def test_edge_series_of_one_two_and_three_days(ndays):
    import spatial_cases
    ids, lon, lat, tmin, tmax, days, _ = spatial_cases.synthetic_pool(
        8, dt.date(2000, 2, 28), dt.date(2000, 2, 28) + dt.timedelta(days=ndays - 1), (45.0, 45.2, -110.0, -109.8), 3,
        spikes_per_stn=0, miss=0.0, gap_every=0)
    tmin[ndays // 2, 2] = 60.0                                    # above every Tmax of the month
    f_tmin, f_tmax, det, _ = _check(ids, lon, lat, tmin, tmax, days)
    assert np.isnan(det["norms"]).all()
    assert not np.isin(f_tmin, (16, 17)).any() and f_tmin[ndays // 2, 2] == QA_MEGA_INCONSIST


def test_edge_two_neighbours_all_nan_target_and_short_neighbours():
    """A cluster of three (two neighbours each: no spatial flags, the mega-inconsistency check still runs); an all-NaN
    target inside the main cluster; a target whose neighbours are all too short for normals (the empty list)."""
    import spatial_cases
    ids, lon, lat, tmin, tmax, days, _ = spatial_cases.synthetic_pool(
        20, dt.date(1995, 1, 1), dt.date(2003, 12, 31), (45.0, 45.3, -110.0, -109.6), 21, spikes_per_stn=2)
    lon[14:17], lat[14:17] = (-104.0, -103.9, -103.95), (41.0, 41.05, 41.1)           # two neighbours each
    lon[17:], lat[17:] = (-100.0, -99.9, -99.95), (47.0, 47.05, 47.1)
    lon[3], lat[3] = -99.93, 47.02                                                     # station 3 joins them: three neighbours
    cut = int(np.nonzero(days[YMD] == 19990101)[0][0])
    tmin[:cut, 17:], tmax[:cut, 17:] = np.nan, np.nan                                  # 17-19: five years of record
    tmin[:, 6], tmax[:, 6] = np.nan, np.nan                                            # all-NaN target
    tmax[100, 15] = -50.0                                                              # below every Tmin of its month
    f_tmin, f_tmax, det, want = _check(ids, lon, lat, tmin, tmax, days)
    assert (det["status"][14:17] == _qalib.SP_FEW_NGHS).all()
    assert not np.isin(f_tmin[:, 14:17], (16, 17)).any() and not np.isin(f_tmax[:, 14:17], (16, 17)).any()
    assert f_tmax[100, 15] == QA_MEGA_INCONSIST
    assert (f_tmin[:, 6] == QA_MISSING).all() and (f_tmax[:, 6] == QA_MISSING).all() and np.isnan(det["norms"][6]).all()
    assert want["empty"][:, :, 3].sum() > 800 and (f_tmin[cut + 5:, 3] == QA_SPATIAL_CORROB).sum() > 800
    assert (f_tmin[1:cut - 1, 3] != QA_SPATIAL_CORROB).all()                           # before 1999 the counts do not pass
    assert (f_tmin == QA_SPATIAL_CORROB).sum() > (f_tmin[:, [3, 17, 18, 19]] == QA_SPATIAL_CORROB).sum()


def test_edge_target_over_the_neighbour_cap():
    import spatial_cases
    n = _qalib.MAX_RADIUS_NGH + 10
    ids, lon, lat, tmin, tmax, days, _ = spatial_cases.synthetic_pool(
        n + 6, dt.date(2000, 1, 1), dt.date(2000, 4, 30), (45.0, 45.2, -110.0, -109.8), 9, spikes_per_stn=1)
    lon[n:], lat[n:] = -100.0 + 0.05 * np.arange(6), 40.0 + 0.03 * np.arange(6)        # six stations far away
    tmin[50, 4] = 70.0
    targets = [ids[i] for i in (n + 2, 4, 0, n)]
    f_tmin, f_tmax, det, _ = _check(ids, lon, lat, tmin, tmax, days, targets=targets, cap=_qalib.MAX_RADIUS_NGH)
    assert det["status"].tolist() == [_qalib.SP_OK, _qalib.SP_NGH_CAP, _qalib.SP_NGH_CAP, _qalib.SP_OK]
    assert not np.isin(f_tmin[:, 1:3], (16, 17)).any() and f_tmin[50, 1] == QA_MEGA_INCONSIST


def test_edge_series_longer_than_the_value_cap():
    years = _qalib.MAX_NORM_VALUES // 15 + 1
    days = get_days_metadata(dt.date(1800, 1, 1), dt.date(1800 + years - 1, 12, 31))
    n = 4
    obs = np.zeros((days.size, n), np.float32)
    pool = StationObsPool(np.array(["S%d" % i for i in range(n)]), -110 + 0.01 * np.arange(n), 45 + 0.01 * np.arange(n), obs,
                          obs + 5, days)
    with pytest.raises(_qalib.QaError, match="TWXQA_MAX_NORM_VALUES"):
        run_qa_spatial_only(pool)
    with pytest.raises(_qalib.QaError, match="TWXQA_MAX_NORM_VALUES"):
        doy_norms(obs, days)
    # one year fewer is inside the cap
    keep = days.YEAR < 1800 + years - 1
    a365, a366 = doy_norms(obs[keep][:, :1], days[keep])
    assert (a365 == 0).all() and (a366 == 0).all()


# ---- the driver -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_step08_spatial_and_write_end_to_end(tmp_path, capsys, gold, gold_pool, fmt):
    import corrob_cases
    from topowx_amd import step08
    p = gold_pool
    n, nd = p.ids.size, p.days.size
    # previous flags: one on a day the stage will flag anyway is irrelevant (masked first), so put them on plain days
    final = (gold["flags_tmin"], gold["flags_tmax"])
    plain = np.argwhere((final[0] == 1) & (final[1] == 1))
    prev = [("qflag_tmin", int(plain[10][0]), int(plain[10][1]), b"D"), ("qflag_tmax", int(plain[999][0]), int(plain[999][1]), b"X")]
    db = corrob_cases.write_db(str(tmp_path / ("all_%s.nc" % fmt)), p.ids, p.lon, p.lat, p.tmin, p.tmax, p.days, fmt, prev=prev)
    masked = StationObsPool.from_netcdf(db, qflags=True)
    w_tmin, w_tmax = run_qa_spatial_only(masked)
    before = open(db, "rb").read()
    out = str(tmp_path / "report.npz")
    assert step08.main(["--db", db, "--out", out, "--spatial"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert open(db, "rb").read() == before                        # --spatial alone leaves the database alone
    rep = np.load(out)
    assert np.array_equal(rep["flags_tmin"], w_tmin) and np.array_equal(rep["flags_tmax"], w_tmax)
    assert rep["status"].shape == (n,) and rep["ids"].tolist() == p.ids.tolist()
    for name, f in (("flags_tmin", w_tmin), ("flags_tmax", w_tmax)):
        assert rec[name] == {str(k): int((f == k).sum()) for k in (1, 2, 16, 17, 18)}
        assert rec[name]["16"] > 0 and rec[name]["17"] > 0 and rec[name]["18"] > 0
    assert rec["stations"] == n and rec["seconds"] > 0 and rec["corrob_kernel_ms"] > 0 and "rows_written" not in rec
    # the two masked observations change little: nearly all flags are the golden's
    assert (w_tmin != final[0]).mean() < 1e-3
    # --write
    assert step08.main(["--db", db, "--out", out, "--spatial", "--write"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    rows = np.isin(w_tmin, (16, 17, 18)) | np.isin(w_tmax, (16, 17, 18))
    assert rec["rows_written"] == int(rows.sum()) > 0
    back = StationObsPool.from_netcdf(db, qflags=True)
    char = {1: b"", 2: b"", 16: b"S", 17: b"S", 18: b"M"}
    want = [np.zeros((nd, n), "S1"), np.zeros((nd, n), "S1")]
    for v, f in enumerate((w_tmin, w_tmax)):
        for k, ch in char.items():
            want[v][rows & (f == k)] = ch
    for name, d, s, ch in prev:
        want[0 if name == "qflag_tmin" else 1][d, s] = ch          # kept: the new flag there is 2 (masked -> missing)
    assert np.array_equal(back.qflag_tmin, want[0]) and np.array_equal(back.qflag_tmax, want[1])
    assert (back.qflag_tmin == b"S").sum() > 0 and (back.qflag_tmin == b"M").sum() + (back.qflag_tmax == b"M").sum() == 2
    assert np.array_equal(StationObsPool.from_netcdf(db).tmin, p.tmin, equal_nan=True)      # the observations are untouched
    # a second run on the written database loses none of the flags written before
    assert step08.main(["--db", db, "--out", out, "--spatial", "--write"]) == 0
    capsys.readouterr()
    again = StationObsPool.from_netcdf(db, qflags=True)
    for a, b in ((again.qflag_tmin, back.qflag_tmin), (again.qflag_tmax, back.qflag_tmax)):
        assert np.array_equal(a[b != b""], b[b != b""])
    # a target list; the default invocation still reports the regression check alone
    tfile = tmp_path / "targets.txt"
    tfile.write_text("%s\n%s\n" % (p.ids[25], p.ids[3]))
    assert step08.main(["--db", db, "--out", out, "--spatial", "--targets", str(tfile)]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["stations"] == 2 and np.load(out)["flags_tmin"].shape == (nd, 2)
