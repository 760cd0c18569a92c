"""GPU: step08's non-spatial checks (``twxqa_non_spatial`` of libtwxqa, ``topowx_amd.qa.run_qa_non_spatial``) against
the executed-reference golden (tests/golden/make_golden_nonspatial.py) and the numpy restatement
(tests/restate_nonspatial.py), the edge cases, and ``python -m topowx_amd.step08 --nonspatial [--write]`` end to end on
both containers.

Flags are compared exactly; a flag's number names the check that set it, so equal final flags mean equal states after
every check.  Exact comparison is fair because the checker's margins are asserted first: the golden maker asserted
|z - 6| > 1e-5 for every z-score the reference formed and >= 1e-4 for every lagged-range comparison; on the random
cases a series on which the restatement sees a |z - 6| below 6e-7 is left out whole (later checks depend on the
removal), and such series are capped at 1 %.  Rows (mean, standard deviation) are compared to 1e-7 degC (``TOL`` of
spatial_cases.py: two fp64 formulations that differ in rounding order only) with identical NaN positions."""
import datetime as dt
import json
import os
import sys

import numpy as np
import pytest

from topowx_amd import _qalib
from topowx_amd.dates import YMD, get_days_metadata
from topowx_amd.qa import NON_SPATIAL_FLAGS, QA_MISSING, QA_OK, StationObsPool, run_qa_non_spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from spatial_cases import FORMATS, TOL  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = (QA_OK,) + NON_SPATIAL_FLAGS


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_nonspatial_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    import make_golden_nonspatial as mk
    tmin, tmax, days, _ = mk.case_inputs()
    assert mk.input_hash(tmin, tmax, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return tmin, tmax, days


def _close(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN positions"
    d = float(np.nanmax(np.abs(got - want))) if np.isfinite(want).any() else 0.0
    print("%s: max |got - want| %.3g over %d values" % (what, d, int(np.isfinite(want).sum())))
    assert d < TOL, what


def _counts(f):
    return {k: int((f == k).sum()) for k in ALL}


# ---- the executed reference ---------------------------------------------------------------------------------------
def test_golden_flags_counts_and_rows(gold, case):
    tmin, tmax, days = case
    tm = {}
    keep = (tmin.copy(), tmax.copy())
    f0, f1, det = run_qa_non_spatial(tmin, tmax, days, details=True, timing=tm)
    assert np.array_equal(tmin, keep[0], equal_nan=True) and np.array_equal(tmax, keep[1], equal_nan=True)
    for k in _qalib.NON_SPATIAL_KERNELS:
        assert tm[k + "_kernel_ms"] > 0, k
    for got, name in ((f0, "flags_tmin"), (f1, "flags_tmax")):
        assert got.dtype == np.uint8 and got.shape == gold[name].shape
        print(name, _counts(got))
        bad = np.argwhere(got != gold[name])
        assert bad.size == 0, (name, bad[:10].tolist(), got[got != gold[name]][:10], gold[name][got != gold[name]][:10])
        assert _counts(got) == _counts(gold[name])
    both = _counts(f0)
    for k, v in _counts(f1).items():
        both[k] += v
    assert all(v > 0 for v in both.values()), both              # every number of the chain occurs
    stns = gold["norm_stns"]
    _close(det["norms"][stns], gold["norms"], "rows (mean, std)")
    nan = np.unpackbits(gold["norms_nan"])[:tmin.shape[1] * 2 * 731].reshape(tmin.shape[1], 2, 731).astype(bool)
    assert np.array_equal(np.isnan(det["norms"][..., 0]), nan) and np.array_equal(np.isnan(det["norms"][..., 1]), nan)


def test_golden_float32_edge_case(gold):
    days = get_days_metadata(dt.date(2001, 1, 1), dt.date(2001, 2, 28))
    assert np.array_equal(days[YMD], gold["edge_ymd"])
    f0, f1 = run_qa_non_spatial(gold["edge_tmin"], gold["edge_tmax"], days)
    for k, name in enumerate(gold["edge_names"]):
        assert np.array_equal(f0[:, k], gold["edge_flags_tmin"][:, k]), name
        assert np.array_equal(f1[:, k], gold["edge_flags_tmax"][:, k]), name
    # the pairs that pin the float32 rule: flagged although their double difference lies below the threshold
    only32 = [k for k, name in enumerate(gold["edge_names"]) if str(name).endswith("f32_only")]
    assert len(only32) == 4 and all((f0[:, k] > 2).sum() + (f1[:, k] > 2).sum() == 1 for k in only32)


def test_one_series_through_the_reference_signature(gold, case):
    tmin, tmax, days = case
    for s in (7, 14):
        f0, f1, det = run_qa_non_spatial(tmin[:, s], tmax[:, s], days, details=True)
        assert f0.shape == (days.size,) and f0.dtype == np.uint8 and det["norms"].shape == (2, 731, 2)
        assert np.array_equal(f0, gold["flags_tmin"][:, s]) and np.array_equal(f1, gold["flags_tmax"][:, s])
    pool = StationObsPool(np.array(["S%02d" % i for i in range(tmin.shape[1])]), np.zeros(tmin.shape[1]),
                          np.zeros(tmin.shape[1]), tmin, tmax, days)
    f0, f1 = pool.run_qa_non_spatial(["S14", "S03"])
    assert np.array_equal(f0, gold["flags_tmin"][:, [14, 3]]) and np.array_equal(f1, gold["flags_tmax"][:, [14, 3]])
    with pytest.raises(KeyError):
        pool.run_qa_non_spatial(["NOT_AN_ID"])
    with pytest.raises(ValueError):
        run_qa_non_spatial(tmin[:-1], tmax, days)


# ---- random cases against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64x12", "5x8_mid_year", "130x7_near_100"])
def test_random_cases_equal_the_restatement(name):
    import nonspatial_cases as NC
    tmin, tmax, days = NC.random_case(name)
    want = NC.restated(name)
    knife = want["knife"]
    print("%s: %d series, %d knife-edge, smallest |z - 6| %.3g" % (name, knife.size, int(knife.sum()), want["z_margin"].min()))
    assert knife.sum() <= NC.MAX_KNIFE * knife.size
    assert not want["std0"].any()                                  # (the lagged range is exact in fp64 on either side)
    f0, f1, det = run_qa_non_spatial(tmin, tmax, days, details=True)
    ok = ~knife
    for got, key in ((f0, "flags_tmin"), (f1, "flags_tmax")):
        print(key, _counts(got))
        bad = np.argwhere(got[:, ok] != want[key][:, ok])
        assert bad.size == 0, (key, bad[:10].tolist())
    _close(det["norms"][ok], want["norms"][ok], "rows (mean, std)")
    if name == "130x7_near_100":                                  # rows at, just under and just over 100 values exist
        n = np.isfinite(det["norms"][..., 0])
        assert n.any() and (~n).any() and (n.any(axis=2) & ~n.all(axis=2)).any()


# ---- edges ----------------------------------------------------------------------------------------------------------
def _check(tmin, tmax, days):
    import restate_nonspatial as RN
    want = RN.run(tmin, tmax, days[YMD])
    assert not want["knife"].any()
    f0, f1, det = run_qa_non_spatial(tmin, tmax, days, details=True)
    assert np.array_equal(f0, want["flags_tmin"]) and np.array_equal(f1, want["flags_tmax"])
    _close(det["norms"], want["norms"], "rows")
    return f0, f1


@pytest.mark.parametrize("ndays", [1, 2, 3])
def test_edge_series_of_one_two_and_three_days(ndays):
    days = get_days_metadata(dt.date(2000, 2, 28), dt.date(2000, 2, 28) + dt.timedelta(days=ndays - 1))
    tmin = np.array([[-30.0, 1.0, np.nan, 0.0], [-25.0, 2.0, 3.0, 5.0], [-5.0, 30.0, 4.0, 6.0]], np.float32)[:ndays]
    tmax = np.array([[20.0, 0.5, 5.0, 0.0], [5.0, 9.0, np.nan, 9.0], [6.0, 9.5, 8.0, 9.5]], np.float32)[:ndays]
    f0, f1 = _check(tmin, tmax, days)
    assert f1[0, 0] == 12 and f0[0, 0] == 12                      # the lagged range on the first day of the series
    assert f0[0, 1] == 11 and f0[0, 3] == 3 and f1[0, 3] == 3
    if ndays == 3:
        assert f0[2, 1] == 11 or f0[2, 1] == 18


def test_edge_all_nan_one_value_one_station_and_a_short_month():
    days = get_days_metadata(dt.date(1999, 6, 3), dt.date(1999, 6, 29))          # 27 days inside one month
    assert days.size == 27
    rs = np.random.RandomState(5)
    tmin = np.round(rs.randn(27, 3) * 4, 1).astype(np.float32)
    tmax = (tmin + 9).astype(np.float32)
    tmin[:, 0], tmax[:, 0] = np.nan, np.nan                       # all NaN
    tmin[:, 1], tmax[:, 1] = np.nan, np.nan
    tmin[11, 1] = 3.5                                             # one finite value
    tmax[4:15, 2] = tmin[4:15, 2]                                 # eleven days of Tmin == Tmax
    f0, f1 = _check(tmin, tmax, days)
    assert (f0[:, 0] == QA_MISSING).all() and (f1[:, 0] == QA_MISSING).all()
    assert f0[11, 1] == QA_OK and (np.delete(f0[:, 1], 11) == QA_MISSING).all()
    # (one of the eleven days holds 0.0 in both variables: the naught check has it first)
    assert np.isin(f0[:, 2], (7, 3)).all() and np.array_equal(f0[:, 2], f1[:, 2]) and (f0[:, 2] == 7).sum() >= 25
    g0, g1 = _check(tmin[:, 2:], tmax[:, 2:], days)               # nstn = 1
    assert np.array_equal(g0[:, 0], f0[:, 2]) and np.array_equal(g1[:, 0], f1[:, 2])


def test_streak_walk_at_the_block_seams():
    """Flag 9 of runs planted where the streak walk's 64-day blocks meet (tests/streak_cases.py), in both variables; the
    NaN days inside the long run also keep the duplicate-month check, which runs first, from taking its months."""
    import restate_nonspatial as RN
    import streak_cases as SC
    days = SC.days()
    base = np.arange(SC.NDAYS)[:, None] * 0.07 - 10.0 + np.arange(SC.NSTN)[None, :] * 0.01
    tmin, planted = SC.build(base, 30.5 + np.arange(len(SC.RUNS)), [np.nan] * len(SC.HOLES))
    tmax = tmin + np.float32(8.0)
    assert planted.sum() == 31 + (146 - len(SC.HOLES)) + 4 * 20
    for s in range(SC.NSTN):                                      # the restatement against the plan, on the CPU
        assert np.array_equal(RN.streaks(tmin[:, s]), planted[:, s]), s
    want = RN.run(tmin, tmax, days[YMD])
    assert np.array_equal(want["flags_tmin"] == 9, planted) and np.array_equal(want["flags_tmax"] == 9, planted)
    f0, f1 = run_qa_non_spatial(tmin, tmax, days)
    assert np.array_equal(f0 == 9, want["flags_tmin"] == 9), np.argwhere((f0 == 9) != planted)[:10].tolist()
    assert np.array_equal(f1 == 9, want["flags_tmax"] == 9), np.argwhere((f1 == 9) != planted)[:10].tolist()


def test_two_calls_give_identical_bytes(case):
    tmin, tmax, days = case
    a = run_qa_non_spatial(tmin, tmax, days, details=True)
    b = run_qa_non_spatial(tmin, tmax, days, details=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2]["norms"].tobytes() == b[2]["norms"].tobytes()


def test_axis_over_the_year_cap_fails_the_call():
    years = _qalib.MAX_GAP_VALUES // 31 + 1
    days = get_days_metadata(dt.date(1800, 1, 1), dt.date(1800 + years - 1, 12, 31))
    obs = np.zeros((days.size, 1), np.float32)
    with pytest.raises(_qalib.QaError, match="TWXQA_MAX_GAP_VALUES"):
        run_qa_non_spatial(obs, obs + 5, days)
    keep = days.YEAR < 1800 + years - 1                           # one year fewer is inside the cap
    f0, f1 = run_qa_non_spatial(obs[keep] + 1, obs[keep] + 5, days[keep])
    assert f0.shape == (int(keep.sum()), 1)


# ---- the driver -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_step08_nonspatial_and_write_end_to_end(tmp_path, capsys, gold, case, fmt):
    import corrob_cases
    from topowx_amd import step08
    tmin, tmax, days = case
    nd, n = tmin.shape
    ids = np.array(["SYN%05d" % i for i in range(n)])
    lon, lat = -110.0 + 0.01 * np.arange(n), 45.0 + 0.01 * np.arange(n)
    final = (gold["flags_tmin"], gold["flags_tmax"])
    db = corrob_cases.write_db(str(tmp_path / ("all_%s.nc" % fmt)), ids, lon, lat, tmin, tmax, days, fmt)
    before = open(db, "rb").read()
    out = str(tmp_path / "report.npz")
    assert step08.main(["--db", db, "--out", out, "--nonspatial"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert open(db, "rb").read() == before                        # --nonspatial alone leaves the database alone
    rep = np.load(out)
    assert np.array_equal(rep["flags_tmin"], final[0]) and np.array_equal(rep["flags_tmax"], final[1])
    assert rep["ids"].tolist() == ids.tolist() and np.array_equal(rep["ymd"], days[YMD])
    for name, f in (("flags_tmin", final[0]), ("flags_tmax", final[1])):
        assert rec[name] == {str(k): int((f == k).sum()) for k in ALL}
    assert rec["stations"] == n and rec["seconds"] > 0 and rec["gap_kernel_ms"] > 0 and "rows_written" not in rec
    # a previous flag on a day the run leaves at 1 / 2 is kept; the observation under it is masked first
    plain = np.argwhere((final[0] == 1) & (final[1] == 1) & (np.arange(n)[None, :] == 6))
    d, s = int(plain[100][0]), 6
    ds = step08.ncio.open_dataset(db, "a")
    q = np.zeros((nd, n), "S1")
    q[d, s] = b"X"
    ds.variables["qflag_tmin"][:] = q
    ds.close()
    assert step08.main(["--db", db, "--out", out, "--nonspatial", "--write"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    w = (np.load(out)["flags_tmin"], np.load(out)["flags_tmax"])
    assert w[0][d, s] == QA_MISSING and (w[0] != final[0]).mean() < 1e-3
    prev = [np.zeros((nd, n), "S1"), np.zeros((nd, n), "S1")]
    prev[0][d, s] = b"X"
    want = []
    for k in range(n):
        want.append(step08.merge_qflags(w[0][:, k], w[1][:, k], prev[0][:, k], prev[1][:, k]))
    rows = np.stack([x[0] for x in want], 1)
    assert rec["rows_written"] == int(rows.sum()) > 0
    back = StationObsPool.from_netcdf(db, qflags=True)
    for v, q in enumerate((back.qflag_tmin, back.qflag_tmax)):
        chars = np.stack([x[1 + v] for x in want], 1)
        expect = np.where(rows, chars, prev[v])
        assert np.array_equal(q, expect)
    assert back.qflag_tmin[d, s] == b"X"
    assert set(np.unique(back.qflag_tmin)) | set(np.unique(back.qflag_tmax)) >= {b"", b"D", b"G", b"I", b"K", b"M", b"N", b"O",
                                                                                 b"R", b"T", b"X"}
    assert np.array_equal(StationObsPool.from_netcdf(db).tmin, tmin, equal_nan=True)       # the observations are untouched
    # the second run of step08 sees the flagged observations as NaN
    flagged = (back.qflag_tmin != b"")
    assert np.isnan(back.tmin[flagged]).all() and flagged.sum() > 1000
    assert step08.main(["--db", db, "--out", out, "--spatial"]) == 0
    capsys.readouterr()
    sp = np.load(out)["flags_tmin"]
    assert (sp[flagged] == QA_MISSING).all()
    # a target list
    tfile = tmp_path / "targets.txt"
    tfile.write_text("%s\n%s\n" % (ids[14], ids[3]))
    assert step08.main(["--db", db, "--out", out, "--nonspatial", "--targets", str(tfile)]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["stations"] == 2 and np.load(out)["flags_tmin"].shape == (nd, 2)
