"""GPU: the non-spatial precipitation QA (``twxpq_non_spatial`` / ``twxpq_percentiles`` of libtwxqa,
``topowx_amd.qa.qa_prcp``) against the executed-reference golden (tests/golden/make_golden_prcp.py) and the numpy
restatement (tests/restate_prcp.py), the shape grid of the percentile-table kernel, and
``python -m topowx_amd.qa.qa_prcp [--write]`` end to end on both containers.

Flags are compared exactly at every stage.  A check writes its number only where the flag is still 1, so the flags
after a stage are the final flags with the numbers of the later stages put back to 1 (``restate_prcp.stage_flags``; the
golden's own stage snapshots are checked to be nested like that in tests/test_prcp_host.py).  Exact comparison is fair
because the margins are asserted first: the golden maker asserted that every comparison of checks 15 and 19 lies more
than 1e-5 relative from equality or is a tie; on the random pool a station on which the restatement sees a comparison
within 1e-6 is left out whole, and at most 1 of 24 may be.

Tables: identical NaN positions and values within 1e-12 relative.  Derivation: the kernel and numpy on float64 copies do
the same fp64 operations on the same exactly widened values -- (n - 1) q, its floor and fraction, b - a, one product, one
sum -- so bit equality is expected; 1e-12 allows for three roundings of 1.1e-16 with a factor for cancellation in b - a."""
import datetime as dt
import json
import os
import sys

import numpy as np
import pytest

from topowx_amd import _qalib
from topowx_amd.dates import YMD, get_days_metadata
from topowx_amd.qa import qa_prcp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prcp_cases as PC  # noqa: E402
import restate_prcp as RP  # noqa: E402
from spatial_cases import FORMATS  # noqa: E402

pytestmark = pytest.mark.gpu
TABLE_TOL = 1e-12
ALL = (1,) + RP.STAGE_ORDER


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_prcp_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    prcp, tavg, days, _ = PC.case_inputs()
    assert PC.input_hash(prcp, tavg, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return prcp, tavg, days


def _tables_close(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN positions"
    fin = np.isfinite(want)
    d = float(np.max(np.abs(got[fin] / want[fin] - 1.0))) if fin.any() else 0.0
    print("%s: max relative difference %.3g over %d values, %d not bit-equal" % (
        what, d, int(fin.sum()), int((got[fin] != want[fin]).sum())))
    assert d <= TABLE_TOL, what
    return d


def _counts(f):
    return {k: int((f == k).sum()) for k in ALL}


def _stn_major(tab):
    return np.ascontiguousarray(np.moveaxis(tab, 2, 0))               # [366, 5, n] -> [n, 366, 5]


# ---- the executed reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True], ids=["default", "streak_frequent"])
def test_golden_flags_at_every_stage_and_tables(gold, case, both):
    prcp, tavg, days = case
    keep = (prcp.copy(), tavg.copy())
    tm = {}
    det = qa_prcp.run_qa_non_spatial(prcp, tavg, days, streak=both, frequent=both, details=True, timing=tm)
    assert np.array_equal(prcp, keep[0], equal_nan=True) and np.array_equal(tavg, keep[1], equal_nan=True)
    for k in _qalib.PQ_KERNELS:
        ran = both or k not in ("pq_streak", "pq_frequent")
        assert (tm[k + "_kernel_ms"] > 0) == ran, k
    got = det["flags"]
    want = gold["flags_all" if both else "flags_default"]
    assert got.dtype == np.uint8 and got.shape == want.shape
    print(_counts(got))
    stages = gold["stage_flags_all" if both else "stage_flags_default"]
    for i, num in enumerate(RP.STAGE_ORDER):                        # every stage, none left out
        bad = np.argwhere(RP.stage_flags(got, num) != stages[i])
        assert bad.size == 0, (num, bad[:10].tolist())
    assert np.array_equal(got, want) and _counts(got) == _counts(want)
    tab = _stn_major(det["pctiles"])
    _tables_close(tab[gold["pct_stns"]], gold["pctiles_all" if both else "pctiles_default"], "tables of check 15")
    if not both:
        n = prcp.shape[1]
        nan = np.unpackbits(gold["pctiles_nan"])[:n * 366].reshape(n, 366).astype(bool)
        for c in range(5):
            assert np.array_equal(np.isnan(tab[..., c]), nan), c


def test_golden_short_record(gold):
    p, tv, days = PC.short_inputs()
    assert PC.input_hash(p, tv, days) == str(gold["short_hash"])
    for both, key in ((False, "short_stage_flags_default"), (True, "short_stage_flags_all")):
        got = qa_prcp.run_qa_non_spatial(p, tv, days, streak=both, frequent=both)
        for i, num in enumerate(RP.STAGE_ORDER):
            assert np.array_equal(RP.stage_flags(got, num), gold[key][i]), (key, num)


def test_one_series_through_the_reference_signature(gold, case):
    prcp, tavg, days = case
    for s in (PC.S_CLIM, PC.S_SPARSE):
        det = qa_prcp.run_qa_non_spatial(prcp[:, s], tavg[:, s], days, details=True)
        assert det["flags"].shape == (days.size,) and det["flags"].dtype == np.uint8 and det["pctiles"].shape == (366, 5)
        assert np.array_equal(det["flags"], gold["flags_default"][:, s])
        k = gold["pct_stns"].tolist().index(s)
        _tables_close(det["pctiles"], gold["pctiles_default"][k], "table of station %d" % s)
    f = qa_prcp.run_qa_non_spatial(prcp[:, 3], np.full(days.size, np.nan, np.float32), days)
    assert f.shape == (days.size,)
    with pytest.raises(ValueError):
        qa_prcp.run_qa_non_spatial(prcp[:-1], tavg, days)


def test_two_calls_give_identical_bytes(case):
    prcp, tavg, days = case
    a = qa_prcp.run_qa_non_spatial(prcp, tavg, days, streak=True, frequent=True, details=True)
    b = qa_prcp.run_qa_non_spatial(prcp, tavg, days, streak=True, frequent=True, details=True)
    assert a["flags"].tobytes() == b["flags"].tobytes() and a["pctiles"].tobytes() == b["pctiles"].tobytes()
    assert qa_prcp.build_percentiles(prcp, days).tobytes() == qa_prcp.build_percentiles(prcp, days).tobytes()


# ---- a random pool against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True], ids=["default", "streak_frequent"])
def test_random_pool_equals_the_restatement(both):
    p, tv, days, _ = PC.random_inputs()
    want = PC.restated("random", both, both)
    knife = want["knife"]
    print("%d stations, %d knife-edge, smallest margin %.3g" % (knife.size, int(knife.sum()), want["margin"].min()))
    assert p.shape[1] == 24 and days.size == 2192 and knife.sum() <= PC.RANDOM_MAX_KNIFE
    det = qa_prcp.run_qa_non_spatial(p, tv, days, streak=both, frequent=both, details=True)
    ok = ~knife
    print(_counts(det["flags"]))
    for num in RP.STAGE_ORDER:
        bad = np.argwhere(RP.stage_flags(det["flags"], num)[:, ok] != want["stages"][num][:, ok])
        assert bad.size == 0, (num, bad[:10].tolist())
    _tables_close(_stn_major(det["pctiles"])[ok], want["pctiles"][ok], "tables of check 15")


# ---- the shape grid of the table kernel --------------------------------------------------------------------------------
GRID_N = (19, 20, 21, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)


def test_table_kernel_shape_grid():
    """One station per window size: the row of 1 July holds exactly N values > 0 (the other rows hold parts of them), at
    every power of two the in-LDS sort pads to (32 .. 1024), one either side, and around MIN_PERCENTILE_VALUES."""
    days = get_days_metadata(dt.date(1960, 1, 1), dt.date(1999, 12, 31))          # 40 years: up to 1160 values in a window
    cal = RP.Calendar(days[YMD])
    centre = int(cal.q[(days.MONTH == 7) & (days.DAY == 1)][0])
    slots = np.nonzero(np.abs(cal.q - centre) <= 14)[0]
    assert slots.size == 29 * 40
    rs = np.random.RandomState(11)
    x = np.zeros((days.size, len(GRID_N)), np.float32)
    for k, n in enumerate(GRID_N):
        x[rs.permutation(slots)[:n], k] = np.round(rs.gamma(0.8, 0.9, n) + 0.01, 2)
    x[100:130, 3] = np.nan
    got = _stn_major(qa_prcp.build_percentiles(x, days))
    want = np.array([RP.percentiles(x[:, k], cal) for k in range(len(GRID_N))])
    _tables_close(got, want, "shape grid")
    for k, n in enumerate(GRID_N):
        assert np.isfinite(got[k, centre]).all() == (n >= 20), n
    assert np.isnan(got[0]).all() and np.isfinite(got[1, centre]).all() and np.isnan(got[1, centre + 15]).all()
    one = qa_prcp.build_percentiles(x[:, 7], days)                  # nstn = 1 through the 1-d signature
    assert one.shape == (366, 5) and np.array_equal(one, got[7], equal_nan=True)


def test_one_year_record_all_dry_all_nan_and_one_station():
    days = get_days_metadata(dt.date(1999, 1, 1), dt.date(1999, 12, 31))          # 365 days: not a multiple of 64
    assert days.size % 64 != 0
    rs = np.random.RandomState(5)
    wet = (np.arange(365)[:, None] + np.arange(4)[None, :]) % 2 == 0     # every other day: at most 15 values in 29 days
    p = np.where(wet, np.round(rs.gamma(0.8, 0.9, (365, 4)) + 0.01, 2), 0.0).astype(np.float32)
    p[200, 0] = 150.0                                               # an outlier by any row, if there were one
    p[:, 1] = 0.0
    p[:, 2] = np.nan
    tv = np.full((365, 4), -2.0, np.float32)
    det = qa_prcp.run_qa_non_spatial(p, tv, days, streak=True, frequent=True, details=True)
    want = RP.run(p, tv, days[YMD], streak=True, frequent=True)
    assert np.array_equal(det["flags"], want["flags"])
    assert np.isnan(det["pctiles"]).all()                           # at most 29 values in a window of one year: >= 20 needs more
    f = det["flags"]
    assert not np.isin(f, (15, 19)).any() and f[200, 0] == 10       # nothing flagged by check 15; the gap check has the 150
    assert (f[:, 1] == 1).all() and (f[:, 2] == 2).all()
    single = qa_prcp.run_qa_non_spatial(p[:, 3:], tv[:, 3:], days)  # nstn = 1
    assert single.shape == (365, 1) and np.array_equal(single[:, 0], f[:, 3])


def test_record_starting_on_29_february():
    days = get_days_metadata(dt.date(1992, 2, 29), dt.date(1997, 3, 3))
    assert days[YMD][0] == 19920229 and days.size % 64 != 0
    rs = np.random.RandomState(29)
    p = np.where(rs.rand(days.size, 3) < 0.6, np.round(rs.gamma(0.8, 0.9, (days.size, 3)) + 0.01, 2), 0.0).astype(np.float32)
    p[0, :] = (0.7, 44.0, np.nan)
    p[rs.rand(days.size, 3) < 0.03] = np.nan
    tv = np.round(rs.randn(days.size, 3) * 8, 1).astype(np.float32)
    want = RP.run(p, tv, days[YMD], streak=True, frequent=True)
    assert not want["knife"].any()
    det = qa_prcp.run_qa_non_spatial(p, tv, days, streak=True, frequent=True, details=True)
    for num in RP.STAGE_ORDER:
        assert np.array_equal(RP.stage_flags(det["flags"], num), want["stages"][num]), num
    _tables_close(_stn_major(det["pctiles"]), want["pctiles"], "record from 29 February")
    assert np.isfinite(det["pctiles"][59]).all()                    # the row of 29 February itself
    _tables_close(_stn_major(qa_prcp.build_percentiles(p, days)), np.array([RP.percentiles(p[:, k], RP.Calendar(days[YMD]))
                                                                             for k in range(3)]), "the table alone")


def test_streak_walk_at_the_block_seams():
    """Flag 9 of runs planted where the streak walk's 64-day blocks meet (tests/streak_cases.py); the long run has zeros and
    NaN days inside it, which break no run and count for none."""
    import streak_cases as SC
    days = SC.days()
    base = 1.0 + np.arange(SC.NDAYS)[:, None] * 0.01 + np.arange(SC.NSTN)[None, :] * 0.003
    p, planted = SC.build(base, 50.5 + np.arange(len(SC.RUNS)), (0.0, np.nan, 0.0, np.nan, 0.0))
    tv = np.full(p.shape, 5.0, np.float32)
    assert planted.sum() == 31 + (146 - len(SC.HOLES)) + 4 * 20
    for s in range(SC.NSTN):                                        # the restatement against the plan, on the CPU
        assert np.array_equal(RP.streak_mask(p[:, s]), planted[:, s]), s
    want = RP.run(p, tv, days[YMD], streak=True)["flags"]
    assert np.array_equal(want == 9, planted)
    got = qa_prcp.run_qa_non_spatial(p, tv, days, streak=True)
    assert np.array_equal(got == 9, want == 9), np.argwhere((got == 9) != planted)[:10].tolist()
    assert not (qa_prcp.run_qa_non_spatial(p, tv, days) == 9).any()     # the default chain leaves the check out


def test_record_over_the_window_cap_fails_the_call():
    years = _qalib.PQ_MAX_WINDOW_VALUES // 29 + 1
    days = get_days_metadata(dt.date(1800, 1, 1), dt.date(1800 + years - 1, 12, 31))
    obs = np.zeros((days.size, 1), np.float32)
    with pytest.raises(_qalib.QaError, match="TWXPQ_MAX_WINDOW_VALUES"):
        qa_prcp.run_qa_non_spatial(obs, obs, days)
    with pytest.raises(_qalib.QaError, match="TWXPQ_MAX_WINDOW_VALUES"):
        qa_prcp.build_percentiles(obs, days)
    keep = days.YEAR < 1800 + years - 1                             # one year fewer is inside the table's cap
    obs[::3] = 0.5
    tab = qa_prcp.build_percentiles(obs[keep], days[keep])
    assert tab.shape == (366, 5, 1) and np.all(tab == 0.5)
    gap_years = _qalib.MAX_GAP_VALUES // 31                         # ... and the chain runs up to the gap check's cap
    keep = days.YEAR < 1800 + gap_years
    f = qa_prcp.run_qa_non_spatial(obs[keep], obs[keep], days[keep])
    assert f.shape == (int(keep.sum()), 1) and set(np.unique(f).tolist()) <= {1, 4, 5, 6}


# ---- the command line -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_command_line_report_and_write_end_to_end(tmp_path, capsys, gold, case, fmt):
    prcp, tavg, days = case
    nd, n = prcp.shape
    ids = np.array(["SYN%05d" % i for i in range(n)])
    lon, lat = -110.0 + 0.01 * np.arange(n), 45.0 + 0.01 * np.arange(n)
    final = gold["flags_all"]
    # Tmin / Tmax whose mean is the case's Tavg exactly (halves and doubles are exact in float32)
    tmin, tmax = tavg - np.float32(4.0), tavg + np.float32(4.0)
    pool_tavg = (tmin + tmax) / np.float32(2.0)
    same = np.array_equal(pool_tavg, tavg, equal_nan=True)
    want = final if same else RP.run(prcp, pool_tavg, days[YMD], streak=True, frequent=True)["flags"]
    db = PC.write_db(str(tmp_path / ("all_%s.nc" % fmt)), ids, lon, lat, prcp, tmin, tmax, days, fmt, qflags=())
    before = open(db, "rb").read()
    out = str(tmp_path / "report.npz")
    assert qa_prcp.main(["--db", db, "--out", out, "--streak", "--frequent"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert open(db, "rb").read() == before                        # a report leaves the database alone
    rep = np.load(out)
    assert np.array_equal(rep["flags_prcp"], want) and rep["ids"].tolist() == ids.tolist() and np.array_equal(rep["ymd"], days[YMD])
    assert rec["flags_prcp"] == {str(k): int((want == k).sum()) for k in ALL}
    assert rec["stations"] == n and rec["seconds"] > 0 and rec["pq_pctiles_kernel_ms"] > 0 and "rows_written" not in rec
    assert qa_prcp.main(["--db", db, "--out", out, "--streak", "--frequent", "--write"]) == 0      # creates qflag_prcp
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    plain = (want == 1) | (want == 2)
    assert rec["rows_written"] == int((~plain).sum()) > 0
    back = qa_prcp.load_prcp_pool(db)
    lut = np.zeros(256, "S1")
    for num, ch in qa_prcp.PRCP_TWX_TO_GHCN_FLAGS_MAP.items():
        lut[num] = ch.encode()
    assert np.array_equal(back.qflag_prcp, lut[want.astype(np.int64)])
    assert set(np.unique(back.qflag_prcp)) == {b"", b"D", b"G", b"K", b"O", b"X"}
    assert np.array_equal(back.prcp, prcp, equal_nan=True)        # the observations are untouched
    # a second --write, of the default chain: a flag that is there is kept wherever the new one is 1 / 2
    assert qa_prcp.main(["--db", db, "--out", out, "--write"]) == 0
    capsys.readouterr()
    dflt = np.load(out)["flags_prcp"]
    assert not np.isin(dflt, (9, 19)).any()
    again = qa_prcp.load_prcp_pool(db)
    keep = (dflt == 1) | (dflt == 2)
    assert np.array_equal(again.qflag_prcp, np.where(keep, back.qflag_prcp, lut[dflt.astype(np.int64)]))
    assert (again.qflag_prcp == b"K").sum() > 0
