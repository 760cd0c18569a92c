"""CPU: step08's spatial regression check without a GPU -- the numpy restatement (tests/restate_spatial.py) against the
executed-reference golden (tests/golden/make_golden_spatial.py), the constants, the header against the binding,
``StationObsPool.from_netcdf`` on both containers and the argument checks that need no device."""
import datetime as dt
import os
import re
import sys

import numpy as np
import pytest

from topowx_amd import ncio
from topowx_amd.dates import YMD, get_days_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from spatial_cases import FORMATS, TOL  # noqa: E402  (shared by both spatial test files)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_spatial_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    import make_golden_spatial as mgs
    c = mgs.case_inputs()
    assert mgs.input_hash(*c[:6]) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return c


def test_golden_input_hash_and_content(gold, case):
    ids, lon, lat, tmin, tmax, days, spikes = case
    assert tmin.dtype == np.float32 and tmin.shape == (days.size, ids.size) == (1095, 40)
    assert np.array_equal(gold["spikes"], spikes)
    # the golden is not trivial: flags, all on planted spikes, the two on the ends of the series among them
    flagged = gold["flags_tmin"] == 16
    planted = np.zeros(flagged.shape, bool)
    planted[spikes[:, 1], spikes[:, 0]] = True
    assert flagged.sum() > 100 and not (flagged & ~planted).any()
    assert flagged[0, 3] and flagged[-1, 11]
    assert int(gold["f32_flag_diff"]) >= 0
    # the margins the maker asserted
    assert (gold["margins"][:3] > 1e-5).all() and gold["margins"][3] > 1e-9 and float(gold["radius_margin"]) > 1e-6


def test_restatement_matches_golden(gold, case):
    import restate_spatial as R
    ids, lon, lat, tmin, tmax, days, _ = case
    res = R.run(lon, lat, tmin, tmax, days[YMD])
    for v, name in enumerate(("flags_tmin", "flags_tmax")):
        want = gold[name]
        assert np.array_equal(res["flags"][v], want == 16)
        obs = (tmin, tmax)[v]
        assert np.array_equal(want == 2, np.isnan(obs))
    assert np.array_equal(np.isnan(res["est"]), np.isnan(gold["est"]))
    assert np.nanmax(np.abs(res["est"] - gold["est"])) < TOL
    assert np.array_equal(np.isnan(res["r"]), np.isnan(gold["r"]))
    assert np.nanmax(np.abs(res["r"] - gold["r"])) < TOL
    reached = gold["nvalid"] >= 0
    assert np.array_equal(res["nvalid"][reached], gold["nvalid"][reached])
    # where the reference did not get to the neighbours the restatement says why
    assert set(np.unique(res["status"][~reached]).tolist()) <= {R.FEW_NGHS, R.FEW_DAYS}
    assert (res["status"][ids.size - 1] == R.FEW_NGHS).all()          # the station placed away from the rest
    assert (res["status"][np.isfinite(gold["r"])] == R.OK).all()
    assert (res["margins"][:3] > 100 * TOL).all()


def test_restatement_models_match_golden(gold, case):
    """The intermediates: the weight-sorted (weight, slope, intercept, column) lists of the first targets."""
    import restate_spatial as R
    ids, lon, lat, tmin, tmax, days, _ = case
    model, col = gold["model"], gold["model_col"]
    seen = 0
    for s in range(model.shape[0]):
        ngh = R.neighbours(lon, lat, s)
        for v, obs in enumerate((tmin, tmax)):
            o = R.check_station(obs, days[YMD], s, ngh)
            for m in range(model.shape[2]):
                k = int((col[s, v, m] >= 0).sum())
                if k == 0:
                    continue
                assert o["col"][:k, m].tolist() == col[s, v, m, :k].tolist()
                got = np.column_stack([o["w"][:k, m], o["slope"][:k, m], o["icpt"][:k, m]])
                assert np.abs(got - model[s, v, m, :k]).max() < TOL
                seen += 1
    assert seen > 200


def test_constants_equal_the_reference(gold):
    from topowx_amd.qa import qa_temp
    for k in ("QA_OK", "QA_MISSING", "QA_SPATIAL_REGRESS", "NGH_RADIUS", "NGH_CORR", "NGH_RESID_CUTOFF",
              "NGH_RESID_STD_CUTOFF", "MIN_DAYS_MTH_WINDOW", "MIN_NGHS", "MAX_NGHS"):
        assert float(getattr(qa_temp, k)) == float(gold["const_" + k]), k
    want = dict(zip(gold["flags_map_keys"].tolist(), gold["flags_map_vals"].tolist()))
    assert qa_temp.TWX_TO_GHCN_FLAGS_MAP == want
    import restate_spatial as R
    assert (R.RADIUS_KM, R.NGH_CORR, R.RESID_CUTOFF, R.RESID_STD_CUTOFF, R.MIN_DAYS, R.MIN_NGHS, R.MAX_NGHS) == tuple(
        float(gold["const_" + k]) for k in ("NGH_RADIUS", "NGH_CORR", "NGH_RESID_CUTOFF", "NGH_RESID_STD_CUTOFF",
                                            "MIN_DAYS_MTH_WINDOW", "MIN_NGHS", "MAX_NGHS"))


def test_header_matches_binding_and_restatement():
    from topowx_amd import _qalib
    from topowx_amd.qa import qa_temp
    import restate_spatial as R
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    twx = open(os.path.join(ROOT, "include", "twx.h")).read()
    assert sorted(set(re.findall(r"\b(twxqa_\w+)\s*\(", h))) == sorted(_qalib.EXPORTS)
    assert "twxqa_spatial_regress" in _qalib.EXPORTS

    def define(name):
        m = re.search(r"#define %s (\S+)" % name, h)
        assert m, name
        tok = m.group(1)
        if tok.startswith("TWX_CELL_"):
            tok = re.search(r"#define %s (\S+)" % tok, twx).group(1)
        return float(tok)

    for name, val in (("TWXQA_MAX_RADIUS_NGH", _qalib.MAX_RADIUS_NGH), ("TWXQA_NGH_RADIUS_KM", qa_temp.NGH_RADIUS),
                      ("TWXQA_MIN_DAYS_MTH_WINDOW", qa_temp.MIN_DAYS_MTH_WINDOW), ("TWXQA_MIN_NGHS", qa_temp.MIN_NGHS),
                      ("TWXQA_MAX_NGHS", qa_temp.MAX_NGHS), ("TWXQA_SP_OK", _qalib.SP_OK),
                      ("TWXQA_SP_FEW_NGHS", _qalib.SP_FEW_NGHS), ("TWXQA_SP_DEGENERATE", _qalib.SP_DEGENERATE),
                      ("TWXQA_SP_NGH_CAP", _qalib.SP_NGH_CAP), ("TWXQA_SP_FEW_DAYS", _qalib.SP_FEW_DAYS),
                      ("TWXQA_SP_FEW_VALID", _qalib.SP_FEW_VALID)):
        assert define(name) == float(val), name
    assert (R.OK, R.FEW_NGHS, R.DEGENERATE, R.NGH_CAP, R.FEW_DAYS, R.FEW_VALID) == (
        _qalib.SP_OK, _qalib.SP_FEW_NGHS, _qalib.SP_DEGENERATE, _qalib.SP_NGH_CAP, _qalib.SP_FEW_DAYS, _qalib.SP_FEW_VALID)
    assert sorted(qa_temp.ITEM_STATUS) == sorted([R.OK, R.FEW_NGHS, R.DEGENERATE, R.NGH_CAP, R.FEW_DAYS, R.FEW_VALID])


def test_qa_library_lists_the_spatial_kernels():
    """build.sh links both translation units into libtwxqa.so; the new kernels spill nothing and the item kernel's
    LDS is what the neighbour cap was sized for (no build in this checkout: skipped, as test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import ctypes
    import isa_resources
    lib = ctypes.CDLL(_qalib.LIB_PATH)
    for name in _qalib.EXPORTS:
        assert hasattr(lib, name), name
    table = isa_resources.parse(res)
    assert "k_outlier_wls" in table
    for k in ("k_qa_radius", "k_spatial_regress"):
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    lds = table["k_spatial_regress"]["lds"]
    assert lds == 34 * _qalib.MAX_RADIUS_NGH                     # 32-byte entry + 2-byte rank per neighbour
    assert (160 * 1024) // lds >= 16                             # >= 4 one-wave workgroups per SIMD fit a CU's LDS
    assert table["k_spatial_regress"]["vgprs"] <= 128            # registers do not cut that further (512 / 4 waves)


def test_month_table_windows():
    """The windows of the restatement are the reference's: month -15 / +15 days, clipped to the series; February of
    a leap year; December and January across a year end."""
    import restate_spatial as R
    days = get_days_metadata(dt.date(1999, 12, 20), dt.date(2001, 1, 10))
    ws, we, ms, me = R.month_table(days[YMD])
    ymd = days[YMD]
    assert ws.size == 14
    assert (ymd[ms[0]], ymd[me[0] - 1], ymd[ws[0]], ymd[we[0] - 1]) == (19991220, 19991231, 19991220, 20000115)
    assert (ymd[ms[1]], ymd[me[1] - 1], ymd[ws[1]], ymd[we[1] - 1]) == (20000101, 20000131, 19991220, 20000215)
    assert (ymd[ms[2]], ymd[me[2] - 1], ymd[ws[2]], ymd[we[2] - 1]) == (20000201, 20000229, 20000117, 20000315)
    assert (ymd[ms[12]], ymd[me[12] - 1], ymd[ws[12]], ymd[we[12] - 1]) == (20001201, 20001231, 20001116, 20010110)
    assert (ymd[ms[13]], ymd[me[13] - 1], ymd[ws[13]]) == (20010101, 20010110, 20001217) and we[13] == days.size
    assert (we - ws).max() == 61


def _pool(n=6, nd=50, seed=3):
    from topowx_amd.qa import StationObsPool
    rs = np.random.RandomState(seed)
    days = get_days_metadata(dt.date(1990, 1, 1), dt.date(1990, 1, 1) + dt.timedelta(days=nd - 1))
    tmin = np.round(rs.randn(nd, n) * 5, 1).astype(np.float32)
    tmax = (tmin + 10).astype(np.float32)
    tmin[rs.rand(nd, n) < 0.1] = np.nan
    tmax[3, 2] = np.nan
    ids = np.array(["GHCN_%03d" % i for i in range(n)])
    return StationObsPool(ids, -110 + rs.rand(n), 45 + rs.rand(n), tmin, tmax, days)


@pytest.mark.parametrize("fmt", FORMATS)
def test_station_obs_pool_from_netcdf_round_trip(tmp_path, fmt):
    from topowx_amd import stationdb as sdb
    from topowx_amd.qa import StationObsPool
    pool = _pool()
    n = pool.ids.size
    stns = np.empty(n, dtype=[(sdb.STN_ID, "U16"), (sdb.LON, np.float64), (sdb.LAT, np.float64), (sdb.ELEV, np.float64)])
    stns[sdb.STN_ID], stns[sdb.LON], stns[sdb.LAT], stns[sdb.ELEV] = pool.ids, pool.lon, pool.lat, 100.0
    path = str(tmp_path / ("all_%s.nc" % fmt))
    ncio.create_quick_db(path, stns, pool.days, [("tmin", "f4", ncio.FILL_F4, "minimum air temperature", "C"),
                                                  ("tmax", "f4", ncio.FILL_F4, "maximum air temperature", "C")], format=fmt)
    ds = ncio.open_dataset(path, "a")
    for name, a in (("tmin", pool.tmin), ("tmax", pool.tmax)):
        v = ds.variables[name]
        v.missing_value = np.float32(ncio.FILL_F4)
        v[:] = np.where(np.isnan(a), np.float32(ncio.FILL_F4), a)
    ds.close()
    back = StationObsPool.from_netcdf(path)
    assert back.ids.tolist() == pool.ids.tolist()
    np.testing.assert_array_equal(back.lon, pool.lon)
    np.testing.assert_array_equal(back.lat, pool.lat)
    assert back.tmin.dtype == np.float32 and back.tmin.shape == pool.tmin.shape
    np.testing.assert_array_equal(back.tmin, pool.tmin)
    np.testing.assert_array_equal(back.tmax, pool.tmax)
    assert np.isnan(back.tmin).sum() == np.isnan(pool.tmin).sum() > 0
    np.testing.assert_array_equal(back.days[YMD], pool.days[YMD])


def test_pool_and_target_validation():
    from topowx_amd.qa import StationObsPool, qa_spatial_regress
    pool = _pool()
    with pytest.raises(ValueError):
        StationObsPool(pool.ids, pool.lon, pool.lat[:-1], pool.tmin, pool.tmax, pool.days)
    with pytest.raises(ValueError):
        StationObsPool(pool.ids, pool.lon, pool.lat, pool.tmin.T, pool.tmax.T, pool.days)
    with pytest.raises(ValueError):
        StationObsPool(np.array(["a"] * pool.ids.size), pool.lon, pool.lat, pool.tmin, pool.tmax, pool.days)
    with pytest.raises(KeyError):                                # an unknown target fails before any device work
        qa_spatial_regress(pool, ["NOT_AN_ID"])


def test_call_level_argument_checks():
    """Non-consecutive days, an index out of range and a non-finite coordinate fail the call before any device work
    (the library is needed, a GPU is not)."""
    from topowx_amd import _qalib
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    pool = _pool()
    args = [pool.lon, pool.lat, pool.tmin.T, pool.tmax.T, pool.days[YMD], np.arange(pool.ids.size)]

    def call(i, val):
        a = list(args)
        a[i] = val
        return _qalib.spatial_regress(*a)

    ymd = np.array(pool.days[YMD])
    gap = ymd.copy()
    gap[20:] = get_days_metadata(dt.date(1990, 1, 22), dt.date(1990, 2, 20))[YMD]      # one day skipped
    with pytest.raises(_qalib.QaError, match="not consecutive"):
        call(4, gap)
    rep = ymd.copy()
    rep[10] = rep[9]
    with pytest.raises(_qalib.QaError, match="not consecutive"):
        call(4, rep)
    bad = ymd.copy()
    bad[0] = 19901301
    with pytest.raises(_qalib.QaError):
        call(4, bad)
    for idx in ([0, 1, pool.ids.size], [-1]):
        with pytest.raises(_qalib.QaError, match="target index"):
            call(5, np.array(idx))
    lon = pool.lon.copy()
    lon[2] = np.nan
    with pytest.raises(_qalib.QaError, match="non-finite"):
        call(0, lon)
    lat = pool.lat.copy()
    lat[4] = np.inf
    with pytest.raises(_qalib.QaError, match="non-finite"):
        call(1, lat)
    with pytest.raises(ValueError):
        call(2, pool.tmin)                                       # [ndays, nstn] where [nstn, ndays] is expected
    assert _qalib.spatial_nmonths(ymd) == 2
