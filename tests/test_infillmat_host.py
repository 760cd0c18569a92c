"""CPU: the infill neighbour matrices without a GPU -- the numpy restatement (tests/restate_infillmat.py) against the
executed-reference golden (tests/golden/make_golden_infillmat.py), the 31-column cap of ``.matrix()``, the four deviation
statuses on hand-made pools, the argument rules of the Python layer and of the library's entry, and the resource table
of the new kernels.

Ranked lists, nnghs, keep and max_dist are compared exactly, ioa to 1e-10 (a d1 sum has at most 25 203 terms, so
re-ordering moves it by about n 2^-53 = 3e-12 relative; the golden maker asserted decision margins of 1e-9) and distances
to the tolerance of the other radius tests (``spatial_cases.TOL``)."""
import datetime as dt
import os
import re
import sys

import numpy as np
import pytest

from topowx_amd.dates import MONTH, YMD, get_days_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restate_infillmat as RI  # noqa: E402
from spatial_cases import TOL  # noqa: E402

NEW_KERNELS = ("k_if_ring", "k_if_pair", "k_if_item", "k_if_compact")
IOA_TOL = 1e-10


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_infillmat_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    import make_golden_infillmat as mk
    ids, lon, lat, tmin, days = mk.case_inputs()
    assert mk.input_hash(ids, lon, lat, tmin, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return ids, lon, lat, tmin, days


@pytest.fixture(scope="module")
def restated(case):
    ids, lon, lat, tmin, days = case
    return RI.run(lon, lat, tmin, np.ones(ids.size, bool), np.arange(ids.size), (days[MONTH] - 1).astype(np.int8))


def test_golden_content(gold, case):
    ids, lon, lat, tmin, days = case
    assert tmin.shape == (2922, 48) and tmin.dtype == np.float32 and gold["nnghs"].shape == (48, 12)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_infillmat_v1.npz")) < 1024 * 1024
    assert gold["nnghs"].min() >= 3 and gold["nnghs"].max() > 3
    nkeep = np.add.reduceat(gold["keep"], gold["off"][:-1]).reshape(48, 12)
    assert (nkeep < gold["nnghs"]).any() and (nkeep >= 3).all() and gold["matrix_ncols"].max() < 30
    assert np.array_equal(nkeep, gold["matrix_ncols"])
    assert gold["cand_kept"].any()
    # each half of the rejection rule (:184) on its own: a candidate >= 0.7 that loses against a ranked station, and
    # a candidate that is the ring's best and below 0.7
    assert (gold["cand_rejected"] == "m").sum() >= 1 and (gold["cand_rejected"] == "7").sum() >= 1
    assert (gold["cand_rejected"] == "m7").sum() >= 1 and not (gold["cand_kept"] & (gold["cand_rejected"] != "")).any()
    assert np.unique(gold["max_dist"]).size >= 3 and (gold["max_dist"] % 37.5 == 0).all() and gold["max_dist"].min() == 75.0
    assert float(gold["ioa_gap"]) > 1e-9 and float(gold["cand_margin"]) > 1e-9 and float(gold["ring_margin"]) > 1e-6
    assert float(gold["dist_gap"]) > 1e-9 and float(gold["ref_items_per_second"]) > 0
    assert (float(gold["const_MAX_DISTANCE"]), float(gold["const_MIN_POR_OVERLAP"]), float(gold["const_MIN_DAILY_NGHBRS"]),
            float(gold["const_MAX_COLS_NORM_IMPUTE"])) == (75.0, 2.0 / 3.0, 3.0, 31.0)
    # ioa descending within every item
    for i in range(48 * 12):
        a = gold["ioa"][gold["off"][i]:gold["off"][i + 1]]
        assert a.size >= 3 and (np.diff(a) < 0).all()


def test_constants_equal_the_reference(gold):
    from topowx_amd import _qalib, infill
    assert (infill.MAX_DISTANCE, infill.MIN_POR_OVERLAP, infill.MIN_DAILY_NGHBRS, infill.MAX_COLS_NORM_IMPUTE) == \
        tuple(float(gold["const_" + k]) for k in ("MAX_DISTANCE", "MIN_POR_OVERLAP", "MIN_DAILY_NGHBRS", "MAX_COLS_NORM_IMPUTE"))
    assert (RI.MAX_DISTANCE, RI.MIN_POR_OVERLAP) == (infill.MAX_DISTANCE, infill.MIN_POR_OVERLAP)
    assert (RI.OK, RI.NUMERIC, RI.NGH_CAP, RI.NO_TARGET_OBS, RI.UNSATISFIED) == \
        (_qalib.IF_OK, _qalib.IF_NUMERIC, _qalib.IF_NGH_CAP, _qalib.IF_NO_TARGET_OBS, _qalib.IF_UNSATISFIED)
    assert sorted(infill.ITEM_STATUS) == [0, 4, 7, 18, 19]


def test_restatement_equals_the_golden(gold, restated, case):
    import make_golden_infillmat as mk
    ids, lon, lat, tmin, days = case
    r = restated
    assert (r["status"] == RI.OK).all() and not RI.knife(r).any()
    for k in ("nrings", "cand_kept", "cand_rejected"):               # recorded from the reference run itself
        assert np.array_equal(r[k], gold[k]), k
    assert np.array_equal(r["nnghs"], gold["nnghs"]) and np.array_equal(r["max_dist"], gold["max_dist"])
    assert np.array_equal(r["off"], gold["off"]) and np.array_equal(r["idx"], gold["idx"])
    assert np.array_equal(r["keep"], gold["keep"])
    print("max |ioa - golden| %.3g, max |dist - golden| %.3g" % (np.abs(r["ioa"] - gold["ioa"]).max(),
                                                                  np.abs(r["dist"] - gold["dist"]).max()))
    assert np.abs(r["ioa"] - gold["ioa"]).max() <= IOA_TOL and np.abs(r["dist"] - gold["dist"]).max() <= TOL
    grp = (days[MONTH] - 1).astype(np.int8)
    tg = np.arange(48)
    for t in range(48):
        for g in range(12):
            m = RI.matrix(tmin, grp, r, tg, t, g)
            assert m.shape[1] == 1 + gold["matrix_ncols"][t, g]
            assert np.array_equal(mk.matrix_hash(m[:, 1:]), gold["matrix_hash"][t, g]), (t, g)
    for t, g in gold["full_items"]:
        want = gold["full_%d_%d" % (t, g)].astype(np.float64)
        assert np.array_equal(RI.matrix(tmin, grp, r, tg, t, g)[:, 1:], want, equal_nan=True)
    # the thresholds as the Python layer passes them
    from topowx_amd.infill import item_thresholds
    nall, npor = item_thresholds(np.ascontiguousarray(tmin.T), grp, 12)
    assert np.array_equal(nall, r["nthres_all"]) and np.array_equal(npor, r["nthres_target_por"])
    assert nall[1] == np.round(2.0 / 3.0 * 226) and nall.dtype == np.int32


def _pool(lon, lat, tmin, first=dt.date(2001, 1, 1)):
    from topowx_amd.qa import StationObsPool
    tmin = np.asarray(tmin, np.float32)
    days = get_days_metadata(first, first + dt.timedelta(days=tmin.shape[0] - 1))
    ids = np.array(["S%03d" % i for i in range(tmin.shape[1])])
    return StationObsPool(ids, lon, lat, tmin, tmin + 10, days)


def _line_pool(n, nd=40, step=0.1, seed=3):
    """n stations on a parallel, `step` degrees apart (about 7.9 km at 45 N), a common signal plus noise, no gaps."""
    rs = np.random.RandomState(seed)
    sig = rs.randn(nd) * 5
    tmin = np.round(sig[:, None] + rs.randn(nd, n), 1)
    return -110.0 + step * np.arange(n), np.full(n, 45.0), tmin


def test_deviation_statuses_of_the_restatement():
    lon, lat, tmin = _line_pool(6)
    grp = np.zeros(40, np.int8)
    all6 = np.ones(6, bool)
    # an all-NaN target month: only that item fails
    g2 = np.repeat([0, 1], 20).astype(np.int8)
    a = tmin.copy()
    a[20:, 0] = np.nan
    r = RI.run(lon, lat, a, all6, [0, 1], g2)
    assert r["status"].tolist() == [[RI.OK, RI.NO_TARGET_OBS], [RI.OK, RI.OK]]
    assert r["off"][2] == r["off"][1] and r["nthres_target_por"][0].tolist() == [13, 0]
    # a d1 denominator of 0: target and neighbour constant and equal
    b = tmin.copy()
    b[:, 0] = 4.0
    b[:, 1] = 4.0
    r = RI.run(lon, lat, b, all6, [0, 2], grp)
    assert r["status"].ravel().tolist() == [RI.NUMERIC, RI.OK] and r["off"][1] == 0
    # two eligible stations: unsatisfied, with the list as far as it got
    r = RI.run(lon, lat, tmin, np.array([1, 1, 1, 0, 0, 0], bool), [0], grp)
    assert r["status"][0, 0] == RI.UNSATISFIED and r["idx"].size == 2 and not r["keep"].any() and r["nnghs"][0, 0] == 3
    assert r["max_dist"][0, 0] == 75.0
    # exactly three: satisfied
    r = RI.run(lon, lat, tmin, np.array([1, 1, 1, 1, 0, 0], bool), [0], grp)
    assert r["status"][0, 0] == RI.OK and r["keep"].tolist() == [1, 1, 1]
    # a ring above the cap, a ranked list above it (the cap lowered: the rule, not the number)
    assert RI.run(lon, lat, tmin, all6, [0], grp, cap=4)["status"][0, 0] == RI.NGH_CAP
    lon9, lat9, t9 = _line_pool(9, step=0.45)                          # 35.4 km apart: rings of 2, 1, 1, ...
    t9[0, 1:] = np.nan                                                  # no neighbour has the first day: never 3 on it
    r = RI.run(lon9, lat9, t9, np.ones(9, bool), [0], np.zeros(40, np.int8), cap=6)
    assert r["status"][0, 0] == RI.NGH_CAP and r["idx"].size == 0
    r = RI.run(lon9, lat9, t9, np.ones(9, bool), [0], np.zeros(40, np.int8))
    assert r["status"][0, 0] == RI.UNSATISFIED and r["idx"].size == 8 and r["nnghs"][0, 0] == 9
    # both in one ring: the first failing station in distance order decides.  Rings of 4 (stations 1-4) and 3 (5-7);
    # with a cap of 5 station 6 would be entry 6 of the list
    lon8, lat8, t8 = _line_pool(8, step=0.2)
    t8[0, 1:] = np.nan
    t8[:, 0] = 4.0
    for const, status in ((7, RI.NGH_CAP), (5, RI.NUMERIC), (6, RI.NUMERIC)):
        e = t8.copy()
        e[:, const] = 4.0
        r = RI.run(lon8, lat8, e, np.ones(8, bool), [0], np.zeros(40, np.int8), cap=5)
        assert r["status"][0, 0] == status and r["nrings"][0, 0] == 2 and r["nnghs"][0, 0] == 5, const


def test_matrix_column_cap():
    """``.matrix()`` keeps the target and the first ``max_cols - 1`` kept stations (MAX_COLS_NORM_IMPUTE = 31)."""
    from topowx_amd.infill import InfillMatrices
    n, nd = 40, 12
    lon, lat, tmin = _line_pool(n, nd, step=0.01)
    pool = _pool(lon, lat, tmin)
    keep = np.ones(36, np.uint8)
    keep[[3, 7]] = 0
    idx = np.arange(1, 37, dtype=np.int32)[::-1].copy()
    res = dict(status=np.zeros((1, 1), np.int32), nnghs=np.full((1, 1), 36, np.int32), max_dist=np.full((1, 1), 75.0),
               off=np.array([0, 36], np.int64), idx=idx, ioa=np.linspace(0.9, 0.5, 36), dist=np.linspace(1, 30, 36),
               nlap=np.full(36, nd, np.int32), nlap_stn=np.full(36, nd, np.int32), keep=keep, rounds=1)
    m = InfillMatrices(pool, "tmin", pool.ids[:1], np.array([0], np.int32), np.zeros(nd, np.int8), 1, res,
                       np.array([8], np.int32), np.array([[8]], np.int32), 3)
    kept = idx[keep != 0]
    assert kept.size == 34
    a = m.matrix("S000", 0)
    assert a.shape == (nd, 31) and a.dtype == np.float64
    assert np.array_equal(a, pool.tmin[:, np.concatenate([[0], kept[:30]])].astype(np.float64))
    assert m.matrix(0, 0, max_cols=40).shape == (nd, 35) and m.matrix(0, 0, max_cols=1).shape == (nd, 1)
    assert np.array_equal(m.columns(0, 0, 5), kept[:4])
    with pytest.raises(ValueError):
        m.matrix(0, 0, max_cols=0)
    with pytest.raises(IndexError):
        m.matrix(0, 1)
    with pytest.raises(KeyError):
        m.matrix("nobody", 0)


def test_argument_validation_of_the_python_layer():
    from topowx_amd.infill import InfillMatrix, build_infill_matrices
    lon, lat, tmin = _line_pool(6)
    pool = _pool(lon, lat, tmin)
    for kw in (dict(var="prcp"), dict(var="tmin", targets=[]), dict(var="tmin", stns_mask=np.ones(5, bool)),
               dict(var="tmin", stns_mask=np.ones(6, int)), dict(var="tmin", day_groups=np.zeros(39, int)),
               dict(var="tmin", day_groups=np.full(40, 12)), dict(var="tmin", day_groups=np.full(40, -1)),
               dict(var="tmin", day_groups=np.full(40, -2)), dict(var="tmin", day_groups=np.zeros(40)),
               dict(var="tmin", day_groups="months"), dict(var="tmin", min_daily_nnghs=0),
               dict(var="tmin", min_daily_nnghs=17), dict(var="tmin", min_daily_nnghs=3.0)):
        with pytest.raises(ValueError):
            build_infill_matrices(pool, **kw)
    with pytest.raises(KeyError, match="not in the pool"):
        build_infill_matrices(pool, "tmin", targets=["S000", "nobody"])
    with pytest.raises(ValueError, match="day_mask"):
        InfillMatrix("S000", pool, None, "tmin", day_mask=np.ones(39, bool))


def test_header_and_binding():
    from topowx_amd import _qalib
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxif_\w+)\s*\(", h))) == sorted(_qalib.IF_EXPORTS) == ["twxif_infill_matrix"]
    for macro, val in (("TWXIF_NO_TARGET_OBS", _qalib.IF_NO_TARGET_OBS), ("TWXIF_UNSATISFIED", _qalib.IF_UNSATISFIED),
                       ("TWXIF_MAX_GROUPS", _qalib.IF_MAX_GROUPS), ("TWXIF_MAX_MIN_NNGHS", _qalib.IF_MAX_MIN_NNGHS),
                       ("TWXIF_MAX_COLS_NORM_IMPUTE", _qalib.IF_MAX_COLS_NORM_IMPUTE),
                       ("TWXIF_NKERNELS", len(_qalib.INFILL_MATRIX_KERNELS)),
                       ("TWXIF_NTIMES", len(_qalib.INFILL_MATRIX_KERNELS) + len(_qalib.INFILL_MATRIX_HOST_TIMES))):
        m = re.search(r"#define %s (\d+)" % macro, h)
        assert m and int(m.group(1)) == val, macro
    assert "#define TWXIF_NUMERIC TWX_CELL_NUMERIC" in h and "#define TWXIF_NGH_CAP TWX_CELL_CAND_OVERFLOW" in h
    assert "topowx_amd/qa/twx_infillmat.hip" in open(os.path.join(ROOT, "build.sh")).read()


def test_resource_table_lists_the_new_kernels():
    """No scratch, no spills, and the LDS of the item kernel is what the header's arithmetic says: 28 + 28 + 4 bytes per
    station of the cap and 1 KiB of reduction scratch (no build in this checkout: skipped, as test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import ctypes
    import isa_resources
    assert hasattr(ctypes.CDLL(_qalib.LIB_PATH), "twxif_infill_matrix")
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    cap = _qalib.MAX_RADIUS_NGH
    lds = table["k_if_item"]["lds"]
    assert 60 * cap + 1024 <= lds <= 60 * cap + 1024 + 512
    assert 8 * lds <= 160 * 1024 and table["k_if_item"]["vgprs"] <= 128        # 8 workgroups of 4 waves per compute unit
    assert table["k_if_ring"]["lds"] == 12 * cap and table["k_if_pair"]["lds"] == 0 and table["k_if_pair"]["vgprs"] <= 64


def test_entry_rejects_bad_arguments_before_any_device_work():
    """Call-level failures (the library is needed, a GPU is not)."""
    from topowx_amd import _qalib
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    lon, lat, tmin = _line_pool(6)
    days = get_days_metadata(dt.date(2001, 1, 1), dt.date(2001, 2, 9))
    obs = np.ascontiguousarray(tmin.T, np.float32)
    grp = np.zeros(40, np.int8)
    ok = dict(lon=lon, lat=lat, obs=obs, ymd=np.array(days[YMD]), eligible=np.ones(6, bool), target_idx=np.array([0]),
              group=grp, nthres_all=np.array([27]), nthres_target_por=np.array([[27]]))

    def call(**kw):
        return _qalib.infill_matrix(**dict(ok, **kw))
    ymd = np.array(days[YMD])
    ymd[7] = ymd[6]
    with pytest.raises(_qalib.QaError, match="not consecutive"):
        call(ymd=ymd)
    with pytest.raises(_qalib.QaError, match="target index"):
        call(target_idx=np.array([6]))
    with pytest.raises(_qalib.QaError, match="group"):
        call(group=np.full(40, 1, np.int8))
    bad = lon.copy()
    bad[3] = np.nan
    with pytest.raises(_qalib.QaError, match="non-finite"):
        call(lon=bad)
    with pytest.raises(_qalib.QaError, match="min_daily_nnghs"):
        call(min_daily_nnghs=0)
    with pytest.raises(ValueError):
        call(nthres_target_por=np.array([27]))
    with pytest.raises(ValueError):
        call(obs=obs[:5])
