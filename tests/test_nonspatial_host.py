"""CPU: step08's non-spatial checks without a GPU -- the numpy restatement (tests/restate_nonspatial.py) against the
executed-reference golden (tests/golden/make_golden_nonspatial.py), the header against the binding, the resource table
of the new kernels, the year cap, the argument rules of the step08 driver and the knife-edge share of the random cases
the GPU test compares exactly.

Flags are compared exactly and rows (mean, standard deviation) to 1e-7 degC: the golden maker asserted that every
z-score the reference formed lies more than 1e-5 from 6 and every lagged-range comparison at least 1e-4 from equality."""
import datetime as dt
import os
import re
import sys

import numpy as np
import pytest

from topowx_amd.dates import YMD, get_days_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from spatial_cases import TOL  # noqa: E402

NEW_KERNELS = ("k_ns_init", "k_ns_dups", "k_ns_streak", "k_ns_gap", "k_ns_norms", "k_ns_clim", "k_ns_spike", "k_ns_lagrange",
               "k_ns_mega")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_nonspatial_v1.npz"))


@pytest.fixture(scope="module")
def case(gold):
    import make_golden_nonspatial as mk
    tmin, tmax, days, plants = mk.case_inputs()
    assert mk.input_hash(tmin, tmax, days) == str(gold["input_hash"]), "synthetic generator drifted: regenerate the golden"
    return tmin, tmax, days, plants


@pytest.fixture(scope="module")
def restated(case):
    import restate_nonspatial as RN
    tmin, tmax, days, _ = case
    return RN.run(tmin, tmax, days[YMD])


def test_golden_content(gold, case):
    tmin, tmax, days, plants = case
    assert tmin.shape == (5844, 16) and tmin.dtype == np.float32
    assert set(np.unique(days.YEAR[days.MONTH * 100 + days.DAY == 229])) == {1992, 1996, 2000, 2004}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_nonspatial_v1.npz")) < 1024 * 1024
    assert float(gold["z_margin"]) > 1e-5 and float(gold["lag_margin"]) >= 1e-4 and int(gold["mad0_rows"]) > 0
    f = (gold["flags_tmin"], gold["flags_tmax"])
    for k in (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 18):
        assert (f[0] == k).sum() + (f[1] == k).sum() > 0, k
    for v, obs in enumerate((tmin, tmax)):
        assert np.array_equal(f[v] == 2, np.isnan(obs))
    for k, want in plants.items():
        assert np.array_equal(gold["plant_" + k], np.asarray(want, np.int32)), k
    # the kept quirks: November copied onto December stays unflagged by the duplicate checks; the run that reaches the
    # end of the series is not a streak; the two equal clusters have no gap flag
    assert not np.isin(f[0][plants["dupmonths_quirk"], 3], (4, 5, 6)).any()
    assert (f[1][plants["streak_end"], 7] == 1).all() and not (f[0][plants["cluster"], 9] == 10).any()
    assert not (gold["norms"][..., 1] == 0).any()                 # no row with standard deviation 0
    assert float(gold["ref_station_years_per_second"]) > 0


def test_restatement_equals_the_golden(gold, restated):
    for name in ("flags_tmin", "flags_tmax"):
        bad = np.argwhere(restated[name] != gold[name])
        assert bad.size == 0, (name, bad[:10].tolist())
    assert not restated["knife"].any() and not restated["std0"].any()
    assert abs(restated["z_margin"].min() - float(gold["z_margin"])) < 1e-4          # (the reference's float32 run is in it)
    assert restated["lag_margin"].min() == pytest.approx(float(gold["lag_margin"]), abs=1e-6)
    got, want = restated["norms"][gold["norm_stns"]], gold["norms"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isfinite(want).sum() > 8000
    print("max |row - golden| %.3g" % np.nanmax(np.abs(got - want)))
    assert np.nanmax(np.abs(got - want)) < TOL
    nan = np.unpackbits(gold["norms_nan"])[:16 * 2 * 731].reshape(16, 2, 731).astype(bool)
    assert np.array_equal(np.isnan(restated["norms"][..., 0]), nan)
    assert int(restated["mad0"].sum()) == int(gold["mad0_rows"])


def test_restatement_equals_the_float32_edge_case(gold):
    import make_golden_nonspatial as mk
    import restate_nonspatial as RN
    e0, e1, days, names = mk.edge_inputs()
    assert mk.input_hash(e0, e1, days) == str(gold["edge_hash"]) and names == gold["edge_names"].tolist()
    assert np.array_equal(e0, gold["edge_tmin"]) and np.array_equal(e1, gold["edge_tmax"])
    res = RN.run(e0, e1, days[YMD])
    assert np.array_equal(res["flags_tmin"], gold["edge_flags_tmin"]) and np.array_equal(res["flags_tmax"], gold["edge_flags_tmax"])
    # 10.2 / 0.2: >= 10.0 as a float32 difference, below it as a double one
    a, b = np.float32(10.2), np.float32(0.2)
    assert np.float32(a - b) >= np.float32(10.0) and float(a) - float(b) < 10.0
    cls = {str(n).split("_", 1)[1] for n in names}
    assert cls == {"both", "f32_only", "neither"}
    for k, n in enumerate(names):
        nflag = int((gold["edge_flags_tmin"][:, k] > 2).sum() + (gold["edge_flags_tmax"][:, k] > 2).sum())
        assert nflag == (0 if str(n).endswith("neither") else 1), n


def test_header_entries_equal_exports():
    from topowx_amd import _qalib
    h = open(os.path.join(ROOT, "include", "twx_qa.h")).read()
    assert sorted(set(re.findall(r"\b(twxqa_\w+)\s*\(", h))) == sorted(_qalib.EXPORTS)
    assert "twxqa_non_spatial" in _qalib.EXPORTS
    m = re.search(r"#define TWXQA_MAX_GAP_VALUES (\d+)", h)
    assert m and int(m.group(1)) == _qalib.MAX_GAP_VALUES
    assert _qalib.MAX_GAP_VALUES // 31 >= 100                     # the gap check admits at least 100 years
    assert _qalib.MAX_GAP_VALUES & (_qalib.MAX_GAP_VALUES - 1) == 0
    m = re.search(r"#define TWXQA_NS_NKERNELS (\d+)", h)
    assert m and int(m.group(1)) == len(_qalib.NON_SPATIAL_KERNELS) == 8
    assert len(_qalib.SPATIAL_ONLY_KERNELS) == 6
    from topowx_amd import qa
    assert qa.NON_SPATIAL_FLAGS == (2, 3, 4, 6, 5, 7, 8, 9, 10, 15, 11, 13, 12, 18)
    for name in ("run_qa_non_spatial", "QA_NAUGHT", "QA_DUP_YEAR", "QA_DUP_MONTH", "QA_DUP_YEAR_MONTH", "QA_DUP_WITHIN_MONTH",
                 "QA_IMPOSS_VALUE", "QA_STREAK", "QA_GAP", "QA_INTERNAL_INCONSIST", "QA_LAGRANGE_INCONSIST", "QA_SPIKE_DIP",
                 "QA_CLIM_OUTLIER"):
        assert name in qa.__all__ and hasattr(qa, name), name


def test_constants_equal_the_reference(gold):
    from topowx_amd.qa import qa_temp
    for k in ("QA_OK", "QA_MISSING", "QA_NAUGHT", "QA_DUP_YEAR", "QA_DUP_MONTH", "QA_DUP_YEAR_MONTH", "QA_DUP_WITHIN_MONTH",
              "QA_IMPOSS_VALUE", "QA_STREAK", "QA_GAP", "QA_INTERNAL_INCONSIST", "QA_LAGRANGE_INCONSIST", "QA_SPIKE_DIP",
              "QA_CLIM_OUTLIER", "QA_MEGA_INCONSIST", "MIN_NORM_VALUES"):
        assert float(getattr(qa_temp, k)) == float(gold["const_" + k]), k
    assert (float(gold["const_TMAX_RECORD"]), float(gold["const_TMIN_RECORD"])) == (57.7, -89.4)


def test_resource_table_lists_the_new_kernels():
    """No scratch, no spills, and the LDS the caps were sized for (no build in this checkout: skipped, as
    test_isa_resources)."""
    from topowx_amd import _qalib
    res = os.path.join(ROOT, "topowx_amd", "libtwxqa.resources.txt")
    if not os.path.exists(_qalib.LIB_PATH) or not os.path.exists(res):
        pytest.skip("no build in this checkout (run ./build.sh)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import ctypes
    import isa_resources
    assert hasattr(ctypes.CDLL(_qalib.LIB_PATH), "twxqa_non_spatial")
    table = isa_resources.parse(res)
    for k in NEW_KERNELS:
        assert k in table, k
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
    lds = table["k_ns_gap"]["lds"]
    assert 4 * _qalib.MAX_GAP_VALUES <= lds <= 4 * _qalib.MAX_GAP_VALUES + 64
    assert 8 * lds <= 160 * 1024 and table["k_ns_gap"]["vgprs"] <= 64           # 8 workgroups of 4 waves per compute unit
    lds = table["k_ns_norms"]["lds"]
    assert 4 * _qalib.MAX_NORM_VALUES + 2048 <= lds <= 4 * _qalib.MAX_NORM_VALUES + 2048 + 64
    assert 8 * lds <= 160 * 1024 and table["k_ns_norms"]["vgprs"] <= 64
    years = _qalib.MAX_GAP_VALUES // 31
    assert table["k_ns_dups"]["lds"] <= 74 * years + 64 and 8 * table["k_ns_dups"]["lds"] <= 160 * 1024


def test_axis_over_the_year_cap_fails_the_call():
    """More years than TWXQA_MAX_GAP_VALUES / 31 is a call-level failure that names the macro, before any device work
    (the library is needed, a GPU is not)."""
    from topowx_amd import _qalib
    if not os.path.exists(_qalib.LIB_PATH):
        pytest.skip("no build in this checkout (run ./build.sh)")
    years = _qalib.MAX_GAP_VALUES // 31 + 1
    days = get_days_metadata(dt.date(1800, 1, 1), dt.date(1800 + years - 1, 12, 31))
    series = np.zeros((1, days.size), np.float32)
    with pytest.raises(_qalib.QaError, match="TWXQA_MAX_GAP_VALUES"):
        _qalib.non_spatial(series, series, days[YMD])
    with pytest.raises(_qalib.QaError, match="%d years" % years):
        _qalib.non_spatial(series, series, days[YMD])
    # the same number of years on an axis that starts and ends mid-year
    mid = get_days_metadata(dt.date(1800, 12, 30), dt.date(1800 + years - 1, 1, 2))
    with pytest.raises(_qalib.QaError, match="TWXQA_MAX_GAP_VALUES"):
        _qalib.non_spatial(series[:, :mid.size], series[:, :mid.size], mid[YMD])
    ymd = np.array(days[YMD][:40])
    ymd[7] = ymd[6]
    with pytest.raises(_qalib.QaError, match="not consecutive"):
        _qalib.non_spatial(series[:, :40], series[:, :40], ymd)
    with pytest.raises(ValueError):
        _qalib.non_spatial(series[0], series[0], days[YMD])


def test_step08_argument_rules(tmp_path, capsys, monkeypatch):
    import corrob_cases
    from topowx_amd import step08
    rs = np.random.RandomState(4)
    days = get_days_metadata(dt.date(1990, 1, 1), dt.date(1990, 2, 9))
    n, nd = 5, days.size
    tmin = np.round(rs.randn(nd, n) * 5, 1).astype(np.float32)
    tmax = (tmin + 10).astype(np.float32)
    ids = np.array(["GHCN_%03d" % i for i in range(n)])
    lon, lat = -110 + rs.rand(n), 45 + rs.rand(n)
    prev = (("qflag_tmin", 3, 1, b"D"),)
    db = corrob_cases.write_db(str(tmp_path / "all.nc"), ids, lon, lat, tmin, tmax, days, "NETCDF3_64BIT", prev=prev)
    bare = corrob_cases.write_db(str(tmp_path / "bare.nc"), ids, lon, lat, tmin, tmax, days, "NETCDF3_64BIT", qflags=False)
    out = str(tmp_path / "r.npz")
    for argv in (["--nonspatial", "--spatial"], ["--write"], ["--nonspatial", "--spatial", "--write"]):
        with pytest.raises(SystemExit):
            step08.main(["--db", db, "--out", out] + argv)
    capsys.readouterr()
    assert step08.main(["--db", bare, "--out", out, "--nonspatial", "--write"]) == 1       # nothing to write into
    assert "qflag" in capsys.readouterr().err and not os.path.exists(out)
    seen = {}

    def fake(a, b, days_, device=0, details=False, timing=None):
        seen["tmin"], seen["shape"] = a.copy(), a.shape
        timing.update(gap_kernel_ms=1.0)
        f = np.where(np.isnan(a), 2, 1).astype(np.uint8)
        f[5, 0] = 10
        return f, np.where(np.isnan(b), 2, 1).astype(np.uint8)

    def never(*a, **k):
        raise AssertionError("--nonspatial must not run the spatial stage")

    monkeypatch.setattr(step08, "run_qa_non_spatial", fake)
    monkeypatch.setattr(step08, "run_qa_spatial_only", never)
    monkeypatch.setattr(step08, "qa_spatial_regress", never)
    tfile = tmp_path / "t.txt"
    tfile.write_text("GHCN_001\nGHCN_004\n")
    assert step08.main(["--db", db, "--out", out, "--nonspatial", "--write", "--targets", str(tfile)]) == 0
    import json
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["shape"] == (nd, 2) and np.isnan(seen["tmin"][3, 0])            # the flagged observation is masked first
    assert line["stations"] == 2 and line["flags_tmin"]["10"] == 1 and line["rows_written"] == 1
    assert sorted(line["flags_tmin"]) == sorted(str(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 18))
    from topowx_amd.qa import StationObsPool
    back = StationObsPool.from_netcdf(db, qflags=True)
    assert back.qflag_tmin[5, 1] == b"G" and back.qflag_tmin[3, 1] == b"D"      # written on the target's column; the old one kept
    assert sorted(np.load(out).files) == ["flags_tmax", "flags_tmin", "ids", "ymd"]


@pytest.mark.parametrize("name", ["64x12", "5x8_mid_year", "130x7_near_100"])
def test_random_cases_have_few_knife_edge_series(name):
    """The GPU test leaves a series out when the restatement sees a |z - 6| within 6e-7; here: at most 1 % of them."""
    import nonspatial_cases as NC
    want = NC.restated(name)
    n, first, last, _ = NC.CASES[name]
    assert want["knife"].shape == (n,) and want["knife"].sum() <= NC.MAX_KNIFE * n
    assert not want["std0"].any()
    f = np.concatenate([want["flags_tmin"].ravel(), want["flags_tmax"].ravel()])
    assert len(set(np.unique(f).tolist())) >= 10                 # most checks of the chain fire in every case
